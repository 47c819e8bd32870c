// shpl_upconv.h -- the host plan that the upconv3 forward (shpl_upconv.hip) and its gradients
// (shpl_upconv_grad.hip) share: the argument checks, in shpl_conv3x3's order, and the tiling of the INPUT map.
#pragma once

#include "shpl_conv_tile.h"

namespace shpl {
namespace {

struct UpPlan : TilePlan {
    size_t wp, row_ptr, part, total;  // the workspace: packed weights, row pointers (pooled), statistics partials
};

// shpl_conv3x3's plan checks, in its order, over the input map; the output's 4 n_frames h w rows are 32-bit too.
int up_plan(int dtype, int n_frames, int64_t h, int64_t w, int64_t c_a, int64_t c_b, int64_t c_out, bool pooled,
            bool stats, int64_t pool_cap, UpPlan *pl) {
    if (dtype != SHPL_F32 && dtype != SHPL_BF16) return SHPL_ERR_ARG;
    if (n_frames < 0 || h < 0 || w < 0 || c_a < 0 || c_b < 0 || c_out < 1 || c_a + c_b < 1) return SHPL_ERR_BAD_SHAPE;
    if (h > (1 << 20) || w > (1 << 20) || c_a + c_b > (1 << 16) || c_out > (1 << 16)) return SHPL_ERR_BAD_SHAPE;
    if (pool_cap < 0 || pool_cap >= (1LL << 31)) return SHPL_ERR_BAD_SHAPE;
    pl->ck = by_dtype(dtype, [](auto t) { return Elem<typename decltype(t)::T>::CK; });
    pl->qa = (int)((c_a + pl->ck - 1) / pl->ck);
    pl->qb = (int)((c_b + pl->ck - 1) / pl->ck);
    pl->n_cob = (int)((c_out + NCO - 1) / NCO);
    pl->tiles_x = (int)((w + TW - 1) / TW);
    pl->tiles_y = (int)((h + TH - 1) / TH);
    pl->tiles_per_frame = pl->tiles_x * pl->tiles_y;
    pl->n_tiles = (int64_t)n_frames * pl->tiles_per_frame;
    if (pl->n_tiles >= (1LL << 31) || (int64_t)n_frames * h * w * 4 >= (1LL << 31)) return SHPL_ERR_BAD_SHAPE;
    Layout l;
    pl->wp = l.take((size_t)pl->n_cob * (pl->qa + pl->qb) * W_ROWS * Elem<float>::CB);
    pl->row_ptr = l.take(pooled ? (size_t)n_frames * (h + 1) * 4 : 0);
    pl->part = l.take(stats ? (size_t)pl->n_cob * NCO * 2 * pl->n_tiles * 8 : 0);
    pl->total = l.end;
    return SHPL_OK;
}

}  // namespace
}  // namespace shpl
