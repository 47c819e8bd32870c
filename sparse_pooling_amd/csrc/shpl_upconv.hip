// shpl_upconv.hip -- the after-VGG upconv3: a 3x3 stride-2 transposed convolution over [a || pooled b], with the
// SHPL concat (and the pooling itself) fused into its input staging.
//
// Reference (avod/avod/core/feature_extractors/fusion_vgg_pyramid.py:53-60, :198-206, switched on by
// rpn_sparse_pooling_after_vgg / rpn_dual_sparse_pooling_after_vgg):
//     conv4 = sparse_pool_layer([conv4_bev, conv4_img], ...)            # both directions, stride 8
//     upconv3 = slim.conv2d_transpose(conv4, vgg_conv3[1], [3, 3], stride=2, normalizer_fn=slim.batch_norm)
// i.e. SAME, stride 2, no bias, BatchNorm (center, no scale, eps 1e-3, decay 0.999), ReLU.
//
// TF computes conv2d_transpose as conv2d_backprop_input of the SAME stride-2 conv over the 2h x 2w output:
// that conv has pad_total = max((h - 1) * 2 + 3 - 2h, 0) = 1, pad_before = pad_total // 2 = 0, pad_after = 1, so
//     out[f, oy, ox, co] = sum over (i, ky): 2i + ky = oy, (j, kx): 2j + kx = ox, ci of
//                          x[f, i, j, ci] * W[ky, kx, co, ci]
// with W slim's variable [3][3][c_out][c_in] (HWOI). Per axis, even o = 2i takes k = 0 from i and k = 2 from
// i - 1, odd o = 2i + 1 takes k = 1 from i: tap k belongs to output parity k & 1 and reads input i - (k >> 1).
// So the four output pixels (2i + py, 2j + px) read the 2 x 2 window x[i-1..i, j-1..j] (zeros outside) through
// 4, 2, 2 and 1 of the nine taps: 9 c_in c_out multiply-adds per input pixel.
//
// The kernel is shpl_conv.hip's tiled implicit GEMM turned round: one workgroup owns an 8 x 32 tile of INPUT
// pixels (16 x 64 output pixels) and 32 output channels; a chunk of the tile's 9 x 33 halo (one row up, one
// column left) and the chunk's 9 x 32 weight rows are staged once by the conv's staging (shpl_conv_stage.h:
// LDS-DMA for dense chunks, the runs of the halo summed in the pull's order for pooled ones) and feed all four
// parity accumulators: wave w keeps 4 parities x 2 input rows of 32 x 32 f32 accumulators (128 registers),
// each tap one MFMA step into the parity it belongs to. f32: v_mfma_f32_32x32x2_f32 (exact f32 products);
// bf16: v_mfma_f32_32x32x16_bf16; f32 accumulation, one rounding at the store, shpl_conv3x3's epilogue.
#include "shpl_upconv.h"

namespace shpl {
namespace {

constexpr int UH = TH + 1, UW = TW + 1;  // the halo tile: one row above, one column left of the input tile

template <typename T, bool POOLED, bool STATS, bool GROUP>
__global__ __launch_bounds__(CONV_BLOCK, 2) void k_upconv3x3(const ConvArgs p) {
    typedef Elem<T> E;
    constexpr int CK = E::CK, NP = E::NP;
    static_assert(NP == 2, "two 16-byte pieces per LDS row (the swizzle)");
    constexpr int IN_BYTES = UH * UW * NP * 16, W_BYTES = W_ROWS * NP * 16;
    // the output rows' transpose (epilogue) reuses the chunk buffers: 4 waves x 32 pixels x OPITCH
    static_assert(4 * 32 * OPITCH<T> <= IN_BYTES + W_BYTES, "epilogue rows fit the chunk buffers");
    __shared__ __attribute__((aligned(16))) uint8_t s_buf[IN_BYTES + W_BYTES];
    uint8_t *const s_in = s_buf, *const s_w = s_buf + IN_BYTES;
    __shared__ float s_red[4][2][NCO];
    __shared__ __attribute__((aligned(16))) float s_par[1][2][NCO];  // scale, shift - center * scale
    const HaloRuns runs = halo_runs_lds<POOLED, UH, UW>();

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int pl = lane & 31, hf = lane >> 5;
    const int tile = (int)xcd_block((int)blockIdx.x, p.n_tiles);
    const int cob = blockIdx.y;
    int f, y0, x0;
    tile_origin<TH>(p, tile, f, y0, x0);
    const int H = p.h, W = p.w;
    const int Q = p.qa + p.qb;

    epilogue_coeffs<1>(p, cob, s_par, tid);
    const int n_run = POOLED ? find_runs<UH, UW>(p, f, y0, x0, runs) : 0;  // (s_par: published by the next barrier)

    f32x16 acc[4][RPW];  // [2 py + px][input row of the wave]
#pragma unroll
    for (int par = 0; par < 4; ++par)
#pragma unroll
        for (int m = 0; m < RPW; ++m)
#pragma unroll
            for (int i = 0; i < 16; ++i) acc[par][m][i] = 0.0f;

    // the weights are packed by k_pack_w's transposing form ([3][3][c_out][c_in] is what it reads there), which
    // puts W[ky][kx] at packed tap 8 - (3 ky + kx)
    const T *wq = reinterpret_cast<const T *>(p.wp) + (int64_t)cob * Q * W_ROWS * CK;
    for (int q = 0; q < Q; ++q) {
        // the tile's origin and the thread's index, opaque per chunk: the staging's per-lane conditions on them
        // (inside the map, inside the halo, a piece of the tile) are then worked out per chunk -- a few compares --
        // instead of being kept for the whole loop as lane masks, two scalar registers each, which ran the
        // kernel out of scalar registers
        int yq = y0, xq = x0, tq = tid;
        asm volatile("" : "+s"(yq), "+s"(xq), "+v"(tq));
        conv_stage<T, POOLED, 1, GROUP, UH, UW>(p, q, f, yq, xq, wq, 0, s_in, s_w, runs, n_run, tq);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // the LDS-DMAs have landed
        __syncthreads();
        // ---- the nine taps: tap (ky, kx) reads input (i - (ky >> 1), j - (kx >> 1)) -- halo row
        // RPW wave + m + 1 - (ky >> 1), halo column pl + 1 - (kx >> 1) -- into parity (ky & 1, kx & 1)
#pragma unroll
        for (int ky = 0; ky < 3; ++ky) {
#pragma unroll
            for (int kx = 0; kx < 3; ++kx) {
                const int par = 2 * (ky & 1) + (kx & 1), dy = ky >> 1, dx = kx >> 1;
                const Frag<T> b = lds_frag<T>(s_w + piece_off<true, 0>((8 - (ky * 3 + kx)) * NCO + pl, hf));
#pragma unroll
                for (int m = 0; m < RPW; ++m) {
                    const Frag<T> a =
                        lds_frag<T>(s_in + piece_off<true, 0>((RPW * wave + m + 1 - dy) * UW + pl + 1 - dx, hf));
                    acc[par][m] = mfma_tap<T>(b, a, acc[par][m]);
                }
            }
        }
        __syncthreads();  // the chunk's buffers are restaged next
    }

    // ---- epilogue (epilogue_row): acc element i of (par, m) is channel cob*32 + 8(i>>2) + 4h + (i&3) of output
    // pixel (2 (y0 + RPW w + m) + py, 2 (x0 + pl) + px); a row of 32 pixels is every second output pixel of one
    // output row. The lane's 8 output pixels are summed parities first, then rows: the statistics' fixed order.
    // The arguments are read again here: read once at the kernel's start they would sit in scalar registers
    // across the whole K loop (and spill).
    const ConvArgs pe = kernarg_again<ConvArgs>(0);
    const int64_t out_row0 = (int64_t)f * 4 * H * W;  // the frame's first output row: 2H x 2W pixels per frame
    uint8_t *const s_o = s_buf + wave * 32 * OPITCH<T>;
    ChanSums sums;
    sums.zero();
#pragma unroll
    for (int par = 0; par < 4; ++par) {
        const int py = par >> 1, px = par & 1;
#pragma unroll
        for (int m = 0; m < RPW; ++m) {
            const int y = y0 + RPW * wave + m;
            const int64_t orow = out_row0 + (int64_t)(2 * y + py) * (2 * W) + px;  // + 2 * input column
            epilogue_row<T, true, STATS>(pe, acc[par][m], s_par[0], s_o, cob * NCO, y < H, x0, W, &sums,
                                         [orow, x0](const ConvArgs &a, int col, int c) {
                                             return reinterpret_cast<T *>(a.out) +
                                                    (orow + 2 * (x0 + col)) * a.out_stride + c;
                                         });
        }
    }
    if (STATS) {
        int te = tid;  // (opaque, as the staging's: `tid < 64` is not kept as a lane mask from the kernel's start)
        asm volatile("" : "+v"(te));
        stats_reduce_tile(pe, sums, s_red, te, cob * NCO, tile);
    }
}

// ---------------------------------------------------------------- host
template <typename T>
int up_launch(const UpPlan &pl, const ConvArgs &a, bool pooled, bool stats, const void *w, const int64_t *frame_off,
              double *d_stats, hipStream_t s) {
    if (const int rc = pack_weights<T>(a, w, pl.n_cob, 1, s)) return rc;
    if (pooled) {
        if (const int rc = row_pointers(a, frame_off, s)) return rc;
    }
    using Kernel = void (*)(const ConvArgs);
    const Kernel kernel = pooled_form<Kernel>(pooled, a.ent_col, [&](auto po, auto gr) {
        return stats ? k_upconv3x3<T, po(), true, gr()> : k_upconv3x3<T, po(), false, gr()>;
    });
    hipLaunchKernelGGL(kernel, dim3((unsigned)pl.n_tiles, (unsigned)pl.n_cob), dim3(CONV_BLOCK), 0, s, a);
    SHPL_LAUNCH_CHECK();
    if (stats) {
        hipLaunchKernelGGL(k_stats_reduce, dim3(pl.n_cob * NCO * 2), dim3(RED_BLOCK), 0, s, a.part, (int)pl.n_tiles,
                           a.c_out, d_stats);
        SHPL_LAUNCH_CHECK();
    }
    return SHPL_OK;
}

}  // namespace
}  // namespace shpl

using namespace shpl;

extern "C" int shpl_upconv3x3_workspace_bytes(int dtype, int n_frames, int64_t h, int64_t w, int64_t c_a, int64_t c_b,
                                              int64_t c_out, int64_t pool_nnz_cap, int stats, size_t *bytes) {
    if (!bytes) return SHPL_ERR_ARG;
    UpPlan pl;
    const bool pooled = pool_nnz_cap >= 0;
    const int rc = up_plan(dtype, n_frames, h, w, c_a, c_b, c_out, pooled, stats != 0, pooled ? pool_nnz_cap : 0, &pl);
    if (rc) return rc;
    *bytes = pl.total;
    return SHPL_OK;
}

extern "C" int shpl_upconv3x3(int dtype, int n_frames, int64_t h, int64_t w, const void *d_a, int64_t a_stride,
                              int64_t a_off, int64_t c_a, const void *d_b, int64_t b_stride, int64_t b_off,
                              int64_t c_b, const shpl_csr *pool, const int64_t *d_frame_off, const void *d_weights,
                              int64_t c_out, const float *d_center, const float *d_scale, const float *d_shift,
                              int act, void *d_out, int64_t out_stride, double *d_stats, void *d_ws, size_t ws_bytes,
                              void *stream) {
    const bool pooled = pool != nullptr, stats = d_stats != nullptr;
    const Src A = {d_a, a_stride, a_off, c_a}, B = {d_b, b_stride, b_off, c_b};
    UpPlan pl;
    int rc = up_plan(dtype, n_frames, h, w, c_a, c_b, c_out, pooled, stats, pooled ? pool->nnz_cap : 0, &pl);
    if (rc) return rc;
    if (act != 0 && act != 1) return SHPL_ERR_ARG;
    if (!d_weights || (ws_bytes > 0 && !d_ws)) return SHPL_ERR_ARG;
    if (ws_bytes < pl.total) return SHPL_ERR_WORKSPACE;
    rc = check_sources(n_frames, h, w, A, B, pool, d_frame_off, out_stride, c_out);
    if (rc) return rc;
    if (pl.n_tiles == 0) return SHPL_OK;
    if (!d_out || (c_a > 0 && !d_a)) return SHPL_ERR_ARG;
    ConvArgs a = conv_args(dtype, n_frames, h, w, pl, A, B, pool);
    a.wp = region<void>(d_ws, pl.wp);
    a.row_ptr = pooled ? region<int32_t>(d_ws, pl.row_ptr) : nullptr;
    a.part = stats ? region<double>(d_ws, pl.part) : nullptr;
    a.center = d_center;
    a.scale = d_scale;
    a.shift = d_shift;
    a.act = act;
    a.out = d_out;
    a.out_stride = out_stride;
    a.c_out = (int)c_out;
    a.vec_out = vec16({d_out, out_stride, 0, c_out}, piece_elems(dtype));
    hipStream_t s = (hipStream_t)stream;
    return by_dtype(dtype, [&](auto t) {
        return up_launch<typename decltype(t)::T>(pl, a, pooled, stats, d_weights, d_frame_off, d_stats, s);
    });
}
