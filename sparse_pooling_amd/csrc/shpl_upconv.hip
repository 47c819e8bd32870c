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
    constexpr int OPITCH = NCO * (int)sizeof(T) + 16;
    static_assert(4 * 32 * OPITCH <= IN_BYTES + W_BYTES, "epilogue rows fit the chunk buffers");
    __shared__ __attribute__((aligned(16))) uint8_t s_buf[IN_BYTES + W_BYTES];
    uint8_t *const s_in = s_buf, *const s_w = s_buf + IN_BYTES;
    __shared__ float s_red[4][2][NCO];
    __shared__ __attribute__((aligned(16))) float s_par[2][NCO];  // scale, shift - center * scale
    const HaloRuns runs = halo_runs_lds<POOLED, UH, UW>();

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int pl = lane & 31, hf = lane >> 5;
    const int tile = (int)xcd_block((int)blockIdx.x, p.n_tiles);
    const int cob = blockIdx.y;
    const int f = tile / p.tiles_per_frame;
    const int t_in = tile - f * p.tiles_per_frame;
    const int ty = t_in / p.tiles_x, tx = t_in - ty * p.tiles_x;
    const int y0 = ty * TH, x0 = tx * TW;
    const int H = p.h, W = p.w;
    const int Q = p.qa + p.qb;

    // epilogue coefficients, as k_conv3x3: scale (1 when absent) and shift - center * scale, applied as one fma
    if (tid < NCO) {
        const int c = cob * NCO + tid;
        const bool in = c < p.c_out;
        const float sc = p.scale && in ? p.scale[c] : 1.0f;
        const float ce = p.center && in ? p.center[c] : 0.0f;
        const float sh = p.shift && in ? p.shift[c] : 0.0f;
        s_par[0][tid] = sc;
        s_par[1][tid] = __fsub_rn(sh, __fmul_rn(ce, sc));
    }
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
                const uint8_t *brow = s_w + piece_off<true, 0>((8 - (ky * 3 + kx)) * NCO + pl, hf);
                if constexpr (sizeof(T) == 4) {
                    const f32x4 b4 = *reinterpret_cast<const f32x4 *>(brow);
#pragma unroll
                    for (int m = 0; m < RPW; ++m) {
                        // lane half h supplies channels 4h+s of the chunk to MFMA s (both operands)
                        const f32x4 a4 = *reinterpret_cast<const f32x4 *>(
                            s_in + piece_off<true, 0>((RPW * wave + m + 1 - dy) * UW + pl + 1 - dx, hf));
#pragma unroll
                        for (int s = 0; s < 4; ++s)
                            acc[par][m] = __builtin_amdgcn_mfma_f32_32x32x2f32(b4[s], a4[s], acc[par][m], 0, 0, 0);
                    }
                } else {
                    const bf16x8 b8 = *reinterpret_cast<const bf16x8 *>(brow);
#pragma unroll
                    for (int m = 0; m < RPW; ++m) {
                        const bf16x8 a8 = *reinterpret_cast<const bf16x8 *>(
                            s_in + piece_off<true, 0>((RPW * wave + m + 1 - dy) * UW + pl + 1 - dx, hf));
                        acc[par][m] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(b8, a8, acc[par][m], 0, 0, 0);
                    }
                }
            }
        }
        __syncthreads();  // the chunk's buffers are restaged next
    }

    // ---- epilogue, k_conv3x3's: acc element i of (par, m) is channel cob*32 + 8(i>>2) + 4h + (i&3) of output
    // pixel (2 (y0 + RPW w + m) + py, 2 (x0 + pl) + px). A row of 32 pixels (every second output pixel of one
    // output row) goes through LDS (wave-private) and out as 16-byte pieces; blocks whose channels are not whole
    // or whose rows are not 16-byte aligned store channel by channel.
    // Its arguments are read again here, through a kernel-argument pointer the compiler cannot see through: read
    // once at the kernel's start they would sit in scalar registers across the whole K loop (and spill).
    uint64_t kargs = (uint64_t)__builtin_amdgcn_kernarg_segment_ptr();
    asm volatile("" : "+s"(kargs));
    const auto &pe = *(const __attribute__((address_space(4))) ConvArgs *)kargs;
    constexpr int HE = E::HE, PPP = NCO / HE;  // channels per piece, pieces per pixel
    const int x = x0 + pl;
    const int64_t out_row0 = (int64_t)f * 4 * H * W;  // the frame's first output row: 2H x 2W pixels per frame
    uint8_t *const s_o = s_buf + wave * 32 * OPITCH;
    const bool fast = pe.vec_out && cob * NCO + NCO <= pe.c_out;
    float s1[16], s2[16];
#pragma unroll
    for (int i = 0; i < 16; ++i) s1[i] = s2[i] = 0.0f;
#pragma unroll
    for (int par = 0; par < 4; ++par) {
        const int py = par >> 1, px = par & 1;
#pragma unroll
        for (int m = 0; m < RPW; ++m) {
            const int y = y0 + RPW * wave + m;
            const bool ok = y < H && x < W;
            const int64_t orow = out_row0 + (int64_t)(2 * y + py) * (2 * W) + px;  // + 2 * input column
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const int cl = 8 * g + 4 * hf, c = cob * NCO + cl;  // first channel of the run
                const f32x4 scl = *reinterpret_cast<const f32x4 *>(&s_par[0][cl]);
                const f32x4 sft = *reinterpret_cast<const f32x4 *>(&s_par[1][cl]);
                T o[4];
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const float v = acc[par][m][4 * g + j];
                    if (STATS && ok) {
                        s1[4 * g + j] = __fadd_rn(s1[4 * g + j], v);
                        s2[4 * g + j] = __fadd_rn(s2[4 * g + j], __fmul_rn(v, v));
                    }
                    o[j] = relu_bits(E::back(__builtin_fmaf(v, scl[j], sft[j])), pe.act == 1);
                }
                if (fast) {
                    __builtin_memcpy(s_o + pl * OPITCH + cl * sizeof(T), o, sizeof(o));
                } else if (ok) {
                    T *dst = reinterpret_cast<T *>(pe.out) + (orow + 2 * x) * pe.out_stride + c;
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        if (c + j >= pe.c_out) break;
                        dst[j] = o[j];
                    }
                }
            }
            if (fast) {
                asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // the wave's row is in LDS (one wave: in order)
#pragma unroll
                for (int k = 0; k < 32 * PPP / 64; ++k) {
                    const int pc = lane + 64 * k, pxl = pc / PPP, pi = pc % PPP;
                    const u32x4 v = *reinterpret_cast<const u32x4 *>(s_o + pxl * OPITCH + pi * 16);
                    if (y < H && x0 + pxl < W)
                        *reinterpret_cast<u32x4 *>(reinterpret_cast<T *>(pe.out) +
                                                   (orow + 2 * (x0 + pxl)) * pe.out_stride + cob * NCO + pi * HE) = v;
                }
            }
        }
    }
    if (STATS) {
        // per channel: the lane's 8 output pixels are summed above (parities, then rows, a fixed order); over the
        // 32 pixels of the lane half by k_conv3x3's halving butterfly, then over the 4 waves in double
#pragma unroll
        for (int n = 8, off = 16; n >= 1; n >>= 1, off >>= 1) {
            const bool up = (pl & off) != 0;
#pragma unroll
            for (int i = 0; i < n; ++i) {
                const float g1 = up ? s1[i] : s1[i + n], k1 = up ? s1[i + n] : s1[i];
                const float g2 = up ? s2[i] : s2[i + n], k2 = up ? s2[i + n] : s2[i];
                s1[i] = __fadd_rn(k1, __shfl_xor(g1, off, 64));
                s2[i] = __fadd_rn(k2, __shfl_xor(g2, off, 64));
            }
        }
        s1[0] = __fadd_rn(s1[0], __shfl_xor(s1[0], 1, 64));
        s2[0] = __fadd_rn(s2[0], __shfl_xor(s2[0], 1, 64));
        if ((pl & 1) == 0) {
            const int i = pl >> 1, cl = 8 * (i >> 2) + 4 * hf + (i & 3);
            s_red[wave][0][cl] = s1[0];
            s_red[wave][1][cl] = s2[0];
        }
        __syncthreads();
        int te = tid;  // (opaque, as the staging's: `tid < 64` is not kept as a lane mask from the kernel's start)
        asm volatile("" : "+v"(te));
        if (te < 2 * NCO) {
            const int st = te >> 5, c = te & 31;
            double sum = 0.0;
            for (int w = 0; w < 4; ++w) sum += (double)s_red[w][st][c];
            pe.part[((int64_t)(cob * NCO + c) * 2 + st) * pe.n_tiles + tile] = sum;
        }
    }
}

// ---------------------------------------------------------------- host
template <typename T>
int up_launch(const UpPlan &pl, const ConvArgs &a, bool pooled, bool stats, const void *w, const int64_t *frame_off,
              double *d_stats, hipStream_t s) {
    T *wp = reinterpret_cast<T *>(const_cast<void *>(a.wp));
    const int64_t wtot = (int64_t)pl.n_cob * (pl.qa + pl.qb) * W_ROWS * Elem<T>::CK;
    hipLaunchKernelGGL(k_pack_w<T>, dim3(grid_for(wtot, SHPL_BLOCK, 4096)), dim3(SHPL_BLOCK), 0, s,
                       reinterpret_cast<const T *>(w), a.c_a, pl.qa, a.c_b, pl.qb, a.c_out, pl.n_cob, 1, wp);
    SHPL_LAUNCH_CHECK();
    if (pooled) {
        hipLaunchKernelGGL(k_row_ptr, dim3(16, a.n_frames), dim3(SHPL_BLOCK), 0, s, a.ent_dst, frame_off, a.h, a.w,
                           const_cast<int32_t *>(a.row_ptr));
        SHPL_LAUNCH_CHECK();
    }
    const bool group = pooled && a.ent_col;  // the pixel-keyed CSR's per-column partials
    using Kernel = void (*)(const ConvArgs);
    const Kernel kernel = by_bools(
        [](auto po, auto st, auto gr) -> Kernel {
            if constexpr (gr() && !po())
                return nullptr;  // no such form: `group` never says so
            else
                return k_upconv3x3<T, po(), st(), gr()>;
        },
        pooled, stats, group);
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
    const int he = piece_elems(dtype);
    ConvArgs a = {};
    a.n_frames = n_frames;
    a.h = (int)h;
    a.w = (int)w;
    a.tiles_x = pl.tiles_x;
    a.tiles_per_frame = pl.tiles_per_frame;
    a.n_tiles = (int)pl.n_tiles;
    a.a = d_a;
    a.a_stride = a_stride;
    a.a_off = a_off;
    a.c_a = (int)c_a;
    a.qa = pl.qa;
    a.b = d_b;
    a.b_stride = b_stride;
    a.b_off = b_off;
    a.c_b = (int)c_b;
    a.qb = pl.qb;
    a.vec_a = vec16(A, he);
    a.vec_b = vec16(B, he);
    a.ent_dst = pooled ? pool->ent_dst : nullptr;
    a.ent_src = pooled ? pool->ent_src : nullptr;
    a.ent_val = pooled ? pool->ent_val : nullptr;
    a.ent_col = pooled ? pool->ent_col : nullptr;
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
    a.vec_out = vec16({d_out, out_stride, 0, c_out}, he);
    hipStream_t s = (hipStream_t)stream;
    return by_dtype(dtype, [&](auto t) {
        return up_launch<typename decltype(t)::T>(pl, a, pooled, stats, d_weights, d_frame_off, d_stats, s);
    });
}
