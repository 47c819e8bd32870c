// shpl_head.hip -- 1x1 heads over [a || pooled b] with the SHPL applied after the projection (MV3D's
// rpn_cls_score / rpn_bbox_pred, MV3D_TF_release/lib/networks/MV3D_voxel_train.py:144-178), forward and backward.
//
// A 1x1 conv and the SHPL are both linear, so the head is applied to the image map before the pooling:
//   Z[p, :]   = b[p, :] . W_b                                   (f32 [rows_b][32], workspace)
//   out[r, :] = a[r, :] . W_a + bias + sum_{k in run(r)} m_k * Z[src_k, :]
// k_head_gemm is a skinny MFMA GEMM (32 rows x 32 padded outputs per wave, K = the channels) that runs once per
// source; over `a` its epilogue walks the cell's run of the cell-keyed CSR (key_range) in CSR order with
// separate multiplies and adds, as walk_run does. The backward multiplies by K = c_out <= 32: plain fused
// multiply-adds at the vector rate (the f32 MFMA's rate) with the small operand in scalar registers, over
// f32 copies of the gradient padded to a multiple of 4 columns so that the pulls and the row loads are whole
// 16-byte pieces. The weight gradient is two-stage: per-row-chunk partials in the workspace, summed in chunk
// order -- no floating-point atomics.
#include "shpl_head.h"

namespace shpl {
namespace head {

constexpr int WGRAD_MIN_ROWS = 64, WGRAD_MAX_CHUNKS = 256;  // the weight gradient's row chunks (its partials)
constexpr int WGRAD_WAVES = 4;  // waves per chunk, a quarter of its rows each

// ---------------------------------------------------------------- weights, packed per lane
// K is walked in steps of SUB * 2 * VEC channels: lane (n = lane % 32, h = lane / 32) holds channels
// step * SUB * 2 * VEC + h * SUB * VEC + j * VEC + i (j < SUB, i < VEC) of its row -- SUB 16-byte loads of 64
// contiguous bytes, the two halves of the wave a whole 128-byte line per row -- and of column n of W. Packed:
// wp[step][j][lane][i], zero past the channels and past c_out. (A sum over K: any assignment of channels to
// MFMA slots serves, as long as both operands use the same.)
template <typename T>
__global__ __launch_bounds__(SHPL_BLOCK) void k_head_pack(const T *__restrict__ w, int64_t w_row0, int64_t c,
                                                          int c_out, T *__restrict__ wp, int64_t n) {
    constexpr int VEC = Vec<T>::N;
    const int64_t t = (int64_t)blockIdx.x * SHPL_BLOCK + threadIdx.x;
    if (t >= n) return;
    const int i = (int)(t % VEC), lane = (int)((t / VEC) % 64), j = (int)((t / (VEC * 64)) % SUB);
    const int64_t step = t / (VEC * 64 * SUB);
    const int64_t k = (step * 2 + (lane >> 5)) * SUB * VEC + j * VEC + i;
    const int col = lane & 31;
    T v = T(0);
    if (k < c && col < c_out) v = w[(w_row0 + k) * c_out + col];
    wp[t] = v;
}

struct GemmArgs {
    Src s[2];
    int64_t rows;
    const float *bias;
    int c_out;
    PoolRef pool;  // the run walk over z [pool.n_src][NP] (key_range NULL: none)
    const float *z;
    void *out;  // to_z: f32 [rows][NP]; else the feature dtype, out_stride elements per row
    int64_t out_stride;
    int to_z;
};

// One wave per 32 rows. ALIGNED: every row of both sources starts on a 16-byte boundary and holds whole K steps.
// The run walk of the epilogue: a lane holds 16 rows of column n; their key ranges are fetched before the K loop,
// and the runs are walked side by side -- round t takes entry t of every row's run (16 independent loads of the
// entry, then of Z) -- so that a row's entries are still added in CSR order, one multiply and one add each, while
// the rows' load latencies overlap instead of queueing up.
template <typename T, bool ALIGNED>
__global__ __launch_bounds__(GEMM_WAVES * 64) void k_head_gemm(GemmArgs a) {
    const int lane = threadIdx.x & 63, n = lane & 31, h = lane >> 5;
    const int64_t row0 = ((int64_t)blockIdx.x * GEMM_WAVES + (threadIdx.x >> 6)) * TILE_ROWS;
    if (row0 >= a.rows) return;
    const int64_t rl = row0 + n < a.rows ? row0 + n : a.rows - 1;  // the row this lane loads (clamped: not stored)
    // acc[i]: row 8 * (i / 4) + 4 * h + i % 4 of the tile, column n
    int32_t first[16], len[16];
    const bool walk = !a.to_z && a.pool.key_range;
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        const int64_t row = row0 + 8 * (i >> 2) + 4 * h + (i & 3);
        first[i] = len[i] = 0;
        if (walk && row < a.rows) {
            int64_t e, end;
            run_of(a.pool, row, e, end);
            first[i] = (int32_t)e;
            len[i] = end > e ? (int32_t)(end - e) : 0;
        }
    }
    f32x16 acc;
#pragma unroll
    for (int i = 0; i < 16; ++i) acc[i] = 0.0f;
    acc = source<T, ALIGNED, false>(a.s[0], rl, lane, acc);
    acc = source<T, ALIGNED, false>(a.s[1], rl, lane, acc);
    const float bias = (a.bias && n < a.c_out) ? a.bias[n] : 0.0f;
    float v[16];
    int32_t longest = 0;
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        v[i] = __fadd_rn(acc[i], bias);
        longest = len[i] > longest ? len[i] : longest;
    }
    for (int32_t t = 0; t < longest; ++t) {
        int64_t src[16];
        float m[16], z[16];
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            src[i] = -1;
            m[i] = 0.0f;
            if (t < len[i]) {
                src[i] = a.pool.ent_src[first[i] + t];
                m[i] = a.pool.ent_val[first[i] + t];
            }
        }
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            src[i] = (src[i] >= 0 && src[i] < a.pool.n_src) ? src[i] : -1;
            z[i] = src[i] >= 0 ? a.z[src[i] * NP + n] : 0.0f;
        }
#pragma unroll
        for (int i = 0; i < 16; ++i)
            if (src[i] >= 0) v[i] = __fadd_rn(v[i], __fmul_rn(m[i], z[i]));
    }
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        const int64_t row = row0 + 8 * (i >> 2) + 4 * h + (i & 3);
        if (row < a.rows) {
            if (a.to_z) {
                reinterpret_cast<float *>(a.out)[row * NP + n] = v[i];
            } else if (n < a.c_out) {
                from_f32(v[i], reinterpret_cast<T *>(a.out) + row * a.out_stride + n);
            }
        }
    }
}

// key_range [n_keys][2] of a CSR that carries none, over zeros: a destination's run is one stretch of equal
// ent_dst (the entries are sorted by destination inside every frame, and frames share no destination).
__global__ __launch_bounds__(SHPL_BLOCK) void k_head_ranges(const int32_t *__restrict__ ent_dst, int64_t nnz_cap,
                                                            int64_t n_keys, int32_t *__restrict__ kr) {
    const int64_t e = (int64_t)blockIdx.x * SHPL_BLOCK + threadIdx.x;
    if (e >= nnz_cap) return;
    const int32_t d = ent_dst[e];
    if (d < 0 || d >= n_keys) return;
    if (e == 0 || ent_dst[e - 1] != d) kr[2 * (int64_t)d] = (int32_t)e;
    if (e == nnz_cap - 1 || ent_dst[e + 1] != d) kr[2 * (int64_t)d + 1] = (int32_t)(e + 1);
}

// ---------------------------------------------------------------- backward
// gp[r][j] = g[r][j] as f32, zero for c_out <= j < CO.
template <typename T>
__global__ __launch_bounds__(SHPL_BLOCK) void k_head_gpad(const T *__restrict__ g, int64_t g_stride, int c_out, int co,
                                                          int64_t n, float *__restrict__ gp) {
    const int64_t t = (int64_t)blockIdx.x * SHPL_BLOCK + threadIdx.x;
    if (t >= n) return;
    const int64_t r = t / co;
    const int j = (int)(t % co);
    gp[t] = j < c_out ? to_f32(g[r * g_stride + j]) : 0.0f;
}

// dx[r][c] = sum_j g[r][j] * W[w_row0 + c][j], j ascending, fused multiply-adds. A thread keeps its COLS
// channels' weights in registers; g's row is the same for the whole wave.
template <typename T, int CO, bool ALIGNED>
__global__ __launch_bounds__(64) void k_head_dgrad(const float *__restrict__ g, int64_t rows, int64_t rows_per,
                                                   const T *__restrict__ w, int64_t w_row0, int64_t c_n, int c_out,
                                                   T *__restrict__ dx, int64_t dx_stride) {
    const int64_t c = ((int64_t)blockIdx.y * 64 + threadIdx.x) * COLS;
    float wr[COLS][CO];
    load_weights<T, CO>(w, w_row0, c, c_n, c_out, wr);
    const int64_t r0 = (int64_t)blockIdx.x * rows_per, r1 = r0 + rows_per < rows ? r0 + rows_per : rows;
    for (int64_t r = r0; r < r1; ++r) {
        float o[COLS];
        project<CO>(g + r * CO, wr, o);
        if (c >= c_n) continue;
        // store_cols, written out: through the helper the unaligned forms took 5 more VGPRs (docs/HISTORY.md §13)
        T ov[COLS];
#pragma unroll
        for (int i = 0; i < COLS; ++i) from_f32(o[i], &ov[i]);
        T *dst = dx + r * dx_stride + c;
        if constexpr (ALIGNED) {
            typedef typename Cols<T>::V V;
            V v;
            __builtin_memcpy(&v, ov, sizeof(V));
            *reinterpret_cast<V *>(dst) = v;
        } else {
#pragma unroll
            for (int i = 0; i < COLS; ++i)
                if (c + i < c_n) dst[i] = ov[i];
        }
    }
}

// Stage 1 of dw[c][j] = sum_r x[r][c] * g[r][j]: row chunk blockIdx.x, a quarter of it per wave (rows ascending,
// fused multiply-adds), the four waves' sums added through LDS in a fixed order ((w0 + w3) + w2) + w1, into
// part[chunk][c][j] ([c_n + 1][CO] per chunk; row c_n: the chunk's sum of g, the bias gradient's partial,
// written when `bias` is set).
template <typename T, int CO, bool ALIGNED>
__global__ __launch_bounds__(WGRAD_WAVES * 64) void k_head_wgrad(const T *__restrict__ x, int64_t x_stride, int64_t x_off,
                                                                 int64_t c_n, const float *__restrict__ g, int64_t rows,
                                                                 int64_t rows_per, int bias, float *__restrict__ part) {
    __shared__ float red[(COLS * CO + 1) * 64];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);  // uniform: g's rows load into scalar registers
    const int64_t c = ((int64_t)blockIdx.y * 64 + lane) * COLS;
    float acc[COLS][CO];
#pragma unroll
    for (int i = 0; i < COLS; ++i)
#pragma unroll
        for (int j = 0; j < CO; ++j) acc[i][j] = 0.0f;
    float bs = 0.0f;
    const bool sum_g = bias && blockIdx.y == 0;
    const int64_t b0 = (int64_t)blockIdx.x * rows_per, b1 = b0 + rows_per < rows ? b0 + rows_per : rows;
    const int64_t quarter = (rows_per + WGRAD_WAVES - 1) / WGRAD_WAVES;
    const int64_t r0 = b0 + wave * quarter, r1 = r0 + quarter < b1 ? r0 + quarter : b1;
    for (int64_t r = r0; r < r1; ++r) {
        const float *gr = g + r * CO;
        const T *xr = x + r * x_stride + x_off + c;
        float xv[COLS];
        load_cols<T, ALIGNED>(xr, c, c_n, xv);
#pragma unroll
        for (int j = 0; j < CO; ++j) {
            const float gj = gr[j];
#pragma unroll
            for (int i = 0; i < COLS; ++i) acc[i][j] = __builtin_fmaf(xv[i], gj, acc[i][j]);
        }
        if (sum_g) bs = __fadd_rn(bs, gr[lane % CO]);
    }
    for (int w = WGRAD_WAVES - 1; w > 0; --w) {
        if (wave == w) {
#pragma unroll
            for (int i = 0; i < COLS; ++i)
#pragma unroll
                for (int j = 0; j < CO; ++j) red[(i * CO + j) * 64 + lane] = acc[i][j];
            red[COLS * CO * 64 + lane] = bs;
        }
        __syncthreads();
        if (wave == 0) {
#pragma unroll
            for (int i = 0; i < COLS; ++i)
#pragma unroll
                for (int j = 0; j < CO; ++j) acc[i][j] = __fadd_rn(acc[i][j], red[(i * CO + j) * 64 + lane]);
            bs = __fadd_rn(bs, red[COLS * CO * 64 + lane]);
        }
        __syncthreads();
    }
    if (wave != 0) return;
    float *p = part + (int64_t)blockIdx.x * (c_n + 1) * CO;
#pragma unroll
    for (int i = 0; i < COLS; ++i) {
        if (c + i >= c_n) continue;
#pragma unroll
        for (int j = 0; j < CO; j += 4)
            *reinterpret_cast<f32x4 *>(p + (c + i) * CO + j) = f32x4{acc[i][j], acc[i][j + 1], acc[i][j + 2], acc[i][j + 3]};
    }
    if (sum_g && lane < CO) p[c_n * CO + lane] = bs;
}

// Stage 2: dw[w_row0 + c][j] = the partials of (c, j) summed in f64 and rounded once; row c_n of the partials is
// the bias gradient (with_bias). A workgroup sums 32 elements: 8 threads per element take every 8th chunk in
// chunk order, and their sums are added in thread order -- a fixed order.
__global__ __launch_bounds__(SHPL_BLOCK) void k_head_wreduce(const float *__restrict__ part, int64_t chunks, int64_t c_n,
                                                             int co, int c_out, int with_bias, float *__restrict__ dw,
                                                             int64_t w_row0, float *__restrict__ dbias) {
    __shared__ double red[8][32];
    const int el = threadIdx.x & 31, sub = threadIdx.x >> 5;
    const int64_t t = (int64_t)blockIdx.x * 32 + el;
    const int64_t n_rows = c_n + (with_bias ? 1 : 0);
    const bool live = t < n_rows * c_out;
    const int64_t c = t / c_out;
    const int j = (int)(t % c_out);
    double s = 0.0;
    if (live)
        for (int64_t k = sub; k < chunks; k += 8) s += (double)part[(k * (c_n + 1) + c) * co + j];
    red[sub][el] = s;
    __syncthreads();
    if (sub != 0 || !live) return;
    s = 0.0;
    for (int k = 0; k < 8; ++k) s += red[k][el];
    if (c < c_n) {
        dw[(w_row0 + c) * c_out + j] = (float)s;
    } else {
        dbias[j] = (float)s;
    }
}

// ---------------------------------------------------------------- host side
struct BwdLayout {
    int co;
    int64_t chunks[2];  // upper bounds of the weight gradient's row chunks per source
    size_t gp, gimg, part[2], bytes;
};
inline BwdLayout bwd_layout(int64_t rows, int64_t c_a, int64_t rows_b, int64_t c_b, int64_t c_out, bool pooled,
                            bool wgrad) {
    BwdLayout l = {};
    l.co = pad_cols(c_out);
    size_t o = 0;
    l.gp = o;
    o = align_up(o + (size_t)rows * l.co * 4, 256);
    l.gimg = o;
    if (pooled) o = align_up(o + (size_t)rows_b * l.co * 4, 256);
    const int64_t rs[2] = {rows, rows_b}, cs[2] = {c_a, c_b};
    for (int s = 0; s < 2; ++s) {
        l.part[s] = o;
        l.chunks[s] = chunking(rs[s], WGRAD_MIN_ROWS, WGRAD_MAX_CHUNKS).chunks_max;
        if (wgrad && cs[s] > 0) o = align_up(o + (size_t)l.chunks[s] * (size_t)(cs[s] + 1) * l.co * 4, 256);
    }
    l.bytes = o;
    return l;
}

// The one published size of the forward's and the input gradient's workspace (shpl_head1x1_workspace_bytes):
// both calls hold the caller to it.
inline size_t ws_need(int dtype, int64_t rows, int64_t c_a, int64_t rows_b, int64_t c_b, int64_t c_out, bool pooled) {
    const size_t f = fwd_layout(dtype, rows, c_a, rows_b, c_b, pooled, true).bytes;
    const size_t b = bwd_layout(rows, c_a, rows_b, c_b, c_out, pooled, false).bytes;
    return f > b ? f : b;
}

int launch_pack(int dtype, const void *d_weights, int64_t w_row0, int64_t c, int64_t c_out, void *wp, hipStream_t s) {
    const int64_t vec = 16 / esize(dtype), n = pack_steps(c, (int)vec) * SUB * 64 * vec;
    if (n == 0) return SHPL_OK;
    by_dtype(dtype, [&](auto tt) {
        typedef typename decltype(tt)::T T;
        hipLaunchKernelGGL(k_head_pack<T>, dim3(blocks_for(n, SHPL_BLOCK)), dim3(SHPL_BLOCK), 0, s,
                           reinterpret_cast<const T *>(d_weights), w_row0, c, (int)c_out, reinterpret_cast<T *>(wp), n);
        return SHPL_OK;
    });
    SHPL_LAUNCH_CHECK();
    return SHPL_OK;
}

int launch_ranges(const shpl_csr *csr, int64_t n_keys, int32_t *kr, hipStream_t s) {
    SHPL_HIP_CHECK(zero_fill(kr, align_up((size_t)n_keys * 8, 16), s));
    if (csr->nnz_cap > 0) {
        hipLaunchKernelGGL(k_head_ranges, dim3(blocks_for(csr->nnz_cap, SHPL_BLOCK)), dim3(SHPL_BLOCK), 0, s,
                           csr->ent_dst, csr->nnz_cap, n_keys, kr);
        SHPL_LAUNCH_CHECK();
    }
    return SHPL_OK;
}

int launch_wreduce(const float *part, int64_t chunks, int64_t c_n, int co, int64_t c_out, bool with_bias, float *dw,
                   int64_t w_row0, float *dbias, hipStream_t s) {
    const int64_t n = (c_n + (with_bias ? 1 : 0)) * c_out;
    hipLaunchKernelGGL(k_head_wreduce, dim3(blocks_for(n, 32)), dim3(SHPL_BLOCK), 0, s, part, chunks, c_n, co,
                       (int)c_out, (int)with_bias, dw, w_row0, dbias);
    SHPL_LAUNCH_CHECK();
    return SHPL_OK;
}

// g (feature dtype) -> gp f32 [rows][co]
int launch_gpad(int dtype, const void *d_gy, int64_t gy_stride, int64_t c_out, int co, int64_t rows, float *gp,
                hipStream_t s) {
    const int64_t n = rows * co;
    if (n == 0) return SHPL_OK;
    by_dtype(dtype, [&](auto tt) {
        typedef typename decltype(tt)::T T;
        hipLaunchKernelGGL(k_head_gpad<T>, dim3(blocks_for(n, SHPL_BLOCK)), dim3(SHPL_BLOCK), 0, s,
                           reinterpret_cast<const T *>(d_gy), gy_stride, (int)c_out, co, n, gp);
        return SHPL_OK;
    });
    SHPL_LAUNCH_CHECK();
    return SHPL_OK;
}

// the gradient pulled back to the pixels: _sparse_pool_trans_op(M, g) at co channels, f32
int pull_to_pixels(const shpl_csr *pool_grad, const float *gp, int co, float *gimg, hipStream_t s) {
    return shpl_pull(SHPL_BY_PIXEL, SHPL_F32, pool_grad, gp, co, 0, co, nullptr, 0, 0, 0, SHPL_OUT_POOL, gimg, co, s);
}

}  // namespace head
}  // namespace shpl

using namespace shpl;
using namespace shpl::head;

extern "C" int shpl_head1x1_workspace_bytes(int dtype, int64_t rows, int64_t c_a, int64_t rows_b, int64_t c_b,
                                            int64_t c_out, int pooled, size_t *bytes) {
    if (!bytes) return SHPL_ERR_ARG;
    const int rc = check_shape(dtype, rows, c_a, rows_b, c_b, c_out);
    if (rc != SHPL_OK) return rc;
    *bytes = ws_need(dtype, rows, c_a, rows_b, c_b, c_out, pooled != 0);
    return SHPL_OK;
}

extern "C" int shpl_head1x1_wgrad_workspace_bytes(int dtype, int64_t rows, int64_t c_a, int64_t rows_b, int64_t c_b,
                                                  int64_t c_out, int pooled, size_t *bytes) {
    if (!bytes) return SHPL_ERR_ARG;
    const int rc = check_shape(dtype, rows, c_a, rows_b, c_b, c_out);
    if (rc != SHPL_OK) return rc;
    *bytes = bwd_layout(rows, c_a, rows_b, c_b, c_out, pooled != 0, true).bytes;
    return SHPL_OK;
}

extern "C" int shpl_head1x1(int dtype, int64_t rows, const void *d_a, int64_t a_stride, int64_t a_off, int64_t c_a,
                            const void *d_b, int64_t b_stride, int64_t b_off, int64_t c_b, int64_t rows_b,
                            const shpl_csr *pool, const void *d_weights, int64_t c_out, const float *d_bias,
                            void *d_out, int64_t out_stride, void *d_ws, size_t ws_bytes, void *stream) {
    const bool pooled = pool != nullptr;
    int rc = check_sources(dtype, rows, d_a, a_stride, a_off, c_a, d_b, b_stride, b_off, c_b, rows_b, pool, false,
                           d_weights, d_out, c_out, out_stride, true, d_ws, ws_bytes,
                           [&] { return ws_need(dtype, rows, c_a, rows_b, c_b, c_out, pooled); });
    if (rc != SHPL_OK || rows == 0) return rc;
    const FwdLayout l = fwd_layout(dtype, rows, c_a, rows_b, c_b, pooled, true);
    hipStream_t s = (hipStream_t)stream;
    char *ws = reinterpret_cast<char *>(d_ws);
    const int64_t esz = esize(dtype), vec = 16 / esz;
    const int64_t cs[2] = {c_a, c_b};

    // the weights of both sources, packed per lane
    for (int k = 0; k < 2; ++k)
        if ((rc = launch_pack(dtype, d_weights, k == 0 ? (int64_t)0 : c_a, cs[k], c_out, ws + l.wp[k], s)) != SHPL_OK)
            return rc;
    auto gemm = [&](const GemmArgs &g, bool al) {
        const unsigned grid = blocks_for(g.rows, (int64_t)TILE_ROWS * GEMM_WAVES);
        by_dtype(dtype, [&](auto tt) {
            typedef typename decltype(tt)::T T;
            by_bools([&](auto al_) {
                hipLaunchKernelGGL((k_head_gemm<T, decltype(al_)::value>), dim3(grid), dim3(GEMM_WAVES * 64), 0, s, g);
            }, al);
            return SHPL_OK;
        });
    };
    const bool al_a = c_a % (SUB * 2 * vec) == 0 && rows_aligned(d_a, a_stride, a_off, c_a, vec, esz);
    const bool al_b = c_b == 0 || (c_b % (SUB * 2 * vec) == 0 && rows_aligned(d_b, b_stride, b_off, c_b, vec, esz));
    GemmArgs g = {};
    g.c_out = (int)c_out;
    if (pooled) {
        // Z = b . W_b, no bias
        g.s[0] = Src{d_b, b_stride, b_off, c_b, ws + l.wp[1]};
        g.rows = rows_b;
        g.out = ws + l.z;
        g.to_z = 1;
        if (rows_b > 0) {
            gemm(g, al_b);
            SHPL_LAUNCH_CHECK();
        }
        g = GemmArgs{};
        g.c_out = (int)c_out;
        g.s[0] = Src{d_a, a_stride, a_off, c_a, ws + l.wp[0]};
        if ((rc = pool_ref(pool, rows, rows_b, reinterpret_cast<int32_t *>(ws + l.kr), s, &g.pool)) != SHPL_OK) return rc;
        g.z = reinterpret_cast<const float *>(ws + l.z);
    } else {
        g.s[0] = Src{d_a, a_stride, a_off, c_a, ws + l.wp[0]};
        g.s[1] = Src{d_b, b_stride, b_off, c_b, ws + l.wp[1]};
    }
    g.rows = rows;
    g.bias = d_bias;
    g.out = d_out;
    g.out_stride = out_stride;
    gemm(g, al_a && (pooled || al_b));
    SHPL_LAUNCH_CHECK();
    return SHPL_OK;
}

extern "C" int shpl_head1x1_dgrad(int dtype, int64_t rows, const void *d_gy, int64_t gy_stride, int64_t c_out,
                                  const void *d_weights, int64_t c_a, int64_t c_b, void *d_da, int64_t da_stride,
                                  void *d_db, int64_t db_stride, int64_t rows_b, const shpl_csr *pool_grad,
                                  void *d_ws, size_t ws_bytes, void *stream) {
    const bool pooled = pool_grad != nullptr;
    int rc = check_dgrad(dtype, rows, d_gy, gy_stride, c_out, d_weights, c_a, c_b, d_da, da_stride, d_db, db_stride,
                         rows_b, pool_grad, true, d_ws, ws_bytes,
                         [&] { return ws_need(dtype, rows, c_a, rows_b, c_b, c_out, pooled); });
    if (rc != SHPL_OK || rows == 0) return rc;
    const BwdLayout l = bwd_layout(rows, c_a, rows_b, c_b, c_out, pooled, false);
    hipStream_t s = (hipStream_t)stream;
    char *ws = reinterpret_cast<char *>(d_ws);
    float *gp = reinterpret_cast<float *>(ws + l.gp), *gimg = reinterpret_cast<float *>(ws + l.gimg);
    if ((rc = launch_gpad(dtype, d_gy, gy_stride, c_out, l.co, rows, gp, s)) != SHPL_OK) return rc;
    const int64_t esz = esize(dtype);
    auto run = [&](const float *g, int64_t n_rows, int64_t w_row0, int64_t c_n, void *dx, int64_t dx_stride) {
        if (n_rows == 0) return;
        const bool al = rows_aligned(dx, dx_stride, 0, c_n, COLS, esz);
        const dim3 grid(blocks_for(n_rows, DGRAD_ROWS), blocks_for(c_n, 64 * COLS));
        by_dtype(dtype, [&](auto tt) {
            typedef typename decltype(tt)::T T;
            return by_cols(l.co, [&](auto cc) {
                constexpr int CO = decltype(cc)::value;
                by_bools([&](auto al_) {
                    hipLaunchKernelGGL((k_head_dgrad<T, CO, decltype(al_)::value>), grid, dim3(64), 0, s, g, n_rows,
                                       (int64_t)DGRAD_ROWS, reinterpret_cast<const T *>(d_weights), w_row0, c_n,
                                       (int)c_out, reinterpret_cast<T *>(dx), dx_stride);
                }, al);
                return SHPL_OK;
            });
        });
    };
    if (d_da) {
        run(gp, rows, 0, c_a, d_da, da_stride);
        SHPL_LAUNCH_CHECK();
    }
    if (d_db) {
        const float *g = gp;
        if (pooled) {
            if (rows_b > 0 && (rc = pull_to_pixels(pool_grad, gp, l.co, gimg, s)) != SHPL_OK) return rc;
            g = gimg;
        }
        run(g, pooled ? rows_b : rows, c_a, c_b, d_db, db_stride);
        SHPL_LAUNCH_CHECK();
    }
    return SHPL_OK;
}

extern "C" int shpl_head1x1_wgrad(int dtype, int64_t rows, const void *d_a, int64_t a_stride, int64_t a_off,
                                  int64_t c_a, const void *d_b, int64_t b_stride, int64_t b_off, int64_t c_b,
                                  int64_t rows_b, const shpl_csr *pool_grad, const void *d_gy, int64_t gy_stride,
                                  int64_t c_out, float *d_dw, float *d_dbias, void *d_ws, size_t ws_bytes,
                                  void *stream) {
    const bool pooled = pool_grad != nullptr;
    int rc = check_sources(dtype, rows, d_a, a_stride, a_off, c_a, d_b, b_stride, b_off, c_b, rows_b, pool_grad, true,
                           d_gy, d_dw, c_out, gy_stride, true, d_ws, ws_bytes,
                           [&] { return bwd_layout(rows, c_a, rows_b, c_b, c_out, pooled, true).bytes; });
    if (rc != SHPL_OK) return rc;
    const BwdLayout l = bwd_layout(rows, c_a, rows_b, c_b, c_out, pooled, true);
    hipStream_t s = (hipStream_t)stream;
    char *ws = reinterpret_cast<char *>(d_ws);
    float *gp = reinterpret_cast<float *>(ws + l.gp), *gimg = reinterpret_cast<float *>(ws + l.gimg);
    if ((rc = launch_gpad(dtype, d_gy, gy_stride, c_out, l.co, rows, gp, s)) != SHPL_OK) return rc;
    if (pooled && rows > 0 && rows_b > 0 && (rc = pull_to_pixels(pool_grad, gp, l.co, gimg, s)) != SHPL_OK) return rc;
    const int64_t esz = esize(dtype);
    // one source: its partials, then their sum into rows [w_row0, w_row0 + c_n) of dw (and the bias gradient)
    auto run = [&](int k, const void *x, int64_t x_stride, int64_t x_off, int64_t c_n, const float *g, int64_t n_rows,
                   int64_t w_row0, bool bias) {
        float *part = reinterpret_cast<float *>(ws + l.part[k]);
        const Chunking ch = chunking(n_rows, WGRAD_MIN_ROWS, WGRAD_MAX_CHUNKS);  // 0 rows: no partial, zeros
        if (ch.chunks > 0) {
            const bool al = rows_aligned(x, x_stride, x_off, c_n, COLS, esz);
            const dim3 grid((unsigned)ch.chunks, blocks_for(c_n, 64 * COLS));
            by_dtype(dtype, [&](auto tt) {
                typedef typename decltype(tt)::T T;
                return by_cols(l.co, [&](auto cc) {
                    constexpr int CO = decltype(cc)::value;
                    by_bools([&](auto al_) {
                        hipLaunchKernelGGL((k_head_wgrad<T, CO, decltype(al_)::value>), grid, dim3(WGRAD_WAVES * 64), 0,
                                           s, reinterpret_cast<const T *>(x), x_stride, x_off, c_n, g, n_rows, ch.per,
                                           (int)bias, part);
                    }, al);
                    return SHPL_OK;
                });
            });
        }
        launch_wreduce(part, ch.chunks, c_n, l.co, c_out, bias, d_dw, w_row0, d_dbias, s);
    };
    run(0, d_a, a_stride, a_off, c_a, gp, rows, 0, d_dbias != nullptr);
    SHPL_LAUNCH_CHECK();
    if (c_b > 0) {
        run(1, d_b, b_stride, b_off, c_b, pooled ? gimg : gp, pooled ? rows_b : rows, c_a, false);
        SHPL_LAUNCH_CHECK();
    }
    return SHPL_OK;
}
