// shpl_head_drop.hip -- the 1x1 heads of shpl_head.hip under dropout over [a || pooled b] (MV3D's training step:
// MV3D_TF_release/lib/networks/MV3D_voxel_train.py:148-178 with use_dropout, keep_prob 0.5), forward and backward.
//
// A mask over the concat sits between the pooling and the projection, so the heads cannot be applied before the
// pooling as shpl_head.hip does. The pooling moves into the GEMM's operand staging instead: a lane walks its
// cell's run of the cell-keyed CSR per K step and sums its 64-byte slice of the image rows in f32 registers
// (shpl_pull's arithmetic: CSR order, one multiply and one add per entry), rounds the sums to the feature dtype
// -- the elements of the materialised bv_fused, bit for bit -- zeroes the dropped ones and issues the MFMAs.
// Neither the pooled map, the concat nor a mask reaches memory. The mask is a pure function of (seed, row,
// channel, keep_prob) -- Philox4x32-10, include/shpl.h states it -- and the backward computes it again.
#include "shpl_head.h"

namespace shpl {
namespace head_drop {

using namespace shpl::head;

constexpr int WG_WAVES = 8;        // waves per row chunk of the weight gradient
constexpr int WG_BATCH = 32;       // rows of gy a wave stages in LDS at a time
constexpr int WG_MIN_ROWS = 64, WG_MAX_CHUNKS = 64;  // its row chunks: the partials stay far below the maps' size

// ---------------------------------------------------------------- the mask
struct Mask {
    uint32_t k0, k1;  // the seed's halves: Philox's key
    uint32_t thr;     // kept iff the element's 16 bits < thr (1 .. 65536)
    float scale;      // 65536 / thr
};

// Random123's Philox4x32-10.
__device__ __forceinline__ void philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0,
                                              uint32_t k1, uint32_t (&w)[4]) {
#pragma unroll
    for (int round = 0; round < 10; ++round) {
        const uint32_t hi0 = __umulhi(0xD2511F53u, c0), lo0 = 0xD2511F53u * c0;
        const uint32_t hi1 = __umulhi(0xCD9E8D57u, c2), lo1 = 0xCD9E8D57u * c2;
        c0 = hi1 ^ c1 ^ k0;
        c1 = lo1;
        c2 = hi0 ^ c3 ^ k1;
        c3 = lo0;
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
    w[0] = c0;
    w[1] = c1;
    w[2] = c2;
    w[3] = c3;
}

// bit j: channel 8 g + j of row r is kept
__device__ __forceinline__ uint32_t keep8(const Mask &m, int64_t r, uint32_t g) {
    uint32_t w[4];
    philox4x32_10((uint32_t)r, (uint32_t)((uint64_t)r >> 32), g, 0u, m.k0, m.k1, w);
    uint32_t bits = 0;
#pragma unroll
    for (int j = 0; j < 8; ++j) bits |= (uint32_t)(((w[j >> 1] >> (16 * (j & 1))) & 0xffffu) < m.thr) << j;
    return bits;
}

// bit i: channel c0 + i of row r is kept, i < NCH <= 32. One Philox call per group of 8 channels the span touches.
template <int NCH>
__device__ __forceinline__ uint32_t keep_bits(const Mask &m, int64_t r, int64_t c0) {
    constexpr int G = (NCH + 7) / 8;
    const uint32_t g0 = (uint32_t)(c0 >> 3);
    const int sh = (int)(c0 & 7);
    uint64_t bits = 0;
#pragma unroll
    for (int q = 0; q < G; ++q) bits |= (uint64_t)keep8(m, r, g0 + q) << (8 * q);
    if (sh + NCH > 8 * G) bits |= (uint64_t)keep8(m, r, g0 + G) << (8 * G);
    return (uint32_t)(bits >> sh);
}

// The backward kernels' form: a lane's COLS = 4 channels [c0, c0 + 4), c0 = off + 4 * lane, of two rows ra and rb
// (wave-uniform; every lane of the wave calls). paired (off % 8 == 0): lanes 2q and 2q + 1 hold the two halves of
// one group of 8, so the even lane computes ra's group, the odd lane rb's, and they exchange the 8 bits -- one
// Philox call per lane for the two rows instead of two.
__device__ __forceinline__ void keep4_two(const Mask &m, int64_t ra, int64_t rb, int64_t c0, bool paired, uint32_t &ba,
                                          uint32_t &bb) {
    if (!paired) {
        ba = keep_bits<COLS>(m, ra, c0);
        bb = keep_bits<COLS>(m, rb, c0);
        return;
    }
    const bool odd = threadIdx.x & 1;
    const uint32_t mine = keep8(m, odd ? rb : ra, (uint32_t)(c0 >> 3));
    const uint32_t theirs = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)mine, 0xB1, 0xF, 0xF, true);  // lane ^ 1
    ba = odd ? (theirs >> 4) & 0xFu : mine & 0xFu;
    bb = odd ? (mine >> 4) & 0xFu : theirs & 0xFu;
}

// mask[r][c] as bytes: a thread per (row, group of 8 channels)
__global__ __launch_bounds__(SHPL_BLOCK) void k_dropout_mask(int64_t rows, int64_t c, int64_t groups, Mask m,
                                                             uint8_t *__restrict__ mask) {
    const int64_t t = (int64_t)blockIdx.x * SHPL_BLOCK + threadIdx.x;
    if (t >= rows * groups) return;
    const int64_t r = t / groups, g = t % groups;
    const uint32_t bits = keep8(m, r, (uint32_t)g);
#pragma unroll
    for (int j = 0; j < 8; ++j)
        if (8 * g + j < c) mask[r * c + 8 * g + j] = (uint8_t)((bits >> j) & 1u);
}

// ---------------------------------------------------------------- forward
struct MaskedSrc : Src {
    int64_t moff;  // the source's first channel in the concat: the mask's channel index
};

struct FwdArgs {
    MaskedSrc s[2];
    int64_t rows;
    const float *bias;
    int c_out;
    PoolRef pool;  // the pooled form (key_range NULL: s[1] is a dense map, or none)
    void *out;
    int64_t out_stride;
    Mask m;
};

// source<DROP>'s step (shpl_head.h): zero the dropped ones of the lane's SUB pieces, channels [c0, c0 + SUB * VEC) of
// row r of the concat
template <typename T>
__device__ __forceinline__ void drop_step(T (&xv)[SUB][Vec<T>::N], const Mask &m, int64_t r, int64_t c0) {
    constexpr int VEC = Vec<T>::N;
    const uint32_t bits = keep_bits<SUB * VEC>(m, r, c0);
#pragma unroll
    for (int j = 0; j < SUB; ++j)
#pragma unroll
        for (int i = 0; i < VEC; ++i)
            if (!((bits >> (j * VEC + i)) & 1u)) xv[j][i] = T(0);
}

// acc += the kept elements of the pooled row of cell rl times the second source's packed weights. K step outer,
// run inner: per step the lane sums its slice of the run's image rows (entries [first, first + len) of the
// cell-keyed CSR, in that order, from zero, one multiply and one add each), rounds once to T, masks, multiplies.
// The run's index words are read again per step: hits in the L1 / L2.
template <typename T, bool ALIGNED>
__device__ __forceinline__ f32x16 pooled_source(const FwdArgs &a, int64_t rl, int32_t first, int32_t len, int lane,
                                                f32x16 acc) {
    constexpr int VEC = Vec<T>::N, NCH = SUB * VEC;
    const MaskedSrc &src = a.s[1];
    const int64_t c = src.c;
    const int h = lane >> 5;
    const T *xb = reinterpret_cast<const T *>(src.x) + src.off + h * NCH;
    const T *wp = reinterpret_cast<const T *>(src.wp) + lane * VEC;
    const int64_t steps = (c + 2 * NCH - 1) / (2 * NCH);
    for (int64_t st = 0; st < steps; ++st) {
        const int64_t k = st * 2 * NCH;
        T wv[SUB][VEC];
#pragma unroll
        for (int j = 0; j < SUB; ++j) {
            const u32x4 wq = *reinterpret_cast<const u32x4 *>(wp + (st * SUB + j) * 64 * VEC);
            __builtin_memcpy(wv[j], &wq, 16);
        }
        float sum[SUB][VEC];
#pragma unroll
        for (int j = 0; j < SUB; ++j)
#pragma unroll
            for (int i = 0; i < VEC; ++i) sum[j][i] = 0.0f;
        for (int32_t t = 0; t < len; ++t) {
            const int64_t p = a.pool.ent_src[first + t];
            const float mv = a.pool.ent_val[first + t];
            if (p < 0 || p >= a.pool.n_src) continue;  // a malformed map addresses nothing outside b
            T xv[SUB][VEC];
#pragma unroll
            for (int j = 0; j < SUB; ++j)
                load_piece<T, ALIGNED>(xb + p * src.stride + k + j * VEC, k + h * NCH + j * VEC, c, xv[j]);
#pragma unroll
            for (int j = 0; j < SUB; ++j)
#pragma unroll
                for (int i = 0; i < VEC; ++i) sum[j][i] = __fadd_rn(sum[j][i], __fmul_rn(mv, to_f32(xv[j][i])));
        }
        T xq[SUB][VEC];
#pragma unroll
        for (int j = 0; j < SUB; ++j)
#pragma unroll
            for (int i = 0; i < VEC; ++i) from_f32(sum[j][i], &xq[j][i]);
        drop_step(xq, a.m, rl, src.moff + k + h * NCH);
#pragma unroll
        for (int j = 0; j < SUB; ++j) acc = mma(xq[j], wv[j], acc);
    }
    return acc;
}

// One wave per 32 rows, as k_head_gemm. ALIGNED: every row of both sources starts on a 16-byte boundary and
// holds whole K steps. A tile whose 32 cells are all empty skips the pooled source.
template <typename T, bool ALIGNED>
__global__ __launch_bounds__(GEMM_WAVES * 64) void k_head_drop_gemm(FwdArgs a) {
    const int lane = threadIdx.x & 63, n = lane & 31, h = lane >> 5;
    const int64_t row0 = ((int64_t)blockIdx.x * GEMM_WAVES + (threadIdx.x >> 6)) * TILE_ROWS;
    if (row0 >= a.rows) return;
    const int64_t rl = row0 + n < a.rows ? row0 + n : a.rows - 1;  // the row this lane loads (clamped: not stored)
    f32x16 acc;
#pragma unroll
    for (int i = 0; i < 16; ++i) acc[i] = 0.0f;
    acc = source<T, ALIGNED, true>(a.s[0], rl, lane, acc, a.m, a.s[0].moff);
    if (a.pool.key_range) {
        int64_t e, end;
        run_of(a.pool, rl, e, end);
        const int32_t len = (end > e && row0 + n < a.rows) ? (int32_t)(end - e) : 0;
        if (__ballot(len > 0) != 0) acc = pooled_source<T, ALIGNED>(a, rl, (int32_t)e, len, lane, acc);
    } else {
        acc = source<T, ALIGNED, true>(a.s[1], rl, lane, acc, a.m, a.s[1].moff);
    }
    const float bias = (a.bias && n < a.c_out) ? a.bias[n] : 0.0f;
    // acc[i]: row 8 * (i / 4) + 4 * h + i % 4 of the tile, column n
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        const int64_t row = row0 + 8 * (i >> 2) + 4 * h + (i & 3);
        if (row < a.rows && n < a.c_out)
            from_f32(__fadd_rn(__fmul_rn(acc[i], a.m.scale), bias), reinterpret_cast<T *>(a.out) + row * a.out_stride + n);
    }
}

// ---------------------------------------------------------------- backward
// dx[r][c] = keep(r, w_row0 + c) * scale * sum_j g[r][j] * W[w_row0 + c][j] over a dense map's rows: k_head_dgrad
// with the mask at the store (a dropped element is exactly 0).
template <typename T, int CO, bool ALIGNED>
__global__ __launch_bounds__(64) void k_head_drop_dgrad(const float *__restrict__ g, int64_t rows, int64_t rows_per,
                                                        const T *__restrict__ w, int64_t w_row0, int64_t c_n, int c_out,
                                                        T *__restrict__ dx, int64_t dx_stride, Mask m) {
    const int64_t c = ((int64_t)blockIdx.y * 64 + threadIdx.x) * COLS;
    float wr[COLS][CO];
    load_weights<T, CO>(w, w_row0, c, c_n, c_out, wr);
    const int64_t r0 = (int64_t)blockIdx.x * rows_per, r1 = r0 + rows_per < rows ? r0 + rows_per : rows;
    const bool paired = (w_row0 & 7) == 0;
    for (int64_t r = r0; r < r1; r += 2) {  // two rows per trip: one mask computation for both
        const int64_t rb = r + 1 < r1 ? r + 1 : r;
        float oa[COLS], ob[COLS];
        project<CO>(g + r * CO, wr, oa);
        project<CO>(g + rb * CO, wr, ob);
        uint32_t ba, bb;
        keep4_two(m, r, rb, w_row0 + c, paired, ba, bb);
#pragma unroll
        for (int i = 0; i < COLS; ++i) {
            oa[i] = ((ba >> i) & 1u) ? __fmul_rn(oa[i], m.scale) : 0.0f;
            ob[i] = ((bb >> i) & 1u) ? __fmul_rn(ob[i], m.scale) : 0.0f;
        }
        store_cols<T, ALIGNED>(dx + r * dx_stride + c, c, c_n, oa);
        if (rb != r) store_cols<T, ALIGNED>(dx + rb * dx_stride + c, c, c_n, ob);
    }
}

// The pooled source's gradient: dx[p][c] = sum over the entries (cell r, m) of pixel p's run of the pixel-keyed
// CSR, in CSR order from zero, of m * (keep(r, w_row0 + c) * scale * sum_j g[r][j] * W[w_row0 + c][j]) -- one
// multiply by scale, one by m and one add per kept entry; a dropped one adds nothing. A wave shares its pixel,
// so the run and g's rows load once for the wave.
template <typename T, int CO, bool ALIGNED>
__global__ __launch_bounds__(64) void k_head_drop_dgrad_pool(const float *__restrict__ g, PoolRef pool, int64_t pix,
                                                             int64_t pix_per, const T *__restrict__ w, int64_t w_row0,
                                                             int64_t c_n, int c_out, T *__restrict__ dx,
                                                             int64_t dx_stride, Mask m) {
    const int64_t c = ((int64_t)blockIdx.y * 64 + threadIdx.x) * COLS;
    float wr[COLS][CO];
    load_weights<T, CO>(w, w_row0, c, c_n, c_out, wr);
    const int64_t p0 = (int64_t)blockIdx.x * pix_per, p1 = p0 + pix_per < pix ? p0 + pix_per : pix;
    const bool paired = (w_row0 & 7) == 0;
    // lane i holds the run of pixel p0 + i (pix_per <= 64): one round trip for all of them
    int64_t e0 = 0, e1 = 0;
    if (p0 + (int64_t)threadIdx.x < p1) run_of(pool, p0 + threadIdx.x, e0, e1);
    for (int64_t p = p0; p < p1; ++p) {
        int32_t e = __builtin_amdgcn_readlane((int32_t)e0, (int)(p - p0));
        const int32_t end = __builtin_amdgcn_readlane((int32_t)e1, (int)(p - p0));
        float s[COLS];
#pragma unroll
        for (int i = 0; i < COLS; ++i) s[i] = 0.0f;
        for (; e < end; e += 2) {  // two entries per trip, added in CSR order: their loads overlap, one mask computation
            const int32_t eb = e + 1 < end ? e + 1 : e;
            int64_t ra = pool.ent_src[e], rb = pool.ent_src[eb];
            const float ma = pool.ent_val[e], mb = pool.ent_val[eb];
            const bool oka = ra >= 0 && ra < pool.n_src, okb = eb != e && rb >= 0 && rb < pool.n_src;
            ra = oka ? ra : 0;  // a malformed map addresses nothing outside g (the kernel runs only over n_src > 0)
            rb = okb ? rb : 0;
            float oa[COLS], ob[COLS];
            project<CO>(g + ra * CO, wr, oa);
            project<CO>(g + rb * CO, wr, ob);
            uint32_t ba, bb;
            keep4_two(m, ra, rb, w_row0 + c, paired, ba, bb);
#pragma unroll
            for (int i = 0; i < COLS; ++i) {
                if (oka && ((ba >> i) & 1u)) s[i] = __fadd_rn(s[i], __fmul_rn(ma, __fmul_rn(oa[i], m.scale)));
                if (okb && ((bb >> i) & 1u)) s[i] = __fadd_rn(s[i], __fmul_rn(mb, __fmul_rn(ob[i], m.scale)));
            }
        }
        store_cols<T, ALIGNED>(dx + p * dx_stride + c, c, c_n, s);
    }
}

struct WgradArgs {
    const void *x;  // the source: a dense map of `rows` rows, or (POOLED) the image map the runs name
    int64_t x_stride, x_off, c_n, moff;
    PoolRef pool;
    const void *gy;
    int64_t gy_stride;
    int c_out;
    int64_t rows, rows_per;
    int bias;
    float *part;
    Mask m;
};

// Stage 1 of dw[c][j] = scale * sum_r keep(r, moff + c) * x[r][c] * gy[r][j]: row chunk blockIdx.x, an eighth of it
// per wave (rows ascending, fused multiply-adds), the waves' sums added through LDS in a fixed order, times
// scale, into part[chunk][c][j] ([c_n + 1][CO] per chunk; row c_n: the chunk's sum of gy, unscaled, when `bias`
// is set). x[r][c] of the POOLED source is the forward's operand: the run sum of cell r rounded to T. gy's rows
// are staged in LDS as f32, WG_BATCH per wave at a time (no padded copy in the workspace).
template <typename T, int CO, bool ALIGNED, bool POOLED>
__global__ __launch_bounds__(WG_WAVES * 64) void k_head_drop_wgrad(WgradArgs a) {
    constexpr int WG_ROWS = CO > 28 ? 2 : 4;  // rows taken side by side: what the registers hold without spilling
    constexpr int GS = WG_WAVES * WG_BATCH * CO, KR = WG_WAVES * WG_BATCH * 2, RED = (COLS * CO + 1) * 64;
    __shared__ float lds[GS + KR > RED ? GS + KR : RED];  // gy's rows and the runs, then the waves' sums
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int64_t c = ((int64_t)blockIdx.y * 64 + lane) * COLS;
    const T *x = reinterpret_cast<const T *>(a.x) + a.x_off + c;
    const T *gy = reinterpret_cast<const T *>(a.gy);
    float acc[COLS][CO];
#pragma unroll
    for (int i = 0; i < COLS; ++i)
#pragma unroll
        for (int j = 0; j < CO; ++j) acc[i][j] = 0.0f;
    float bs = 0.0f;
    const bool sum_g = a.bias && blockIdx.y == 0;
    const bool paired = (a.moff & 7) == 0;
    const int64_t b0 = (int64_t)blockIdx.x * a.rows_per, b1 = b0 + a.rows_per < a.rows ? b0 + a.rows_per : a.rows;
    const int64_t share = (a.rows_per + WG_WAVES - 1) / WG_WAVES;
    const int64_t r0 = b0 + wave * share, r1 = r0 + share < b1 ? r0 + share : b1;
    float *gs = lds + wave * WG_BATCH * CO;
    int32_t *krs = reinterpret_cast<int32_t *>(lds + GS) + wave * WG_BATCH * 2;  // (first entry, entries) per row
    for (int64_t rb = 0; rb < share; rb += WG_BATCH) {  // the same trips in every wave: the barriers are uniform
        __syncthreads();
        for (int idx = lane; idx < WG_BATCH * CO; idx += 64) {
            const int64_t r = r0 + rb + idx / CO;
            const int j = idx % CO;
            gs[idx] = (r < r1 && j < a.c_out) ? to_f32(gy[r * a.gy_stride + j]) : 0.0f;
        }
        if (POOLED && lane < WG_BATCH) {
            int64_t e = 0, end = 0;
            if (r0 + rb + lane < r1) run_of(a.pool, r0 + rb + lane, e, end);
            krs[2 * lane] = (int32_t)e;
            krs[2 * lane + 1] = end > e ? (int32_t)(end - e) : 0;
        }
        __syncthreads();
        // WG_ROWS rows side by side: their loads (and the entries of their runs, round t taking entry t of every
        // row's run) are in flight together; every row's run is still summed in CSR order
        for (int rr = 0; rr < WG_BATCH; rr += WG_ROWS) {
            const int64_t rg = r0 + rb + rr;
            if (rg >= r1) break;
            float xv[WG_ROWS][COLS];
            if constexpr (POOLED) {
                int32_t first[WG_ROWS], len[WG_ROWS], longest = 0;
#pragma unroll
                for (int u = 0; u < WG_ROWS; ++u) {
                    first[u] = krs[2 * (rr + u)];
                    len[u] = krs[2 * (rr + u) + 1];
                    longest = len[u] > longest ? len[u] : longest;
                }
                float s[WG_ROWS][COLS];
#pragma unroll
                for (int u = 0; u < WG_ROWS; ++u)
#pragma unroll
                    for (int i = 0; i < COLS; ++i) s[u][i] = 0.0f;
                for (int32_t t = 0; t < longest; ++t) {
                    float v[WG_ROWS][COLS], mv[WG_ROWS];
                    bool ok[WG_ROWS];
#pragma unroll
                    for (int u = 0; u < WG_ROWS; ++u) {  // unconditional loads (slot 0, pixel 0 when there is none)
                        ok[u] = t < len[u];
                        const int32_t e = ok[u] ? first[u] + t : 0;
                        int64_t p = a.pool.ent_src[e];
                        mv[u] = a.pool.ent_val[e];
                        ok[u] = ok[u] && p >= 0 && p < a.pool.n_src;
                        p = ok[u] ? p : 0;
                        load_cols<T, ALIGNED>(x + p * a.x_stride, c, a.c_n, v[u]);
                    }
#pragma unroll
                    for (int u = 0; u < WG_ROWS; ++u)
#pragma unroll
                        for (int i = 0; i < COLS; ++i)
                            if (ok[u]) s[u][i] = __fadd_rn(s[u][i], __fmul_rn(mv[u], v[u][i]));
                }
#pragma unroll
                for (int u = 0; u < WG_ROWS; ++u)
#pragma unroll
                    for (int i = 0; i < COLS; ++i) {
                        T q;
                        from_f32(s[u][i], &q);
                        xv[u][i] = to_f32(q);
                    }
            } else {
#pragma unroll
                for (int u = 0; u < WG_ROWS; ++u) {
                    const int64_t r = rg + u < r1 ? rg + u : r1 - 1;  // past the wave's rows: a row again, times zeros
                    load_cols<T, ALIGNED>(x + r * a.x_stride, c, a.c_n, xv[u]);
                }
            }
#pragma unroll
            for (int u = 0; u < WG_ROWS; u += 2) {
                uint32_t ba, bb;
                keep4_two(a.m, rg + u, rg + u + 1, a.moff + c, paired, ba, bb);
#pragma unroll
                for (int i = 0; i < COLS; ++i) {
                    if (!((ba >> i) & 1u) || rg + u >= r1) xv[u][i] = 0.0f;
                    if (!((bb >> i) & 1u) || rg + u + 1 >= r1) xv[u + 1][i] = 0.0f;
                }
            }
#pragma unroll
            for (int u = 0; u < WG_ROWS; ++u) {
                const float *gr = gs + (rr + u) * CO;  // zeros past the wave's rows
                if (sum_g) bs = __fadd_rn(bs, gr[lane % CO]);
#pragma unroll
                for (int j = 0; j < CO; ++j) {
                    const float gj = gr[j];
#pragma unroll
                    for (int i = 0; i < COLS; ++i) acc[i][j] = __builtin_fmaf(xv[u][i], gj, acc[i][j]);
                }
            }
        }
    }
    __syncthreads();  // gy's rows are done with: the same LDS takes the waves' sums
    // k_head_wgrad's reduction over eight waves, times scale at the store; one helper for both raised the
    // VGPR count of forms of both kernels (docs/HISTORY.md §13), so each keeps its own
    for (int w = WG_WAVES - 1; w > 0; --w) {
        if (wave == w) {
#pragma unroll
            for (int i = 0; i < COLS; ++i)
#pragma unroll
                for (int j = 0; j < CO; ++j) lds[(i * CO + j) * 64 + lane] = acc[i][j];
            lds[COLS * CO * 64 + lane] = bs;
        }
        __syncthreads();
        if (wave == 0) {
#pragma unroll
            for (int i = 0; i < COLS; ++i)
#pragma unroll
                for (int j = 0; j < CO; ++j) acc[i][j] = __fadd_rn(acc[i][j], lds[(i * CO + j) * 64 + lane]);
            bs = __fadd_rn(bs, lds[COLS * CO * 64 + lane]);
        }
        __syncthreads();
    }
    if (wave != 0) return;
    float *p = a.part + (int64_t)blockIdx.x * (a.c_n + 1) * CO;
#pragma unroll
    for (int i = 0; i < COLS; ++i) {
        if (c + i >= a.c_n) continue;
#pragma unroll
        for (int j = 0; j < CO; j += 4)
            *reinterpret_cast<f32x4 *>(p + (c + i) * CO + j) =
                f32x4{__fmul_rn(acc[i][j], a.m.scale), __fmul_rn(acc[i][j + 1], a.m.scale),
                      __fmul_rn(acc[i][j + 2], a.m.scale), __fmul_rn(acc[i][j + 3], a.m.scale)};
    }
    if (sum_g && lane < CO) p[a.c_n * CO + lane] = bs;
}

// ---------------------------------------------------------------- host side
// keep_prob in (0, 1] -> the threshold and the scale of include/shpl.h; false for anything else (NaN included)
inline bool make_mask(double keep_prob, uint64_t seed, Mask *m) {
    if (!(keep_prob > 0.0 && keep_prob <= 1.0)) return false;
    double t = __builtin_floor(keep_prob * 65536.0 + 0.5);
    t = t < 1.0 ? 1.0 : t > 65536.0 ? 65536.0 : t;
    m->k0 = (uint32_t)seed;
    m->k1 = (uint32_t)(seed >> 32);
    m->thr = (uint32_t)t;
    m->scale = (float)(65536.0 / t);
    return true;
}

// The workspaces hold packed weights, key ranges (for a CSR that carries none), the f32 padded copy of gy and
// the weight gradient's partials: nothing of the size of a map or of the entries times the channels.
struct DgradLayout {
    int co;
    size_t gp, kr, bytes;
};
inline DgradLayout dgrad_layout(int64_t rows, int64_t rows_b, int64_t c_out, bool pooled) {
    DgradLayout l = {};
    l.co = pad_cols(c_out);
    size_t o = 0;
    l.gp = o;
    o = align_up(o + (size_t)rows * l.co * 4, 256);
    l.kr = o;
    if (pooled) o = align_up(o + (size_t)rows_b * 8, 256);
    l.bytes = o;
    return l;
}

// The one published size of the forward's and the input gradient's workspace.
inline size_t ws_need(int dtype, int64_t rows, int64_t c_a, int64_t rows_b, int64_t c_b, int64_t c_out, bool pooled) {
    const size_t f = fwd_layout(dtype, rows, c_a, rows_b, c_b, pooled, false).bytes;
    const size_t b = dgrad_layout(rows, rows_b, c_out, pooled).bytes;
    return f > b ? f : b;
}

struct WgradLayout {
    int co;
    Chunking ch;  // the row chunks (both sources run over the cells)
    size_t kr, part[2], bytes;
};
inline WgradLayout wgrad_layout(int64_t rows, int64_t c_a, int64_t c_b, int64_t c_out, bool pooled) {
    WgradLayout l = {};
    l.co = pad_cols(c_out);
    l.ch = chunking(rows, WG_MIN_ROWS, WG_MAX_CHUNKS);
    size_t o = 0;
    l.kr = o;
    if (pooled) o = align_up(o + (size_t)rows * 8, 256);
    const int64_t cs[2] = {c_a, c_b};
    for (int s = 0; s < 2; ++s) {
        l.part[s] = o;
        if (cs[s] > 0) o = align_up(o + (size_t)l.ch.chunks_max * (size_t)(cs[s] + 1) * l.co * 4, 256);
    }
    l.bytes = o;
    return l;
}

}  // namespace head_drop
}  // namespace shpl

using namespace shpl;
using namespace shpl::head_drop;

extern "C" int shpl_dropout_mask(int64_t rows, int64_t c, double keep_prob, uint64_t seed, uint8_t *d_mask,
                                 void *stream) {
    Mask m;
    if (!make_mask(keep_prob, seed, &m)) return SHPL_ERR_ARG;
    if (rows < 0 || c < 1 || c >= ((int64_t)1 << 31)) return SHPL_ERR_BAD_SHAPE;
    if (!d_mask) return SHPL_ERR_ARG;
    const int64_t groups = (c + 7) / 8, n = rows * groups;
    if (n >= ((int64_t)1 << 31) * SHPL_BLOCK) return SHPL_ERR_BAD_SHAPE;
    if (n == 0) return SHPL_OK;
    hipLaunchKernelGGL(k_dropout_mask, dim3(blocks_for(n, SHPL_BLOCK)), dim3(SHPL_BLOCK), 0, (hipStream_t)stream, rows, c,
                       groups, m, d_mask);
    SHPL_LAUNCH_CHECK();
    return SHPL_OK;
}

extern "C" int shpl_head1x1_drop_workspace_bytes(int dtype, int64_t rows, int64_t c_a, int64_t rows_b, int64_t c_b,
                                                 int64_t c_out, int pooled, size_t *bytes) {
    if (!bytes) return SHPL_ERR_ARG;
    const int rc = check_shape(dtype, rows, c_a, rows_b, c_b, c_out);
    if (rc != SHPL_OK) return rc;
    *bytes = ws_need(dtype, rows, c_a, rows_b, c_b, c_out, pooled != 0);
    return SHPL_OK;
}

extern "C" int shpl_head1x1_drop_wgrad_workspace_bytes(int dtype, int64_t rows, int64_t c_a, int64_t rows_b,
                                                       int64_t c_b, int64_t c_out, int pooled, size_t *bytes) {
    if (!bytes) return SHPL_ERR_ARG;
    const int rc = check_shape(dtype, rows, c_a, rows_b, c_b, c_out);
    if (rc != SHPL_OK) return rc;
    *bytes = wgrad_layout(rows, c_a, c_b, c_out, pooled != 0).bytes;
    return SHPL_OK;
}

extern "C" int shpl_head1x1_drop(int dtype, int64_t rows, const void *d_a, int64_t a_stride, int64_t a_off,
                                 int64_t c_a, const void *d_b, int64_t b_stride, int64_t b_off, int64_t c_b,
                                 int64_t rows_b, const shpl_csr *pool, const void *d_weights, int64_t c_out,
                                 const float *d_bias, void *d_out, int64_t out_stride, double keep_prob, uint64_t seed,
                                 void *d_ws, size_t ws_bytes, void *stream) {
    Mask m;
    const bool mask_ok = make_mask(keep_prob, seed, &m), pooled = pool != nullptr;
    int rc = check_sources(dtype, rows, d_a, a_stride, a_off, c_a, d_b, b_stride, b_off, c_b, rows_b, pool, false,
                           d_weights, d_out, c_out, out_stride, mask_ok, d_ws, ws_bytes,
                           [&] { return ws_need(dtype, rows, c_a, rows_b, c_b, c_out, pooled); });
    if (rc != SHPL_OK || rows == 0) return rc;
    const FwdLayout l = fwd_layout(dtype, rows, c_a, rows_b, c_b, pooled, false);
    hipStream_t s = (hipStream_t)stream;
    char *ws = reinterpret_cast<char *>(d_ws);
    const int64_t esz = esize(dtype), vec = 16 / esz;
    if ((rc = launch_pack(dtype, d_weights, 0, c_a, c_out, ws + l.wp[0], s)) != SHPL_OK) return rc;
    if ((rc = launch_pack(dtype, d_weights, c_a, c_b, c_out, ws + l.wp[1], s)) != SHPL_OK) return rc;
    FwdArgs g = {};
    g.s[0] = MaskedSrc{{d_a, a_stride, a_off, c_a, ws + l.wp[0]}, 0};
    g.s[1] = MaskedSrc{{d_b, b_stride, b_off, c_b, ws + l.wp[1]}, c_a};
    g.rows = rows;
    g.bias = d_bias;
    g.c_out = (int)c_out;
    if (pooled && (rc = pool_ref(pool, rows, rows_b, reinterpret_cast<int32_t *>(ws + l.kr), s, &g.pool)) != SHPL_OK)
        return rc;
    g.out = d_out;
    g.out_stride = out_stride;
    g.m = m;
    const bool al = c_a % (SUB * 2 * vec) == 0 && rows_aligned(d_a, a_stride, a_off, c_a, vec, esz) &&
                    (c_b == 0 || (c_b % (SUB * 2 * vec) == 0 && rows_aligned(d_b, b_stride, b_off, c_b, vec, esz)));
    const unsigned grid = blocks_for(rows, (int64_t)TILE_ROWS * GEMM_WAVES);
    by_dtype(dtype, [&](auto tt) {
        typedef typename decltype(tt)::T T;
        by_bools([&](auto al_) {
            hipLaunchKernelGGL((k_head_drop_gemm<T, decltype(al_)::value>), dim3(grid), dim3(GEMM_WAVES * 64), 0, s, g);
        }, al);
        return SHPL_OK;
    });
    SHPL_LAUNCH_CHECK();
    return SHPL_OK;
}

extern "C" int shpl_head1x1_drop_dgrad(int dtype, int64_t rows, const void *d_gy, int64_t gy_stride, int64_t c_out,
                                       const void *d_weights, int64_t c_a, int64_t c_b, void *d_da, int64_t da_stride,
                                       void *d_db, int64_t db_stride, int64_t rows_b, const shpl_csr *pool_grad,
                                       double keep_prob, uint64_t seed, void *d_ws, size_t ws_bytes, void *stream) {
    Mask m;
    const bool mask_ok = make_mask(keep_prob, seed, &m), pooled = pool_grad != nullptr;
    int rc = check_dgrad(dtype, rows, d_gy, gy_stride, c_out, d_weights, c_a, c_b, d_da, da_stride, d_db, db_stride,
                         rows_b, pool_grad, mask_ok, d_ws, ws_bytes,
                         [&] { return ws_need(dtype, rows, c_a, rows_b, c_b, c_out, pooled); });
    if (rc != SHPL_OK || rows == 0) return rc;
    const DgradLayout l = dgrad_layout(rows, rows_b, c_out, pooled);
    hipStream_t s = (hipStream_t)stream;
    char *ws = reinterpret_cast<char *>(d_ws);
    float *gp = reinterpret_cast<float *>(ws + l.gp);
    if ((rc = launch_gpad(dtype, d_gy, gy_stride, c_out, l.co, rows, gp, s)) != SHPL_OK) return rc;
    const int64_t esz = esize(dtype);
    // the rows of a dense map: d_a, or a dense second source
    auto dense = [&](int64_t w_row0, int64_t c_n, void *dx, int64_t dx_stride) {
        const bool al = rows_aligned(dx, dx_stride, 0, c_n, COLS, esz);
        const dim3 grid(blocks_for(rows, DGRAD_ROWS), blocks_for(c_n, 64 * COLS));
        by_dtype(dtype, [&](auto tt) {
            typedef typename decltype(tt)::T T;
            return by_cols(l.co, [&](auto cc) {
                constexpr int CO = decltype(cc)::value;
                by_bools([&](auto al_) {
                    hipLaunchKernelGGL((k_head_drop_dgrad<T, CO, decltype(al_)::value>), grid, dim3(64), 0, s, gp, rows,
                                       (int64_t)DGRAD_ROWS, reinterpret_cast<const T *>(d_weights), w_row0, c_n,
                                       (int)c_out, reinterpret_cast<T *>(dx), dx_stride, m);
                }, al);
                return SHPL_OK;
            });
        });
    };
    if (d_da) {
        dense(0, c_a, d_da, da_stride);
        SHPL_LAUNCH_CHECK();
    }
    if (d_db && !pooled) {
        dense(c_a, c_b, d_db, db_stride);
        SHPL_LAUNCH_CHECK();
    }
    if (d_db && pooled && rows_b > 0) {
        PoolRef p;
        if ((rc = pool_ref(pool_grad, rows_b, rows, reinterpret_cast<int32_t *>(ws + l.kr), s, &p)) != SHPL_OK) return rc;
        const bool al = rows_aligned(d_db, db_stride, 0, c_b, COLS, esz);
        // few pixels per wave: the runs are uneven (the horizon's pixels take tens of entries) and a wave walks its
        // pixels one after the other, so the longest wave sets the kernel's time (at MV3D's shape 32 per wave took
        // 0.75 ms and 4 take 0.3 ms; at 1 the weights' loads per wave cost more: 0.8 ms)
        const int64_t pix_per = 4;
        const dim3 grid(blocks_for(rows_b, pix_per), blocks_for(c_b, 64 * COLS));
        by_dtype(dtype, [&](auto tt) {
            typedef typename decltype(tt)::T T;
            return by_cols(l.co, [&](auto cc) {
                constexpr int CO = decltype(cc)::value;
                by_bools([&](auto al_) {
                    hipLaunchKernelGGL((k_head_drop_dgrad_pool<T, CO, decltype(al_)::value>), grid, dim3(64), 0, s, gp, p,
                                       rows_b, pix_per, reinterpret_cast<const T *>(d_weights), c_a, c_b, (int)c_out,
                                       reinterpret_cast<T *>(d_db), db_stride, m);
                }, al);
                return SHPL_OK;
            });
        });
        SHPL_LAUNCH_CHECK();
    }
    return SHPL_OK;
}

extern "C" int shpl_head1x1_drop_wgrad(int dtype, int64_t rows, const void *d_a, int64_t a_stride, int64_t a_off,
                                       int64_t c_a, const void *d_b, int64_t b_stride, int64_t b_off, int64_t c_b,
                                       int64_t rows_b, const shpl_csr *pool, const void *d_gy, int64_t gy_stride,
                                       int64_t c_out, float *d_dw, float *d_dbias, double keep_prob, uint64_t seed,
                                       void *d_ws, size_t ws_bytes, void *stream) {
    Mask m;
    const bool mask_ok = make_mask(keep_prob, seed, &m), pooled = pool != nullptr;
    int rc = check_sources(dtype, rows, d_a, a_stride, a_off, c_a, d_b, b_stride, b_off, c_b, rows_b, pool, false, d_gy,
                           d_dw, c_out, gy_stride, mask_ok, d_ws, ws_bytes,
                           [&] { return wgrad_layout(rows, c_a, c_b, c_out, pooled).bytes; });
    if (rc != SHPL_OK) return rc;
    const WgradLayout l = wgrad_layout(rows, c_a, c_b, c_out, pooled);
    hipStream_t s = (hipStream_t)stream;
    char *ws = reinterpret_cast<char *>(d_ws);
    const int64_t esz = esize(dtype);
    const int64_t per = l.ch.per, chunks = l.ch.chunks;  // 0 rows: no partial, zeros
    PoolRef p = {};
    if (pooled && chunks > 0 &&
        (rc = pool_ref(pool, rows, rows_b, reinterpret_cast<int32_t *>(ws + l.kr), s, &p)) != SHPL_OK)
        return rc;
    // one source: its partials, then their sum into rows [moff, moff + c_n) of dw (and the bias gradient)
    auto run = [&](int k, const void *x, int64_t x_stride, int64_t x_off, int64_t c_n, int64_t moff, bool from_pool,
                   bool bias) {
        float *part = reinterpret_cast<float *>(ws + l.part[k]);
        const int64_t n_chunks = (from_pool && rows_b == 0) ? 0 : chunks;  // a pooling of no pixels: zeros
        if (n_chunks > 0) {
            WgradArgs a = {x, x_stride, x_off, c_n, moff, p, d_gy, gy_stride, (int)c_out, rows, per, (int)bias, part, m};
            const bool al = rows_aligned(x, x_stride, x_off, c_n, COLS, esz);
            const dim3 grid((unsigned)chunks, blocks_for(c_n, 64 * COLS));
            by_dtype(dtype, [&](auto tt) {
                typedef typename decltype(tt)::T T;
                return by_cols(l.co, [&](auto cc) {
                    constexpr int CO = decltype(cc)::value;
                    by_bools([&](auto al_, auto pl_) {
                        hipLaunchKernelGGL((k_head_drop_wgrad<T, CO, decltype(al_)::value, decltype(pl_)::value>), grid,
                                           dim3(WG_WAVES * 64), 0, s, a);
                    }, al, from_pool);
                    return SHPL_OK;
                });
            });
        }
        launch_wreduce(part, n_chunks, c_n, l.co, c_out, bias, d_dw, moff, d_dbias, s);
    };
    run(0, d_a, a_stride, a_off, c_a, 0, false, d_dbias != nullptr);
    SHPL_LAUNCH_CHECK();
    if (c_b > 0) {
        run(1, d_b, b_stride, b_off, c_b, c_a, pooled, false);
        SHPL_LAUNCH_CHECK();
    }
    return SHPL_OK;
}
