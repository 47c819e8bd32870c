// shpl_head.h -- what the 1x1 head kernels (shpl_head.hip) and their dropout forms (shpl_head_drop.hip) share:
// the tile constants, the 16-byte pieces and their MFMA, the GEMM's K loop, the backward kernels' steps (weight
// load, projection, COLS loads and stores, a CSR's runs), the host-side argument checks (one order for all six
// calls), layouts and dispatchers, and the launchers of the helper kernels that live in shpl_head.hip (weight
// packing, key ranges, the padded gradient, the partials' reduce).
#pragma once

#include "shpl_common.h"

namespace shpl {
namespace head {

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef uint16_t u16x4 __attribute__((ext_vector_type(4)));

constexpr int NP = 32;        // output columns of a GEMM tile: c_out padded
constexpr int TILE_ROWS = 32; // rows of a GEMM tile (one wave)
constexpr int GEMM_WAVES = 4; // waves per GEMM workgroup
constexpr int SUB = 4;        // 16-byte pieces per lane and K step: 64 contiguous bytes of its row
constexpr int COLS = 4;       // channels per thread of the backward kernels
constexpr int DGRAD_ROWS = 128;  // rows per wave of the input gradient

template <typename T>
struct Vec;  // elements of one 16-byte piece
template <>
struct Vec<float> {
    static constexpr int N = 4;
};
template <>
struct Vec<uint16_t> {
    static constexpr int N = 8;
};

__device__ __forceinline__ float to_f32(float v) { return v; }
__device__ __forceinline__ float to_f32(uint16_t v) { return bf16_to_f32(v); }
__device__ __forceinline__ void from_f32(float v, float *o) { *o = v; }
__device__ __forceinline__ void from_f32(float v, uint16_t *o) { *o = f32_to_bf16(v); }

inline int64_t pack_steps(int64_t c, int vec) { return (c + SUB * 2 * vec - 1) / (SUB * 2 * vec); }

__device__ __forceinline__ f32x16 mma(const float (&x)[4], const float (&w)[4], f32x16 acc) {
#pragma unroll
    for (int i = 0; i < 4; ++i) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(x[i], w[i], acc, 0, 0, 0);
    return acc;
}
__device__ __forceinline__ f32x16 mma(const uint16_t (&x)[8], const uint16_t (&w)[8], f32x16 acc) {
    bf16x8 xa, wb;
    __builtin_memcpy(&xa, x, 16);
    __builtin_memcpy(&wb, w, 16);
    return __builtin_amdgcn_mfma_f32_32x32x16_bf16(xa, wb, acc, 0, 0, 0);
}

// ---------------------------------------------------------------- the GEMM's K loop
struct Src {
    const void *x;
    int64_t stride, off, c;
    const void *wp;
};

// one 16-byte piece of a row: channels [k, k + VEC) of the c the row holds
template <typename T, bool ALIGNED>
__device__ __forceinline__ void load_piece(const T *p, int64_t k, int64_t c, T (&v)[Vec<T>::N]) {
    constexpr int VEC = Vec<T>::N;
    if constexpr (ALIGNED) {
        const u32x4 q = *reinterpret_cast<const u32x4 *>(p);
        __builtin_memcpy(v, &q, 16);
    } else {
#pragma unroll
        for (int i = 0; i < VEC; ++i) v[i] = k + i < c ? p[i] : T(0);
    }
}

struct NoMask {};

// acc += row rl of one source times its packed weights (a source of no channels: nothing). Two register stages:
// the loads of the next K step are issued before the MFMAs of the current one. DROP: a step's dropped elements
// are zeroed before its MFMAs by drop_step(pieces, m, row, the step's first channel in the concat: moff is the
// source's) -- found through the mask's type (shpl_head_drop.hip) -- so the lane's slice of the mask is computed
// while the next step's loads are in flight. (moff is no field of Src: a sixth word split the plain kernel's one
// scalar load of both sources into four, docs/HISTORY.md §13; the dropout kernel's MaskedSrc adds it.)
template <typename T, bool ALIGNED, bool DROP, typename M = NoMask>
__device__ __forceinline__ f32x16 source(const Src &src, int64_t rl, int lane, f32x16 acc, const M &m = M(),
                                         int64_t moff = 0) {
    constexpr int VEC = Vec<T>::N, NCH = SUB * VEC;
    const int64_t c = src.c;
    const int h = lane >> 5;
    const T *xr = reinterpret_cast<const T *>(src.x) + rl * src.stride + src.off + h * NCH;
    const T *wp = reinterpret_cast<const T *>(src.wp) + lane * VEC;
    const int64_t steps = (c + 2 * NCH - 1) / (2 * NCH);
    auto load = [&](int64_t st, T (&xv)[SUB][VEC], T (&wv)[SUB][VEC]) {
        const int64_t k = st * 2 * NCH, kh = k + h * NCH;  // the lane's first channel of the step
#pragma unroll
        for (int j = 0; j < SUB; ++j) {
            load_piece<T, ALIGNED>(xr + k + j * VEC, kh + j * VEC, c, xv[j]);
            const u32x4 wq = *reinterpret_cast<const u32x4 *>(wp + (st * SUB + j) * 64 * VEC);
            __builtin_memcpy(wv[j], &wq, 16);
        }
    };
    auto mul = [&](int64_t st, T (&xv)[SUB][VEC], const T (&wv)[SUB][VEC]) {
        if constexpr (DROP) drop_step(xv, m, rl, moff + st * 2 * NCH + h * NCH);
#pragma unroll
        for (int j = 0; j < SUB; ++j) acc = mma(xv[j], wv[j], acc);
    };
    if (steps == 0) return acc;
    T xa[SUB][VEC], wa[SUB][VEC], xb[SUB][VEC], wb[SUB][VEC];
    load(0, xa, wa);
    // a branch-free body (a load under a condition makes the wait before the MFMAs drain the loads just issued): the
    // second load of the last pair of an even count re-reads the last step, unused
    for (int64_t p = 0; p < steps / 2; ++p) {
        load(2 * p + 1, xb, wb);
        mul(2 * p, xa, wa);
        load(2 * p + 2 < steps ? 2 * p + 2 : steps - 1, xa, wa);
        mul(2 * p + 1, xb, wb);
    }
    if (steps & 1) mul(steps - 1, xa, wa);
    return acc;
}

// ---------------------------------------------------------------- the backward kernels' steps
template <typename T>
struct Cols {  // COLS elements as one vector
    typedef typename std::conditional<sizeof(T) == 4, f32x4, u16x4>::type V;
};

template <typename T, bool ALIGNED>
__device__ __forceinline__ void load_cols(const T *p, int64_t c, int64_t c_n, float (&xv)[COLS]) {
    if constexpr (ALIGNED) {
        typedef typename Cols<T>::V V;
        T raw[COLS];
        V v = {};
        if (c < c_n) v = *reinterpret_cast<const V *>(p);
        __builtin_memcpy(raw, &v, sizeof(V));
#pragma unroll
        for (int i = 0; i < COLS; ++i) xv[i] = to_f32(raw[i]);
    } else {
#pragma unroll
        for (int i = 0; i < COLS; ++i) xv[i] = c + i < c_n ? to_f32(p[i]) : 0.0f;
    }
}

template <typename T, bool ALIGNED>
__device__ __forceinline__ void store_cols(T *dst, int64_t c, int64_t c_n, const float (&o)[COLS]) {
    if (c >= c_n) return;
    T ov[COLS];
#pragma unroll
    for (int i = 0; i < COLS; ++i) from_f32(o[i], &ov[i]);
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

// a thread's COLS channels of W[w_row0 + c .. ][.] in registers
template <typename T, int CO>
__device__ __forceinline__ void load_weights(const T *w, int64_t w_row0, int64_t c, int64_t c_n, int c_out,
                                             float (&wr)[COLS][CO]) {
#pragma unroll
    for (int i = 0; i < COLS; ++i)
#pragma unroll
        for (int j = 0; j < CO; ++j) wr[i][j] = (c + i < c_n && j < c_out) ? to_f32(w[(w_row0 + c + i) * c_out + j]) : 0.0f;
}

// o[i] = sum_j gr[j] * wr[i][j], j ascending, fused multiply-adds
template <int CO>
__device__ __forceinline__ void project(const float *gr, const float (&wr)[COLS][CO], float (&o)[COLS]) {
#pragma unroll
    for (int i = 0; i < COLS; ++i) o[i] = 0.0f;
#pragma unroll
    for (int j = 0; j < CO; ++j) {
        const float gj = gr[j];
#pragma unroll
        for (int i = 0; i < COLS; ++i) o[i] = __builtin_fmaf(gj, wr[i][j], o[i]);
    }
}

struct PoolRef {  // a CSR's runs, as the kernels read them
    const int32_t *key_range, *ent_src;
    const float *ent_val;
    int64_t nnz_cap, n_src;  // entries; rows of the source the entries name
};

__device__ __forceinline__ void run_of(const PoolRef &p, int64_t key, int64_t &e, int64_t &end) {
    e = p.key_range[2 * key];
    end = p.key_range[2 * key + 1];
    if (e < 0) e = 0;
    if (end > p.nnz_cap) end = p.nnz_cap;
}

// ---------------------------------------------------------------- host side
inline int pad_cols(int64_t c_out) { return (int)((c_out + 3) / 4 * 4); }  // whole 16-byte pieces of f32
inline int64_t esize(int dtype) { return dtype == SHPL_F32 ? 4 : 2; }

inline bool pixel_keyed(const shpl_csr *p) { return p->ent_col || (p->flags & SHPL_CSR_IDENTITY_COLS); }

// rows of source `x` in pieces of `vec` elements: whole pieces, each on its own alignment
inline bool rows_aligned(const void *x, int64_t stride, int64_t off, int64_t c, int64_t vec, int64_t esz) {
    return c % vec == 0 && stride % vec == 0 && off % vec == 0 && ((uintptr_t)x % (size_t)(vec * esz)) == 0;
}

// The checks every entry point shares: dtype, channel counts, rows; then the second source's form.
inline int check_shape(int dtype, int64_t rows, int64_t c_a, int64_t rows_b, int64_t c_b, int64_t c_out) {
    if (dtype != SHPL_F32 && dtype != SHPL_BF16) return SHPL_ERR_ARG;
    if (c_out < 1 || c_out > NP) return SHPL_ERR_BAD_SHAPE;
    const int64_t lim = (int64_t)1 << 31;
    if (rows < 0 || rows >= lim || rows_b < 0 || rows_b >= lim) return SHPL_ERR_BAD_SHAPE;
    if (c_a < 1 || c_b < 0 || c_a >= (1 << 22) || c_b >= (1 << 22)) return SHPL_ERR_BAD_SHAPE;  // grid.y, 32-bit rows
    return SHPL_OK;
}

// pool: the CSR of the pooled form (NULL: dense b); want_pixel: the gradient's pixel-keyed list.
inline int check_pool(const shpl_csr *pool, bool want_pixel, int64_t rows, int64_t rows_b, int64_t c_b) {
    if (!pool) return (c_b > 0 && rows_b != rows) ? SHPL_ERR_BAD_SHAPE : SHPL_OK;
    if (c_b < 1) return SHPL_ERR_BAD_SHAPE;
    if (pixel_keyed(pool) != want_pixel) return SHPL_ERR_ARG;
    if (pool->n_keys != (want_pixel ? rows_b : rows)) return SHPL_ERR_BAD_SHAPE;
    if (pool->nnz_cap < 0 || pool->nnz_cap >= ((int64_t)1 << 31)) return SHPL_ERR_BAD_SHAPE;
    if (pool->nnz_cap > 0 && (!pool->ent_dst || !pool->ent_src || !pool->ent_val)) return SHPL_ERR_ARG;
    return SHPL_OK;
}

// What follows check_shape in every call: the dropout calls' keep_prob (mask_ok), the pointers, the second
// source's form, the strides, then the workspace (need(): its bytes, computed once the shape is known to be
// sound). The order is what callers observe (tests/golden/head_host_plan.json).
inline int check_ws(const void *d_ws, size_t ws_bytes, size_t need) {
    if (!d_ws) return SHPL_ERR_ARG;
    if (ws_bytes < need) return SHPL_ERR_WORKSPACE;
    return aligned16(d_ws) ? SHPL_OK : SHPL_ERR_BAD_SHAPE;
}

// The forward (p1, p2: the weights and the output; last_stride: the output's) and the weight gradient (p1, p2: gy
// and dw; last_stride: gy's): two strided sources and a row of c_out elements.
template <typename Need>
int check_sources(int dtype, int64_t rows, const void *d_a, int64_t a_stride, int64_t a_off, int64_t c_a,
                  const void *d_b, int64_t b_stride, int64_t b_off, int64_t c_b, int64_t rows_b, const shpl_csr *pool,
                  bool want_pixel, const void *p1, const void *p2, int64_t c_out, int64_t last_stride, bool mask_ok,
                  const void *d_ws, size_t ws_bytes, Need &&need) {
    int rc = check_shape(dtype, rows, c_a, rows_b, c_b, c_out);
    if (rc != SHPL_OK) return rc;
    if (!mask_ok || !d_a || !p1 || !p2 || (c_b > 0 && !d_b)) return SHPL_ERR_ARG;
    if ((rc = check_pool(pool, want_pixel, rows, rows_b, c_b)) != SHPL_OK) return rc;
    if (a_off < 0 || b_off < 0 || a_stride < a_off + c_a || (c_b > 0 && b_stride < b_off + c_b) || last_stride < c_out)
        return SHPL_ERR_BAD_SHAPE;
    return check_ws(d_ws, ws_bytes, need());
}

template <typename Need>
int check_dgrad(int dtype, int64_t rows, const void *d_gy, int64_t gy_stride, int64_t c_out, const void *d_weights,
                int64_t c_a, int64_t c_b, const void *d_da, int64_t da_stride, const void *d_db, int64_t db_stride,
                int64_t rows_b, const shpl_csr *pool_grad, bool mask_ok, const void *d_ws, size_t ws_bytes,
                Need &&need) {
    int rc = check_shape(dtype, rows, c_a, rows_b, c_b, c_out);
    if (rc != SHPL_OK) return rc;
    if (!mask_ok || !d_gy || !d_weights || (!d_da && !d_db)) return SHPL_ERR_ARG;
    if (d_db && c_b < 1) return SHPL_ERR_BAD_SHAPE;
    if ((rc = check_pool(pool_grad, true, rows, rows_b, c_b)) != SHPL_OK) return rc;
    if (gy_stride < c_out || (d_da && da_stride < c_a) || (d_db && db_stride < c_b)) return SHPL_ERR_BAD_SHAPE;
    return check_ws(d_ws, ws_bytes, need());
}

// The weight gradient's row chunks: `per` rows each, at least min_rows, in at most max_chunks chunks; chunks_max:
// the bound the workspace is sized by.
struct Chunking {
    int64_t per, chunks, chunks_max;
};
inline Chunking chunking(int64_t rows, int64_t min_rows, int64_t max_chunks) {
    int64_t per = (rows + max_chunks - 1) / max_chunks;
    if (per < min_rows) per = min_rows;
    const int64_t most = (rows + min_rows - 1) / min_rows;
    return {per, (rows + per - 1) / per, most < 1 ? 1 : most > max_chunks ? max_chunks : most};
}

// The forward's workspace: both sources' packed weights, then for the pooled form Z [rows_b][NP] f32 (with_z: the
// plain form; under dropout the pooling runs in the operand staging) and the key ranges of a CSR that has none.
struct FwdLayout {
    size_t wp[2], z, kr, bytes;
};
inline FwdLayout fwd_layout(int dtype, int64_t rows, int64_t c_a, int64_t rows_b, int64_t c_b, bool pooled,
                            bool with_z) {
    const int vec = (int)(16 / esize(dtype));
    FwdLayout l = {};
    size_t o = 0;
    const int64_t cs[2] = {c_a, c_b};
    for (int s = 0; s < 2; ++s) {
        l.wp[s] = o;
        o = align_up(o + (size_t)pack_steps(cs[s], vec) * SUB * 64 * 16, 256);
    }
    l.z = o;
    if (pooled && with_z) o = align_up(o + (size_t)rows_b * NP * 4, 256);
    l.kr = o;
    if (pooled) o = align_up(o + (size_t)rows * 8, 256);
    l.bytes = o;
    return l;
}

template <typename F>
int by_dtype(int dtype, F &&fn) {
    return dtype == SHPL_F32 ? fn(TypeOf<float>()) : fn(TypeOf<uint16_t>());
}
template <typename F>
int by_cols(int co, F &&fn) {
    switch (co) {
        case 4: return fn(std::integral_constant<int, 4>());
        case 8: return fn(std::integral_constant<int, 8>());
        case 12: return fn(std::integral_constant<int, 12>());
        case 16: return fn(std::integral_constant<int, 16>());
        case 20: return fn(std::integral_constant<int, 20>());
        case 24: return fn(std::integral_constant<int, 24>());
        case 28: return fn(std::integral_constant<int, 28>());
        default: return fn(std::integral_constant<int, 32>());
    }
}

inline unsigned blocks_for(int64_t n, int64_t per) { return (unsigned)((n + per - 1) / per); }

// The launchers of shpl_head.hip's helper kernels (each returns SHPL_OK or SHPL_ERR_HIP):
// rows [w_row0, w_row0 + c) of the weights [.][c_out], packed per lane into wp (k_head_pack's layout)
int launch_pack(int dtype, const void *d_weights, int64_t w_row0, int64_t c, int64_t c_out, void *wp, hipStream_t s);
// kr [n_keys][2]: the key ranges of a CSR that carries none, over zeros
int launch_ranges(const shpl_csr *csr, int64_t n_keys, int32_t *kr, hipStream_t s);
// g (feature dtype) -> gp f32 [rows][co], zero past c_out
int launch_gpad(int dtype, const void *d_gy, int64_t gy_stride, int64_t c_out, int co, int64_t rows, float *gp,
                hipStream_t s);
// part [chunks][c_n + 1][co] -> dw[w_row0 + c][j] (and dbias from row c_n: with_bias), summed in f64 in chunk order
int launch_wreduce(const float *part, int64_t chunks, int64_t c_n, int co, int64_t c_out, bool with_bias, float *dw,
                   int64_t w_row0, float *dbias, hipStream_t s);


// the runs of `csr` over n_keys keys: its own key ranges, or ones built at kr
inline int pool_ref(const shpl_csr *csr, int64_t n_keys, int64_t n_src, int32_t *kr, hipStream_t s, PoolRef *out) {
    const int32_t *ranges = csr->key_range;
    if (!ranges) {
        const int rc = launch_ranges(csr, n_keys, kr, s);
        if (rc != SHPL_OK) return rc;
        ranges = kr;
    }
    *out = PoolRef{ranges, csr->ent_src, csr->ent_val, csr->nnz_cap, n_src};
    return SHPL_OK;
}

}  // namespace head
}  // namespace shpl
