// shpl_head.h -- what the 1x1 head kernels (shpl_head.hip) and their dropout forms (shpl_head_drop.hip) share:
// the tile constants, the 16-byte pieces and their MFMA, the host-side shape checks and dispatchers, and the
// launchers of the helper kernels that live in shpl_head.hip (weight packing, key ranges, the padded gradient,
// the partials' reduce).
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

}  // namespace head
}  // namespace shpl
