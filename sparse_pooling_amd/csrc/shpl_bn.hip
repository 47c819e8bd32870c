// shpl_bn.hip -- BatchNorm (+ ReLU) after the post-fusion conv (shpl_conv.hip): the training forward from the
// conv's batch statistics and the backward; vector kernels over 16-byte pieces when bn_vector_form holds.
#include <initializer_list>
#include <type_traits>

#include "shpl_conv_bn.h"

namespace shpl {
namespace {

// k_bn_finalize (shpl_conv_bn.h), then y = act((x - mean) * gamma / sqrt(var + eps) + beta) in place.
template <typename T>
__global__ __launch_bounds__(SHPL_BLOCK) void k_bn_apply(const T *x, T *y, int64_t rows, int64_t stride, int c,
                                                         const float *mean, const float *scale, const float *beta,
                                                         int act) {
    const int64_t total = rows * c;
    for (int64_t t = (int64_t)blockIdx.x * SHPL_BLOCK + threadIdx.x; t < total;
         t += (int64_t)gridDim.x * SHPL_BLOCK) {
        const int64_t r = t / c;
        const int ch = (int)(t - r * c);
        float v = __fmul_rn(__fsub_rn(Elem<T>::f(x[r * stride + ch]), mean[ch]), scale[ch]);
        if (beta) v = __fadd_rn(v, beta[ch]);
        if (act == 1) v = v > 0.0f ? v : 0.0f;
        y[r * stride + ch] = Elem<T>::back(v);
    }
}

// 16-byte pieces of a row (VEC channels): the vector forms of the BatchNorm
// streams, used when rows and channel counts are multiples of VEC and aligned.
// Rows per thread of the BatchNorm apply kernels' grid-stride loops: enough
// to amortise the per-thread channel parameters (six loads and a division
// per channel in the backward), few enough to keep loads in flight. Measured
// at 64 frames: f32 17 -> 4 rows took apply 1.78 -> 1.61 ms and backward
// apply 2.68 -> 2.35 ms; bf16 at 2 rows per thread was 1.7x slower than at 8.
constexpr int64_t bn_rows_per_thread(int esz) { return esz == 4 ? 4 : 8; }

// f(std::bool_constant<b0>{}, std::bool_constant<b1>{}, ...) for run-time switches b0, b1, ...: the
// instance of a vector BatchNorm kernel for one combination of its compile-time forms.
template <bool... Bs, typename F>
void bn_forms(F &&f) {
    f(std::bool_constant<Bs>{}...);
}
template <bool... Bs, typename F, typename... R>
void bn_forms(F &&f, bool b, R... rest) {
    if (b)
        bn_forms<Bs..., true>(f, rest...);
    else
        bn_forms<Bs..., false>(f, rest...);
}

// 16-byte pieces of the BatchNorm streams, nontemporal (each byte is touched
// once per pass; the maps are far larger than the caches).
template <typename T, int VEC>
struct Piece {
    static __device__ __forceinline__ void load(const T *p, float (&x)[VEC]) {
        const u32x4 r = __builtin_nontemporal_load(reinterpret_cast<const u32x4 *>(p));
        T e[VEC];
        __builtin_memcpy(e, &r, 16);
#pragma unroll
        for (int k = 0; k < VEC; ++k) x[k] = Elem<T>::f(e[k]);
    }
    static __device__ __forceinline__ void store(T *p, const float (&x)[VEC]) {
        T e[VEC];
#pragma unroll
        for (int k = 0; k < VEC; ++k) e[k] = Elem<T>::back(x[k]);
        u32x4 r;
        __builtin_memcpy(&r, e, 16);
        __builtin_nontemporal_store(r, reinterpret_cast<u32x4 *>(p));
    }
};

constexpr int BN_U = 4;  // rows per iteration of the vector apply kernels: their loads in flight together

// Thread layout of the vector forms: c / VEC piece lanes (a power of two
// dividing the block) times SHPL_BLOCK / (c / VEC) row lanes, so each thread
// keeps one channel group and its per-channel coefficients in registers.
// The vector apply kernels take their switches (ReLU, beta, y, training) as
// template arguments: as run-time flags they put a branch around every element
// of the unrolled loops (bn_forms picks the instance; bf16 at 64 frames: the
// backward apply 1,199 -> 1,147 us, the forward apply 777 -> 750 us,
// profiles/r04_bn_ab.log).
template <typename T, bool BETA, bool ACT>
__global__ __launch_bounds__(SHPL_BLOCK) void k_bn_apply_vec(const T *x, T *y, int64_t rows, int64_t stride, int c,
                                                             const float *mean, const float *scale,
                                                             const float *beta) {
    constexpr int VEC = 16 / sizeof(T);
    const int pr = c / VEC, rpb = SHPL_BLOCK / pr;
    const int ch0 = (threadIdx.x % pr) * VEC;
    float m[VEC], sc[VEC], b[VEC];
#pragma unroll
    for (int k = 0; k < VEC; ++k) {
        m[k] = mean[ch0 + k];
        sc[k] = scale[ch0 + k];
        b[k] = BETA ? beta[ch0 + k] : 0.0f;
    }
    const int64_t step = (int64_t)gridDim.x * rpb;
    for (int64_t r0 = (int64_t)blockIdx.x * rpb + threadIdx.x / pr; r0 < rows; r0 += BN_U * step) {
        float v[BN_U][VEC];
#pragma unroll
        for (int u = 0; u < BN_U; ++u)
            if (r0 + u * step < rows) Piece<T, VEC>::load(x + (r0 + u * step) * stride + ch0, v[u]);
#pragma unroll
        for (int u = 0; u < BN_U; ++u) {
            if (r0 + u * step >= rows) break;
#pragma unroll
            for (int k = 0; k < VEC; ++k) {
                float t = __fmul_rn(__fsub_rn(v[u][k], m[k]), sc[k]);
                if constexpr (BETA) t = __fadd_rn(t, b[k]);
                v[u][k] = (ACT && !(t > 0.0f)) ? 0.0f : t;
            }
            Piece<T, VEC>::store(y + (r0 + u * step) * stride + ch0, v[u]);
        }
    }
}

// ---------------------------------------------------------------- backward
// BatchNorm (+ ReLU) backward. g_bn = g * [y > 0] (act), xhat = (raw - mean)
// * scale / gamma; per-channel sums dbeta = sum g_bn, dgamma = sum g_bn xhat
// over rows in a fixed order (f64 partials per block, then per channel), and
//   training:  g_raw = scale * (g_bn - dbeta / N - xhat * dgamma / N)
//   inference: g_raw = scale * g_bn     (moving statistics are constants)
// mean / scale NULL: 0 / 1 (a conv bias instead of BN: g_raw = g_bn).
// The ReLU mask [y > 0] is read from y, or (y NULL) recomputed from the BN
// input with the forward's rounded operations, u = (raw - mean) * scale
// (+ beta), so that it is bitwise the forward's: [u > 0] == [y > 0].
__device__ __forceinline__ float bn_pre_act(float x, float m, float sc, const float *beta, int ch) {
    const float u = __fmul_rn(__fsub_rn(x, m), sc);
    return beta ? __fadd_rn(u, beta[ch]) : u;
}

template <typename T>
__device__ __forceinline__ float bn_gbn(const T *y, const T *raw, const T *gy, int64_t o, int ch, int act,
                                        const float *mean, const float *scale, const float *beta) {
    const float gv = Elem<T>::f(gy[o]);
    if (act != 1) return gv;
    const float yv = y ? Elem<T>::f(y[o])
                       : bn_pre_act(Elem<T>::f(raw[o]), mean ? mean[ch] : 0.0f, scale ? scale[ch] : 1.0f, beta, ch);
    return yv > 0.0f ? gv : 0.0f;
}

template <typename T>
__global__ __launch_bounds__(SHPL_BLOCK) void k_bn_bwd_partial(const T *y, const T *raw, const T *gy, int64_t rows,
                                                               int64_t stride, int c, const float *mean,
                                                               const float *scale, const float *gamma,
                                                               const float *beta, int act, int64_t rows_per_block,
                                                               double *part) {
    __shared__ double red[2][SHPL_BLOCK];
    int cc_n = 1;
    while (cc_n * 2 <= c && cc_n * 2 <= SHPL_BLOCK) cc_n *= 2;  // channels per pass (a power of two)
    const int rl_n = SHPL_BLOCK / cc_n, rl = threadIdx.x / cc_n, cc = threadIdx.x % cc_n;
    const int64_t r0 = (int64_t)blockIdx.x * rows_per_block;
    const int64_t r1 = r0 + rows_per_block < rows ? r0 + rows_per_block : rows;
    for (int c0 = 0; c0 < c; c0 += cc_n) {
        const int ch = c0 + cc;
        double s1 = 0.0, s2 = 0.0;
        if (ch < c) {
            const float m = mean ? mean[ch] : 0.0f;
            const float inv = scale ? __fdiv_rn(scale[ch], gamma ? gamma[ch] : 1.0f) : 1.0f;
            for (int64_t r = r0 + rl; r < r1; r += rl_n) {
                const int64_t o = r * stride + ch;
                const float gb = bn_gbn(y, raw, gy, o, ch, act, mean, scale, beta);
                const float xh = __fmul_rn(__fsub_rn(Elem<T>::f(raw[o]), m), inv);
                s1 += (double)gb;
                s2 += (double)gb * (double)xh;
            }
        }
        red[0][threadIdx.x] = s1;
        red[1][threadIdx.x] = s2;
        __syncthreads();
        if ((int)threadIdx.x < cc_n && c0 + (int)threadIdx.x < c) {
            double a = 0.0, b = 0.0;
            for (int k = 0; k < rl_n; ++k) {
                a += red[0][k * cc_n + threadIdx.x];
                b += red[1][k * cc_n + threadIdx.x];
            }
            part[((int64_t)blockIdx.x * 2 + 0) * c + c0 + threadIdx.x] = a;
            part[((int64_t)blockIdx.x * 2 + 1) * c + c0 + threadIdx.x] = b;
        }
        __syncthreads();
    }
}

// Vector form of k_bn_bwd_partial: thread (row lane rl, channel group cg)
// reads VEC channels of every rl_n-th row; c / VEC a power of two <= 256.
template <typename T>
__global__ __launch_bounds__(SHPL_BLOCK) void k_bn_bwd_partial_vec(const T *y, const T *raw, const T *gy,
                                                                   int64_t rows, int64_t stride, int c,
                                                                   const float *mean, const float *scale,
                                                                   const float *gamma, const float *beta, int act,
                                                                   int64_t rows_per_block, double *part) {
    constexpr int VEC = 16 / sizeof(T);
    __shared__ double red[2][SHPL_BLOCK * VEC];
    const int cg_n = c / VEC, rl_n = SHPL_BLOCK / cg_n;
    const int rl = threadIdx.x / cg_n, cg = threadIdx.x % cg_n, ch0 = cg * VEC;
    const int64_t r0 = (int64_t)blockIdx.x * rows_per_block;
    const int64_t r1 = r0 + rows_per_block < rows ? r0 + rows_per_block : rows;
    float m[VEC], inv[VEC], sc[VEC], b[VEC];
#pragma unroll
    for (int k = 0; k < VEC; ++k) {
        m[k] = mean ? mean[ch0 + k] : 0.0f;
        sc[k] = scale ? scale[ch0 + k] : 1.0f;
        inv[k] = scale ? __fdiv_rn(scale[ch0 + k], gamma ? gamma[ch0 + k] : 1.0f) : 1.0f;
        b[k] = beta ? beta[ch0 + k] : 0.0f;
    }
    double s1[VEC], s2[VEC];
#pragma unroll
    for (int k = 0; k < VEC; ++k) s1[k] = s2[k] = 0.0;
    // rows in flight per iteration (the sums stay in row order): bf16 4 (0.81 -> 0.73 ms per 64-frame
    // step; the apply kernels are slower with more, profiles/r02_bn_sweep.log)
    constexpr int U = sizeof(T) == 2 ? 4 : BN_U / 2;
    for (int64_t rb = r0 + rl; rb < r1; rb += U * rl_n) {
        float gv[U][VEC], xv[U][VEC], yv[U][VEC];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            if (rb + u * rl_n >= r1) break;
            const int64_t o = (rb + u * rl_n) * stride + ch0;
            Piece<T, VEC>::load(gy + o, gv[u]);
            Piece<T, VEC>::load(raw + o, xv[u]);
            if (act == 1 && y) Piece<T, VEC>::load(y + o, yv[u]);
        }
        // the sums in row order, as before
#pragma unroll
        for (int u = 0; u < U; ++u) {
            if (rb + u * rl_n >= r1) break;
#pragma unroll
            for (int k = 0; k < VEC; ++k) {
                if (act == 1 && !y) {
                    const float t = __fmul_rn(__fsub_rn(xv[u][k], m[k]), sc[k]);
                    yv[u][k] = beta ? __fadd_rn(t, b[k]) : t;
                }
                const float gb = (act == 1 && !(yv[u][k] > 0.0f)) ? 0.0f : gv[u][k];
                const float xh = __fmul_rn(__fsub_rn(xv[u][k], m[k]), inv[k]);
                s1[k] += (double)gb;
                s2[k] += (double)gb * (double)xh;
            }
        }
    }
#pragma unroll
    for (int k = 0; k < VEC; ++k) {
        red[0][threadIdx.x * VEC + k] = s1[k];
        red[1][threadIdx.x * VEC + k] = s2[k];
    }
    __syncthreads();
    for (int ch = threadIdx.x; ch < c; ch += SHPL_BLOCK) {
        const int g2 = ch / VEC, k = ch % VEC;
        double a = 0.0, b = 0.0;
        for (int q = 0; q < rl_n; ++q) {
            a += red[0][(q * cg_n + g2) * VEC + k];
            b += red[1][(q * cg_n + g2) * VEC + k];
        }
        part[((int64_t)blockIdx.x * 2 + 0) * c + ch] = a;
        part[((int64_t)blockIdx.x * 2 + 1) * c + ch] = b;
    }
}

template <typename T, bool ACT, bool HASY, bool BETA, bool TRAIN>
__global__ __launch_bounds__(SHPL_BLOCK) void k_bn_bwd_apply_vec(const T *y, const T *raw, const T *gy,
                                                                 int64_t rows, int64_t stride, int c,
                                                                 const float *mean, const float *scale,
                                                                 const float *gamma, const float *beta,
                                                                 const float *mean_terms, T *graw) {
    constexpr int VEC = 16 / sizeof(T);
    const int pr = c / VEC, rpb = SHPL_BLOCK / pr;
    const int ch0 = (threadIdx.x % pr) * VEC;
    float sc[VEC], m[VEC], inv[VEC], t0[VEC], t1[VEC], b[VEC];
#pragma unroll
    for (int k = 0; k < VEC; ++k) {
        const int ch = ch0 + k;
        b[k] = BETA ? beta[ch] : 0.0f;
        sc[k] = scale ? scale[ch] : 1.0f;
        m[k] = mean ? mean[ch] : 0.0f;
        inv[k] = __fdiv_rn(sc[k], gamma ? gamma[ch] : 1.0f);
        t0[k] = TRAIN ? mean_terms[ch] : 0.0f;
        t1[k] = TRAIN ? mean_terms[c + ch] : 0.0f;
    }
    const int64_t step = (int64_t)gridDim.x * rpb;
    constexpr int U = BN_U / 2;  // two or three streams in per row
    for (int64_t r0 = (int64_t)blockIdx.x * rpb + threadIdx.x / pr; r0 < rows; r0 += U * step) {
        float gv[U][VEC], yv[U][VEC], xv[U][VEC];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            if (r0 + u * step >= rows) break;
            const int64_t o = (r0 + u * step) * stride + ch0;
            Piece<T, VEC>::load(gy + o, gv[u]);
            if constexpr (ACT && HASY) Piece<T, VEC>::load(y + o, yv[u]);
            if constexpr (TRAIN || (ACT && !HASY)) Piece<T, VEC>::load(raw + o, xv[u]);
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            if (r0 + u * step >= rows) break;
            float out[VEC];
#pragma unroll
            for (int k = 0; k < VEC; ++k) {
                if constexpr (ACT && !HASY) {
                    const float t = __fmul_rn(__fsub_rn(xv[u][k], m[k]), sc[k]);
                    yv[u][k] = BETA ? __fadd_rn(t, b[k]) : t;
                }
                const float gb = (ACT && !(yv[u][k] > 0.0f)) ? 0.0f : gv[u][k];
                if constexpr (TRAIN) {
                    const float xh = __fmul_rn(__fsub_rn(xv[u][k], m[k]), inv[k]);
                    out[k] = __fmul_rn(sc[k], __fsub_rn(__fsub_rn(gb, t0[k]), __fmul_rn(xh, t1[k])));
                } else {
                    out[k] = __fmul_rn(sc[k], gb);
                }
            }
            Piece<T, VEC>::store(graw + (r0 + u * step) * stride + ch0, out);
        }
    }
}

// one block per channel (strided_sum / block_sum of shpl_conv_bn.h)
__global__ __launch_bounds__(SHPL_BLOCK) void k_bn_bwd_finalize(const double *part, int n_blocks, int c,
                                                                double count, float *dbeta, float *dgamma,
                                                                float *mean_terms) {
    __shared__ double red[SHPL_BLOCK / 64];
    const int ch = blockIdx.x;
    const double a = block_sum<SHPL_BLOCK>(strided_sum<SHPL_BLOCK>(part + ch, n_blocks, 2 * c, threadIdx.x), red);
    const double b =
        block_sum<SHPL_BLOCK>(strided_sum<SHPL_BLOCK>(part + c + ch, n_blocks, 2 * c, threadIdx.x), red);
    if (threadIdx.x == 0) {
        if (dbeta) dbeta[ch] = (float)a;
        if (dgamma) dgamma[ch] = (float)b;
        mean_terms[ch] = (float)(a / count);
        mean_terms[c + ch] = (float)(b / count);
    }
}

template <typename T>
__global__ __launch_bounds__(SHPL_BLOCK) void k_bn_bwd_apply(const T *y, const T *raw, const T *gy, int64_t rows,
                                                             int64_t stride, int c, const float *mean,
                                                             const float *scale, const float *gamma, const float *beta,
                                                             int act, int training, const float *mean_terms, T *graw) {
    const int64_t total = rows * c;
    for (int64_t t = (int64_t)blockIdx.x * SHPL_BLOCK + threadIdx.x; t < total;
         t += (int64_t)gridDim.x * SHPL_BLOCK) {
        const int64_t r = t / c;
        const int ch = (int)(t - r * c);
        const int64_t o = r * stride + ch;
        const float gb = bn_gbn(y, raw, gy, o, ch, act, mean, scale, beta);
        const float sc = scale ? scale[ch] : 1.0f;
        float v;
        if (training) {
            const float inv = __fdiv_rn(sc, gamma ? gamma[ch] : 1.0f);
            const float xh = __fmul_rn(__fsub_rn(Elem<T>::f(raw[o]), mean ? mean[ch] : 0.0f), inv);
            v = __fmul_rn(sc, __fsub_rn(__fsub_rn(gb, mean_terms[ch]), __fmul_rn(xh, mean_terms[c + ch])));
        } else {
            v = __fmul_rn(sc, gb);
        }
        graw[o] = Elem<T>::back(v);
    }
}

// Whether a call runs the vector kernels: whole 16-byte pieces per row at a 16-byte aligned stride, c / VEC
// piece lanes a power of two of at most a block, and every stream in `ptrs` 16-byte aligned (NULL: not read).
bool bn_vector_form(int dtype, int64_t c, int64_t stride, std::initializer_list<const void *> ptrs) {
    const int vec = dtype == SHPL_F32 ? 4 : 8, pr = (int)(c / vec);
    bool vform = c % vec == 0 && stride % vec == 0 && pr <= SHPL_BLOCK && (pr & (pr - 1)) == 0;
    for (const void *p : ptrs) vform = vform && aligned16(p);
    return vform;
}

// Grid of the apply kernels (forward and backward) in either form.
int bn_apply_grid(int dtype, int64_t rows, int64_t c, bool vform) {
    const int vec = dtype == SHPL_F32 ? 4 : 8;
    return grid_for(rows * c / (vform ? vec : 1), SHPL_BLOCK * bn_rows_per_thread(16 / vec), 1 << 22);
}

}  // namespace
}  // namespace shpl

using namespace shpl;

extern "C" int shpl_batch_norm(int dtype, int64_t rows, void *d_x, void *d_y, int64_t stride, int64_t c,
                               const double *d_stats, double count, float eps, const float *d_gamma,
                               const float *d_beta, int act, float *d_moving_mean, float *d_moving_var, float decay,
                               float *d_batch_mean, float *d_batch_var, float *d_ws, void *stream) {
    if (dtype != SHPL_F32 && dtype != SHPL_BF16) return SHPL_ERR_ARG;
    if (rows < 0 || c < 1 || stride < c || c > (1 << 16)) return SHPL_ERR_BAD_SHAPE;
    if (act != 0 && act != 1) return SHPL_ERR_ARG;
    if (!d_stats || !d_ws || (rows > 0 && !d_x) || !(count > 0.0)) return SHPL_ERR_ARG;
    if (!d_y) d_y = d_x;
    hipStream_t s = (hipStream_t)stream;
    float *mean = d_ws, *scale = d_ws + c;
    hipLaunchKernelGGL(k_bn_finalize, dim3(1), dim3(SHPL_BLOCK), 0, s, d_stats, count, (int)c, eps, d_gamma, mean,
                       scale, d_moving_mean, d_moving_var, decay, d_batch_mean, d_batch_var);
    SHPL_LAUNCH_CHECK();
    if (rows == 0) return SHPL_OK;
    const bool vform = bn_vector_form(dtype, c, stride, {d_x, d_y});
    const int grid = bn_apply_grid(dtype, rows, c, vform);
    auto launch = [&](auto tag) {
        typedef decltype(tag) T;
        if (vform)
            bn_forms([&](auto B, auto A) {
                hipLaunchKernelGGL((k_bn_apply_vec<T, B.value, A.value>), dim3(grid), dim3(SHPL_BLOCK), 0, s,
                                   (const T *)d_x, (T *)d_y, rows, stride, (int)c, mean, scale, d_beta);
            }, d_beta != nullptr, act == 1);
        else
            hipLaunchKernelGGL(k_bn_apply<T>, dim3(grid), dim3(SHPL_BLOCK), 0, s, (const T *)d_x, (T *)d_y, rows,
                               stride, (int)c, mean, scale, d_beta, act);
    };
    dtype == SHPL_F32 ? launch(float()) : launch(uint16_t());
    SHPL_LAUNCH_CHECK();
    return SHPL_OK;
}

extern "C" int shpl_batch_norm_backward_workspace_bytes(int64_t rows, int64_t c, size_t *bytes) {
    if (!bytes || rows < 0 || c < 1) return SHPL_ERR_ARG;
    *bytes = align_up((size_t)bn_bwd_blocks(rows) * 2 * c * sizeof(double), 256) + align_up(2 * c * sizeof(float), 256);
    return SHPL_OK;
}

extern "C" int shpl_batch_norm_backward(int dtype, int64_t rows, const void *d_y, const void *d_raw,
                                        const void *d_gy, int64_t stride, int64_t c, const float *d_mean,
                                        const float *d_scale, const float *d_gamma, const float *d_beta, int act,
                                        int training, void *d_graw, float *d_dbeta, float *d_dgamma, void *d_ws,
                                        size_t ws_bytes, void *stream) {
    if (dtype != SHPL_F32 && dtype != SHPL_BF16) return SHPL_ERR_ARG;
    if (rows < 0 || c < 1 || stride < c || c > (1 << 16)) return SHPL_ERR_BAD_SHAPE;
    if (act != 0 && act != 1) return SHPL_ERR_ARG;
    size_t need;
    shpl_batch_norm_backward_workspace_bytes(rows, c, &need);
    if (!d_ws || ws_bytes < need) return SHPL_ERR_WORKSPACE;
    if (rows > 0 && (!d_gy || !d_graw || (act == 1 && !d_y && !d_raw) || (training && !d_raw))) return SHPL_ERR_ARG;
    if (rows == 0) return SHPL_OK;
    hipStream_t s = (hipStream_t)stream;
    const int nb = bn_bwd_blocks(rows);
    const int64_t rpb = (rows + nb - 1) / nb;
    double *part = reinterpret_cast<double *>(d_ws);
    float *mt = reinterpret_cast<float *>((uint8_t *)d_ws + align_up((size_t)nb * 2 * c * sizeof(double), 256));
    // x-hat needs raw only in training (dgamma); otherwise any row-shaped input stands in
    const void *rw = d_raw ? d_raw : d_gy;
    const bool vform = bn_vector_form(dtype, c, stride, {d_gy, rw, d_graw, d_y});
    // y NULL: the ReLU mask from raw (bn_pre_act), so only the y argument of the kernels changes
    const float *beta = act == 1 && !d_y ? d_beta : nullptr;
    const int grid = bn_apply_grid(dtype, rows, c, vform);
    auto launch = [&](auto tag) {
        typedef decltype(tag) T;
        const T *y = (const T *)d_y, *r = (const T *)rw, *g = (const T *)d_gy;
        if (vform)
            // (its switches as template arguments measured slower: 785 vs 747 us, profiles/r04_bn_ab.log)
            hipLaunchKernelGGL(k_bn_bwd_partial_vec<T>, dim3(nb), dim3(SHPL_BLOCK), 0, s, y, r, g, rows, stride,
                               (int)c, d_mean, d_scale, d_gamma, beta, act, rpb, part);
        else
            hipLaunchKernelGGL(k_bn_bwd_partial<T>, dim3(nb), dim3(SHPL_BLOCK), 0, s, y, r, g, rows, stride, (int)c,
                               d_mean, d_scale, d_gamma, beta, act, rpb, part);
        hipLaunchKernelGGL(k_bn_bwd_finalize, dim3((unsigned)c), dim3(SHPL_BLOCK), 0, s, part, nb,
                           (int)c, (double)rows, d_dbeta, d_raw ? d_dgamma : nullptr, mt);
        if (vform)
            bn_forms([&](auto A, auto Y, auto B, auto TR) {
                hipLaunchKernelGGL((k_bn_bwd_apply_vec<T, A.value, Y.value, B.value, TR.value>), dim3(grid),
                                   dim3(SHPL_BLOCK), 0, s, y, r, g, rows, stride, (int)c, d_mean, d_scale, d_gamma,
                                   beta, mt, (T *)d_graw);
            }, act == 1, d_y != nullptr, beta != nullptr, training != 0);
        else
            hipLaunchKernelGGL(k_bn_bwd_apply<T>, dim3(grid), dim3(SHPL_BLOCK), 0, s, y, r, g, rows, stride, (int)c,
                               d_mean, d_scale, d_gamma, beta, act, training, mt, (T *)d_graw);
    };
    dtype == SHPL_F32 ? launch(float()) : launch(uint16_t());
    SHPL_LAUNCH_CHECK();
    return SHPL_OK;
}
