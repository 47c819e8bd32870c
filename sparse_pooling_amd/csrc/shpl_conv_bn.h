// shpl_conv_bn.h -- the few pieces the conv (shpl_conv.hip) and BatchNorm (shpl_bn.hip) share: the element
// conversions, the deterministic sums of their f64 partials.
#pragma once

#include "shpl_common.h"

namespace shpl {

namespace {

// One chunk = the input channels staged per LDS round, 32 B per pixel: 8
// f32 channels (4 f32 MFMAs of K=2 per tap) or 16 bf16 channels (one bf16
// MFMA of K=16 per tap). 64 B bf16 chunks measured slower (fewer workgroups
// per CU).
template <typename T>
struct Elem {
    static constexpr int CB = 32;                        // chunk bytes per pixel
    static constexpr int CK = CB / sizeof(T);            // channels per chunk
    static constexpr int HE = 16 / sizeof(T);            // channels per 16-byte piece
    static constexpr int NP = CB / 16;                   // pieces per pixel
    static __device__ __forceinline__ float f(T v) {
        if constexpr (sizeof(T) == 4)
            return v;
        else
            return bf16_to_f32(v);
    }
    static __device__ __forceinline__ T back(float v) {
        if constexpr (sizeof(T) == 4)
            return v;
        else
            return f32_to_bf16(v);
    }
};

// Deterministic sums of long strided lists (the per-tile / per-block /
// per-group partials): thread t adds elements t, t + n_thr, ... into 8
// independent accumulators (8 loads in flight, then a fixed pairwise
// combine), the wave and the block then reduce in a fixed order. A thread per
// list walking it serially (550-4096 dependent loads) cost 0.2-0.3 ms per
// reduction.
template <int NT>
__device__ __forceinline__ double strided_sum(const double *v, int64_t n, int64_t step, int t) {
    double acc[8] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    int64_t i = t;
    for (; i + 7 * NT < n; i += 8 * NT) {
#pragma unroll
        for (int u = 0; u < 8; ++u) acc[u] += v[(i + u * NT) * step];
    }
    for (int u = 0; i < n; i += NT, ++u) acc[u & 7] += v[i * step];
    return ((acc[0] + acc[1]) + (acc[2] + acc[3])) + ((acc[4] + acc[5]) + (acc[6] + acc[7]));
}

// Block sum of one double per thread (fixed order); valid in thread 0.
template <int NT>
__device__ __forceinline__ double block_sum(double s, double *red) {
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0)
        for (int w = 1; w < NT / 64; ++w) s += red[w];
    __syncthreads();
    return s;
}

// BatchNorm (training) from the batch statistics [sum x, sum x^2] (c each): mean, biased variance (clamped
// at 0) for the normalisation, Bessel-corrected variance for the moving average (TF FusedBatchNorm); mean and
// scale = gamma / sqrt(var + eps) are left for the apply kernels (shpl_bn.hip, shpl_concat_bn.hip).
__global__ __launch_bounds__(SHPL_BLOCK) void k_bn_finalize(const double *stats, double count, int c, float eps,
                                                            const float *gamma, float *mean_out, float *scale_out,
                                                            float *moving_mean, float *moving_var, float decay,
                                                            float *batch_mean, float *batch_var) {
    for (int ch = threadIdx.x; ch < c; ch += SHPL_BLOCK) {
        const double mean = stats[ch] / count;
        double var = stats[c + ch] / count - mean * mean;
        if (var < 0.0) var = 0.0;
        const float mf = (float)mean, vf = (float)var;
        const float g = gamma ? gamma[ch] : 1.0f;
        mean_out[ch] = mf;
        scale_out[ch] = __fmul_rn(g, __fdiv_rn(1.0f, __fsqrt_rn(__fadd_rn(vf, eps))));
        const float vu = count > 1.0 ? (float)(var * count / (count - 1.0)) : vf;
        if (moving_mean) moving_mean[ch] = __fsub_rn(moving_mean[ch], __fmul_rn(__fsub_rn(moving_mean[ch], mf), 1.0f - decay));
        if (moving_var) moving_var[ch] = __fsub_rn(moving_var[ch], __fmul_rn(__fsub_rn(moving_var[ch], vu), 1.0f - decay));
        if (batch_mean) batch_mean[ch] = mf;
        if (batch_var) batch_var[ch] = vu;
    }
}

// Blocks of the per-channel partial sums over `rows` rows (the BatchNorm backward's, the fused concat's
// statistics): 4096 rows each, at most 1024 blocks.
inline int bn_bwd_blocks(int64_t rows) {
    int64_t nb = (rows + 4095) / 4096;
    if (nb < 1) nb = 1;
    if (nb > 1024) nb = 1024;
    return (int)nb;
}

}  // namespace
}  // namespace shpl
