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

}  // namespace
}  // namespace shpl
