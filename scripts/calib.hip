// Calibration kernels for the pull sweep (not part of libshpl): the best a
// plain streaming kernel does on this box for the same traffic shapes.
#include <hip/hip_runtime.h>
#include <stdint.h>
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

template <int U, bool NT>
__global__ __launch_bounds__(256) void k_copy(const u32x4 *__restrict__ s, u32x4 *__restrict__ d, uint64_t n) {
    uint64_t i0 = ((uint64_t)blockIdx.x * 256 + threadIdx.x);
    const uint64_t step = (uint64_t)gridDim.x * 256;
    for (; i0 < n; i0 += U * step) {
        u32x4 v[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const uint64_t i = i0 + u * step;
            if (i < n) v[u] = NT ? __builtin_nontemporal_load(s + i) : s[i];
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const uint64_t i = i0 + u * step;
            if (i < n) {
                if (NT) __builtin_nontemporal_store(v[u], d + i); else d[i] = v[u];
            }
        }
    }
}

// out row r (cpr chunks): first cpass chunks copied from src row r, rest zero
template <bool NT>
__global__ __launch_bounds__(256) void k_concat_zero(const u32x4 *__restrict__ s, u32x4 *__restrict__ d, uint32_t rows,
                                                     uint32_t cpr, uint32_t cpass) {
    const uint32_t total = rows * cpr;
    for (uint32_t g = blockIdx.x * 256 + threadIdx.x; g < total; g += gridDim.x * 256) {
        const uint32_t r = g / cpr, c = g - r * cpr;
        u32x4 v = {0, 0, 0, 0};
        if (c < cpass) v = NT ? __builtin_nontemporal_load(s + (uint64_t)r * cpass + c) : s[(uint64_t)r * cpass + c];
        if (NT) __builtin_nontemporal_store(v, d + g); else d[g] = v;
    }
}

// zero fill only
__global__ __launch_bounds__(256) void k_zero(u32x4 *__restrict__ d, uint64_t n) {
    for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (uint64_t)gridDim.x * 256) {
        u32x4 z = {0, 0, 0, 0};
        __builtin_nontemporal_store(z, d + i);
    }
}

// Pass-only row copy (scripts/calib_copy_rows.py): chunk g of the source (contiguous rows of 1 << shift
// chunks) goes to chunk (g >> shift) * ocpr + (g & mask) of the output; ocpr = 1 << shift is the plain copy.
// 28 bytes of kernarg. A workgroup owns U adjacent blocks of B chunks: chunk = block * B * U + u * B + t.
// Whole workgroups run unguarded, so a thread's U loads issue back to back; the last one is guarded.
// LNT / SNT: non-temporal loads / stores.
template <int U, int B, bool LNT, bool SNT>
__global__ __launch_bounds__(B) void k_copy_rows(const u32x4 *__restrict__ s, u32x4 *__restrict__ d, uint32_t n,
                                                 uint32_t shift, uint32_t ocpr) {
    const uint32_t g0 = blockIdx.x * (uint32_t)(B * U) + threadIdx.x;
    const uint32_t mask = (1u << shift) - 1u;
    u32x4 v[U];
    if (n - blockIdx.x * (uint32_t)(B * U) >= (uint32_t)(B * U)) {
#pragma unroll
        for (int u = 0; u < U; ++u) v[u] = LNT ? __builtin_nontemporal_load(s + (g0 + u * B)) : s[g0 + u * B];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const uint32_t g = g0 + u * B;
            u32x4 *p = d + ((uint64_t)(g >> shift) * ocpr + (g & mask));
            if (SNT) __builtin_nontemporal_store(v[u], p); else *p = v[u];
        }
        return;
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
        const uint32_t g = g0 + u * B;
        if (g >= n) break;
        const u32x4 w = LNT ? __builtin_nontemporal_load(s + g) : s[g];
        u32x4 *p = d + ((uint64_t)(g >> shift) * ocpr + (g & mask));
        if (SNT) __builtin_nontemporal_store(w, p); else *p = w;
    }
}

// The one-chunk-per-thread form of k_copy_rows (non-temporal both ways) under other launch shapes: B threads
// per workgroup, at most W waves per SIMD (8: no limit), XCD: workgroup ids remapped so that each of the 8
// XCDs (which take workgroups round-robin by id) walks one contiguous eighth of the rows (the grid is a
// multiple of 8).
template <int B, int W, bool XCD>
__global__ __launch_bounds__(B) __attribute__((amdgpu_waves_per_eu(W, W)))
void k_copy_rows_shape(const u32x4 *__restrict__ s, u32x4 *__restrict__ d, uint32_t n, uint32_t shift, uint32_t ocpr) {
    uint32_t b = blockIdx.x;
    if (XCD) b = (b & 7u) * (gridDim.x >> 3) + (b >> 3);
    const uint32_t g = b * (uint32_t)B + threadIdx.x;
    if (g >= n) return;
    const u32x4 v = __builtin_nontemporal_load(s + g);
    __builtin_nontemporal_store(v, d + ((uint64_t)(g >> shift) * ocpr + (g & ((1u << shift) - 1u))));
}

extern "C" int calib_copy_rows_shape(const void *s, void *d, uint32_t n, uint32_t shift, uint32_t ocpr, int block,
                                     int waves, int xcd, void *stream) {
    hipStream_t st = (hipStream_t)stream;
    if (n == 0) return 0;
    if (n > 0x80000000u) return 1;
    unsigned grid = (unsigned)(((uint64_t)n + block - 1) / block);
    if (xcd) grid = (grid + 7u) & ~7u;
#define LS(B, W, X)                                                                                         \
    if (block == B && waves == W && (xcd != 0) == X) {                                                      \
        hipLaunchKernelGGL((k_copy_rows_shape<B, W, X>), dim3(grid), dim3(B), 0, st, (const u32x4 *)s, (u32x4 *)d, n,   \
                           shift, ocpr);                                                                    \
        return hipGetLastError() == hipSuccess ? 0 : 3;                                                     \
    }
    LS(64, 8, false) LS(128, 8, false) LS(256, 8, false) LS(1024, 8, false)
    LS(256, 2, false) LS(256, 3, false) LS(256, 4, false) LS(256, 5, false) LS(256, 6, false)
    LS(256, 8, true) LS(256, 4, true) LS(128, 8, true)
    LS(256, 7, false) LS(256, 5, true) LS(256, 6, true) LS(256, 7, true) LS(128, 6, true) LS(512, 8, true) LS(64, 8, true)
#undef LS
    return 1;
}

// n < 2^31 chunks; policy: bit 0 non-temporal loads, bit 1 non-temporal stores
extern "C" int calib_copy_rows(const void *s, void *d, uint32_t n, uint32_t shift, uint32_t ocpr, int unroll, int block,
                               int policy, void *stream) {
    hipStream_t st = (hipStream_t)stream;
    if (n == 0) return 0;
    if (n > 0x80000000u || (block != 256 && block != 512) || policy < 0 || policy > 3) return 1;
    const unsigned grid = (unsigned)(((uint64_t)n + (uint64_t)block * unroll - 1) / ((uint64_t)block * unroll));
#define L4(U, B, LN, SN)                                                                                    \
    hipLaunchKernelGGL((k_copy_rows<U, B, LN, SN>), dim3(grid), dim3(B), 0, st, (const u32x4 *)s, (u32x4 *)d, n, shift, \
                       ocpr)
#define L3(U, B)                                                                                            \
    do {                                                                                                    \
        if (policy == 0) L4(U, B, false, false);                                                            \
        else if (policy == 1) L4(U, B, true, false);                                                        \
        else if (policy == 2) L4(U, B, false, true);                                                        \
        else L4(U, B, true, true);                                                                          \
    } while (0)
#define L2(U)                                                                                               \
    do {                                                                                                    \
        if (block == 256) L3(U, 256); else L3(U, 512);                                                      \
    } while (0)
    if (unroll == 1) L2(1);
    else if (unroll == 2) L2(2);
    else if (unroll == 4) L2(4);
    else if (unroll == 8) L2(8);
    else return 1;
#undef L2
#undef L3
#undef L4
    return hipGetLastError() == hipSuccess ? 0 : 3;
}

extern "C" int calib_copy(const void *s, void *d, uint64_t n16, int unroll, int nt, int grid, void *stream) {
    hipStream_t st = (hipStream_t)stream;
    if (grid <= 0) grid = (int)((n16 + 256ull * unroll - 1) / (256ull * unroll));
#define L(U, N) hipLaunchKernelGGL((k_copy<U, N>), dim3(grid), dim3(256), 0, st, (const u32x4 *)s, (u32x4 *)d, n16)
    if (unroll == 1) { if (nt) L(1, true); else L(1, false); }
    else if (unroll == 2) { if (nt) L(2, true); else L(2, false); }
    else { if (nt) L(4, true); else L(4, false); }
#undef L
    return hipGetLastError() == hipSuccess ? 0 : 3;
}

extern "C" int calib_concat_zero(const void *s, void *d, uint32_t rows, uint32_t cpr, uint32_t cpass, int nt, int grid,
                                 void *stream) {
    hipStream_t st = (hipStream_t)stream;
    if (grid <= 0) grid = (int)(((uint64_t)rows * cpr + 255) / 256);
    if (nt) hipLaunchKernelGGL(k_concat_zero<true>, dim3(grid), dim3(256), 0, st, (const u32x4 *)s, (u32x4 *)d, rows, cpr, cpass);
    else hipLaunchKernelGGL(k_concat_zero<false>, dim3(grid), dim3(256), 0, st, (const u32x4 *)s, (u32x4 *)d, rows, cpr, cpass);
    return hipGetLastError() == hipSuccess ? 0 : 3;
}

extern "C" int calib_zero(void *d, uint64_t n16, int grid, void *stream) {
    if (grid <= 0) grid = (int)((n16 + 255) / 256);
    hipLaunchKernelGGL(k_zero, dim3(grid), dim3(256), 0, (hipStream_t)stream, (u32x4 *)d, n16);
    return hipGetLastError() == hipSuccess ? 0 : 3;
}
