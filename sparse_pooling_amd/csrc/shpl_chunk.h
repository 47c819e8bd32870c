// shpl_chunk.h -- the pulls' work unit, shared by shpl_pull.hip and shpl_concat_bn.hip: one chunk of VEC
// elements of a feature row (16 bytes: 4 f32 / 8 bf16 under the pull's alignment rule, else one element), its
// loads and stores and its conversions to and from f32.
#pragma once

#include "shpl_common.h"

namespace shpl {
namespace {

typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));


template <int BYTES>
struct Raw;
template <>
struct Raw<16> {
    typedef u32x4 type;
};
template <>
struct Raw<8> {
    typedef u32x2 type;
};
template <>
struct Raw<4> {
    typedef uint32_t type;
};
template <>
struct Raw<2> {
    typedef uint16_t type;
};

template <typename T, int VEC>
struct Chunk {
    typedef typename Raw<sizeof(T) * VEC>::type raw_t;

    static __device__ __forceinline__ raw_t load(const T *p) { return *reinterpret_cast<const raw_t *>(p); }
    static __device__ __forceinline__ raw_t load_nt(const T *p) {
        return __builtin_nontemporal_load(reinterpret_cast<const raw_t *>(p));
    }
    static __device__ __forceinline__ void store_nt(T *p, raw_t v) {
        __builtin_nontemporal_store(v, reinterpret_cast<raw_t *>(p));
    }
    static __device__ __forceinline__ void to_f32(raw_t r, float (&x)[VEC]) {
        T e[VEC];
        __builtin_memcpy(e, &r, sizeof(r));
#pragma unroll
        for (int j = 0; j < VEC; ++j) x[j] = cvt(e[j]);
    }
    static __device__ __forceinline__ raw_t from_f32(const float (&x)[VEC]) {
        T e[VEC];
#pragma unroll
        for (int j = 0; j < VEC; ++j) e[j] = back(x[j]);
        raw_t r;
        __builtin_memcpy(&r, e, sizeof(r));
        return r;
    }
    static __device__ __forceinline__ raw_t zero() {
        raw_t r;
        __builtin_memset(&r, 0, sizeof(r));
        return r;
    }
    static __device__ __forceinline__ float cvt(float v) { return v; }
    static __device__ __forceinline__ float cvt(uint16_t v) { return bf16_to_f32(v); }
    static __device__ __forceinline__ T back(float v) {
        if constexpr (sizeof(T) == 4)
            return v;
        else
            return f32_to_bf16(v);
    }
};

}  // namespace
}  // namespace shpl
