// shpl_conv_tile.h -- what the tiled kernels COMPUTE and WRITE per tile, each step once (k_conv3x3 in shpl_conv.hip;
// k_upconv3x3 in shpl_upconv.hip; k_upconv3x3_dgrad and k_upconv3x3_wgrad in shpl_upconv_grad.hip): the tile's frame
// and origin, the kernel arguments read again, the MFMA step of one tap, the epilogue of one row of 32 pixels x 32
// channels (coefficients, rounding, the LDS transpose, the stores) and the per-channel batch statistics of a tile.
// A header of its own, beside shpl_conv_stage.h (what a tile reads, and the host's helpers), so that a change to
// the store path or to the statistics' order is made in a file that holds nothing else.
//
// These kernels sit at the edge of the scalar register file: every step takes the ConvArgs it is to read -- the
// kernel's own, or a copy read again after the K loop -- and a caller builds what it hands in (the address
// callable, an opaque thread index) where the step runs, not before the K loop.
#pragma once

#include <type_traits>

#include "shpl_conv_stage.h"

namespace shpl {
namespace {

// Frame and origin of tile `tile` of the TH_ x TW tiling. OPAQUE: worked out from an opaque copy of the index,
// for a kernel that works them out again wherever it reads its arguments again, instead of holding them in three
// scalar registers across the tile's steps.
template <int TH_, bool OPAQUE = false>
__device__ __forceinline__ void tile_origin(const ConvArgs &p, int tile, int &f, int &y0, int &x0) {
    if constexpr (OPAQUE) asm volatile("" : "+s"(tile));
    f = tile / p.tiles_per_frame;
    const int t_in = tile - f * p.tiles_per_frame;
    const int ty = t_in / p.tiles_x, tx = t_in - ty * p.tiles_x;
    y0 = ty * TH_;
    x0 = tx * TW;
}

// A kernel argument read again from the kernel-argument segment (at: its byte offset there), word by word, through
// a pointer the compiler cannot see through: read once at the kernel's start the arguments would sit in scalar
// registers across the whole K loop (and spill).
template <typename S>
__device__ __forceinline__ S kernarg_again(unsigned at) {
    static_assert(sizeof(S) % 4 == 0, "whole words");
    uint64_t kargs = (uint64_t)__builtin_amdgcn_kernarg_segment_ptr();
    asm volatile("" : "+s"(kargs));
    const __attribute__((address_space(4))) uint32_t *src =
        (const __attribute__((address_space(4))) uint32_t *)(kargs + at);
    uint32_t w[sizeof(S) / 4];
#pragma unroll
    for (unsigned i = 0; i < sizeof(S) / 4; ++i) w[i] = src[i];
    S out;
    __builtin_memcpy(&out, w, sizeof(S));
    return out;
}

// One tap of the 32 x 32 implicit GEMM: a lane's 16-byte piece of a chunk's LDS row is its MFMA operand -- lane half
// h supplies channels 4h+s of the chunk to MFMA s of four v_mfma_f32_32x32x2_f32 (f32, both operands), channels
// 8h .. 8h+7 to one v_mfma_f32_32x32x16_bf16 (bf16). b: the weights' row, a: the pixel's.
template <typename T>
using Frag = std::conditional_t<sizeof(T) == 4, f32x4, bf16x8>;

template <typename T>
__device__ __forceinline__ Frag<T> lds_frag(const uint8_t *at) {
    return *reinterpret_cast<const Frag<T> *>(at);
}

template <typename T>
__device__ __forceinline__ f32x16 mfma_tap(Frag<T> b, Frag<T> a, f32x16 acc) {
    if constexpr (sizeof(T) == 4) {
#pragma unroll
        for (int s = 0; s < 4; ++s) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(b[s], a[s], acc, 0, 0, 0);
    } else {
        acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(b, a, acc, 0, 0, 0);
    }
    return acc;
}

// Epilogue coefficients of the NCB output blocks from cob0 into s_par, as k_conv_rows: scale (1 when absent) and
// shift - center * scale, applied as one fma -- the kernels give the same bits for the same call. Published by the
// caller's next barrier.
template <int NCB>
__device__ __forceinline__ void epilogue_coeffs(const ConvArgs &p, int cob0, float (*s_par)[2][NCO], int tid) {
    if (tid < NCO * NCB) {
        const int cb = tid / NCO, c = (cob0 + cb) * NCO + (tid & 31);
        const bool in = c < p.c_out;
        const float sc = p.scale && in ? p.scale[c] : 1.0f;
        const float ce = p.center && in ? p.center[c] : 0.0f;
        const float sh = p.shift && in ? p.shift[c] : 0.0f;
        s_par[cb][0][tid & 31] = sc;
        s_par[cb][1][tid & 31] = __fsub_rn(sh, __fmul_rn(ce, sc));
    }
}

// Where channel c of output pixel `row` is stored: in out, or -- the input gradients' second map -- in out2 as
// channel c - c_split (the host sets c_split = c_out when there is no second map).
template <typename T>
__device__ __forceinline__ T *out_ptr(const ConvArgs &p, int64_t row, int c) {
    return p.out2 && c >= p.c_split ? reinterpret_cast<T *>(p.out2) + row * p.out2_stride + (c - p.c_split)
                                    : reinterpret_cast<T *>(p.out) + row * p.out_stride + c;
}

// The lane's running sums of the pre-activation values and of their squares (STATS), element i as the accumulator's.
// Vectors, handed to the steps below as values: arrays handed on by reference stay in memory until late in the
// compilation, which cost these kernels registers and scratch.
struct ChanSums {
    f32x16 s1, s2;
    __device__ __forceinline__ void zero() {
#pragma unroll
        for (int i = 0; i < 16; ++i) s1[i] = s2[i] = 0.0f;
    }
    // one pixel's values, if it lies inside the map
    __device__ __forceinline__ void add(f32x16 v, bool ok) {
        f32x16 n1, n2;
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            n1[i] = __fadd_rn(s1[i], v[i]);
            n2[i] = __fadd_rn(s2[i], __fmul_rn(v[i], v[i]));
        }
        s1 = ok ? n1 : s1;
        s2 = ok ? n2 : s2;
    }
};

// The epilogue's LDS rows: a pixel's 32 channels and 16 bytes of padding; 32 rows per wave.
template <typename T>
constexpr int OPITCH = NCO * (int)sizeof(T) + 16;

// The epilogue of one accumulator. The MFMAs take the weights as A and the pixels as B (D = W^T X^T), so element i
// of acc is channel c0 + 8(i>>2) + 4h + (i&3) of the pixel at column pl of the tile (lane = 32 h + pl): four runs
// of 4 channels per lane. AFFINE: each value through fma(v, scale, shift') of par (a block's s_par) and ReLU
// (p.act); rounded once. The row of 32 pixels then goes through LDS (s_o: wave-private, rows of OPITCH bytes) and
// out as 16-byte pieces, consecutive lanes on consecutive pieces: 2 (bf16) / 4 (f32) store instructions per row,
// each one contiguous 1 KB where the pixels are, instead of 16 two- or four-byte stores (the texture addresser was
// the bf16 conv's busiest unit). Blocks whose channels are not whole or whose rows are not 16-byte aligned
// (p.vec_out) store channel by channel. y_in: the row lies in the map (its columns: x0 + column < W); at(p, column
// of the tile, channel): where that value goes (p handed on, so that the callable holds no ConvArgs of its own).
// STATS: the values of pixels inside the map are added to *sums before the fma -- the callers' order of rows is
// the statistics' summation order.
template <typename T, bool AFFINE, bool STATS, typename At>
__device__ __forceinline__ void epilogue_row(const ConvArgs &p, f32x16 acc, const float (*par)[NCO],
                                             uint8_t *s_o, int c0, bool y_in, int x0, int W, ChanSums *sums, At at) {
    typedef Elem<T> E;
    constexpr int HE = E::HE, PPP = NCO / HE;  // channels per piece, pieces per pixel
    const int lane = threadIdx.x & 63, pl = lane & 31, hf = lane >> 5;
    // the block's first channel, opaque per row: what hangs on it alone -- each channel's bound and map, 16 of them
    // on the channel-by-channel path -- is then worked out where a row stores, as it would be inside the callers'
    // loops, instead of once ahead of them and kept in registers across all their rows
    asm volatile("" : "+s"(c0));
    const bool fast = p.vec_out && c0 + NCO <= p.c_out;
    const bool ok = y_in && x0 + pl < W;
    if constexpr (STATS) sums->add(acc, ok);
#pragma unroll
    for (int g = 0; g < 4; ++g) {
        const int cl = 8 * g + 4 * hf, c = c0 + cl;  // first channel of the run
        f32x4 scl, sft;
        if constexpr (AFFINE) {
            scl = *reinterpret_cast<const f32x4 *>(&par[0][cl]);
            sft = *reinterpret_cast<const f32x4 *>(&par[1][cl]);
        }
        T o[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const float v = acc[4 * g + j];
            if constexpr (AFFINE)
                o[j] = relu_bits(E::back(__builtin_fmaf(v, scl[j], sft[j])), p.act == 1);
            else
                o[j] = E::back(v);
        }
        if (fast) {
            __builtin_memcpy(s_o + pl * OPITCH<T> + cl * sizeof(T), o, sizeof(o));
        } else if (ok) {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                if (c + j >= p.c_out) break;
                *at(p, pl, c + j) = o[j];
            }
        }
    }
    if (fast) {
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // the wave's row is in LDS (one wave: in order)
#pragma unroll
        for (int k = 0; k < 32 * PPP / 64; ++k) {
            const int pc = lane + 64 * k, px = pc / PPP, pi = pc % PPP;
            const u32x4 v = *reinterpret_cast<const u32x4 *>(s_o + px * OPITCH<T> + pi * 16);
            if (y_in && x0 + px < W) *reinterpret_cast<u32x4 *>(at(p, px, c0 + pi * HE)) = v;
        }
    }
}

// The sum of each of a lane's N values over the 32 lanes of its half of the wave, by a halving butterfly: each
// exchange hands the partner the half of the values it keeps (8 + 4 + 2 + 1 + 1 shuffles for 16 values instead of
// 16 x 5), after which lanes 2j and 2j+1 both hold value j. pl: the lane's index in its half.
template <int N>
__device__ __forceinline__ float half_wave_sums(float __attribute__((ext_vector_type(N))) v, int pl) {
    const bool up = (pl & N) != 0;
    if constexpr (N == 2) {
        const float s = __fadd_rn(up ? v[1] : v[0], __shfl_xor(up ? v[0] : v[1], 2, 64));
        return __fadd_rn(s, __shfl_xor(s, 1, 64));
    } else {
        const auto give = up ? v.lo : v.hi, keep = up ? v.hi : v.lo;
        float __attribute__((ext_vector_type(N / 2))) out;
#pragma unroll
        for (int i = 0; i < N / 2; ++i) out[i] = __fadd_rn(keep[i], __shfl_xor(give[i], N, 64));
        return half_wave_sums<N / 2>(out, pl);
    }
}

// The tile's statistics of the 32 channels from c0: each channel's sums over the 32 pixels of the lane half
// (half_wave_sums), then over the 4 waves in double (s_red), into the tile's partial. tid: the thread's index for
// that last step (a caller may hand it in opaque, so that `tid < 64` is not kept as a lane mask from the kernel's
// start).
__device__ __forceinline__ void stats_reduce_tile(const ConvArgs &p, ChanSums s, float (*s_red)[2][NCO], int tid,
                                                  int c0, int tile) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, pl = lane & 31, hf = lane >> 5;
    const float t1 = half_wave_sums<16>(s.s1, pl), t2 = half_wave_sums<16>(s.s2, pl);
    if ((pl & 1) == 0) {
        const int i = pl >> 1, cl = 8 * (i >> 2) + 4 * hf + (i & 3);
        s_red[wave][0][cl] = t1;
        s_red[wave][1][cl] = t2;
    }
    __syncthreads();
    if (tid < 2 * NCO) {
        const int st = tid >> 5, c = tid & 31;
        double sum = 0.0;
        for (int w = 0; w < 4; ++w) sum += (double)s_red[w][st][c];
        p.part[((int64_t)(c0 + c) * 2 + st) * p.n_tiles + tile] = sum;
    }
}

}  // namespace
}  // namespace shpl
