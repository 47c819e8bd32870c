// shpl_conv_stage.h -- what the tiled kernels over [a || pooled b] READ, and the host's helpers (shpl_conv.hip: the
// 3x3 conv, its gradients; shpl_upconv.hip, shpl_upconv_grad.hip: the stride-2 transposed conv and its): the kernel
// arguments, the staging of one chunk's weight rows and of one input chunk of a tile's halo into LDS -- dense chunks
// by LDS-DMA, pooled chunks summed from the CSR's runs in the pull's order -- the weight packing, the row pointers
// over a destination-sorted CSR, the statistics reduction, and on the host the kernel arguments every form fills,
// the small launches and the form selection. What a tile computes and writes is in shpl_conv_tile.h. The halo tile
// starts one row above and one column left of the output tile; its size (HH_ x HWD_) is a template parameter that
// defaults to the 3x3 conv's (TH + 2) x (TW + 2).
#pragma once

#include "shpl_conv_bn.h"

namespace shpl {
namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));

// Output rows per wave: 2 at both dtypes (8 x 32 tiles). Tried for bf16 and not shipped: 4 rows per wave (16 x 32
// tiles: half the staging round trips, halo rows and weight rows per output pixel, each A operand reused for up
// to three kernel rows); its timings are not recorded in docs/HISTORY.md or profiles/.
constexpr int RPW = 2;
constexpr int TH = 4 * RPW, TW = 32;        // output tile (rows x columns)
constexpr int HH = TH + 2, HWD = TW + 2;    // halo tile
constexpr int NCO = 32;                     // output channels per workgroup
constexpr int CONV_BLOCK = 256;             // 4 waves, wave w: tile rows 2w, 2w+1
constexpr int W_ROWS = 9 * NCO;             // weight rows of a chunk (tap, out channel)

// ReLU of a stored value as max(bits, 0) on its bit pattern as a signed integer of its width: negatives,
// -0 and -NaN become +0, +NaN stays -- k_conv_rows' packed 16-bit max, so both kernels give the same bits.
__device__ __forceinline__ float relu_bits(float v, bool on) {
    const int32_t b = __float_as_int(v);
    return on ? __int_as_float(b > 0 ? b : 0) : v;
}
__device__ __forceinline__ uint16_t relu_bits(uint16_t v, bool on) {
    return on ? ((int16_t)v > 0 ? v : (uint16_t)0) : v;
}

struct ConvArgs {
    int n_frames, h, w;
    int tiles_x, tiles_per_frame, n_tiles;
    const void *a;
    int64_t a_stride, a_off;
    int c_a, qa;  // channels of A, chunks of A
    const void *b;
    int64_t b_stride, b_off;
    int c_b, qb;
    bool vec_a, vec_b;  // 16-byte aligned rows and offsets
    // POOLED: B rows are read through the pool's CSR -- image pixels through the cell-keyed one; BEV cells
    // through the pixel-keyed one, whose ent_col (when set) groups each run by column (GROUP)
    const int32_t *ent_dst, *ent_src, *ent_col, *row_ptr;
    const float *ent_val;
    const void *wp;  // packed weights [co_block][chunk][tap][32][CK]
    const float *center, *scale, *shift;
    int act;
    void *out;
    int64_t out_stride;
    int c_out;
    // channels >= c_split go to out2 (channel co - c_split), when out2 is set
    void *out2;
    int64_t out2_stride;
    int c_split;
    const uint32_t *occ2;  // rows form: out2 written only at the cells set in these occupancy words (NULL: all)
    bool vec_out;  // out (and out2) rows and c_split 16-byte aligned: 16-byte stores
    double *part;  // STATS: [(co_block*32 + co)*2 + stat][n_tiles]
};

// 16 bytes of channels [c, c + HE) of one row, channels >= c_src read as 0.
template <typename T>
__device__ __forceinline__ u32x4 load_piece(const T *row, int c, int c_src, bool vec) {
    constexpr int HE = Elem<T>::HE;
    if (vec && c + HE <= c_src) return *reinterpret_cast<const u32x4 *>(row + c);
    T e[HE];
#pragma unroll
    for (int j = 0; j < HE; ++j) e[j] = c + j < c_src ? row[c + j] : T(0);
    u32x4 r;
    __builtin_memcpy(&r, e, 16);
    return r;
}

// A 16-byte word of zeros in global memory: the LDS-DMA source of pieces
// outside the map (an LDS-DMA writes what it reads; it cannot write zeros).
__device__ u32x4 g_zero_piece;

// One LDS-DMA of 16 bytes per lane: lane l's piece lands at wave_dst + 16 l.
__device__ __forceinline__ void dma16(const void *src, uint8_t *wave_dst) {
    __builtin_amdgcn_global_load_lds(reinterpret_cast<const u32x4 *>(src), wave_dst, 16, 0, 0);
}

// Piece g (0/1) of LDS row `row` (32-byte rows: two 16-byte pieces). SWZ: the
// unpadded, swizzled image the forward conv reads with ds_read_b128 -- slot
// 2 row + (g ^ bit 3 of row): any 16 consecutive rows of one half fall on 16
// distinct bank quads -- which an LDS-DMA can fill (its destination is
// lane-linear; the swizzle goes on the source side). Otherwise rows of PSTR bytes.
template <bool SWZ, int PSTR>
__device__ __forceinline__ int piece_off(int row, int g) {
    if constexpr (SWZ)
        return (2 * row + (g ^ ((row >> 3) & 1))) * 16;
    else
        return row * PSTR + g * 16;
}

// The piece of channels [c, c + HE) of `row` (NULL: outside the map) into the
// lane's LDS slot: an LDS-DMA when the piece is whole or all padding, a
// masked load + ds_write when it straddles the channel count (or the rows are
// not 16-byte aligned).
template <typename T>
__device__ __forceinline__ void piece_to_lds(const T *row, int c, int c_src, bool vec, uint8_t *wave_dst, int lane) {
    constexpr int HE = Elem<T>::HE;
    if (!row || c >= c_src || (vec && c + HE <= c_src))
        dma16(row && c < c_src ? static_cast<const void *>(row + c) : &g_zero_piece, wave_dst);
    else
        *reinterpret_cast<u32x4 *>(wave_dst + lane * 16) = load_piece<T>(row, c, c_src, vec);
}

// One 16-byte piece (channels [c, c + HE)) of an occupied cell's pooled vector, written to the cell's LDS
// row: the sum over the cell's run of CSR entries [e0, e1) of val * img[src], in entry order with separate
// multiply and add from 0 -- the arithmetic of k_sparse (shpl_pull.hip), so the fused conv is bitwise the conv
// of the materialised map. The entries' loads are issued POOL_BATCH at a time (one round trip for runs of up to
// POOL_BATCH entries). GROUP: a pixel's run of the pixel-keyed CSR with ent_col, summed per column first
// (RunSum: walk_run<GROUP>'s order).
constexpr int POOL_BATCH = 4;
template <typename T, bool SWZ, int PSTR, bool GROUP>
__device__ __forceinline__ void pool_piece(const ConvArgs &p, const T *img, int c, int32_t e0, int32_t e1,
                                           int32_t src0, float val0, uint8_t *s_base, int pix, int g) {
    typedef Elem<T> E;
    constexpr int HE = E::HE;
    RunSum<GROUP, HE> sum;
    sum.init();
    for (int32_t i0 = e0; i0 < e1; i0 += POOL_BATCH) {
        u32x4 raw[POOL_BATCH];
        float wv[POOL_BATCH];
        int32_t kc[POOL_BATCH];
#pragma unroll
        for (int u = 0; u < POOL_BATCH; ++u) {
            const int32_t i = i0 + u;
            if (i < e1) {
                const int32_t sr = i == e0 ? src0 : p.ent_src[i];
                wv[u] = i == e0 ? val0 : p.ent_val[i];
                kc[u] = GROUP ? p.ent_col[i] : 0;
                raw[u] = load_piece<T>(img + (int64_t)sr * p.b_stride, c, p.c_b, p.vec_b);
            }
        }
#pragma unroll
        for (int u = 0; u < POOL_BATCH; ++u) {
            if (i0 + u >= e1) break;
            T x[HE];
            __builtin_memcpy(x, &raw[u], sizeof(raw[u]));
            float xf[HE];
#pragma unroll
            for (int j = 0; j < HE; ++j) xf[j] = E::f(x[j]);
            sum.add(kc[u], wv[u], xf);
        }
    }
    sum.finish();
    T o[HE];
#pragma unroll
    for (int j = 0; j < HE; ++j) o[j] = E::back(sum.acc[j]);
    __builtin_memcpy(s_base + piece_off<SWZ, PSTR>(pix, g), o, 16);
}

// The halo tile's runs of CSR entries in LDS (POOLED): one run per occupied
// halo cell, with its first entry's source row and weight.
struct HaloRuns {
    int32_t *lo, *pre;                    // [HH], [HH+1]: entry range of each halo row
    int32_t *pix, *e, *end, *src;         // [HH*HWD]
    float *val;                           // [HH*HWD]
    uint8_t *occ;                         // [HH*HWD]: cell holds a run
    int64_t *scan;                        // [SHPL_BLOCK/64+1]
};

// Lists the runs of the halo of output tile (f, y0, x0): per halo
// row the entry range of cells [x0-1, x0-1+HWD_) (row pointers + counting the
// row's sorted entries below each bound), then one block scan in entry
// order. Every thread of the 256 calls it (tid: its index; a caller may hand it in opaque, as to conv_stage).
template <int HH_ = HH, int HWD_ = HWD>
__device__ int find_runs(const ConvArgs &p, int f, int y0, int x0, const HaloRuns &r, int tid = threadIdx.x) {
    constexpr int NPIX = HH_ * HWD_;
    const int H = p.h, W = p.w;
    const int64_t frame_row0 = (int64_t)f * H * W;
    for (int j = tid; j < NPIX; j += CONV_BLOCK) r.occ[j] = 0;
    // wave w takes halo rows w, w+4, w+8; a row's sorted entries are counted
    // 64 at a time against the two cell bounds (ballots), the rows' loads in
    // flight together: two round trips for rows of up to 64 entries.
    const int lane = tid & 63, wave = tid >> 6;
    constexpr int HRW = (HH_ + 3) / 4;  // halo rows per wave
    int32_t ra[HRW], rb[HRW], kl[HRW], kh[HRW];
#pragma unroll
    for (int u = 0; u < HRW; ++u) {
        const int k = wave + 4 * u, y = y0 - 1 + k;
        ra[u] = rb[u] = 0;
        kl[u] = kh[u] = 0;
        if (k < HH_ && y >= 0 && y < H) {
            ra[u] = p.row_ptr[(int64_t)f * (H + 1) + y];
            rb[u] = p.row_ptr[(int64_t)f * (H + 1) + y + 1];
            kl[u] = (int32_t)(frame_row0 + (int64_t)y * W + (x0 > 0 ? x0 - 1 : 0));
            kh[u] = (int32_t)(frame_row0 + (int64_t)y * W + (x0 - 1 + HWD_ < W ? x0 - 1 + HWD_ : W));
        }
    }
    int32_t d[HRW];
#pragma unroll
    for (int u = 0; u < HRW; ++u) d[u] = ra[u] + lane < rb[u] ? p.ent_dst[ra[u] + lane] : 0x7fffffff;
#pragma unroll
    for (int u = 0; u < HRW; ++u) {
        const int k = wave + 4 * u;
        int32_t n_lo = __popcll(__ballot(d[u] < kl[u])), n_hi = __popcll(__ballot(d[u] < kh[u]));
        for (int32_t base = ra[u] + 64; base < rb[u] && n_hi == base - ra[u]; base += 64) {  // rows over 64 entries
            const int32_t dd = base + lane < rb[u] ? p.ent_dst[base + lane] : 0x7fffffff;
            n_lo += __popcll(__ballot(dd < kl[u]));
            n_hi += __popcll(__ballot(dd < kh[u]));
        }
        if (lane == 0 && k < HH_) {
            r.lo[k] = ra[u] + n_lo;
            r.pre[k + 1] = n_hi - n_lo;
        }
    }
    __syncthreads();
    if (tid == 0) {
        r.pre[0] = 0;
        for (int k = 0; k < HH_; ++k) r.pre[k + 1] += r.pre[k];
    }
    __syncthreads();
    const int n_ent = r.pre[HH_];
    int n_run = 0, n_tail = 0;
    for (int base = 0; base < n_ent; base += CONV_BLOCK) {
        const int j = base + tid;
        int64_t flags = 0;
        int32_t e = 0, pix = 0;
        if (j < n_ent) {
            int k = 0;
            while (j >= r.pre[k + 1]) ++k;
            e = r.lo[k] + (j - r.pre[k]);
            const int32_t last = r.lo[k] + (r.pre[k + 1] - r.pre[k]) - 1;
            const int32_t d = p.ent_dst[e];
            const bool head = j == r.pre[k] || p.ent_dst[e - 1] != d;
            const bool tail = e == last || p.ent_dst[e + 1] != d;
            flags = (head ? 1 : 0) | (tail ? (int64_t)1 << 32 : 0);
            const int y = y0 - 1 + k;
            pix = k * HWD_ + (int)((int64_t)d - frame_row0 - (int64_t)y * W) - (x0 - 1);
        }
        int64_t tot;
        const int64_t ex = block_excl_scan(flags, r.scan, &tot);
        if (flags & 1) {
            const int k = n_run + (int)(ex & 0xffffffff);
            r.e[k] = e;
            r.pix[k] = pix;
            r.occ[pix] = 1;
            r.src[k] = p.ent_src[e];
            r.val[k] = p.ent_val[e];
        }
        if (flags >> 32) r.end[n_tail + (int)(ex >> 32)] = e + 1;
        n_run += (int)(tot & 0xffffffff);
        n_tail += (int)(tot >> 32);  // a run may open in one round and close in the next
    }
    __syncthreads();
    return n_run;
}

// The dense source of input chunk q: A for the chunks [0, qa), B after them -- its rows' first element, their
// stride, the source's channels, the chunk's first channel in it, and whether every row is 16-byte aligned. PAST
// (the weight gradient, whose last block of WG_CI input channels may reach past the last chunk): chunks q >= Q
// hold zeros and are addressed in a source that exists -- A, or B when c_a == 0. Outputs by reference:
// the form whose code is closest to the four open-coded copies it replaced (docs/HISTORY.md §9).
template <typename T, bool PAST = false>
__device__ __forceinline__ void chunk_src(const ConvArgs &p, int q, const T *&src, int64_t &stride, int &c_src, int &c0,
                                          bool &vec) {
    const bool from_a = PAST ? p.c_a > 0 && (q < p.qa || q >= p.qa + p.qb) : q < p.qa;
    src = reinterpret_cast<const T *>(from_a ? p.a : p.b) + (from_a ? p.a_off : p.b_off);
    stride = from_a ? p.a_stride : p.b_stride;
    c_src = from_a ? p.c_a : p.c_b;
    c0 = (from_a ? q : q - p.qa) * Elem<T>::CK;
    vec = from_a ? p.vec_a : p.vec_b;
}

// Halo pixel pix (row-major in the HH x HWD halo) of the output tile at (y0, x0) of an H x W map: its halo row
// and column, its map row and column, and whether those lie inside the map.
struct HaloPix { int hr, hc, y, x; bool in; };
template <int HWD_ = HWD>
__device__ __forceinline__ HaloPix halo_pix(int pix, int y0, int x0, int H, int W) {
    const int hr = pix / HWD_, hc = pix - hr * HWD_;
    const int y = y0 - 1 + hr, x = x0 - 1 + hc;
    return {hr, hc, y, x, y >= 0 && y < H && x >= 0 && x < W};
}

// Stages input chunk q (channels of A, then of B) of the 10 x 34 halo of
// output tile (f, y0, x0) into s_in ([pixel][chunk] rows, piece_off); zero
// outside the map. Pooled chunks: zeros where no entry lands, each run's sum
// elsewhere (disjoint cells: no barrier between the two). The caller
// synchronises after.
template <typename T, bool POOLED, int PSTR, bool SWZ = false, bool GROUP = false, int HH_ = HH, int HWD_ = HWD>
__device__ __forceinline__ void stage_halo(const ConvArgs &p, int q, int f, int y0, int x0, uint8_t *s_in,
                                           const HaloRuns &r, int n_run, int tid = threadIdx.x) {
    typedef Elem<T> E;
    constexpr int CK = E::CK, HE = E::HE, NP = E::NP;
    constexpr int IN_PIECES = HH_ * HWD_ * NP;
    constexpr int IN_IT = (IN_PIECES + CONV_BLOCK - 1) / CONV_BLOCK;
    const int H = p.h, W = p.w;
    const int64_t frame_row0 = (int64_t)f * H * W;
    if (q < p.qa || !POOLED) {
        const T *src;
        int64_t stride;
        int c_src, c0;
        bool vec;
        chunk_src<T>(p, q, src, stride, c_src, c0, vec);
        u32x4 v[IN_IT];
#pragma unroll
        for (int u = 0; u < IN_IT; ++u) {
            const int j = tid + u * CONV_BLOCK;
            v[u] = u32x4{0u, 0u, 0u, 0u};
            if (j < IN_PIECES) {
                const HaloPix h = halo_pix<HWD_>(j / NP, y0, x0, H, W);
                if (h.in)
                    v[u] = load_piece<T>(src + (frame_row0 + (int64_t)h.y * W + h.x) * stride, c0 + (j % NP) * HE,
                                         c_src, vec);
            }
        }
#pragma unroll
        for (int u = 0; u < IN_IT; ++u) {
            const int j = tid + u * CONV_BLOCK;
            if (j < IN_PIECES) *reinterpret_cast<u32x4 *>(s_in + piece_off<SWZ, PSTR>(j / NP, j % NP)) = v[u];
        }
    } else {
#pragma unroll
        for (int u = 0; u < IN_IT; ++u) {
            const int j = tid + u * CONV_BLOCK;
            if (j < IN_PIECES && !r.occ[j / NP])
                *reinterpret_cast<u32x4 *>(s_in + piece_off<SWZ, PSTR>(j / NP, j % NP)) = u32x4{0u, 0u, 0u, 0u};
        }
        const T *img = reinterpret_cast<const T *>(p.b) + p.b_off;
        // one (run, 16-byte piece) pair per thread, POOL_BATCH entries' loads in flight per round trip
        for (int t = tid; t < n_run * NP; t += CONV_BLOCK)
            pool_piece<T, SWZ, PSTR, GROUP>(p, img, (q - p.qa) * CK + (t % NP) * HE, r.e[t / NP], r.end[t / NP],
                                            r.src[t / NP], r.val[t / NP], s_in, r.pix[t / NP], t % NP);
    }
}

// The workgroup's HaloRuns (one element per array when the kernel is not POOLED: it never reads them).
template <bool POOLED, int HH_ = HH, int HWD_ = HWD>
__device__ __forceinline__ HaloRuns halo_runs_lds() {
    constexpr int N = POOLED ? HH_ * HWD_ : 1;
    __shared__ int32_t s_lo[HH_], s_pre[HH_ + 1];
    __shared__ int32_t s_run_pix[N], s_run_e[N], s_run_end[N], s_run_src[N];
    __shared__ float s_run_val[N];
    __shared__ uint8_t s_occ[N];
    __shared__ int64_t s_scan[SHPL_BLOCK / 64 + 1];
    return {s_lo, s_pre, s_run_pix, s_run_e, s_run_end, s_run_src, s_run_val, s_occ, s_scan};
}

// Chunk q's 9x32 weight rows of NCB output blocks (wq: the first block's packed weights, wq_cb elements to the next
// block's) into s_w, the blocks W_ROWS rows apart: LDS-DMAs into swizzled 32-byte rows (lane k of the wave fills
// slot k: it loads the piece the swizzle puts there). The caller waits and synchronises.
template <typename T, int NCB>
__device__ __forceinline__ void stage_weights(const T *wq, int64_t wq_cb, int q, uint8_t *s_w, int tid) {
    constexpr int CK = Elem<T>::CK, HE = Elem<T>::HE, W_PIECES = W_ROWS * Elem<T>::NP;
    const int lane = tid & 63, wave = tid >> 6;
#pragma unroll
    for (int cb = 0; cb < NCB; ++cb) {
#pragma unroll
        for (int u = 0; u < (W_PIECES + CONV_BLOCK - 1) / CONV_BLOCK; ++u) {
            const int base = u * CONV_BLOCK + wave * 64;  // the wave's first slot
            if (base >= W_PIECES) break;
            const int k = base + lane, row = k >> 1, g = (k & 1) ^ ((row >> 3) & 1);
            if (k < W_PIECES)
                dma16(wq + cb * wq_cb + ((int64_t)q * W_ROWS + row) * CK + g * HE,
                      s_w + (cb * W_PIECES + base) * 16);
        }
    }
}

// Stages input chunk q of output tile (f, y0, x0) -- its 9x32 weight rows
// (stage_weights) and its HH_ x HWD_ halo -- into one LDS buffer pair (swizzled
// 32-byte rows). Dense halo chunks are LDS-DMAs as the weights are; pooled
// chunks are computed (stage_halo). The caller waits and synchronises. tid: the thread's index (a caller may hand it in opaque, so
// that the conditions on it are evaluated per chunk instead of kept as lane masks across its chunk loop).
template <typename T, bool POOLED, int NCB = 1, bool GROUP = false, int HH_ = HH, int HWD_ = HWD>
__device__ __forceinline__ void conv_stage(const ConvArgs &p, int q, int f, int y0, int x0, const T *wq,
                                           int64_t wq_cb, uint8_t *s_in, uint8_t *s_w, const HaloRuns &runs,
                                           int n_run, int tid = threadIdx.x) {
    typedef Elem<T> E;
    constexpr int HE = E::HE, NP = E::NP;
    constexpr int IN_PIECES = HH_ * HWD_ * NP;
    const int lane = tid & 63, wave = tid >> 6;
    stage_weights<T, NCB>(wq, wq_cb, q, s_w, tid);
    if (!POOLED || q < p.qa) {
        const int H = p.h, W = p.w;
        const int64_t frame_row0 = (int64_t)f * H * W;
        const T *src;
        int64_t stride;
        int c_src, c0;
        bool vec;
        chunk_src<T>(p, q, src, stride, c_src, c0, vec);
#pragma unroll
        for (int u = 0; u < (IN_PIECES + CONV_BLOCK - 1) / CONV_BLOCK; ++u) {
            const int base = u * CONV_BLOCK + wave * 64;
            if (base >= IN_PIECES) break;
            const int k = base + lane, pix = k >> 1, g = (k & 1) ^ ((pix >> 3) & 1);
            const HaloPix h = halo_pix<HWD_>(pix, y0, x0, H, W);
            if (k < IN_PIECES)
                piece_to_lds<T>(h.in ? src + (frame_row0 + (int64_t)h.y * W + h.x) * stride : nullptr, c0 + g * HE,
                                c_src, vec, s_in + base * 16, lane);
        }
    } else {
        stage_halo<T, true, E::CB, true, GROUP, HH_, HWD_>(p, q, f, y0, x0, s_in, runs, n_run, tid);
    }
}

// Packed weights: HWIO [3][3][c_a+c_b][c_out] -> [co_block][chunk][tap][32][CK],
// chunks of A's channels first, then B's, zero padded. transpose (the input
// gradient): w is the forward's HWIO [3][3][c_out][c_a+c_b] and the packed
// tap t takes W[8-t] transposed (W'[ky][kx][co][ci] = W[2-ky][2-kx][ci][co]).
template <typename T>
__global__ __launch_bounds__(SHPL_BLOCK) void k_pack_w(const T *w, int c_a, int qa, int c_b, int qb, int c_out,
                                                       int n_cob, int transpose, T *wp) {
    constexpr int CK = Elem<T>::CK;
    const int Q = qa + qb;
    const int64_t total = (int64_t)n_cob * Q * W_ROWS * CK;
    const int cin = c_a + c_b;
    for (int64_t t = (int64_t)blockIdx.x * SHPL_BLOCK + threadIdx.x; t < total;
         t += (int64_t)gridDim.x * SHPL_BLOCK) {
        const int k = (int)(t % CK);
        int64_t r = t / CK;
        const int co_l = (int)(r % NCO);
        r /= NCO;
        const int tap = (int)(r % 9);
        r /= 9;
        const int q = (int)(r % Q);
        const int cob = (int)(r / Q);
        const int co = cob * NCO + co_l;
        int ci;
        bool ok;
        if (q < qa) {
            ci = q * CK + k;
            ok = ci < c_a;
        } else {
            const int cb = (q - qa) * CK + k;
            ci = c_a + cb;
            ok = cb < c_b;
        }
        const int64_t src = transpose ? ((int64_t)(8 - tap) * c_out + co) * cin + ci
                                      : ((int64_t)tap * cin + ci) * c_out + co;
        wp[t] = (ok && co < c_out) ? w[src] : T(0);
    }
}

// Entry pointer of every BEV row of every frame over the destination-sorted
// CSR: row_ptr[f*(H+1) + y] = first entry of frame f whose cell lies in row
// >= y (empty slots, dst -1, count as row H).
__global__ __launch_bounds__(SHPL_BLOCK) void k_row_ptr(const int32_t *dst, const int64_t *frame_off, int H, int W,
                                                        int32_t *row_ptr) {
    const int f = blockIdx.y;
    const int64_t s = frame_off[f], e_end = frame_off[f + 1];
    const int64_t base = (int64_t)f * H * W;
    int32_t *rp = row_ptr + (int64_t)f * (H + 1);
    for (int64_t e = s + (int64_t)blockIdx.x * SHPL_BLOCK + threadIdx.x; e <= e_end;
         e += (int64_t)gridDim.x * SHPL_BLOCK) {
        const int32_t dc = e < e_end ? dst[e] : -1;
        const int yc = dc < 0 ? H : (int)((dc - base) / W);
        int yp = -1;
        if (e > s) {
            const int32_t dp = dst[e - 1];
            yp = dp < 0 ? H : (int)((dp - base) / W);
        }
        for (int y = yp + 1; y <= yc; ++y) rp[y] = (int32_t)e;
    }
}

// Per-channel sum / sum of squares of the pre-activation output, summed over
// the per-tile partials in a fixed order (deterministic): one block per
// (channel, statistic; strided_sum / block_sum of shpl_conv_bn.h).
constexpr int RED_BLOCK = 1024;
__global__ __launch_bounds__(RED_BLOCK) void k_stats_reduce(const double *part, int n_tiles, int c_out,
                                                            double *stats) {
    __shared__ double red[RED_BLOCK / 64];
    const int ch = blockIdx.x >> 1, st = blockIdx.x & 1;
    const double s = block_sum<RED_BLOCK>(
        strided_sum<RED_BLOCK>(part + ((int64_t)ch * 2 + st) * n_tiles, n_tiles, 1, threadIdx.x), red);
    if (threadIdx.x == 0 && ch < c_out) stats[st * c_out + ch] = s;
}

// ---------------------------------------------------------------- host
// A dtype code to its element type, beside shpl_common.h's by_bools: fn(TypeOf<float>()) for SHPL_F32,
// fn(TypeOf<uint16_t>()) for SHPL_BF16 (conv_plan has rejected every other code by then).
template <typename F>
auto by_dtype(int dtype, F &&fn) {
    return dtype == SHPL_F32 ? fn(TypeOf<float>()) : fn(TypeOf<uint16_t>());
}

// Channels per 16-byte piece of a dtype (Elem<T>::HE).
int piece_elems(int dtype) { return by_dtype(dtype, [](auto t) { return Elem<typename decltype(t)::T>::HE; }); }

// One source of the conv: rows of `stride` elements, of which the channels [off, off + c) are read.
struct Src { const void *p; int64_t stride, off, c; };

bool vec16(const Src &s, int he) { return aligned16(s.p) && s.stride % he == 0 && s.off % he == 0; }

// A workspace is a run of regions, each a multiple of 256 bytes; take(bytes) is the next one's byte offset.
// Only the plans below lay one out: everything else reads a region's address from the plan (region<T>; NULL
// in a NULL workspace, which shpl_conv3x3_rows_form plans with).
struct Layout {
    size_t end = 0;
    size_t take(size_t bytes) { const size_t at = end; end = at + align_up(bytes, 256); return at; }
};

template <typename T>
T *region(const void *ws, size_t at) {
    return ws ? reinterpret_cast<T *>(reinterpret_cast<uint8_t *>(const_cast<void *>(ws)) + at) : nullptr;
}

// The tiled weight gradients' cut of n_tiles tiles into groups, one partial per (group, channel block pair): about
// 1024 workgroups in all, which bounds the partials' bytes; a group holds at least one tile.
void wgrad_groups(int64_t n_tiles, int64_t blocks_per_group, int *tiles_per_group, int *n_groups) {
    int64_t ng = 1024 / blocks_per_group;
    if (ng < 1) ng = 1;
    if (ng > n_tiles) ng = n_tiles > 0 ? n_tiles : 1;
    *tiles_per_group = (int)((n_tiles + ng - 1) / ng);
    if (*tiles_per_group < 1) *tiles_per_group = 1;
    *n_groups = (int)((n_tiles + *tiles_per_group - 1) / *tiles_per_group);
    if (*n_groups < 1) *n_groups = 1;
}

// A pool counts as pixel-keyed (shpl_build_csr SHPL_BY_PIXEL, SHPL_ORDER_COL_ROW: the keys are image pixels, the
// sources BEV cells) when it carries ent_col or is flagged as one column per entry; only the former needs the
// per-column partials, as in the pulls (grouped() in shpl_pull.hip).
bool pixel_keyed(const shpl_csr *pool) {
    return pool->ent_col != nullptr || (pool->flags & SHPL_CSR_IDENTITY_COLS) != 0;
}

// The checks on the sources and the pool that the forward and the weight gradient share, in their order.
// o_stride: the row stride of the map of c_out channels (the output, or its gradient).
int check_sources(int n_frames, int64_t h, int64_t w, const Src &A, const Src &B, const shpl_csr *pool,
                  const int64_t *d_frame_off, int64_t o_stride, int64_t c_out) {
    if (A.stride < A.off + A.c || o_stride < c_out || A.off < 0 || B.off < 0) return SHPL_ERR_BAD_SHAPE;
    if (B.c > 0 && B.stride < B.off + B.c) return SHPL_ERR_BAD_SHAPE;
    if (pool) {
        if (!d_frame_off || B.c < 1 || !B.p) return SHPL_ERR_ARG;
        if (pool->n_keys != (int64_t)n_frames * h * w) return SHPL_ERR_BAD_SHAPE;
        if (pool->nnz_cap > 0 && (!pool->ent_dst || !pool->ent_src || !pool->ent_val)) return SHPL_ERR_ARG;
    } else if (B.c > 0 && !B.p) {
        return SHPL_ERR_ARG;
    }
    return SHPL_OK;
}

// What the plans of the tiled kernels share: elements per chunk, chunks of A and of B, output blocks, the tiling.
struct TilePlan {
    int ck, qa, qb, n_cob, tiles_x, tiles_y, tiles_per_frame;
    int64_t n_tiles;
};

// The fields of ConvArgs every form fills: frame and tile geometry, the sources, the pool's arrays; the rest 0.
ConvArgs conv_args(int dtype, int n_frames, int64_t h, int64_t w, const TilePlan &pl, const Src &A, const Src &B,
                   const shpl_csr *pool) {
    const int he = piece_elems(dtype);
    ConvArgs a = {};
    a.n_frames = n_frames;
    a.h = (int)h;
    a.w = (int)w;
    a.tiles_x = pl.tiles_x;
    a.tiles_per_frame = pl.tiles_per_frame;
    a.n_tiles = (int)pl.n_tiles;
    a.a = A.p;
    a.a_stride = A.stride;
    a.a_off = A.off;
    a.c_a = (int)A.c;
    a.qa = pl.qa;
    a.b = B.p;
    a.b_stride = B.stride;
    a.b_off = B.off;
    a.c_b = (int)B.c;
    a.qb = pl.qb;
    a.vec_a = vec16(A, he);
    a.vec_b = vec16(B, he);
    a.ent_dst = pool ? pool->ent_dst : nullptr;
    a.ent_src = pool ? pool->ent_src : nullptr;
    a.ent_val = pool ? pool->ent_val : nullptr;
    a.ent_col = pool ? pool->ent_col : nullptr;
    return a;
}

// ConvArgs::vec_out of an input gradient's one or two maps (d_dx_b: channels >= c_split, or NULL): the rows of
// each map that is there are 16-byte aligned, and with two the split falls on a whole piece.
bool vec_out_split(const void *d_dx, int64_t dx_stride, const void *d_dx_b, int64_t dx_b_stride, int64_t c_split,
                   int he) {
    return (!d_dx || (aligned16(d_dx) && dx_stride % he == 0)) &&
           (!d_dx_b || (aligned16(d_dx_b) && dx_b_stride % he == 0 && c_split % he == 0));
}

// k_pack_w of the weights w over a's chunks and n_cob output blocks, into a.wp.
template <typename T>
int pack_weights(const ConvArgs &a, const void *w, int n_cob, int transpose, hipStream_t s) {
    const int64_t wtot = (int64_t)n_cob * (a.qa + a.qb) * W_ROWS * Elem<T>::CK;
    hipLaunchKernelGGL(k_pack_w<T>, dim3(grid_for(wtot, SHPL_BLOCK, 4096)), dim3(SHPL_BLOCK), 0, s,
                       reinterpret_cast<const T *>(w), a.c_a, a.qa, a.c_b, a.qb, a.c_out, n_cob, transpose,
                       reinterpret_cast<T *>(const_cast<void *>(a.wp)));
    SHPL_LAUNCH_CHECK();
    return SHPL_OK;
}

// k_row_ptr over the pool's destinations (pooled forms), into a.row_ptr.
int row_pointers(const ConvArgs &a, const int64_t *frame_off, hipStream_t s) {
    hipLaunchKernelGGL(k_row_ptr, dim3(16, a.n_frames), dim3(SHPL_BLOCK), 0, s, a.ent_dst, frame_off, a.h, a.w,
                       const_cast<int32_t *>(a.row_ptr));
    SHPL_LAUNCH_CHECK();
    return SHPL_OK;
}

// The (POOLED, GROUP) form of a kernel family: fn(po, gr) returns the instantiation's address. GROUP -- the
// pixel-keyed CSR's per-column partials -- is pooled && ent_col, so (GROUP && !POOLED) never runs, and fn is not
// instantiated for it: the family has no such kernel.
template <typename Kernel, typename F>
Kernel pooled_form(bool pooled, const int32_t *ent_col, F &&fn) {
    return by_bools(
        [&](auto po, auto gr) -> Kernel {
            if constexpr (gr() && !po())
                return nullptr;
            else
                return fn(po, gr);
        },
        pooled, pooled && ent_col);
}

}  // namespace
}  // namespace shpl
