// shpl_upconv_grad.hip -- the gradients of the after-VGG upconv3 (shpl_upconv.hip: the 3x3 stride-2 transposed conv
// over x = [a || pooled b]):
//     dx[f, i, j, ci]    = sum over ky, kx, co        of gy[f, 2i+ky, 2j+kx, co] W[ky, kx, co, ci]
//     dW[ky, kx, co, ci] = sum over f, i, j           of gy[f, 2i+ky, 2j+kx, co] x[f, i, j, ci]
// a tap whose output pixel lies outside the 2h x 2w map contributes nothing (ky = 2 at i = h-1, kx = 2 at j = w-1).
//
// Both kernels read gy through its four PARITY PLANES: plane (py, px) of a tile of R x 32 input pixels at (y0, x0)
// holds the (R+1) x 33 output pixels (2 (y0 + r) + py, 2 (x0 + c) + px), zeros outside the map -- the tile's
// 2R+1 x 65 output pixels (one halo row below, one halo column right) de-interleaved at staging time by which
// global piece each lane fetches. Tap (ky, kx) of input pixel (r, c) then reads plane (ky & 1, kx & 1) at pixel
// (r + (ky >> 1), c + (kx >> 1)): consecutive lanes read consecutive LDS rows, the forward's conflict-free
// image, where the interleaved tile at a pixel stride of 2 would put lanes 64 B apart.
//
// Input gradient (k_upconv3x3_dgrad): the forward mirrored. One workgroup owns an 8 x 32 tile of input pixels
// and NB <= 4 blocks of 32 dx channels: M = dx channels, N = pixels, K = 9 taps x c_gy in chunks of 32 B per pixel
// (8 f32 / 16 bf16 channels). A chunk's four 9 x 33 planes (swizzled 32-byte rows, 38016 B) are staged ONCE and
// feed all NB blocks (the forward stages its input once per block); the chunk's 9 x 32 weight rows of every block
// sit beside them (NB x 9216 B). Wave w keeps NB x 2 input rows of 32 x 32 f32 accumulators (128 registers at
// NB = 4). LDS at NB = 4: 38016 + 36864 = 74880 B, two workgroups per CU (149760 B of 160 KiB).
// f32: v_mfma_f32_32x32x2_f32 (exact f32 products); bf16: v_mfma_f32_32x32x16_bf16; f32 sums, one rounding at the
// store, through LDS as 16-byte pieces (channel by channel for ragged channel counts / unaligned rows).
//
// Weight gradient (k_upconv3x3_wgrad): one workgroup per (group of input tiles, 32 input channels, 32 output
// channels), M = input channels, N = output channels, K = pixels. The tile is 4 x 32 input pixels: the x tile
// [pixel][32 channels] (no halo; dense chunks by LDS-DMA, pooled chunks from the CSR's runs by stage_halo, in the
// pull's order, rounded once) and the four 5 x 33 planes of gy [pixel][32 channels]. 8 rows would need
// 4 x 9 x 33 x 128 B = 152 KB for the f32 planes alone; at 4 rows the LDS is 16384 + 84480 = 100864 B (f32, one
// workgroup per CU) and 8192 + 42240 = 50432 B (bf16, + 2784 B of run lists when pooled: three per CU by LDS).
// Wave (wm, wn) owns the 16 x 16 block (input channels 16 wm.., output channels 16 wn..) of all nine taps over
// ALL the tile's pixels -- 36 accumulator registers, no sum across waves; a K split (every wave the whole
// 32 x 32 block over its own rows, 144 registers) left the pooled form at one wave per SIMD, where nothing hides
// the latency chains of its run listing and gathers: 1.31 ms against 0.28 ms dense at the reference's bf16 shape.
// f32: v_mfma_f32_16x16x4_f32, both operands one ds_read_b32 per lane. bf16: v_mfma_f32_16x16x32_bf16 (K = one
// tile row), both operands read transposed from the [pixel][64 B] images (ds_read_b64_tr_b16, as the
// row-streaming weight gradient does). A workgroup adds its tiles in tile order, the groups' partials are added
// in group order by k_upwgrad_reduce (f64): no atomics, bitwise repeatable.
#include "shpl_upconv.h"

namespace shpl {
namespace {

// Stages the four parity planes of the tile of ROWS x 32 input pixels at (y0, x0) of frame f: channels
// [c0, c0 + NPP * HE) of gy (c_src channels per row, zeros past them), NPP 16-byte pieces per plane pixel.
// SWZ (NPP == 2): piece_off<true>'s swizzled 32-byte rows; otherwise rows of NPP * 16 bytes. Whole pieces and
// zeros are LDS-DMAs (lane-linear destinations; the de-interleave and the swizzle go on the source side), ragged
// ones masked loads. The caller waits (vmcnt(0)) and synchronises.
template <typename T, int ROWS, int NPP, bool SWZ>
__device__ __forceinline__ void stage_planes(const T *gy, int64_t stride, int c_src, bool vec, int c0, int f, int y0,
                                             int x0, int H, int W, uint8_t *s_dst, int tid) {
    constexpr int HE = Elem<T>::HE, PW = TW + 1, PLN = (ROWS + 1) * PW, PIECES = 4 * PLN * NPP;
    static_assert(!SWZ || NPP == 2, "the swizzle is over two pieces per row");
    const int lane = tid & 63, wave = tid >> 6;
    const int64_t row0 = (int64_t)f * 4 * H * W;  // the frame's first output row
#pragma unroll
    for (int u = 0; u < (PIECES + CONV_BLOCK - 1) / CONV_BLOCK; ++u) {
        const int base = u * CONV_BLOCK + wave * 64;  // the wave's first slot
        if (base >= PIECES) break;
        const int k = base + lane, pix = k / NPP;
        const int g = SWZ ? ((k & 1) ^ ((pix >> 3) & 1)) : k % NPP;
        const int par = pix / PLN, pr = pix - par * PLN, r = pr / PW, c = pr - r * PW;
        const int oy = 2 * (y0 + r) + (par >> 1), ox = 2 * (x0 + c) + (par & 1);
        const bool in = oy < 2 * H && ox < 2 * W;
        if (k < PIECES)
            piece_to_lds<T>(in ? gy + (row0 + (int64_t)oy * (2 * W) + ox) * stride : nullptr, c0 + g * HE, c_src, vec,
                            s_dst + base * 16, lane);
    }
}

// ---------------------------------------------------------------- input gradient
constexpr int DPW = TW + 1, DPLN = (TH + 1) * DPW;  // a parity plane of the 8 x 32 tile: 9 x 33 pixels

// ConvArgs as the forward fills them, with gy as source A (c_a = c_gy, qa its chunks), dx as out / out2 / c_split
// (c_out = c_dx) and wp the weights packed [dx block][chunk][tap][32][CK] (k_pack_w, untransposed: HWOI is
// [tap][K = c_gy][N = c_dx] already).
template <typename T, int NB>
__global__ __launch_bounds__(CONV_BLOCK, 2) void k_upconv3x3_dgrad(const ConvArgs p) {
    typedef Elem<T> E;
    constexpr int CK = E::CK, NP = E::NP;
    static_assert(NP == 2, "two 16-byte pieces per LDS row (the swizzle)");
    constexpr int G_BYTES = 4 * DPLN * NP * 16, W_PIECES = W_ROWS * NP, W_BYTES = NB * W_PIECES * 16;
    static_assert(4 * 32 * OPITCH<T> <= G_BYTES + W_BYTES, "the epilogue's rows reuse the chunk buffers");
    __shared__ __attribute__((aligned(16))) uint8_t s_buf[G_BYTES + W_BYTES];
    uint8_t *const s_g = s_buf, *const s_w = s_buf + G_BYTES;

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int pl = lane & 31, hf = lane >> 5;
    const int tile = (int)xcd_block((int)blockIdx.x, p.n_tiles);
    const int cib0 = blockIdx.y * NB;  // the workgroup's first dx block
    int f, y0, x0;
    tile_origin<TH>(p, tile, f, y0, x0);
    const int H = p.h, W = p.w, Q = p.qa;

    f32x16 acc[NB][RPW];
#pragma unroll
    for (int cb = 0; cb < NB; ++cb)
#pragma unroll
        for (int m = 0; m < RPW; ++m)
#pragma unroll
            for (int i = 0; i < 16; ++i) acc[cb][m][i] = 0.0f;

    const T *gy = reinterpret_cast<const T *>(p.a);
    const int64_t wq_cb = (int64_t)Q * W_ROWS * CK;  // one dx block further in the packed weights
    const T *wq = reinterpret_cast<const T *>(p.wp) + cib0 * wq_cb;
    for (int q = 0; q < Q; ++q) {
        stage_weights<T, NB>(wq, wq_cb, q, s_w, tid);
        // the tile's origin and the thread's index, opaque per chunk, as in k_upconv3x3: each lane's part of the
        // planes' addresses is worked out per chunk, not kept in some 20 registers across the loop (which the
        // compiler does or does not do at the slightest change here; at NB = 4 that is past the 256 there are)
        int yq = y0, xq = x0, tq = tid;
        asm volatile("" : "+s"(yq), "+s"(xq), "+v"(tq));
        stage_planes<T, TH, NP, true>(gy, p.a_stride, p.c_a, p.vec_a, q * CK, f, yq, xq, H, W, s_g, tq);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // the LDS-DMAs have landed
        __syncthreads();
#pragma unroll
        for (int ky = 0; ky < 3; ++ky) {
#pragma unroll
            for (int kx = 0; kx < 3; ++kx) {
                const int par = 2 * (ky & 1) + (kx & 1), dy = ky >> 1, dx = kx >> 1;
                Frag<T> a[RPW];
#pragma unroll
                for (int m = 0; m < RPW; ++m)
                    a[m] = lds_frag<T>(s_g +
                                       piece_off<true, 0>(par * DPLN + (RPW * wave + m + dy) * DPW + pl + dx, hf));
#pragma unroll
                for (int cb = 0; cb < NB; ++cb) {
                    const Frag<T> b =
                        lds_frag<T>(s_w + cb * W_PIECES * 16 + piece_off<true, 0>((ky * 3 + kx) * NCO + pl, hf));
#pragma unroll
                    for (int m = 0; m < RPW; ++m) acc[cb][m] = mfma_tap<T>(b, a[m], acc[cb][m]);
                }
            }
        }
        __syncthreads();  // the chunk's buffers are restaged next
    }

    // ---- epilogue (epilogue_row, without the fma): acc element i of (cb, m) is dx channel (cib0 + cb) * 32 +
    // 8 (i >> 2) + 4 h + (i & 3) of input pixel (y0 + RPW w + m, x0 + pl); each 16-byte piece goes to the map its
    // channels belong to (out_ptr; vec_out: c_split is a whole number of pieces).
    uint8_t *const s_o = s_buf + wave * 32 * OPITCH<T>;
#pragma unroll
    for (int cb = 0; cb < NB; ++cb) {
        const int cb0 = (cib0 + cb) * NCO;
        if (cb0 >= p.c_out) break;
#pragma unroll
        for (int m = 0; m < RPW; ++m) {
            const int y = y0 + RPW * wave + m;
            const int64_t row = ((int64_t)f * H + y) * W + x0;  // + column of the tile
            epilogue_row<T, false, false>(
                p, acc[cb][m], nullptr, s_o, cb0, y < H, x0, W, nullptr,
                [row](const ConvArgs &a, int col, int c) { return out_ptr<T>(a, row + col, c); });
        }
    }
}

// ---------------------------------------------------------------- weight gradient
constexpr int WTH = 4;                              // input rows per tile: wave w owns row w
constexpr int WPW = TW + 1, WPLN = (WTH + 1) * WPW;  // a parity plane of the tile: 5 x 33 pixels
constexpr int WG_BLK = 32;                          // input channels per workgroup (NCO output channels)

struct UwArgs {
    const void *gy;
    int64_t gy_stride;
    bool vec_g;
    int n_cib, n_cob, tiles_per_group;
    float *part;  // [group][cib][cob][tap][32 co][32 ci]
};

// where k_upconv3x3_wgrad's second argument lies in its kernel-argument segment: after the first, at its own alignment
constexpr unsigned UW_AT = (sizeof(ConvArgs) + alignof(UwArgs) - 1) / alignof(UwArgs) * alignof(UwArgs);

typedef short s16x4 __attribute__((ext_vector_type(4)));
typedef short s16x8 __attribute__((ext_vector_type(8)));

// 8 consecutive pixels of one channel from an LDS image [pixel][32 bf16 channels]: lane (l = lane & 15,
// kq = lane >> 4) gets channel c0 + l of pixels 8 kq .. 8 kq + 7 past `at`, which holds the lane's part of the
// address (tr_lane) -- the 16x16x32 MFMA's operand; two transposed reads of 4 pixels x 16 channels per 16-lane
// group (lane 4 q + p of a group addresses pixel q, channels 4 p .. 4 p + 3).
__device__ __forceinline__ int tr_lane(int lane, int c0) {
    return (8 * (lane >> 4) + ((lane & 15) >> 2)) * 64 + 2 * c0 + 8 * (lane & 3);
}
__device__ __forceinline__ bf16x8 tr_pixels(const uint8_t *at) {
    typedef __attribute__((address_space(3))) s16x4 lds_s16x4;
    const s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4 *)at);
    const s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4 *)(at + 4 * 64));
    const s16x8 v = __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
    bf16x8 out;
    __builtin_memcpy(&out, &v, 16);
    return out;
}


// ConvArgs as the forward fills them (the sources, the pool, the row pointers), tiled by WTH x 32.
template <typename T, bool POOLED, bool GROUP>
__global__ __launch_bounds__(CONV_BLOCK, sizeof(T) == 4 ? 1 : 2) void k_upconv3x3_wgrad(const ConvArgs p,
                                                                                       const UwArgs g) {
    typedef Elem<T> E;
    constexpr int CK = E::CK, HE = E::HE, NQ = WG_BLK / CK;
    constexpr int PB = WG_BLK * (int)sizeof(T), NPP = PB / 16;  // bytes, pieces per pixel of either image
    constexpr int X_PIECES = WTH * TW * NPP, X_BYTES = X_PIECES * 16, G_BYTES = 4 * WPLN * PB;
    __shared__ __attribute__((aligned(16))) uint8_t s_x[X_BYTES];
    __shared__ __attribute__((aligned(16))) uint8_t s_g[G_BYTES];
    const HaloRuns runs = halo_runs_lds<POOLED, WTH, TW>();
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int l16 = lane & 15, kq = lane >> 4, wm = wave >> 1, wn = wave & 1;
    const int cib = blockIdx.y;
    // the group, the output block and the group's last tile wait in vector registers (read back with
    // readfirstlane where they are used: once per tile, and at the end): the pooled grouped bf16 form is short
    // of exactly these scalar registers
    int grp_v = blockIdx.x, cob_v = blockIdx.z;
    f32x4 acc[9];  // [tap]: input channels 16 wm + 4 kq + i, output channel 16 wn + l16
#pragma unroll
    for (int t = 0; t < 9; ++t) acc[t] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
    const int t0 = grp_v * g.tiles_per_group;
    int t1_v = t0 + g.tiles_per_group < p.n_tiles ? t0 + g.tiles_per_group : p.n_tiles;
    asm volatile("" : "+v"(grp_v), "+v"(cob_v), "+v"(t1_v));
    for (int tile = t0; tile < __builtin_amdgcn_readfirstlane(t1_v); ++tile) {
        // the arguments, read again before each step of the tile through a kernel-argument pointer the compiler
        // cannot see through: read once at the kernel's start they sit in scalar registers across the whole tile
        // loop, and read once per tile across all of its steps (and spill)
        ConvArgs pq = kernarg_again<ConvArgs>(0);
        int f, y0, x0;
        tile_origin<WTH, true>(pq, tile, f, y0, x0);
        // the thread's index, opaque per tile: the staging's per-lane conditions on it (a piece of the tile, inside
        // the map, a pooled chunk) are then worked out per tile instead of kept across the tile loop as lane masks,
        // two scalar registers each, which ran the pooled forms out of scalar registers (as in k_upconv3x3)
        int tq = tid;
        asm volatile("" : "+v"(tq));
        // the runs of the tile itself (the staging's halo tile starts one row above and one column left of its
        // origin), listed only by the workgroups whose block holds pooled channels
        const bool pooled_blk = POOLED && cib * NQ + NQ > pq.qa && cib * NQ < pq.qa + pq.qb;
        const int n_run = pooled_blk ? find_runs<WTH, TW>(pq, f, y0 + 1, x0 + 1, runs, tq) : 0;
        // ---- x: [pixel][chunk of the block][2 pieces]; chunks past the last one hold zeros
        pq = kernarg_again<ConvArgs>(0);
        tile_origin<WTH, true>(pq, tile, f, y0, x0);
        const int H = pq.h, W = pq.w, Q = pq.qa + pq.qb;
        const int64_t frame_row0 = (int64_t)f * H * W;
#pragma unroll
        for (int u = 0; u < X_PIECES / CONV_BLOCK; ++u) {
            const int base = u * CONV_BLOCK + (tq >> 6) * 64;
            const int k = base + (tq & 63), pix = k / NPP, pr = k % NPP;
            const int q = cib * NQ + (pr >> 1);
            const int y = y0 + pix / TW, x = x0 + pix % TW;
            if (!(POOLED && q >= pq.qa && q < Q)) {
                const T *src;
                int64_t stride;
                int c_src, c0;
                bool vec;
                chunk_src<T, true>(pq, q, src, stride, c_src, c0, vec);
                const bool in = q < Q && y < H && x < W;
                piece_to_lds<T>(in ? src + (frame_row0 + (int64_t)y * W + x) * stride : nullptr, c0 + (pr & 1) * HE,
                                c_src, vec, s_x + base * 16, tq & 63);
            }
        }
        static_assert(X_PIECES % CONV_BLOCK == 0, "x pieces");
        if constexpr (POOLED) {
#pragma unroll 1  // (one copy of the pooled staging's loops, not NQ)
            for (int j = 0; j < NQ; ++j) {
                const int q = cib * NQ + j;
                pq = kernarg_again<ConvArgs>(0);
                tile_origin<WTH, true>(pq, tile, f, y0, x0);
                if (q >= pq.qa && q < pq.qa + pq.qb)
                    stage_halo<T, true, PB, false, GROUP, WTH, TW>(pq, q, f, y0 + 1, x0 + 1, s_x + j * E::CB, runs,
                                                                   n_run, tq);
            }
        }
        pq = kernarg_again<ConvArgs>(0);
        tile_origin<WTH, true>(pq, tile, f, y0, x0);
        const UwArgs gq = kernarg_again<UwArgs>(UW_AT);
        stage_planes<T, WTH, NPP, false>(reinterpret_cast<const T *>(gq.gy), gq.gy_stride, pq.c_out, gq.vec_g,
                                         __builtin_amdgcn_readfirstlane(cob_v) * NCO, f,
                                         y0, x0, pq.h, pq.w, s_g, tq);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // the LDS-DMAs have landed
        __syncthreads();
        // ---- K = the tile's pixels, row by row; tap (ky, kx) of row r meets plane (ky & 1, kx & 1) at
        // (r + (ky >> 1), column + (kx >> 1))
        if constexpr (sizeof(T) == 4) {
            const float *sx = reinterpret_cast<const float *>(s_x) + 16 * wm + l16;
            const float *sg = reinterpret_cast<const float *>(s_g) + 16 * wn + l16;
#pragma unroll 1
            for (int r = 0; r < WTH; ++r) {
#pragma unroll 2
                for (int st = 0; st < TW / 4; ++st) {
                    const int kp = 4 * st + kq;  // lane group kq supplies pixel 4 st + kq (both operands)
                    const float a = sx[(r * TW + kp) * WG_BLK];
#pragma unroll
                    for (int ky = 0; ky < 3; ++ky)
#pragma unroll
                        for (int kx = 0; kx < 3; ++kx) {
                            const int par = 2 * (ky & 1) + (kx & 1);
                            const float b = sg[(par * WPLN + (r + (ky >> 1)) * WPW + kp + (kx >> 1)) * NCO];
                            acc[ky * 3 + kx] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, acc[ky * 3 + kx], 0, 0, 0);
                        }
                }
            }
        } else {
            const uint8_t *sx = s_x + tr_lane(lane, 16 * wm), *sg = s_g + tr_lane(lane, 16 * wn);
#pragma unroll
            for (int r = 0; r < WTH; ++r) {
                const bf16x8 a = tr_pixels(sx + r * TW * PB);
#pragma unroll
                for (int ky = 0; ky < 3; ++ky)
#pragma unroll
                    for (int kx = 0; kx < 3; ++kx) {
                        const int par = 2 * (ky & 1) + (kx & 1);
                        const bf16x8 b = tr_pixels(sg + (par * WPLN + (r + (ky >> 1)) * WPW + (kx >> 1)) * PB);
                        acc[ky * 3 + kx] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, acc[ky * 3 + kx], 0, 0, 0);
                    }
            }
        }
        __syncthreads();
    }
    // the workgroup's partial [tap][32 co][32 ci]: D of the 16x16 MFMAs has column = lane & 15 (output channel)
    // and rows 4 (lane >> 4) + i (input channels)
    const UwArgs ge = kernarg_again<UwArgs>(UW_AT);
    const int grp = __builtin_amdgcn_readfirstlane(grp_v), cob = __builtin_amdgcn_readfirstlane(cob_v);
    float *out = ge.part + (((int64_t)grp * ge.n_cib + cib) * ge.n_cob + cob) * (9 * WG_BLK * NCO) +
                 (16 * wn + l16) * WG_BLK + 16 * wm + 4 * kq;
#pragma unroll
    for (int t = 0; t < 9; ++t) *reinterpret_cast<f32x4 *>(out + t * (WG_BLK * NCO)) = acc[t];
}

// dW (f32, HWOI [3][3][c_out][c_a+c_b]) = the groups' partials summed in group order (f64, four independent
// sums combined in a fixed order), channels mapped back from the chunk layout.
__global__ __launch_bounds__(SHPL_BLOCK) void k_upwgrad_reduce(const float *part, int n_groups, int n_cib, int n_cob,
                                                               int c_a, int c_b, int qa, int ck, int c_out,
                                                               float *dw) {
    const int cin = c_a + c_b;
    const int64_t total = (int64_t)9 * c_out * cin;
    const int64_t gstride = (int64_t)n_cib * n_cob * (9 * WG_BLK * NCO);  // one group further
    for (int64_t t = (int64_t)blockIdx.x * SHPL_BLOCK + threadIdx.x; t < total; t += (int64_t)gridDim.x * SHPL_BLOCK) {
        const int ci = (int)(t % cin);
        const int co = (int)((t / cin) % c_out);
        const int tap = (int)(t / ((int64_t)cin * c_out));
        const int cs = ci < c_a ? ci : qa * ck + (ci - c_a);  // channel in the chunk layout
        const int cib = cs / WG_BLK, cil = cs % WG_BLK, cob = co / NCO, col = co % NCO;
        const float *v = part + (((int64_t)cib * n_cob + cob) * 9 + tap) * (WG_BLK * NCO) + col * WG_BLK + cil;
        double acc[4] = {0.0, 0.0, 0.0, 0.0};
        int k = 0;
        for (; k + 3 < n_groups; k += 4) {
#pragma unroll
            for (int u = 0; u < 4; ++u) acc[u] += (double)v[(int64_t)(k + u) * gstride];
        }
        for (int u = 0; k < n_groups; ++k, ++u) acc[u] += (double)v[(int64_t)k * gstride];
        dw[t] = (float)((acc[0] + acc[1]) + (acc[2] + acc[3]));
    }
}

// ---------------------------------------------------------------- host
// The input gradient's plan: shpl_upconv3x3's checks with gy as the source (c_gy channels) and dx as the output.
struct DgPlan {
    UpPlan up;
    int nb, n_cbg;  // dx blocks per workgroup, workgroups per tile
    size_t wp, total;
};

int dg_plan(int dtype, int n_frames, int64_t h, int64_t w, int64_t c_gy, int64_t c_dx, DgPlan *dp) {
    const int rc = up_plan(dtype, n_frames, h, w, c_gy, 0, c_dx, false, false, 0, &dp->up);
    if (rc) return rc;
    const int n_cib = dp->up.n_cob;
    dp->nb = n_cib >= 3 ? 4 : n_cib;
    dp->n_cbg = (n_cib + dp->nb - 1) / dp->nb;
    Layout l;  // the packed weights, zero blocks up to a whole number of workgroups
    dp->wp = l.take((size_t)dp->n_cbg * dp->nb * dp->up.qa * W_ROWS * Elem<float>::CB);
    dp->total = l.end;
    return SHPL_OK;
}

// The weight gradient's plan: shpl_upconv3x3's checks, the WTH x 32 tiling, wgrad_plan's rule for the groups.
struct UwPlan {
    UpPlan up;
    int n_cib, tiles_per_frame, n_groups, tiles_per_group;
    int64_t n_tiles;
    size_t row_ptr, part, total;
};

int uw_plan(int dtype, int n_frames, int64_t h, int64_t w, int64_t c_a, int64_t c_b, int64_t c_out, bool pooled,
            int64_t pool_cap, UwPlan *wp) {
    const int rc = up_plan(dtype, n_frames, h, w, c_a, c_b, c_out, pooled, false, pool_cap, &wp->up);
    if (rc) return rc;
    wp->n_cib = ((wp->up.qa + wp->up.qb) * wp->up.ck + WG_BLK - 1) / WG_BLK;
    wp->tiles_per_frame = wp->up.tiles_x * (int)((h + WTH - 1) / WTH);
    wp->n_tiles = (int64_t)n_frames * wp->tiles_per_frame;
    if (wp->n_tiles >= (1LL << 31)) return SHPL_ERR_BAD_SHAPE;
    const int64_t blocks_per_group = (int64_t)wp->n_cib * wp->up.n_cob;
    wgrad_groups(wp->n_tiles, blocks_per_group, &wp->tiles_per_group, &wp->n_groups);
    Layout l;
    wp->row_ptr = l.take(pooled ? (size_t)n_frames * (h + 1) * 4 : 0);
    wp->part = l.take((size_t)wp->n_groups * blocks_per_group * 9 * WG_BLK * NCO * sizeof(float));
    wp->total = l.end;
    return SHPL_OK;
}

}  // namespace
}  // namespace shpl

using namespace shpl;

// ---------------------------------------------------------------- the C ABI (include/shpl.h)
extern "C" int shpl_upconv3x3_dgrad_workspace_bytes(int dtype, int n_frames, int64_t h, int64_t w, int64_t c_gy,
                                                    int64_t c_dx, size_t *bytes) {
    if (!bytes) return SHPL_ERR_ARG;
    DgPlan dp;
    const int rc = dg_plan(dtype, n_frames, h, w, c_gy, c_dx, &dp);
    if (rc) return rc;
    *bytes = dp.total;
    return SHPL_OK;
}

extern "C" int shpl_upconv3x3_dgrad(int dtype, int n_frames, int64_t h, int64_t w, const void *d_gy, int64_t gy_stride,
                                    int64_t c_gy, const void *d_weights, int64_t c_dx, void *d_dx, int64_t dx_stride,
                                    int64_t c_split, void *d_dx_b, int64_t dx_b_stride, void *d_ws, size_t ws_bytes,
                                    void *stream) {
    DgPlan dp;
    int rc = dg_plan(dtype, n_frames, h, w, c_gy, c_dx, &dp);
    if (rc) return rc;
    if (!d_weights || (ws_bytes > 0 && !d_ws)) return SHPL_ERR_ARG;
    if (ws_bytes < dp.total) return SHPL_ERR_WORKSPACE;
    if (!d_dx_b) c_split = c_dx;
    if (c_split < 0 || c_split > c_dx) return SHPL_ERR_BAD_SHAPE;
    // the forward's source checks, dx's first map as the source and gy as the map of c_gy channels
    rc = check_sources(n_frames, h, w, {d_dx, dx_stride, 0, c_split}, {}, nullptr, nullptr, gy_stride, c_gy);
    if (rc) return rc;
    if (d_dx_b && dx_b_stride < c_dx - c_split) return SHPL_ERR_BAD_SHAPE;
    const UpPlan &pl = dp.up;
    if (pl.n_tiles == 0) return SHPL_OK;
    if (!d_gy || (c_split > 0 && !d_dx)) return SHPL_ERR_ARG;
    ConvArgs a = conv_args(dtype, n_frames, h, w, pl, {d_gy, gy_stride, 0, c_gy}, {}, nullptr);
    a.wp = region<void>(d_ws, dp.wp);
    a.out = d_dx;
    a.out_stride = dx_stride;
    a.c_out = (int)c_dx;
    a.out2 = d_dx_b;
    a.out2_stride = dx_b_stride;
    a.c_split = (int)c_split;
    a.vec_out = vec_out_split(d_dx, dx_stride, d_dx_b, dx_b_stride, c_split, piece_elems(dtype));
    hipStream_t s = (hipStream_t)stream;
    const int n_blk = dp.n_cbg * dp.nb;
    return by_dtype(dtype, [&](auto t) -> int {
        typedef typename decltype(t)::T T;
        if (const int rc = pack_weights<T>(a, d_weights, n_blk, 0, s)) return rc;
        using Kernel = void (*)(const ConvArgs);
        const Kernel kernel = dp.nb == 4   ? k_upconv3x3_dgrad<T, 4>
                              : dp.nb == 2 ? k_upconv3x3_dgrad<T, 2>
                                           : k_upconv3x3_dgrad<T, 1>;
        hipLaunchKernelGGL(kernel, dim3((unsigned)pl.n_tiles, (unsigned)dp.n_cbg), dim3(CONV_BLOCK), 0, s, a);
        SHPL_LAUNCH_CHECK();
        return SHPL_OK;
    });
}

extern "C" int shpl_upconv3x3_wgrad_workspace_bytes(int dtype, int n_frames, int64_t h, int64_t w, int64_t c_a,
                                                    int64_t c_b, int64_t c_out, int64_t pool_nnz_cap, size_t *bytes) {
    if (!bytes) return SHPL_ERR_ARG;
    UwPlan wp;
    const bool pooled = pool_nnz_cap >= 0;
    const int rc = uw_plan(dtype, n_frames, h, w, c_a, c_b, c_out, pooled, pooled ? pool_nnz_cap : 0, &wp);
    if (rc) return rc;
    *bytes = wp.total;
    return SHPL_OK;
}

extern "C" int shpl_upconv3x3_wgrad(int dtype, int n_frames, int64_t h, int64_t w, const void *d_a, int64_t a_stride,
                                    int64_t a_off, int64_t c_a, const void *d_b, int64_t b_stride, int64_t b_off,
                                    int64_t c_b, const shpl_csr *pool, const int64_t *d_frame_off, const void *d_gy,
                                    int64_t gy_stride, int64_t c_out, float *d_dw, void *d_ws, size_t ws_bytes,
                                    void *stream) {
    const bool pooled = pool != nullptr;
    const Src A = {d_a, a_stride, a_off, c_a}, B = {d_b, b_stride, b_off, c_b};
    UwPlan wp;
    int rc = uw_plan(dtype, n_frames, h, w, c_a, c_b, c_out, pooled, pooled ? pool->nnz_cap : 0, &wp);
    if (rc) return rc;
    if (!d_dw || (ws_bytes > 0 && !d_ws)) return SHPL_ERR_ARG;
    if (ws_bytes < wp.total) return SHPL_ERR_WORKSPACE;
    rc = check_sources(n_frames, h, w, A, B, pool, d_frame_off, gy_stride, c_out);
    if (rc) return rc;
    if (wp.n_tiles == 0) return SHPL_OK;
    if (!d_gy || (c_a > 0 && !d_a)) return SHPL_ERR_ARG;
    const UpPlan &pl = wp.up;
    const int he = piece_elems(dtype);
    ConvArgs a = conv_args(dtype, n_frames, h, w, pl, A, B, pool);
    a.tiles_per_frame = wp.tiles_per_frame;  // the WTH x 32 tiling
    a.n_tiles = (int)wp.n_tiles;
    a.row_ptr = pooled ? region<int32_t>(d_ws, wp.row_ptr) : nullptr;
    a.c_out = (int)c_out;
    UwArgs g = {};
    g.gy = d_gy;
    g.gy_stride = gy_stride;
    g.vec_g = vec16({d_gy, gy_stride, 0, c_out}, he);
    g.n_cib = wp.n_cib;
    g.n_cob = pl.n_cob;
    g.tiles_per_group = wp.tiles_per_group;
    g.part = region<float>(d_ws, wp.part);
    hipStream_t s = (hipStream_t)stream;
    if (pooled) {
        rc = row_pointers(a, d_frame_off, s);
        if (rc) return rc;
    }
    using Kernel = void (*)(const ConvArgs, const UwArgs);
    const Kernel kernel = by_dtype(dtype, [&](auto t) {
        typedef typename decltype(t)::T T;
        return pooled_form<Kernel>(pooled, a.ent_col,
                                   [](auto po, auto gr) -> Kernel { return k_upconv3x3_wgrad<T, po(), gr()>; });
    });
    hipLaunchKernelGGL(kernel, dim3((unsigned)wp.n_groups, (unsigned)wp.n_cib, (unsigned)pl.n_cob), dim3(CONV_BLOCK),
                       0, s, a, g);
    SHPL_LAUNCH_CHECK();
    const int64_t n_out = 9 * (c_a + c_b) * c_out;
    hipLaunchKernelGGL(k_upwgrad_reduce, dim3(grid_for(n_out, SHPL_BLOCK, 4096)), dim3(SHPL_BLOCK), 0, s, g.part,
                       wp.n_groups, wp.n_cib, pl.n_cob, (int)c_a, (int)c_b, pl.qa, pl.ck, (int)c_out, d_dw);
    SHPL_LAUNCH_CHECK();
    return SHPL_OK;
}
