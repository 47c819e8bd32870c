// shpl_conv.hip -- the post-fusion 3x3 convolution, with
// the SHPL concat (and, optionally, the img->BEV pooling itself) fused into
// its input staging.
//
// Reference (avod/avod/core/models/rpn_model.py:338-355, config switch
// rpn_sparse_pooling_conv_after_fusion, model.proto:88):
//     bv_fused = sparse_pool_layer([bev, img], ...)          # [1,Hb,Wb,Cb+Ci]
//     bev_out  = slim.conv2d(bv_fused, Ci, [3,3], normalizer_fn=slim.batch_norm,
//                            normalizer_params={'is_training': ...})
// i.e. SAME padding, stride 1, no bias, BatchNorm (center, no scale,
// eps 1e-3, decay 0.999), ReLU; and retinanet_model.py:343-348 (conv2d with
// bias + ReLU, no BN). Both epilogues are  y = act((acc - center) * scale + shift).
//
// Implicit GEMM on MFMA: M = output pixels, N = output channels (32 per
// workgroup), K = 9 taps x input channels. One workgroup owns an 8 x 32
// output tile of one frame; wave w owns tile rows 2w and 2w+1 (two 32-pixel
// M subtiles against all 32 channels: v_mfma_f32_32x32x2_f32 for f32,
// v_mfma_f32_32x32x16_bf16 for bf16 storage, f32 accumulation in both).
// The input channels are walked in chunks (8 f32 / 16 bf16 channels): a
// chunk of the 10 x 34 halo tile and the chunk's 9 x 32 weights are staged
// in LDS as 32-byte rows, unpadded and swizzled (conflict-free ds_read_b128)
// by LDS-DMA, then 9 taps of MFMAs consume them. Staging is synchronous;
// 5 workgroups per CU keep the MFMAs busy across each other's staging.
//
// Input channels [0, c_a) come from tensor A (the BEV map), [c_a, c_a+c_b)
// from tensor B. B is either a dense tensor (the materialised pooled map, or
// nothing) or -- POOLED -- the image feature map read through the img->BEV
// CSR of shpl_build_csr: the tile's runs of entries (one per occupied halo
// cell) are listed once in LDS; each pooled chunk is zero where no entry
// lands and the run's pooled vector elsewhere, computed on the spot with the
// arithmetic of k_sparse (shpl_pull.hip: TF order, separate multiply and
// add), so the conv of the fused form is bitwise the conv of
// [bev || shpl_pull(...)] and bv_fused never reaches HBM.
//
// The image side (rpn_model.py:347-354 over img_fused = [img || trans(bev)])
// is the same call with A the image map, B the BEV map and the pixel-keyed CSR
// as the pool: nothing here reads a key's meaning, only the sum of a run
// changes -- with ent_col it is TF's sum of per-column partials (GROUP:
// RunSum in shpl_common.h, walk_run<GROUP>'s arithmetic in shpl_pull.hip).
#include "shpl_conv_bn.h"
#include "shpl_conv_rows.h"
#include "shpl_conv_wide.h"
#include "shpl_conv_tile.h"

namespace shpl {
namespace {

// NCB: output-channel blocks per workgroup (blockIdx.y covers NCB of them):
// 2 for the input gradient's 64 output channels, so each staged input chunk
// feeds twice the MFMAs (one halo staging per tile instead of two). GROUP (POOLED): the pool is the pixel-keyed
// CSR with ent_col, its runs summed per column first (pool_piece).
template <typename T, bool POOLED, bool STATS, int NCB = 1, bool GROUP = false>
__global__ __launch_bounds__(CONV_BLOCK, NCB == 2 ? 3 : 4) void k_conv3x3(const ConvArgs p) {
    typedef Elem<T> E;
    constexpr int CK = E::CK, NP = E::NP;
    static_assert(NCB == 1 || !STATS, "statistics: one output block per workgroup");
    static_assert(NP == 2, "two 16-byte pieces per LDS row (the swizzle)");
    constexpr int IN_BYTES = HH * HWD * NP * 16, W_BYTES = W_ROWS * NP * 16 * NCB;
    // the output rows' transpose (epilogue) reuses the chunk buffers: 4 waves x 32 pixels x OPITCH
    static_assert(4 * 32 * OPITCH<T> <= IN_BYTES + W_BYTES, "epilogue rows fit the chunk buffers");
    __shared__ __attribute__((aligned(16))) uint8_t s_buf[IN_BYTES + W_BYTES];
    uint8_t *const s_in = s_buf, *const s_w = s_buf + IN_BYTES;
    __shared__ float s_red[4][2][NCO];
    __shared__ __attribute__((aligned(16))) float s_par[NCB][2][NCO];  // scale, shift - center * scale of the block's channels
    const HaloRuns runs = halo_runs_lds<POOLED>();

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int pl = lane & 31, hf = lane >> 5;
    // each XCD gets one contiguous run of tiles: neighbouring tiles share halo rows through that XCD's L2
    const int tile = (int)xcd_block((int)blockIdx.x, p.n_tiles);
    const int cob0 = blockIdx.y * NCB;
    int f, y0, x0;
    tile_origin<TH>(p, tile, f, y0, x0);
    const int H = p.h, W = p.w;
    const int64_t frame_row0 = (int64_t)f * H * W;
    const int Q = p.qa + p.qb;

    epilogue_coeffs<NCB>(p, cob0, s_par, tid);
    const int n_run = POOLED ? find_runs(p, f, y0, x0, runs) : 0;  // (s_par: published by the next barrier)

    f32x16 acc[NCB][RPW];
#pragma unroll
    for (int cb = 0; cb < NCB; ++cb)
#pragma unroll
        for (int m = 0; m < RPW; ++m)
#pragma unroll
            for (int i = 0; i < 16; ++i) acc[cb][m][i] = 0.0f;

    const int64_t wq_cb = (int64_t)Q * W_ROWS * CK;  // one output block further in the packed weights
    const T *wq = reinterpret_cast<const T *>(p.wp) + cob0 * wq_cb;
    for (int q = 0; q < Q; ++q) {
        // ---- stage chunk q, synchronously: the other workgroups on the CU (5
        // at f32) keep the MFMAs busy meanwhile. Measured and dropped: two LDS
        // buffers with chunk q+1's LDS-DMAs in flight under chunk q's MFMAs
        // (3 workgroups per CU: f32 fused 11.3 -> 12.1 ms), and a register-staged
        // prefetch (VGPRs 62 -> 86-168: 11.8 -> 12.5 ms)
        conv_stage<T, POOLED, NCB, GROUP>(p, q, f, y0, x0, wq, wq_cb, s_in, s_w, runs, n_run);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // the LDS-DMAs have landed
        __syncthreads();
        const uint8_t *si = s_in, *sw = s_w;
        // ---- 9 taps of MFMA over chunk q
        if constexpr (sizeof(T) == 4) {
#pragma unroll
            for (int ky = 0; ky < 3; ++ky) {
#pragma unroll
                for (int kx = 0; kx < 3; ++kx) {
                    f32x4 b4[NCB];
#pragma unroll
                    for (int cb = 0; cb < NCB; ++cb)
                        b4[cb] = *reinterpret_cast<const f32x4 *>(
                            sw + cb * (W_BYTES / NCB) + piece_off<true, 0>((ky * 3 + kx) * NCO + pl, hf));
#pragma unroll
                    for (int m = 0; m < RPW; ++m) {
                        const uint8_t *arow = si + piece_off<true, 0>((RPW * wave + m + ky) * HWD + pl + kx, hf);
                        // lane half h supplies channels 4h+s of the chunk to MFMA s (both operands)
                        const f32x4 a4 = *reinterpret_cast<const f32x4 *>(arow);
#pragma unroll
                        for (int cb = 0; cb < NCB; ++cb)
#pragma unroll
                            for (int s = 0; s < 4; ++s)
                                acc[cb][m] =
                                    __builtin_amdgcn_mfma_f32_32x32x2f32(b4[cb][s], a4[s], acc[cb][m], 0, 0, 0);
                    }
                }
            }
        } else {
            // channels 0..15 of the chunk; lane half h holds 8h .. 8h+7. Per kernel
            // column kx: the three kernel rows' weights, then each of the wave's
            // RPW + 2 halo rows read once and fed to every output row it reaches.
#pragma unroll
            for (int kx = 0; kx < 3; ++kx) {
                bf16x8 b8[NCB][3];
#pragma unroll
                for (int cb = 0; cb < NCB; ++cb)
#pragma unroll
                    for (int ky = 0; ky < 3; ++ky)
                        b8[cb][ky] = *reinterpret_cast<const bf16x8 *>(
                            sw + cb * (W_BYTES / NCB) + piece_off<true, 0>((ky * 3 + kx) * NCO + pl, hf));
#pragma unroll
                for (int r = 0; r < RPW + 2; ++r) {
                    const bf16x8 a8 = *reinterpret_cast<const bf16x8 *>(
                        si + piece_off<true, 0>((RPW * wave + r) * HWD + pl + kx, hf));
#pragma unroll
                    for (int cb = 0; cb < NCB; ++cb)
#pragma unroll
                        for (int ky = 0; ky < 3; ++ky)
                            if (r - ky >= 0 && r - ky < RPW)
                                acc[cb][r - ky] =
                                    __builtin_amdgcn_mfma_f32_32x32x16_bf16(b8[cb][ky], a8, acc[cb][r - ky], 0, 0, 0);
                }
            }
        }
        __syncthreads();  // the chunk's buffers are restaged next
    }

    // ---- epilogue (epilogue_row): acc element i of subtile m is channel cob*32 + 8(i>>2) + 4h + (i&3) of pixel
    // (y0 + RPW w + m, x0 + pl). The rows' transpose reuses the chunk buffers; the order of the two loops is the
    // statistics' summation order.
    uint8_t *const s_o = s_buf + wave * 32 * OPITCH<T>;
    ChanSums sums;
    sums.zero();
#pragma unroll
    for (int cb = 0; cb < NCB; ++cb) {
#pragma unroll
        for (int m = 0; m < RPW; ++m) {
            const int y = y0 + RPW * wave + m;
            const int64_t row = frame_row0 + (int64_t)y * W + x0;  // + column of the tile
            epilogue_row<T, true, STATS>(
                p, acc[cb][m], s_par[cb], s_o, (cob0 + cb) * NCO, y < H, x0, W, &sums,
                [row](const ConvArgs &a, int col, int c) { return out_ptr<T>(a, row + col, c); });
        }
    }
    if (STATS) stats_reduce_tile(p, sums, s_red, tid, cob0 * NCO, tile);
}

// Weight gradient: dW[tap][ci][co] = sum over pixels p of x[p + tap offset][ci] * g[p][co].
// One workgroup per (group of output tiles, 32 input channels, 32 output
// channels). Per tile it stages the input halo of its 32 channels ([chunk]
// [pixel][32 B], unpadded) and the 8x32-pixel gradient tile ([pixel][32
// channels], raw) in LDS -- dense sources by LDS-DMA, the whole tile in one
// round trip; pooled channels recomputed from the CSR by stage_halo, so
// bv_fused need not exist -- and wave w accumulates the 9 taps over tile
// rows 2w, 2w+1 with v_mfma_f32_16x16x4_f32 (M = 16 input channels, N = 16
// output channels, K = 4 pixels; 2 x 2 blocks per tap). Lane group kq walks
// 16 consecutive pixels of one row, so the three kx taps of a (ky, channel)
// are a sliding window: one new LDS read per (ky, channel half) per step.
// ~76 KB of LDS (f32): two workgroups per CU, so one stages while the
// other multiplies. The four waves' sums and then the groups' partials are
// added in a fixed order (k_wgrad_reduce): deterministic. Measured and
// dropped: 32 channels per workgroup with padded rows at one workgroup per
// CU (3.3x the forward's time), 16 channels per workgroup (2x: the gradient
// tile and the run list staged once per 16 channels), a register-staged
// prefetch of the next tile's halo (2 %: 256 registers).
constexpr int WG_CI = 32;  // input channels per workgroup

typedef float f32x4v __attribute__((ext_vector_type(4)));

struct WgArgs {
    const void *gy;
    int64_t gy_stride;
    int n_cib, n_cob, tiles_per_group;
    bool vec_g;
    bool whole;   // every 16-byte piece of A, B and gy lies inside its row: unmasked vector loads
    float *part;  // [((group * n_cib + cib) * n_cob + cob)][9][32][32]
};

// Stages one tile's inputs of the weight gradient in LDS, as 16-byte pieces:
// HALO: the 10x34 halo of the workgroup's WG_CI input channels (dense
// sources), s_x [chunk][pixel][CB bytes]; always: the 8x32 gradient tile of
// output channels [cob*32, cob*32+32), s_g [pixel][32 channels] raw. With
// g.whole (every piece inside its row) each piece is one LDS-DMA
// (global_load_lds_dwordx4: no registers, the whole tile in one round trip,
// the destination lane-linear per wave); otherwise masked loads + ds_write.
// The caller waits (vmcnt(0)) and synchronises.
template <typename T, bool HALO>
__device__ __forceinline__ void wg_stage(const ConvArgs &p, const WgArgs &g, int f, int y0, int x0, int cib, int cob,
                                         uint8_t *s_x, uint8_t *s_g) {
    typedef Elem<T> E;
    constexpr int CK = E::CK, HE = E::HE, NP = E::NP, CB = E::CB, NQ = WG_CI / CK;
    constexpr int NPIX = HH * HWD, IN_PIECES = NPIX * NP;
    constexpr int GPP = NCO / HE, G_PIECES = TH * TW * GPP;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int H = p.h, W = p.w;
    const int64_t frame_row0 = (int64_t)f * H * W;
    const u32x4 *zero = &g_zero_piece;
    const u32x4 z = u32x4{0u, 0u, 0u, 0u};
    if constexpr (HALO) {
        const int Q = p.qa + p.qb;
#pragma unroll
        for (int j = 0; j < NQ; ++j) {
            const int q = cib * NQ + j;
            const T *src;
            int64_t stride;
            int c_src, c0;
            bool vec;
            chunk_src<T, true>(p, q, src, stride, c_src, c0, vec);
#pragma unroll
            for (int u = 0; u < (IN_PIECES + CONV_BLOCK - 1) / CONV_BLOCK; ++u) {
                const int base = u * CONV_BLOCK + wave * 64;  // the wave's first piece
                if (base >= IN_PIECES) break;
                const int jj = base + lane;
                const HaloPix h = halo_pix(jj / NP, y0, x0, H, W);
                const bool ok = q < Q && jj < IN_PIECES && h.in;
                const int64_t row = frame_row0 + (int64_t)h.y * W + h.x;
                const int c = c0 + (jj % NP) * HE;
                uint8_t *dst = s_x + j * NPIX * CB + base * 16;
                if (jj < IN_PIECES) {
                    if (g.whole)
                        __builtin_amdgcn_global_load_lds(ok ? reinterpret_cast<const u32x4 *>(src + row * stride + c) : zero,
                                                         dst, 16, 0, 0);
                    else
                        *reinterpret_cast<u32x4 *>(dst + lane * 16) = ok ? load_piece<T>(src + row * stride, c, c_src, vec) : z;
                }
            }
        }
    }
    const T *gy = reinterpret_cast<const T *>(g.gy);
#pragma unroll
    for (int u = 0; u < G_PIECES / CONV_BLOCK; ++u) {
        const int base = u * CONV_BLOCK + wave * 64;
        const int i = base + lane;
        const int pix = i / GPP, pc = i - pix * GPP;
        const int y = y0 + pix / TW, xx = x0 + pix % TW;
        const bool ok = y < H && xx < W;
        const int64_t row = frame_row0 + (int64_t)y * W + xx;
        const int c = cob * NCO + pc * HE;
        uint8_t *dst = s_g + base * 16;
        if (g.whole)
            __builtin_amdgcn_global_load_lds(ok ? reinterpret_cast<const u32x4 *>(gy + row * g.gy_stride + c) : zero, dst,
                                             16, 0, 0);
        else
            *reinterpret_cast<u32x4 *>(dst + lane * 16) = ok ? load_piece<T>(gy + row * g.gy_stride, c, p.c_out, g.vec_g) : z;
    }
    static_assert(G_PIECES % CONV_BLOCK == 0, "gradient pieces");
}

template <typename T, bool POOLED, bool GROUP = false>
__global__ __launch_bounds__(CONV_BLOCK, POOLED ? 1 : 2) void k_conv3x3_wgrad(const ConvArgs p, const WgArgs g) {
    typedef Elem<T> E;
    constexpr int CK = E::CK, CB = E::CB, NQ = WG_CI / CK;
    constexpr int NPIX = HH * HWD;
    __shared__ __attribute__((aligned(16))) uint8_t s_x[NQ * NPIX * CB];
    __shared__ __attribute__((aligned(16))) uint8_t s_g[TH * TW * NCO * sizeof(T)];
    const HaloRuns runs = halo_runs_lds<POOLED>();
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int l16 = lane & 15, kq = lane >> 4;
    const int grp = blockIdx.x, cib = blockIdx.y, cob = blockIdx.z;
    const int Q = p.qa + p.qb;
    f32x4v acc[9][2][2];  // [tap][input-channel half][output-channel half]
#pragma unroll
    for (int t = 0; t < 9; ++t)
#pragma unroll
        for (int h = 0; h < 2; ++h)
#pragma unroll
            for (int o = 0; o < 2; ++o) acc[t][h][o] = f32x4v{0.0f, 0.0f, 0.0f, 0.0f};
    const int t0 = grp * g.tiles_per_group;
    const int t1 = t0 + g.tiles_per_group < p.n_tiles ? t0 + g.tiles_per_group : p.n_tiles;
    // this lane's input channels (rows of A): h*16 + l16 -> chunk (h*16 + l16) / CK, element % CK
    int a_off[2];
#pragma unroll
    for (int h = 0; h < 2; ++h) a_off[h] = ((h * 16 + l16) / CK) * NPIX * CB + ((h * 16 + l16) % CK) * (int)sizeof(T);
    for (int tile = t0; tile < t1; ++tile) {
        int f, y0, x0;
        tile_origin<TH>(p, tile, f, y0, x0);
        if constexpr (POOLED) {
            const int n_run = find_runs(p, f, y0, x0, runs);
#pragma unroll
            for (int j = 0; j < NQ; ++j) {
                const int q = cib * NQ + j;
                if (q < Q)
                    stage_halo<T, POOLED, CB, false, GROUP>(p, q, f, y0, x0, s_x + j * NPIX * CB, runs, n_run);
            }
        }
        wg_stage<T, !POOLED>(p, g, f, y0, x0, cib, cob, s_x, s_g);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // the LDS-DMAs have landed
        __syncthreads();
        // lane group kq walks tile row 2w + (kq >> 1), columns (kq & 1) * 16 + sp, sp = 0..15: the
        // three kx taps of a (ky, channel) are a sliding window over the halo row, so each
        // step reads one new input value per (ky, channel half) instead of three
        const int r = 2 * wave + (kq >> 1), cb = (kq & 1) * 16;
        float win[3][2][3];  // [ky][h][kx]: x at halo (r + ky, cb + sp + kx), channel h*16 + l16
#pragma unroll
        for (int ky = 0; ky < 3; ++ky)
#pragma unroll
            for (int h = 0; h < 2; ++h)
#pragma unroll
                for (int kx = 0; kx < 2; ++kx)
                    win[ky][h][kx] = E::f(*reinterpret_cast<const T *>(s_x + a_off[h] + ((r + ky) * HWD + cb + kx) * CB));
#pragma unroll 2
        for (int sp = 0; sp < 16; ++sp) {
#pragma unroll
            for (int ky = 0; ky < 3; ++ky)
#pragma unroll
                for (int h = 0; h < 2; ++h)
                    win[ky][h][2] =
                        E::f(*reinterpret_cast<const T *>(s_x + a_off[h] + ((r + ky) * HWD + cb + sp + 2) * CB));
            float b[2];
#pragma unroll
            for (int o = 0; o < 2; ++o)
                b[o] = E::f(reinterpret_cast<const T *>(s_g)[(r * TW + cb + sp) * NCO + o * 16 + l16]);
#pragma unroll
            for (int ky = 0; ky < 3; ++ky)
#pragma unroll
                for (int kx = 0; kx < 3; ++kx)
#pragma unroll
                    for (int h = 0; h < 2; ++h)
#pragma unroll
                        for (int o = 0; o < 2; ++o)
                            acc[ky * 3 + kx][h][o] =
                                __builtin_amdgcn_mfma_f32_16x16x4f32(win[ky][h][kx], b[o], acc[ky * 3 + kx][h][o], 0, 0, 0);
#pragma unroll
            for (int ky = 0; ky < 3; ++ky)
#pragma unroll
                for (int h = 0; h < 2; ++h) {
                    win[ky][h][0] = win[ky][h][1];
                    win[ky][h][1] = win[ky][h][2];
                }
        }
        __syncthreads();
    }
    // the four waves' sums, in wave order, into this workgroup's partial
    // (D of 16x16x4: column = lane & 15 (output channel), row = 4 (lane >> 4) + reg (input channel))
    float *red = reinterpret_cast<float *>(s_x);  // 4 x 1024 floats
    float *out = g.part + (((int64_t)grp * g.n_cib + cib) * g.n_cob + cob) * (9 * WG_CI * NCO);
#pragma unroll
    for (int t = 0; t < 9; ++t) {
#pragma unroll
        for (int h = 0; h < 2; ++h)
#pragma unroll
            for (int o = 0; o < 2; ++o)
#pragma unroll
                for (int i = 0; i < 4; ++i)
                    red[wave * 1024 + (h * 16 + 4 * kq + i) * NCO + o * 16 + l16] = acc[t][h][o][i];
        __syncthreads();
        for (int e = tid; e < WG_CI * NCO; e += CONV_BLOCK)
            out[t * 1024 + e] = __fadd_rn(__fadd_rn(__fadd_rn(red[e], red[1024 + e]), red[2048 + e]), red[3072 + e]);
        __syncthreads();
    }
}

// bf16 weight gradient on bf16 MFMA (v_mfma_f32_16x16x32_bf16: M = 16 input
// channels, N = 16 output channels, K = 32 pixels of one tile row). K runs
// along each lane's registers, so the staging transposes: the halo goes to
// LDS as [kx][channel][halo row][32 columns] -- three copies shifted by the
// tap's kx, so that every A fragment (8 pixels of one channel) is one
// aligned ds_read_b128 -- and the gradient tile as [co][row][32 columns]; the
// channel pitches are padded by 16 bytes (16 lanes' reads on distinct bank
// quads). Dense sources only (the pooled form stays on k_conv3x3_wgrad).
// Products of bf16 values are exact in f32; sums in f32 per workgroup, the
// same partials and k_wgrad_reduce as k_conv3x3_wgrad. Staging goes through
// registers, synchronously (one round trip per tile; two workgroups per CU).
// Measured and dropped: loading the next tile's pieces under this tile's
// MFMAs (4.50 -> 4.57 ms, 167 -> 197 VGPRs).
constexpr int WB_CIP = HH * TW * 2 + 16;  // bytes per input channel of one kx copy (10 rows x 32 bf16 + pad)
constexpr int WB_KXS = WG_CI * WB_CIP;    // bytes per kx copy
constexpr int WB_COP = TH * TW * 2 + 16;  // bytes per output channel of the gradient tile

__global__ __launch_bounds__(CONV_BLOCK, 2) void k_wgrad_bf16(const ConvArgs p, const WgArgs g) {
    typedef Elem<uint16_t> E;
    constexpr int CK = E::CK, HE = E::HE, NQ = WG_CI / CK;  // 16 channels per chunk, 2 chunks
    constexpr int IN_PIECES = NQ * HH * HWD * 2;              // (chunk, halo pixel, 8-channel piece)
    constexpr int IN_IT = (IN_PIECES + CONV_BLOCK - 1) / CONV_BLOCK;
    constexpr int G_PIECES = TH * TW * (NCO / HE);            // (pixel, 8-channel piece)
    constexpr int G_IT = G_PIECES / CONV_BLOCK;
    __shared__ __attribute__((aligned(16))) uint8_t s_x[3 * WB_KXS];
    __shared__ __attribute__((aligned(16))) uint8_t s_g[NCO * WB_COP];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int l16 = lane & 15, kq = lane >> 4;
    const int grp = blockIdx.x, cib = blockIdx.y, cob = blockIdx.z;
    const int Q = p.qa + p.qb;
    const int H = p.h, W = p.w;
    const uint16_t *gy = reinterpret_cast<const uint16_t *>(g.gy);
    // wave w owns input-channel half h = w >> 1 and output-channel half o = w & 1, all 8 rows and 9 taps
    const int h = wave >> 1, o = wave & 1;
    f32x4v acc[9];
#pragma unroll
    for (int t = 0; t < 9; ++t) acc[t] = f32x4v{0.0f, 0.0f, 0.0f, 0.0f};
    const int t0 = grp * g.tiles_per_group;
    const int t1 = t0 + g.tiles_per_group < p.n_tiles ? t0 + g.tiles_per_group : p.n_tiles;
    const u32x4 z = u32x4{0u, 0u, 0u, 0u};
    u32x4 xv[IN_IT], gv[G_IT];
    // the tile's pieces into registers, issued together
    auto load = [&](int tile) {
        int f, y0, x0;
        tile_origin<TH>(p, tile, f, y0, x0);
        const int64_t frame_row0 = (int64_t)f * H * W;
#pragma unroll
        for (int u = 0; u < IN_IT; ++u) {
            const int j = tid + u * CONV_BLOCK;
            const int q = cib * NQ + j / (HH * HWD * 2);
            const int rem = j % (HH * HWD * 2), pix = rem >> 1, pc = rem & 1;
            const HaloPix hp = halo_pix(pix, y0, x0, H, W);
            const bool ok = j < IN_PIECES && q < Q && hp.in;
            const uint16_t *src;
            int64_t stride;
            int c_src, c0;
            bool vec;
            chunk_src<uint16_t, true>(p, q, src, stride, c_src, c0, vec);
            const int64_t row = ok ? frame_row0 + (int64_t)hp.y * W + hp.x : frame_row0;
            const int c = ok ? c0 + pc * HE : 0;
            if (g.whole) {  // unmasked, branch-free: out-of-map pieces read row 0 and are zeroed
                const u32x4 v = *reinterpret_cast<const u32x4 *>(src + row * stride + c);
                xv[u] = ok ? v : z;
            } else {
                xv[u] = ok ? load_piece<uint16_t>(src + row * stride, c, c_src, vec) : z;
            }
        }
#pragma unroll
        for (int u = 0; u < G_IT; ++u) {
            const int i = tid + u * CONV_BLOCK;
            const int pix = i / (NCO / HE), pc = i % (NCO / HE);
            const int y = y0 + pix / TW, x = x0 + pix % TW;
            const bool ok = y < H && x < W;
            const int64_t row = ok ? frame_row0 + (int64_t)y * W + x : frame_row0;
            if (g.whole) {
                const u32x4 v = *reinterpret_cast<const u32x4 *>(gy + row * g.gy_stride + cob * NCO + pc * HE);
                gv[u] = ok ? v : z;
            } else {
                gv[u] = ok ? load_piece<uint16_t>(gy + row * g.gy_stride, cob * NCO + pc * HE, p.c_out, g.vec_g) : z;
            }
        }
    };
    for (int tile = t0; tile < t1; ++tile) {
        load(tile);
        // ---- transposed writes: halo pixel (hr, hc) feeds column hc - kx of copy kx
#pragma unroll
        for (int u = 0; u < IN_IT; ++u) {
            const int j = tid + u * CONV_BLOCK;
            if (j >= IN_PIECES) continue;
            const int jq = j / (HH * HWD * 2);
            const int rem = j % (HH * HWD * 2), pix = rem >> 1, pc = rem & 1;
            const int hr = pix / HWD, hc = pix - hr * HWD;
            uint16_t e[HE];
            __builtin_memcpy(e, &xv[u], 16);
#pragma unroll
            for (int kx = 0; kx < 3; ++kx) {
                const int c = hc - kx;
                if (c < 0 || c >= TW) continue;
                uint8_t *base = s_x + kx * WB_KXS + (jq * CK + pc * HE) * WB_CIP + (hr * TW + c) * 2;
#pragma unroll
                for (int k = 0; k < HE; ++k) *reinterpret_cast<uint16_t *>(base + k * WB_CIP) = e[k];
            }
        }
#pragma unroll
        for (int u = 0; u < G_IT; ++u) {
            const int i = tid + u * CONV_BLOCK;
            const int pix = i / (NCO / HE), pc = i % (NCO / HE);
            uint16_t e[HE];
            __builtin_memcpy(e, &gv[u], 16);
            uint8_t *base = s_g + (pc * HE) * WB_COP + pix * 2;
#pragma unroll
            for (int k = 0; k < HE; ++k) *reinterpret_cast<uint16_t *>(base + k * WB_COP) = e[k];
        }
        __syncthreads();
        // ---- one K step (the 32 pixels of a tile row) per row and tap
#pragma unroll 2
        for (int r = 0; r < TH; ++r) {
            const bf16x8 b = *reinterpret_cast<const bf16x8 *>(s_g + (o * 16 + l16) * WB_COP + (r * TW + kq * 8) * 2);
#pragma unroll
            for (int ky = 0; ky < 3; ++ky)
#pragma unroll
                for (int kx = 0; kx < 3; ++kx) {
                    const bf16x8 a = *reinterpret_cast<const bf16x8 *>(
                        s_x + kx * WB_KXS + (h * 16 + l16) * WB_CIP + ((r + ky) * TW + kq * 8) * 2);
                    acc[ky * 3 + kx] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, acc[ky * 3 + kx], 0, 0, 0);
                }
        }
        __syncthreads();
    }
    // this wave's block of the workgroup's partial
    // (D of 16x16x32: column = lane & 15 (output channel), row = 4 (lane >> 4) + reg (input channel))
    float *out = g.part + (((int64_t)grp * g.n_cib + cib) * g.n_cob + cob) * (9 * WG_CI * NCO);
#pragma unroll
    for (int t = 0; t < 9; ++t)
#pragma unroll
        for (int i = 0; i < 4; ++i) out[t * 1024 + (h * 16 + 4 * kq + i) * NCO + o * 16 + l16] = acc[t][i];
}

// dW (f32, HWIO [3][3][c_a+c_b][c_out]) = the groups' partials summed in
// group order (f64), channels mapped back from the chunk layout.
// dW[tap][ci][co] = sum over the n_groups partials, in group order. A block
// takes 32 consecutive outputs; its 8 lane groups walk every 8th group (4
// independent accumulators each, 4 loads in flight) and their sums are
// added in lane-group order: deterministic.
constexpr int WR_OUT = 32, WR_K = SHPL_BLOCK / WR_OUT;
__global__ __launch_bounds__(SHPL_BLOCK) void k_wgrad_reduce(const float *part, int n_groups, int n_cib, int n_cob,
                                                             int c_a, int c_b, int qa, int ck, int c_out, float *dw) {
    __shared__ double red[WR_K][WR_OUT];
    const int cin = c_a + c_b;
    const int64_t total = (int64_t)9 * cin * c_out;
    const int j = threadIdx.x % WR_OUT, kk = threadIdx.x / WR_OUT;
    for (int64_t t0 = (int64_t)blockIdx.x * WR_OUT; t0 < total; t0 += (int64_t)gridDim.x * WR_OUT) {
        const int64_t t = t0 + j;
        double sum = 0.0;
        if (t < total) {
            const int co = (int)(t % c_out);
            const int ci = (int)((t / c_out) % cin);
            const int tap = (int)(t / ((int64_t)c_out * cin));
            const int cs = ci < c_a ? ci : qa * ck + (ci - c_a);  // channel in the chunk layout
            const int cib = cs / WG_CI, cil = cs % WG_CI, cob = co / NCO, col = co % NCO;
            const int64_t gstride = (int64_t)n_cib * n_cob * (9 * WG_CI * NCO);  // one group further
            const float *v = part + ((int64_t)cib * n_cob + cob) * (9 * WG_CI * NCO) + tap * (WG_CI * NCO) +
                             cil * NCO + col;
            double acc[4] = {0.0, 0.0, 0.0, 0.0};
            int k = kk;
            for (; k + 3 * WR_K < n_groups; k += 4 * WR_K) {
#pragma unroll
                for (int u = 0; u < 4; ++u) acc[u] += (double)v[(int64_t)(k + u * WR_K) * gstride];
            }
            for (int u = 0; k < n_groups; k += WR_K, ++u) acc[u & 3] += (double)v[(int64_t)k * gstride];
            sum = (acc[0] + acc[1]) + (acc[2] + acc[3]);
        }
        red[kk][j] = sum;
        __syncthreads();
        if (kk == 0 && t < total) {
            double s2 = red[0][j];
            for (int q = 1; q < WR_K; ++q) s2 += red[q][j];
            dw[t] = (float)s2;
        }
        __syncthreads();
    }
}

// ---------------------------------------------------------------- host: plans
// The pooled operand of the row and wide forms (rows::prep_pooled, wide::prep; bf16): the occupancy words of
// every BEV row, their prefix counts, one compact pooled row per run -- as byte offsets and as addresses.
struct PooledAt { size_t occ, occ_base, cmp; };
struct Pooled { uint32_t *occ; int32_t *occ_base; uint16_t *cmp; };

PooledAt pooled_layout(Layout &l, bool on, int n_frames, int64_t h, int wpr, int64_t pool_cap, int64_t c_b) {
    const size_t words = on ? (size_t)n_frames * h * wpr * 4 : 0, runs = on ? (size_t)pool_cap * c_b * 2 : 0;
    const size_t occ = l.take(words), occ_base = l.take(words);
    return {occ, occ_base, l.take(runs)};
}

Pooled pooled_in(const void *ws, const PooledAt &at) {
    return {region<uint32_t>(ws, at.occ), region<int32_t>(ws, at.occ_base), region<uint16_t>(ws, at.cmp)};
}

// How the row kernels (k_conv_rows, k_wgrad_rows) cut an h x w map: strips of TW columns, wpr occupancy
// words per row, n_bands equal bands of about 60 rows (the kernels stage band + 2 rows, at most 64).
struct RowGeom { int strips, wpr, n_bands, band; };

RowGeom row_geom(int64_t h, int64_t w) {
    RowGeom g;
    g.strips = (int)((w + TW - 1) / TW);
    g.wpr = (int)((w + 31) / 32);
    g.n_bands = (int)((h + 59) / 60);
    g.band = (int)((h + g.n_bands - 1) / g.n_bands);
    return g;
}

struct ConvPlan : TilePlan {
    // the workspace, as byte offsets in this order: packed weights; k_row_ptr's row pointers (pooled); statistics
    // partials; the pooled operand (pooled, rows or wide_cmp); k_conv_rows' junk rows; the pooled map
    // materialised by shpl_pull (pooled, wide and not wide_cmp); its size
    size_t wp, row_ptr, part;
    PooledAt pooled;
    size_t junk, map, total;
    // k_conv_rows (bf16, at most 4 input chunks) and its bands and strips
    bool rows;
    RowGeom g;
    // k_conv_wide (bf16, input chunks of 64 channels, whole 256-channel output blocks, no statistics); pooled:
    // wide_cmp, or past the occupancy table's limits the materialised map
    bool wide, wide_cmp;
    int64_t pool_cap;
};

// Whether rows of `stride` bf16 elements keep every byte offset inside a frame of px > 0 pixels below 2^31
// (k_conv_wide's halo offsets are signed 32-bit).
bool frame_fits31(int64_t px, int64_t stride) { return stride <= ((1LL << 30) - 1) / px; }

// The tiles are TH x TW output pixels at both dtypes, for the forward and the weight gradient alike. pool_cap:
// the pooling CSR's entry capacity (pooled forward: sizes the compact buffer of pooled runs).
int conv_plan(int dtype, int n_frames, int64_t h, int64_t w, int64_t c_a, int64_t c_b, int64_t c_out, bool pooled,
              bool stats, ConvPlan *pl, int64_t pool_cap = 0) {
    if (dtype != SHPL_F32 && dtype != SHPL_BF16) return SHPL_ERR_ARG;
    if (n_frames < 0 || h < 0 || w < 0 || c_a < 0 || c_b < 0 || c_out < 1 || c_a + c_b < 1) return SHPL_ERR_BAD_SHAPE;
    if (h > (1 << 20) || w > (1 << 20) || c_a + c_b > (1 << 16) || c_out > (1 << 16)) return SHPL_ERR_BAD_SHAPE;
    if (pool_cap < 0 || pool_cap >= (1LL << 31)) return SHPL_ERR_BAD_SHAPE;
    const int chunk_b = Elem<float>::CB;  // the same at both dtypes
    pl->ck = by_dtype(dtype, [](auto t) { return Elem<typename decltype(t)::T>::CK; });
    pl->qa = (int)((c_a + pl->ck - 1) / pl->ck);
    pl->qb = (int)((c_b + pl->ck - 1) / pl->ck);
    pl->n_cob = (int)((c_out + NCO - 1) / NCO);
    pl->tiles_x = (int)((w + TW - 1) / TW);
    pl->tiles_y = (int)((h + TH - 1) / TH);
    pl->tiles_per_frame = pl->tiles_x * pl->tiles_y;
    pl->n_tiles = (int64_t)n_frames * pl->tiles_per_frame;
    if (pl->n_tiles >= (1LL << 31) || (int64_t)n_frames * h * w >= (1LL << 31)) return SHPL_ERR_BAD_SHAPE;
    pl->g = row_geom(h, w);
    const int64_t n_items = (int64_t)n_frames * pl->g.n_bands * pl->g.strips;
    // the occupancy table and the compact pooled rows hold this map
    const bool occ_fits = h * pl->g.wpr <= rows::OCC_MAX_WORDS && pool_cap * c_b * 2 < (1LL << 31);
    pl->rows = dtype == SHPL_BF16 && pl->qa + pl->qb <= 4 && c_a % 8 == 0 && c_b % 8 == 0 && h > 0 &&
               w > 0 && rows::supported(pl->qa + pl->qb, pl->qa) && (!pooled || occ_fits) && n_items < (1LL << 31);
    pl->wide = dtype == SHPL_BF16 && !stats && !pl->rows && h > 0 && w > 0 &&
               wide::supported(c_a, c_b, c_out) && (int64_t)n_frames * h * w * (c_b > 0 ? c_b : 1) < (1LL << 40) &&
               (!pooled || occ_fits || frame_fits31(h * w, c_b));  // the materialised map, in rows of c_b
    pl->wide_cmp = pl->wide && pooled && occ_fits;
    pl->pool_cap = pool_cap;
    size_t wp_bytes = (size_t)pl->n_cob * (pl->qa + pl->qb) * W_ROWS * chunk_b;
    if (pl->wide && wide::packed_bytes(c_a, c_b, c_out) > wp_bytes) wp_bytes = wide::packed_bytes(c_a, c_b, c_out);
    // statistics partials: one per tile (tiled kernel) or per item (k_conv_rows); a band is several tile rows
    // (ceil(h / 60) <= ceil(h / TH)) over the same strips, so the items never outnumber the tiles
    const int64_t n_part = stats ? pl->n_tiles : 0;
    Layout l;
    pl->wp = l.take(wp_bytes);
    pl->row_ptr = l.take(pooled ? (size_t)n_frames * (h + 1) * 4 : 0);
    pl->part = l.take((size_t)pl->n_cob * NCO * 2 * n_part * 8);
    pl->pooled = pooled_layout(l, pooled && (pl->rows || pl->wide_cmp), n_frames, h, pl->g.wpr, pool_cap, c_b);
    pl->junk = l.take(pl->rows ? 32 * NCO * 2 : 0);
    pl->map = l.take(pl->wide && pooled && !pl->wide_cmp ? (size_t)n_frames * h * w * c_b * 2 : 0);
    pl->total = l.end;
    return SHPL_OK;
}

// ---------------------------------------------------------------- host: forward and input gradient
// k_conv_rows (shpl_conv_rows.hip) and, pooled, its two preparatory launches
// (occupancy words + prefix counts per frame; the pooled vector of every run
// into the compact buffer). The packed weights are already in a.wp.
int conv_rows_launch(const ConvPlan &pl, const ConvArgs &a, void *ws, bool pooled, bool stats,
                     const int64_t *frame_off, double *d_stats, hipStream_t s) {
    rows::RowArgs r = {};
    r.a = reinterpret_cast<const uint16_t *>(a.a) + a.a_off;
    r.b = reinterpret_cast<const uint16_t *>(a.b) + a.b_off;
    r.a_stride = a.a_stride;
    r.b_stride = a.b_stride;
    r.c_a = a.c_a;
    r.c_b = a.c_b;
    r.h = a.h;
    r.w = a.w;
    r.strips = pl.g.strips;
    r.band = pl.g.band;
    r.n_bands = pl.g.n_bands;
    r.n_items = a.n_frames * pl.g.n_bands * pl.g.strips;
    r.wp = reinterpret_cast<const uint16_t *>(a.wp);
    r.center = a.center;
    r.scale = a.scale;
    r.shift = a.shift;
    r.out = reinterpret_cast<uint16_t *>(a.out);
    r.out_stride = a.out_stride;
    r.wpr = pl.g.wpr;
    r.frame_off = frame_off;
    r.out2 = reinterpret_cast<uint16_t *>(a.out2);
    r.out2_stride = a.out2_stride;
    r.c_split = a.c_split;
    r.occ2 = a.occ2;
    r.n_cob = pl.n_cob;
    r.part = stats ? a.part : nullptr;
    r.junk = region<uint16_t>(ws, pl.junk);
    if (pooled) {
        const Pooled po = pooled_in(ws, pl.pooled);
        const int rc = rows::prep_pooled(a.n_frames, a.h, a.w, pl.g.wpr, a.ent_dst, a.ent_src, a.ent_val, a.ent_col,
                                         pl.pool_cap, frame_off, reinterpret_cast<const uint16_t *>(a.b), a.b_stride,
                                         a.b_off, a.c_b, po.occ, po.occ_base, po.cmp, s);
        if (rc) return rc;
        r.occ = po.occ;
        r.occ_base = po.occ_base;
        r.cmp = po.cmp;
    }
    int rc = rows::launch(r, pl.qa + pl.qb, pl.qa, pooled, a.act == 1, stats, s);
    if (rc || !stats) return rc;
    hipLaunchKernelGGL(k_stats_reduce, dim3(pl.n_cob * NCO * 2), dim3(RED_BLOCK), 0, s, a.part, r.n_items, a.c_out,
                       d_stats);
    SHPL_LAUNCH_CHECK();
    return SHPL_OK;
}

// Whether a bf16 call with this plan and these arguments runs the row-streaming form (k_conv_rows, and pooled
// its prep: the occupancy maps and per-run pooled rows in the workspace). The one predicate conv_launch and
// shpl_conv3x3_rows_form (which the weight gradient's reuse of the forward's workspace hangs on) share.
bool rows_forward(const ConvPlan &pl, const ConvArgs &a, bool pooled, bool stats) {
    return pl.rows && a.vec_a && (a.c_b == 0 || a.vec_b) && (!a.out2 || a.c_split % NCO == 0) && a.vec_out &&
           a.c_out % NCO == 0 && a.n_frames > 0 &&
           (!stats || (a.act == 0 && rows::supported_st(pl.qa + pl.qb, pl.qa, pooled)));
}

// Which form of the wide bf16 kernel (k_conv_wide) a forward with this plan and these arguments runs: 0 none
// (the row or tiled kernels), 1 with B dense or absent, 2 over the compact pooled runs (wide::prep), 3 over
// the pooled map materialised by shpl_pull. The one predicate conv_launch and shpl_conv3x3_wide_form share.
// k_conv_wide keeps a lane's halo source as a signed 32-bit byte offset inside its frame, so every map it
// reads by rows -- A, a dense B, the materialised map -- must end within 2^31 bytes of its frame's start; the
// tiled kernel, which addresses in 64 bits, takes the rest.
int wide_forward(const ConvPlan &pl, const ConvArgs &a, const shpl_csr *pool, bool stats) {
    if (!pl.wide || stats || a.out2 || !a.vec_a || (a.c_b != 0 && !a.vec_b) || !a.vec_out || a.n_frames <= 0)
        return 0;
    const int64_t px = (int64_t)a.h * a.w;
    if (!frame_fits31(px, a.a_stride)) return 0;
    if (!pool) return a.c_b == 0 || frame_fits31(px, a.b_stride) ? 1 : 0;
    return pl.wide_cmp ? 2 : 3;  // the map's rows of c_b elements: conv_plan has counted them
}

// The wide bf16 form (k_conv_wide). Pooled: B's rows are the compact pooled runs (wide::prep), or -- past
// the occupancy table -- the pooled map, materialised first by shpl_pull (the same arithmetic as the tiled
// staging: the conv of [a || map] is the fused conv's).
int conv_wide_launch(const ConvPlan &pl, const ConvArgs &a, void *ws, const shpl_csr *pool, const int64_t *frame_off,
                     const void *w, hipStream_t s) {
    wide::WideArgs r = {};
    r.a = reinterpret_cast<const uint16_t *>(a.a) + a.a_off;
    r.a_stride = a.a_stride;
    r.c_a = a.c_a;
    r.c_b = a.c_b;
    if (pool && pl.wide_cmp) {
        const Pooled po = pooled_in(ws, pl.pooled);
        const int rc = wide::prep(a.n_frames, a.h, a.w, pl.g.wpr, pool->ent_dst, pool->ent_src, pool->ent_val,
                                  pool->ent_col, pool->nnz_cap, frame_off, reinterpret_cast<const uint16_t *>(a.b),
                                  a.b_stride, a.b_off, a.c_b, po.occ, po.occ_base, po.cmp, s);
        if (rc) return rc;
        r.occ = po.occ;
        r.occ_base = po.occ_base;
        r.frame_off = frame_off;
        r.cmp = po.cmp;
        r.wpr = pl.g.wpr;
    } else if (pool) {
        uint16_t *map = region<uint16_t>(ws, pl.map);
        const int rc = shpl_pull(pixel_keyed(pool) ? SHPL_BY_PIXEL : SHPL_BY_CELL, SHPL_BF16, pool, a.b, a.b_stride,
                                 a.b_off, a.c_b, nullptr, 0, 0, 0, SHPL_OUT_POOL, map, a.c_b, s);
        if (rc) return rc;
        r.b = map;
        r.b_stride = a.c_b;
    } else {
        r.b = a.c_b > 0 ? reinterpret_cast<const uint16_t *>(a.b) + a.b_off : nullptr;
        r.b_stride = a.b_stride;
    }
    r.n_frames = a.n_frames;
    r.h = a.h;
    r.w = a.w;
    r.center = a.center;
    r.scale = a.scale;
    r.shift = a.shift;
    r.act = a.act;
    r.out = reinterpret_cast<uint16_t *>(a.out);
    r.out_stride = a.out_stride;
    r.c_out = a.c_out;
    return wide::launch(r, reinterpret_cast<const uint16_t *>(w),
                        reinterpret_cast<uint16_t *>(const_cast<void *>(a.wp)), s);
}

// ws: the call's workspace, laid out by pl.
template <typename T>
int conv_launch(const ConvPlan &pl, ConvArgs &a, void *ws, bool pooled, bool stats, const void *w,
                const int64_t *frame_off, double *d_stats, hipStream_t s, int transpose = 0,
                const shpl_csr *pool = nullptr) {
    if constexpr (sizeof(T) == 2) {
        if (!transpose && (!pooled || pool) && wide_forward(pl, a, pooled ? pool : nullptr, stats))
            return conv_wide_launch(pl, a, ws, pooled ? pool : nullptr, frame_off, w, s);
    }
    if (const int rc = pack_weights<T>(a, w, pl.n_cob, transpose, s)) return rc;
    if constexpr (sizeof(T) == 2) {
        // bf16 with at most 64 input channels: the row-streaming kernel (k_conv_rows), also for the input
        // gradient's two maps (split at a whole output block) and the training forward's statistics
        if (rows_forward(pl, a, pooled, stats))
            return conv_rows_launch(pl, a, ws, pooled, stats, frame_off, d_stats, s);
    }
    if (pooled) {
        if (const int rc = row_pointers(a, frame_off, s)) return rc;
    }
    const dim3 grid((unsigned)pl.n_tiles, (unsigned)pl.n_cob);
    // f32, an even number of dense output blocks (the input gradient's 64
    // channels): two per workgroup, 12.11 -> 11.47 ms at 64 frames. bf16 gains
    // nothing (2.73 / 2.77 ms: 3 waves per SIMD instead of 6 for a
    // memory-pipeline-bound kernel) and keeps one.
    const bool pair = sizeof(T) == 4 && !pooled && !stats && pl.n_cob % 2 == 0;
    using Kernel = void (*)(const ConvArgs);
    const Kernel kernel = pooled_form<Kernel>(pooled, a.ent_col, [&](auto po, auto gr) -> Kernel {
        if constexpr (sizeof(T) == 4 && !po())  // the only pair form: `pair` says so for no other
            if (pair) return k_conv3x3<T, false, false, 2>;
        return stats ? k_conv3x3<T, po(), true, 1, gr()> : k_conv3x3<T, po(), false, 1, gr()>;
    });
    hipLaunchKernelGGL(kernel, pair ? dim3(grid.x, grid.y / 2) : grid, dim3(CONV_BLOCK), 0, s, a);
    SHPL_LAUNCH_CHECK();
    if (stats) {
        hipLaunchKernelGGL(k_stats_reduce, dim3(pl.n_cob * NCO * 2), dim3(RED_BLOCK), 0, s, a.part, (int)pl.n_tiles,
                           a.c_out, d_stats);
        SHPL_LAUNCH_CHECK();
    }
    return SHPL_OK;
}

// shpl_conv3x3's argument checks and kernel arguments (shared with shpl_conv3x3_rows_form). *empty: no pixel.
int forward_setup(int dtype, int n_frames, int64_t h, int64_t w, const Src &A, const Src &B, const shpl_csr *pool,
                  const int64_t *d_frame_off, const void *d_weights, int64_t c_out, const float *d_center,
                  const float *d_scale, const float *d_shift, int act, void *d_out, int64_t out_stride, bool stats,
                  void *d_ws, size_t ws_bytes, bool check_ws, ConvPlan &pl, ConvArgs &a, bool *empty) {
    const bool pooled = pool != nullptr;
    *empty = false;
    int rc = conv_plan(dtype, n_frames, h, w, A.c, B.c, c_out, pooled, stats, &pl, pooled ? pool->nnz_cap : 0);
    if (rc) return rc;
    if (act != 0 && act != 1) return SHPL_ERR_ARG;
    if (!d_weights || (check_ws && ws_bytes > 0 && !d_ws)) return SHPL_ERR_ARG;
    if (check_ws && ws_bytes < pl.total) return SHPL_ERR_WORKSPACE;
    rc = check_sources(n_frames, h, w, A, B, pool, d_frame_off, out_stride, c_out);
    if (rc) return rc;
    if (pl.n_tiles == 0) {
        *empty = true;
        return SHPL_OK;
    }
    if (!d_out || (A.c > 0 && !A.p)) return SHPL_ERR_ARG;
    a = conv_args(dtype, n_frames, h, w, pl, A, B, pool);  // what the forward does not set (out2: the dgrad split) is zero
    a.wp = region<void>(d_ws, pl.wp);
    a.row_ptr = pooled ? region<int32_t>(d_ws, pl.row_ptr) : nullptr;
    a.part = stats ? region<double>(d_ws, pl.part) : nullptr;
    a.center = d_center;
    a.scale = d_scale;
    a.shift = d_shift;
    a.act = act;
    a.out = d_out;
    a.out_stride = out_stride;
    a.c_out = (int)c_out;
    a.vec_out = vec16({d_out, out_stride, 0, c_out}, piece_elems(dtype));
    return SHPL_OK;
}

// The pooled operand that a pooled bf16 forward (shpl_conv3x3 of [A (c_a) || B pooled (c_b)] to c_out channels,
// with statistics or not) left in its workspace, where its plan put it. SHPL_ERR_ARG when that forward did not
// run the row form or its workspace is smaller than its plan, as far as can be told here: the rest of
// rows_forward (its act and output alignment) is the caller's to establish with shpl_conv3x3_rows_form (shpl.h).
int forward_pooled(int dtype, int n_frames, int64_t h, int64_t w, int64_t c_a, int64_t c_b, int64_t c_out,
                   int64_t pool_cap, int fwd_stats, const void *d_fwd_ws, size_t fwd_ws_bytes, Pooled *po) {
    ConvPlan fp;
    const int rc = conv_plan(dtype, n_frames, h, w, c_a, c_b, c_out, true, fwd_stats != 0, &fp, pool_cap);
    if (rc) return rc;
    if (!fp.rows || fwd_ws_bytes < fp.total || c_out % NCO != 0 ||
        (fwd_stats != 0 && !rows::supported_st(fp.qa + fp.qb, fp.qa, true)))
        return SHPL_ERR_ARG;
    *po = pooled_in(d_fwd_ws, fp.pooled);
    return SHPL_OK;
}

// shpl_conv3x3_dgrad; occ2: the occupancy words (wpr per row) limiting d_dx_b's stores (shpl_conv3x3_dgrad_reuse)
int dgrad_impl(int dtype, int n_frames, int64_t h, int64_t w, const void *d_gy, int64_t gy_stride, int64_t c_gy,
               const void *d_weights, int64_t c_dx, void *d_dx, int64_t dx_stride, int64_t c_split, void *d_dx_b,
               int64_t dx_b_stride, void *d_ws, size_t ws_bytes, const uint32_t *occ2, void *stream) {
    ConvPlan pl;
    int rc = conv_plan(dtype, n_frames, h, w, c_gy, 0, c_dx, false, false, &pl);
    if (rc) return rc;
    if (!d_weights || (ws_bytes > 0 && !d_ws)) return SHPL_ERR_ARG;
    if (ws_bytes < pl.total) return SHPL_ERR_WORKSPACE;
    if (!d_dx_b) c_split = c_dx;
    if (c_split < 0 || c_split > c_dx) return SHPL_ERR_BAD_SHAPE;
    if (gy_stride < c_gy || dx_stride < c_split || (d_dx_b && dx_b_stride < c_dx - c_split))
        return SHPL_ERR_BAD_SHAPE;
    if (pl.n_tiles == 0) return SHPL_OK;
    if (!d_gy || (c_split > 0 && !d_dx)) return SHPL_ERR_ARG;
    ConvArgs a = conv_args(dtype, n_frames, h, w, pl, {d_gy, gy_stride, 0, c_gy}, {}, nullptr);
    a.wp = region<void>(d_ws, pl.wp);
    a.out = d_dx;
    a.out_stride = dx_stride;
    a.c_out = (int)c_dx;
    a.out2 = d_dx_b;
    a.out2_stride = dx_b_stride;
    a.c_split = (int)c_split;
    a.vec_out = vec_out_split(d_dx, dx_stride, d_dx_b, dx_b_stride, c_split, piece_elems(dtype));
    a.occ2 = d_dx_b ? occ2 : nullptr;
    hipStream_t s = (hipStream_t)stream;
    return by_dtype(dtype, [&](auto t) {
        return conv_launch<typename decltype(t)::T>(pl, a, d_ws, false, false, d_weights, nullptr, nullptr, s, 1);
    });
}

// ---------------------------------------------------------------- host: weight gradient
struct WgPlan {
    ConvPlan cp;
    int n_cib, n_groups, tiles_per_group;
    // the workspace holds either form. The tiled form's regions (byte offsets): row pointers (pooled), partials
    size_t row_ptr, part, total;
    // bf16: k_wgrad_rows when the pointers are 16-byte aligned, over its own 60-row bands. Its regions: the
    // groups' partials, their f64 sums, the pooled operand (pooled; unused when a forward lends its own)
    bool rows;
    RowGeom g;
    int r_groups;
    size_t r_part, r_part2;
    PooledAt r_pooled;
};

int wgrad_plan(int dtype, int n_frames, int64_t h, int64_t w, int64_t c_a, int64_t c_b, int64_t c_out, bool pooled,
               WgPlan *wp, int64_t pool_cap = 0) {
    int rc = conv_plan(dtype, n_frames, h, w, c_a, c_b, c_out, pooled, false, &wp->cp);
    if (rc) return rc;
    const int Q = wp->cp.qa + wp->cp.qb;
    wp->n_cib = (Q * wp->cp.ck + WG_CI - 1) / WG_CI;
    const int64_t blocks_per_group = (int64_t)wp->n_cib * wp->cp.n_cob;
    wgrad_groups(wp->cp.n_tiles, blocks_per_group, &wp->tiles_per_group, &wp->n_groups);
    Layout t;
    wp->row_ptr = t.take(pooled ? (size_t)n_frames * (h + 1) * 4 : 0);
    wp->part = t.take((size_t)wp->n_groups * blocks_per_group * 9 * WG_CI * NCO * sizeof(float));
    wp->total = t.end;
    // the row-streaming bf16 weight gradient: bands and strips of the forward's row kernel
    wp->g = row_geom(h, w);
    const int64_t n_items = (int64_t)n_frames * wp->g.n_bands * wp->g.strips;
    // pooled: B gathered from the compact pooled rows of prep_pooled (the forward's k_occ_frame + k_pool_runs)
    wp->rows = dtype == SHPL_BF16 && h > 0 && w > 0 && n_items > 0 && n_items < (1LL << 31) &&
               rows::wgrad_supported((int)c_a, (int)c_b, (int)c_out) &&
               (!pooled || (c_a > 0 && c_b <= 64 && h * wp->g.wpr <= rows::OCC_MAX_WORDS && pool_cap >= 0 &&
                            pool_cap * c_b * 2 < (1LL << 31)));
    if (wp->rows) {
        size_t part_bytes, part2_bytes;
        rows::wgrad_sizes((int)n_items, (int)c_a, (int)c_b, (int)c_out, &wp->r_groups, &part_bytes, &part2_bytes);
        Layout r;
        wp->r_part = r.take(part_bytes);
        wp->r_part2 = r.take(part2_bytes);
        wp->r_pooled = pooled_layout(r, pooled, n_frames, h, wp->g.wpr, pool_cap, c_b);
        if (r.end > wp->total) wp->total = r.end;
    }
    return SHPL_OK;
}

// shpl_conv3x3_wgrad; d_fwd_ws: the workspace of a pooled bf16 forward shpl_conv3x3 call over the same map
// (shpl_conv3x3_wgrad_reuse) whose pooled operand the row-streaming form reads instead of preparing its own
int wgrad_impl(int dtype, int n_frames, int64_t h, int64_t w, const Src &A, const Src &B, const shpl_csr *pool,
               const int64_t *d_frame_off, const void *d_gy, int64_t gy_stride, int64_t c_out, float *d_dw,
               void *d_ws, size_t ws_bytes, const void *d_fwd_ws, size_t fwd_ws_bytes, int fwd_stats,
               void *stream) {
    const bool pooled = pool != nullptr;
    WgPlan wp;
    int rc = wgrad_plan(dtype, n_frames, h, w, A.c, B.c, c_out, pooled, &wp, pooled ? pool->nnz_cap : 0);
    if (rc) return rc;
    if (!d_dw || (ws_bytes > 0 && !d_ws)) return SHPL_ERR_ARG;
    if (ws_bytes < wp.total) return SHPL_ERR_WORKSPACE;
    rc = check_sources(n_frames, h, w, A, B, pool, d_frame_off, gy_stride, c_out);
    if (rc) return rc;
    if ((A.c > 0 && !A.p) || !d_gy) return SHPL_ERR_ARG;
    const ConvPlan &pl = wp.cp;
    const int he = piece_elems(dtype);
    const bool vec_g = vec16({d_gy, gy_stride, 0, c_out}, he);
    hipStream_t s = (hipStream_t)stream;
    if (pl.n_tiles == 0) {  // no pixels: dW = 0
        SHPL_HIP_CHECK(hipMemsetAsync(d_dw, 0, sizeof(float) * 9 * (size_t)(A.c + B.c) * c_out, s));
        return SHPL_OK;
    }
    if (wp.rows && (A.c == 0 || vec16(A, he)) && (B.c == 0 || vec16(B, he)) && vec_g &&
        (!pooled || A.c % 32 == 0)) {
        rows::WgRowArgs r = {};
        r.a = reinterpret_cast<const uint16_t *>(A.p) + A.off;
        r.b = B.c > 0 ? reinterpret_cast<const uint16_t *>(B.p) + B.off : nullptr;
        r.a_stride = A.stride;
        r.b_stride = B.stride;
        r.c_a = (int)A.c;
        r.c_b = (int)B.c;
        r.gy = reinterpret_cast<const uint16_t *>(d_gy);
        r.gy_stride = gy_stride;
        r.c_out = (int)c_out;
        r.h = (int)h;
        r.w = (int)w;
        r.strips = wp.g.strips;
        r.n_bands = wp.g.n_bands;
        r.band = wp.g.band;
        r.n_items = n_frames * r.n_bands * r.strips;
        r.n_cit = (int)((A.c + 31) / 32 + (B.c + 31) / 32);
        r.n_cot = (int)((c_out + 31) / 32);
        r.n_groups = wp.r_groups;
        r.part = region<float>(d_ws, wp.r_part);
        if (pooled) {
            // the forward call's occupancy maps and pooled runs when it lends them (what is checkable of that and
            // fails is an error, not a fallback); otherwise this call's own, by the forward's prep
            Pooled po = pooled_in(d_ws, wp.r_pooled);
            if (d_fwd_ws) {
                if (forward_pooled(dtype, n_frames, h, w, A.c, B.c, c_out, pool->nnz_cap, fwd_stats, d_fwd_ws,
                                   fwd_ws_bytes, &po) != SHPL_OK)
                    return SHPL_ERR_ARG;
            } else {
                rc = rows::prep_pooled(n_frames, (int)h, (int)w, wp.g.wpr, pool->ent_dst, pool->ent_src,
                                       pool->ent_val, pool->ent_col, pool->nnz_cap, d_frame_off,
                                       reinterpret_cast<const uint16_t *>(B.p), B.stride, B.off, (int)B.c, po.occ,
                                       po.occ_base, po.cmp, s);
                if (rc) return rc;
            }
            r.b = nullptr;
            r.cmp = po.cmp;
            r.cmp_stride = (int)B.c;
            r.occ = po.occ;
            r.occ_base = po.occ_base;
            r.wpr = wp.g.wpr;
            r.frame_off = d_frame_off;
        }
        return rows::wgrad_launch(r, d_dw, region<double>(d_ws, wp.r_part2), s);
    }
    ConvArgs a = conv_args(dtype, n_frames, h, w, pl, A, B, pool);
    a.row_ptr = pooled ? region<int32_t>(d_ws, wp.row_ptr) : nullptr;
    a.c_out = (int)c_out;
    WgArgs g = {};
    g.gy = d_gy;
    g.gy_stride = gy_stride;
    g.n_cib = wp.n_cib;
    g.n_cob = pl.n_cob;
    g.tiles_per_group = wp.tiles_per_group;
    g.vec_g = vec_g;
    g.whole = (A.c == 0 || (a.vec_a && A.c % pl.ck == 0)) && (B.c == 0 || (a.vec_b && B.c % pl.ck == 0)) &&
              g.vec_g && c_out % NCO == 0;
    g.part = region<float>(d_ws, wp.part);
    if (pooled) {
        rc = row_pointers(a, d_frame_off, s);
        if (rc) return rc;
    }
    const dim3 grid((unsigned)wp.n_groups, (unsigned)wp.n_cib, (unsigned)pl.n_cob);
    using Kernel = void (*)(const ConvArgs, const WgArgs);
    const Kernel kernel = by_dtype(dtype, [&](auto t) {
        typedef typename decltype(t)::T T;
        return pooled_form<Kernel>(pooled, a.ent_col, [](auto po, auto gr) -> Kernel {
            if constexpr (sizeof(T) == 2 && !po())
                return k_wgrad_bf16;  // dense bf16 sources: the bf16 MFMA kernel
            else
                return k_conv3x3_wgrad<T, po(), gr()>;
        });
    });
    hipLaunchKernelGGL(kernel, grid, dim3(CONV_BLOCK), 0, s, a, g);
    SHPL_LAUNCH_CHECK();
    const int64_t n_out = 9 * (A.c + B.c) * c_out;
    hipLaunchKernelGGL(k_wgrad_reduce, dim3(grid_for(n_out, WR_OUT, 4096)), dim3(SHPL_BLOCK), 0, s, g.part,
                       wp.n_groups, wp.n_cib, pl.n_cob, (int)A.c, (int)B.c, pl.qa, pl.ck, (int)c_out, d_dw);
    SHPL_LAUNCH_CHECK();
    return SHPL_OK;
}

}  // namespace
}  // namespace shpl

using namespace shpl;

// ---------------------------------------------------------------- the C ABI (include/shpl.h)
extern "C" int shpl_conv3x3_workspace_bytes(int dtype, int n_frames, int64_t h, int64_t w, int64_t c_a, int64_t c_b,
                                            int64_t c_out, int64_t pool_nnz_cap, int stats, size_t *bytes) {
    if (!bytes) return SHPL_ERR_ARG;
    ConvPlan pl;
    const bool pooled = pool_nnz_cap >= 0;
    const int rc = conv_plan(dtype, n_frames, h, w, c_a, c_b, c_out, pooled, stats != 0, &pl,
                             pooled ? pool_nnz_cap : 0);
    if (rc) return rc;
    *bytes = pl.total;
    return SHPL_OK;
}

extern "C" int shpl_conv3x3(int dtype, int n_frames, int64_t h, int64_t w, const void *d_a, int64_t a_stride,
                            int64_t a_off, int64_t c_a, const void *d_b, int64_t b_stride, int64_t b_off,
                            int64_t c_b, const shpl_csr *pool, const int64_t *d_frame_off, const void *d_weights,
                            int64_t c_out, const float *d_center, const float *d_scale, const float *d_shift,
                            int act, void *d_out, int64_t out_stride, double *d_stats, void *d_ws, size_t ws_bytes,
                            void *stream) {
    const bool pooled = pool != nullptr, stats = d_stats != nullptr;
    ConvPlan pl;
    ConvArgs a;
    bool empty;
    const int rc = forward_setup(dtype, n_frames, h, w, {d_a, a_stride, a_off, c_a}, {d_b, b_stride, b_off, c_b}, pool,
                                 d_frame_off, d_weights, c_out, d_center, d_scale, d_shift, act, d_out, out_stride,
                                 stats, d_ws, ws_bytes, true, pl, a, &empty);
    if (rc || empty) return rc;
    hipStream_t s = (hipStream_t)stream;
    return by_dtype(dtype, [&](auto t) {
        return conv_launch<typename decltype(t)::T>(pl, a, d_ws, pooled, stats, d_weights, d_frame_off, d_stats, s, 0,
                                                    pool);
    });
}

extern "C" int shpl_conv3x3_rows_form(int dtype, int n_frames, int64_t h, int64_t w, const void *d_a,
                                      int64_t a_stride, int64_t a_off, int64_t c_a, const void *d_b, int64_t b_stride,
                                      int64_t b_off, int64_t c_b, const shpl_csr *pool, const int64_t *d_frame_off,
                                      const void *d_weights, int64_t c_out, int act, const void *d_out,
                                      int64_t out_stride, int stats, int *rows_form) {
    if (!rows_form) return SHPL_ERR_ARG;
    *rows_form = 0;
    ConvPlan pl;
    ConvArgs a;
    bool empty;
    const int rc = forward_setup(dtype, n_frames, h, w, {d_a, a_stride, a_off, c_a}, {d_b, b_stride, b_off, c_b}, pool,
                                 d_frame_off, d_weights, c_out, nullptr, nullptr, nullptr, act,
                                 const_cast<void *>(d_out), out_stride, stats != 0, nullptr, 0, false, pl, a, &empty);
    if (rc) return rc;
    *rows_form = !empty && dtype == SHPL_BF16 && rows_forward(pl, a, pool != nullptr, stats != 0);
    return SHPL_OK;
}

extern "C" int shpl_conv3x3_wide_form(int dtype, int n_frames, int64_t h, int64_t w, const void *d_a,
                                      int64_t a_stride, int64_t a_off, int64_t c_a, const void *d_b, int64_t b_stride,
                                      int64_t b_off, int64_t c_b, const shpl_csr *pool, const int64_t *d_frame_off,
                                      const void *d_weights, int64_t c_out, int act, const void *d_out,
                                      int64_t out_stride, int stats, int *form) {
    if (!form) return SHPL_ERR_ARG;
    *form = 0;
    ConvPlan pl;
    ConvArgs a;
    bool empty;
    const int rc = forward_setup(dtype, n_frames, h, w, {d_a, a_stride, a_off, c_a}, {d_b, b_stride, b_off, c_b}, pool,
                                 d_frame_off, d_weights, c_out, nullptr, nullptr, nullptr, act,
                                 const_cast<void *>(d_out), out_stride, stats != 0, nullptr, 0, false, pl, a, &empty);
    if (rc) return rc;
    *form = !empty && dtype == SHPL_BF16 ? wide_forward(pl, a, pool, stats != 0) : 0;
    return SHPL_OK;
}

extern "C" int shpl_conv3x3_dgrad(int dtype, int n_frames, int64_t h, int64_t w, const void *d_gy, int64_t gy_stride,
                                  int64_t c_gy, const void *d_weights, int64_t c_dx, void *d_dx, int64_t dx_stride,
                                  int64_t c_split, void *d_dx_b, int64_t dx_b_stride, void *d_ws, size_t ws_bytes,
                                  void *stream) {
    return dgrad_impl(dtype, n_frames, h, w, d_gy, gy_stride, c_gy, d_weights, c_dx, d_dx, dx_stride, c_split, d_dx_b,
                      dx_b_stride, d_ws, ws_bytes, nullptr, stream);
}

extern "C" int shpl_conv3x3_dgrad_reuse(int dtype, int n_frames, int64_t h, int64_t w, const void *d_gy,
                                        int64_t gy_stride, int64_t c_gy, const void *d_weights, int64_t c_dx,
                                        void *d_dx, int64_t dx_stride, int64_t c_split, void *d_dx_b,
                                        int64_t dx_b_stride, void *d_ws, size_t ws_bytes, const shpl_csr *pool,
                                        const void *d_fwd_ws, size_t fwd_ws_bytes, int fwd_stats, void *stream) {
    // the forward is the conv of [A (c_split) || B pooled (c_dx - c_split)] to c_gy channels
    if (!pool || !d_fwd_ws || !d_dx_b) return SHPL_ERR_ARG;
    if (pool->n_keys != (int64_t)n_frames * h * w || c_split < 1 || c_split >= c_dx) return SHPL_ERR_BAD_SHAPE;
    Pooled po;
    const int rc = forward_pooled(dtype, n_frames, h, w, c_split, c_dx - c_split, c_gy, pool->nnz_cap, fwd_stats,
                                  d_fwd_ws, fwd_ws_bytes, &po);
    if (rc) return rc;
    return dgrad_impl(dtype, n_frames, h, w, d_gy, gy_stride, c_gy, d_weights, c_dx, d_dx, dx_stride, c_split, d_dx_b,
                      dx_b_stride, d_ws, ws_bytes, po.occ, stream);
}

extern "C" int shpl_conv3x3_wgrad_workspace_bytes(int dtype, int n_frames, int64_t h, int64_t w, int64_t c_a,
                                                  int64_t c_b, int64_t c_out, int64_t pool_nnz_cap, size_t *bytes) {
    if (!bytes) return SHPL_ERR_ARG;
    WgPlan wp;
    const bool pooled = pool_nnz_cap >= 0;
    const int rc = wgrad_plan(dtype, n_frames, h, w, c_a, c_b, c_out, pooled, &wp, pooled ? pool_nnz_cap : 0);
    if (rc) return rc;
    *bytes = wp.total;
    return SHPL_OK;
}

extern "C" int shpl_conv3x3_wgrad(int dtype, int n_frames, int64_t h, int64_t w, const void *d_a, int64_t a_stride,
                                  int64_t a_off, int64_t c_a, const void *d_b, int64_t b_stride, int64_t b_off,
                                  int64_t c_b, const shpl_csr *pool, const int64_t *d_frame_off, const void *d_gy,
                                  int64_t gy_stride, int64_t c_out, float *d_dw, void *d_ws, size_t ws_bytes,
                                  void *stream) {
    return wgrad_impl(dtype, n_frames, h, w, {d_a, a_stride, a_off, c_a}, {d_b, b_stride, b_off, c_b}, pool,
                      d_frame_off, d_gy, gy_stride, c_out, d_dw, d_ws, ws_bytes, nullptr, 0, 0, stream);
}

extern "C" int shpl_conv3x3_wgrad_reuse(int dtype, int n_frames, int64_t h, int64_t w, const void *d_a,
                                        int64_t a_stride, int64_t a_off, int64_t c_a, const void *d_b,
                                        int64_t b_stride, int64_t b_off, int64_t c_b, const shpl_csr *pool,
                                        const int64_t *d_frame_off, const void *d_gy, int64_t gy_stride,
                                        int64_t c_out, float *d_dw, void *d_ws, size_t ws_bytes,
                                        const void *d_fwd_ws, size_t fwd_ws_bytes, int fwd_stats, void *stream) {
    if (!pool || !d_fwd_ws || dtype != SHPL_BF16) return SHPL_ERR_ARG;
    return wgrad_impl(dtype, n_frames, h, w, {d_a, a_stride, a_off, c_a}, {d_b, b_stride, b_off, c_b}, pool,
                      d_frame_off, d_gy, gy_stride, c_out, d_dw, d_ws, ws_bytes, d_fwd_ws, fwd_ws_bytes, fwd_stats,
                      stream);
}
