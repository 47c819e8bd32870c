// shpl_index_levels.hip -- the index build for several fusion levels in one pass over the points
// (shpl_build_index_levels, and shpl_build_index_levels_ragged for batches of mixed image sizes).
//
// The reference's AVOD RPN pools at two levels of one network: the full-resolution SHPL at stride 1 over the BEV
// map, and the after-VGG SHPL at stride 8 over the BEV input padded by 4 rows (rpn_model.py:291-336). Its feed
// code reads sparse_pooling_inputs[0] and [1] (rpn_model.py:841-862); the dataset's comment block builds the
// pair by running gen_sparse_pooling_input_avod and produce_sparse_pooling_input once per level over the same
// points, voxel indices, calibration and image shape (kitti_dataset.py:374-389).
//
// Everything up to the rounded image index is the same at every level: the point and voxel loads, the f64
// projection (twice for a one-survivor frame), the clip and the round-half-even. Only produce() depends on the
// level -- the stride division and its clamp, the BEV flatten bz * bwq + bx and the in-grid filter r < n_cells
// -- and with it the kept set, the entry slots and nnz. So the two launches of the flat builder (shpl_compact.h)
// are kept, each thread evaluates its point once, and every level gets its own count, ranks and writes.
//
// The levels' geometry and output pointers travel BY VALUE in the kernel arguments (LevelsStage::lv), so every
// per-level constant comes from a scalar load of the kernel-argument segment, never from a per-point load
// through a pointer (docs/HISTORY.md §24 measured what that costs). The level count NL is a compile-time
// constant: k_count_levels unrolls over it (every lv[l] a fixed offset), k_compact_levels rolls its per-level
// loops (lv[l] at a wave-uniform offset) so that its registers do not grow with NL (docs/HISTORY.md §25).
//
// Ragged batches (LevelsStage<..., RAGGED = true>): every frame is clipped once against its own (W_f, H_f), read
// from im_sizes[f]; each level's Geometry holds that level's padded map (make_geometry_ragged), and the frame's
// own strided size floor(size / s_img_l) -- the clamp -- is computed per level where an entry is written. The
// frame is blockIdx.y, so its size is workgroup-uniform: both kernels read it once, at their start beside the
// frame's offsets and ahead of every store, where the compiler issues scalar loads (docs/HISTORY.md §26).
#include "shpl_index_stage.h"

namespace shpl {
namespace {

struct Level {
    Geometry g;
    int32_t *cell, *pix;
    float *val;
    int64_t *mij, *flip;
    int64_t *frame_nnz;
};

// (ragged) the frame's own image size, read once per workgroup; the uniform stage clips against its im_w, im_h
// and carries nothing here
template <bool RAGGED>
struct FrameSize {};
template <>
struct FrameSize<true> {
    double w, h;
};

// The ragged stage's own member, in a base that is empty for the uniform stage (its kernel arguments are what
// they were).
template <bool RAGGED>
struct LevelsDims {};
template <>
struct LevelsDims<true> {
    const double *im_sizes;  // [n_frames, 2] f64 (W_f, H_f)
};

template <typename PT, typename VT, int NL_, bool RAGGED_ = false>
struct LevelsStage : LevelsDims<RAGGED_> {
    static constexpr int NL = NL_;
    static constexpr bool RAGGED = RAGGED_;
    // the single-level stage: its load, emit and hole are each level's (ragged: emit's in_map per level)
    using One = FusedStage<PT, VT, RAGGED_>;
    using In = typename One::In;
    const void *pts;
    const void *vox;
    int64_t vstride;
    const double *P;
    double im_w, im_h;
    const float *mval;
    uint32_t *err;
    Level lv[NL_];

    __device__ One level(int l) const {
        FrameDims<RAGGED_> fd{};
        if constexpr (RAGGED_) fd.im_sizes = this->im_sizes;
        return One{fd, pts, vox, vstride, P, lv[l].g, mval, lv[l].cell, lv[l].pix, lv[l].val, lv[l].mij, lv[l].flip,
                   err};
    }
    // (ragged) frame f's image size: two loads at a workgroup-uniform address, once per workgroup
    __device__ FrameSize<RAGGED_> size_of(int f) const {
        if constexpr (RAGGED_) return {frame_size(this->im_sizes, f, 0), frame_size(this->im_sizes, f, 1)};
        else return {};
    }
    __device__ void load(int64_t i, In &in) const { level(0).load(i, in); }
    // The level-independent half of FusedStage::eval: true when the point lies inside the clip (AUX), and then
    // (ur, vr) its rounded image index -- from the second projection exactly where the single-level stage runs it.
    __device__ bool clip(const Ctx &c, int f, const FrameSize<RAGGED_> &sz, const In &in, double &ur, double &vr) const {
        double u, v, Pf[12];
#pragma unroll
        for (int k = 0; k < 12; ++k) Pf[k] = P[12 * f + k];
        project(Pf, in.x, in.y, in.z, u, v, c.n_live == 1);
        if constexpr (RAGGED_) {
            if (!in_image(u, v, sz.w, sz.h)) return false;
        } else {
            if (!in_image(u, v, im_w, im_h)) return false;
        }
        if (c.n_aux == 1 && c.n_live != 1) project(Pf, in.x, in.y, in.z, u, v, true);
        ur = (double)(int64_t)rint(u);
        vr = (double)(int64_t)rint(v);
        return true;
    }
    // (ragged) the clamp is against the frame's own strided size at this level, make_geometry's division
    __device__ Produced produce_at(int l, const FrameSize<RAGGED_> &sz, double ur, double vr, const In &in) const {
        if constexpr (RAGGED_) {
            const double wq = floor(div_stride(sz.w, lv[l].g.s_img, lv[l].g.inv_img));
            const double hq = floor(div_stride(sz.h, lv[l].g.s_img, lv[l].g.inv_img));
            return produce(lv[l].g, wq, hq, ur, vr, in.vx, in.vz);
        } else {
            return produce(lv[l].g, lv[l].g.wq, lv[l].g.hq, ur, vr, in.vx, in.vz);
        }
    }
};

// Per-chunk counts: Frames::chunk_kept's layout with 1 + NL planes, [1 + NL][n_frames][n_chunks] -- plane 0 the
// clip's survivors (AUX), plane 1 + l level l's kept points. One keep count per level is enough (the flat
// builder keeps two, one per product order): a point is kept when it is inside the clip, which the FIRST
// projection decides, and inside the level's grid, which is a function of its voxel index alone; the order of
// the second projection's products moves the rounded image index, never the keep flag.
__device__ __forceinline__ int32_t *count_plane(const Frames &fr, int k, int f) {
    return fr.chunk_kept + ((int64_t)k * fr.n_frames + f) * fr.n_chunks;
}

// Pass 1 (grid n_chunks x n_frames): k_count's structure; the AUX count (once per chunk: the clip does not
// depend on the level) and every level's keep count.
template <typename Stage>
__global__ __launch_bounds__(IDX_BLOCK) void k_count_levels(Stage st, Frames fr) {
    constexpr int NL = Stage::NL;
    __shared__ int32_t wsum[1 + NL][IDX_BLOCK / 64];
    const int f = blockIdx.y, j = (int)blockIdx.x;
    int64_t p0, p1, cap_end;
    frame_range(fr, f, p0, p1, cap_end);
    const auto sz = st.size_of(f);
    const int64_t base = p0 + (int64_t)j * IDX_CHUNK;
    if (j == fr.n_chunks - 1 && p1 > base + IDX_CHUNK && threadIdx.x == 0 && fr.err)
        atomicOr(fr.err, SHPL_EBIT_CAPACITY);  // frame larger than max_points_per_frame
    const Ctx ctx{p1 - p0, -1};
    const int64_t i = base + threadIdx.x;
    typename Stage::In in = {};
    if (i < p1) st.load(i, in);
    double ur = 0.0, vr = 0.0;
    const bool aux = i < p1 && st.clip(ctx, f, sz, in, ur, vr);
    uint32_t m = aux ? 1u : 0u;
#pragma unroll
    for (int l = 0; l < NL; ++l) m |= aux && st.produce_at(l, sz, ur, vr, in).inside ? 2u << l : 0u;
#pragma unroll
    for (int k = 0; k < 1 + NL; ++k) {
        const int32_t n = wave_sum((m >> k) & 1u);
        if ((threadIdx.x & 63) == 0) wsum[k][threadIdx.x >> 6] = n;
    }
    __syncthreads();
    if (threadIdx.x < 1 + NL) {
        int32_t t = 0;
        for (int w = 0; w < IDX_BLOCK / 64; ++w) t += wsum[threadIdx.x][w];
        store_agent(count_plane(fr, threadIdx.x, f) + j, t);
    }
}

// Pass 2 (same grid): k_compact's structure. The frame's AUX count selects the order of the second projection's
// products for all levels; the point is loaded, projected, clipped and rounded once; then per level produce(),
// the keep flag, the stable slot within the frame (the level's kept points of earlier chunks, of the chunk's
// earlier waves, of the wave's earlier lanes), emit, and the level's capacity holes and frame count.
template <typename Stage>
__global__ __launch_bounds__(IDX_BLOCK) void k_compact_levels(Stage st, Frames fr) {
    constexpr int NL = Stage::NL, NW = IDX_BLOCK / 64;
    __shared__ int32_t wsum[NL][NW], pre[NL][NW], all[NL][NW], naux[NW];
    const int f = blockIdx.y, j = (int)blockIdx.x;
    int64_t p0, p1, cap_end;
    frame_range(fr, f, p0, p1, cap_end);
    const auto sz = st.size_of(f);
    const int wid = threadIdx.x >> 6;
    // every chunk's AUX count and every level's keep counts in one round trip, then the frame's and the earlier
    // chunks' sums of each
    int32_t na = 0, mb[NL], ea[NL];
#pragma unroll
    for (int l = 0; l < NL; ++l) mb[l] = ea[l] = 0;
    for (int q = threadIdx.x; q < fr.n_chunks; q += IDX_BLOCK) {
        const int32_t a = load_agent(count_plane(fr, 0, f) + q);
        int32_t c[NL];
#pragma unroll
        for (int l = 0; l < NL; ++l) c[l] = load_agent(count_plane(fr, 1 + l, f) + q);
        na += a;
#pragma unroll
        for (int l = 0; l < NL; ++l) {
            mb[l] += q < j ? c[l] : 0;
            ea[l] += c[l];
        }
    }
    na = wave_sum(na);
#pragma unroll
    for (int l = 0; l < NL; ++l) {
        mb[l] = wave_sum(mb[l]);
        ea[l] = wave_sum(ea[l]);
    }
    if ((threadIdx.x & 63) == 0) {
        naux[wid] = na;
#pragma unroll
        for (int l = 0; l < NL; ++l) {
            pre[l][wid] = mb[l];
            all[l][wid] = ea[l];
        }
    }
    __syncthreads();
    int64_t n_aux = 0;
    for (int w = 0; w < NW; ++w) n_aux += naux[w];
    const Ctx ctx{p1 - p0, n_aux};
    const int64_t base = p0 + (int64_t)j * IDX_CHUNK;
    const int64_t i = base + threadIdx.x;
    typename Stage::In in = {};
    if (i < p1) st.load(i, in);
    double ur = 0.0, vr = 0.0;
    const bool aux = i < p1 && st.clip(ctx, f, sz, in, ur, vr);
    // Per level, rolled: the level's geometry and pointers are read from the kernel arguments inside the loop
    // (scalar loads at a uniform offset), so registers do not grow with the level count. What a thread carries
    // over the barrier is packed: bit l of keepm its keep flag at level l, byte l of ranks its rank among the
    // wave's kept points of that level (< 64). produce() is evaluated again where an entry is written.
    uint32_t keepm = 0, ranks = 0;
#pragma unroll 1
    for (int l = 0; l < NL; ++l) {
        const bool keep = aux && st.produce_at(l, sz, ur, vr, in).inside;
        const uint64_t mk = __ballot(keep);
        keepm |= (keep ? 1u : 0u) << l;
        ranks |= lane_rank(mk) << (8 * l);
        if ((threadIdx.x & 63) == 0) wsum[l][wid] = (int32_t)__popcll(mk);
    }
    lds_barrier();
#pragma unroll 1
    for (int l = 0; l < NL; ++l) {
        int64_t kept = 0;    // the frame's entries at this level in earlier chunks
        int32_t before = 0;  // the chunk's in earlier waves
        for (int w = 0; w < NW; ++w) {
            kept += pre[l][w];
            const int32_t c = wsum[l][w];
            before += w < wid ? c : 0;
        }
        const int64_t slot = kept + before + ((ranks >> (8 * l)) & 63u);
        // compact_phase's rule: every write the frame's aggregates address stays inside the frame's capacity
        const bool keep = (keepm >> l) & 1u, in_cap = slot >= 0 && slot < cap_end - p0;
        if (keep && !in_cap && fr.err) atomicOr(fr.err, SHPL_EBIT_BARRIER);
        if (keep && in_cap)
            st.level(l).emit(f, i, p0 + slot, p0, typename Stage::One::Payload{st.produce_at(l, sz, ur, vr, in)});
    }
    // sentinels of every level's unused capacity [p0 + total, cap_end), each chunk its own stretch, and the
    // frame's count per level (a loop of its own: fewer scalars live beside emit's)
    const int64_t h1 = j == fr.n_chunks - 1 ? cap_end : (base + IDX_CHUNK < cap_end ? base + IDX_CHUNK : cap_end);
#pragma unroll 1
    for (int l = 0; l < NL; ++l) {
        int64_t total = 0;
        for (int w = 0; w < NW; ++w) total += all[l][w];
        const typename Stage::One one = st.level(l);
        const int64_t h0 = p0 + total > base ? p0 + total : base;
        for (int64_t pos = h0 + threadIdx.x; pos < h1; pos += IDX_BLOCK) one.hole(pos);
        if (j == fr.n_chunks - 1 && threadIdx.x == 0) st.lv[l].frame_nnz[f] = total;
    }
    if (j == fr.n_chunks - 1 && threadIdx.x == 0 && fr.frame_out_off) {
        fr.frame_out_off[f] = p0;
        if (f == fr.n_frames - 1) fr.frame_out_off[fr.n_frames] = cap_end;
    }
}

// 1 + n_levels count planes; never fewer than the flat builder's three, so that one level needs its workspace
size_t levels_ws_bytes(int n_frames, int64_t max_points, int n_levels) {
    const size_t planes = n_levels + 1 > 3 ? n_levels + 1 : 3;
    return IDX_WS_HEAD + align_up(planes * sizeof(int32_t) * (size_t)n_frames * (size_t)n_chunks_for(max_points), 256);
}

// what the levels share, as the host call hands it on
struct LevelsArgs {
    const void *pts, *vox;
    int64_t vstride;
    const double *P;
    double im_w, im_h;
    const double *im_sizes;  // ragged: the frames' own sizes (im_w, im_h then NaN)
    const float *mval;
    uint32_t *err;
    Level lv[SHPL_MAX_INDEX_LEVELS];
};

template <typename PT, typename VT, int NL, bool RAGGED>
int launch_levels(const LevelsArgs &a, const Frames &fr, hipStream_t stream) {
    using Stage = LevelsStage<PT, VT, NL, RAGGED>;
    LevelsDims<RAGGED> fd{};
    if constexpr (RAGGED) fd.im_sizes = a.im_sizes;
    Stage st{fd, a.pts, a.vox, a.vstride, a.P, a.im_w, a.im_h, a.mval, a.err, {}};
    for (int l = 0; l < NL; ++l) st.lv[l] = a.lv[l];
    const dim3 grid(fr.n_chunks, fr.n_frames);
    hipLaunchKernelGGL((k_count_levels<Stage>), grid, dim3(IDX_BLOCK), 0, stream, st, fr);
    SHPL_LAUNCH_CHECK();
    hipLaunchKernelGGL((k_compact_levels<Stage>), grid, dim3(IDX_BLOCK), 0, stream, st, fr);
    SHPL_LAUNCH_CHECK();
    return SHPL_OK;
}

bool levels_ok(int n_levels) { return n_levels >= 1 && n_levels <= SHPL_MAX_INDEX_LEVELS; }

// shpl_build_index_levels (d_im_sizes, level_img_hw unused) and shpl_build_index_levels_ragged (im_w, im_h
// unused): shpl_build_index's order of checks (index_args) -- frames and pointers, the point arrays, shapes, the
// 2^31 bound -- with the level count checked before the first read of levels[] and level_img_hw[].
template <bool RAGGED>
int build_levels(int n_frames, const int64_t *d_point_offsets, const int64_t *d_point_counts,
                 int64_t max_points_per_frame, const void *d_points, int points_dtype, const void *d_voxels,
                 int voxels_itype, int64_t vox_stride, const double *d_P, double im_w, double im_h,
                 const double *d_im_sizes, const float *d_mval, int n_levels, const shpl_index_level *levels,
                 const int64_t *level_img_hw, int64_t *d_frame_out_off, uint32_t *d_err, void *d_ws,
                 size_t ws_bytes, void *stream) {
    if (n_frames < 1 || !d_point_offsets || !d_P || !d_ws || !levels) return SHPL_ERR_ARG;
    if (RAGGED && (!d_im_sizes || !level_img_hw)) return SHPL_ERR_ARG;
    if (!levels_ok(n_levels)) return SHPL_ERR_BAD_SHAPE;
    const int nl = n_levels;
    for (int l = 0; l < nl; ++l) {
        if (!levels[l].frame_nnz) return SHPL_ERR_ARG;
        if (max_points_per_frame > 0 && (!levels[l].cell || !levels[l].pix || !levels[l].val)) return SHPL_ERR_ARG;
    }
    if (max_points_per_frame > 0 && (!d_points || !d_voxels)) return SHPL_ERR_ARG;
    if (vox_stride < 2) return SHPL_ERR_BAD_SHAPE;
    LevelsArgs all{d_points, d_voxels, vox_stride, d_P, im_w, im_h, d_im_sizes, d_mval, d_err, {}};
    for (int l = 0; l < nl; ++l) {
        const shpl_index_level &lv = levels[l];
        if (!(lv.s_img > 0) || !(lv.s_bv > 0) || !(lv.bv_h >= 0 && lv.bv_h < HUGE_VAL) ||
            !(lv.bv_w >= 0 && lv.bv_w < HUGE_VAL))
            return SHPL_ERR_BAD_SHAPE;
        if (RAGGED && (level_img_hw[2 * l] < 1 || level_img_hw[2 * l + 1] < 1)) return SHPL_ERR_BAD_SHAPE;
        const Geometry g =
            RAGGED ? make_geometry_ragged(level_img_hw[2 * l], level_img_hw[2 * l + 1], lv.bv_h, lv.bv_w, lv.s_img,
                                          lv.s_bv)
                   : make_geometry(im_w, im_h, lv.bv_h, lv.bv_w, lv.s_img, lv.s_bv);
        if ((double)n_frames * (double)(g.n_cells > 0 ? g.n_cells : 0) >= 2147483647.0 ||
            (double)n_frames * (double)(g.n_pix > 0 ? g.n_pix : 0) >= 2147483647.0)
            return SHPL_ERR_BAD_SHAPE;  // the level's global ids in 32 bits
        all.lv[l] = Level{g, lv.cell, lv.pix, lv.val, lv.mij, lv.flip, lv.frame_nnz};
    }
    if (ws_bytes < levels_ws_bytes(n_frames, max_points_per_frame, n_levels)) return SHPL_ERR_WORKSPACE;
    const Frames fr{d_point_offsets, d_point_counts, n_frames, n_chunks_for(max_points_per_frame),
                    (int32_t *)((char *)d_ws + IDX_WS_HEAD), nullptr, d_frame_out_off, d_err};
    return by_point_types(points_dtype, voxels_itype, [&](auto pt, auto vt) {
        using PT = typename decltype(pt)::T;
        using VT = typename decltype(vt)::T;
        const hipStream_t s = (hipStream_t)stream;
        switch (n_levels) {
            case 1: return launch_levels<PT, VT, 1, RAGGED>(all, fr, s);
            case 2: return launch_levels<PT, VT, 2, RAGGED>(all, fr, s);
            case 3: return launch_levels<PT, VT, 3, RAGGED>(all, fr, s);
            default: return launch_levels<PT, VT, 4, RAGGED>(all, fr, s);
        }
    });
}

}  // namespace
}  // namespace shpl

using namespace shpl;

extern "C" int shpl_build_index_levels_workspace_bytes(int n_frames, int64_t max_points_per_frame, int n_levels,
                                                       size_t *bytes) {
    if (!bytes || n_frames < 1 || max_points_per_frame < 0) return SHPL_ERR_ARG;
    if (!levels_ok(n_levels)) return SHPL_ERR_BAD_SHAPE;
    *bytes = levels_ws_bytes(n_frames, max_points_per_frame, n_levels);
    return SHPL_OK;
}

extern "C" int shpl_build_index_levels(int n_frames, const int64_t *d_point_offsets, const int64_t *d_point_counts,
                                       int64_t max_points_per_frame, const void *d_points, int points_dtype,
                                       const void *d_voxels, int voxels_itype, int64_t vox_stride,
                                       const double *d_P, double im_w, double im_h, const float *d_mval,
                                       int n_levels, const shpl_index_level *levels, int64_t *d_frame_out_off,
                                       uint32_t *d_err, void *d_ws, size_t ws_bytes, void *stream) {
    return build_levels<false>(n_frames, d_point_offsets, d_point_counts, max_points_per_frame, d_points,
                               points_dtype, d_voxels, voxels_itype, vox_stride, d_P, im_w, im_h, nullptr, d_mval,
                               n_levels, levels, nullptr, d_frame_out_off, d_err, d_ws, ws_bytes, stream);
}

extern "C" int shpl_build_index_levels_ragged(int n_frames, const int64_t *d_point_offsets,
                                              const int64_t *d_point_counts, int64_t max_points_per_frame,
                                              const void *d_points, int points_dtype, const void *d_voxels,
                                              int voxels_itype, int64_t vox_stride, const double *d_P,
                                              const double *d_im_sizes, const float *d_mval, int n_levels,
                                              const shpl_index_level *levels, const int64_t *level_img_hw,
                                              int64_t *d_frame_out_off, uint32_t *d_err, void *d_ws,
                                              size_t ws_bytes, void *stream) {
    return build_levels<true>(n_frames, d_point_offsets, d_point_counts, max_points_per_frame, d_points,
                              points_dtype, d_voxels, voxels_itype, vox_stride, d_P, NAN, NAN, d_im_sizes, d_mval,
                              n_levels, levels, level_img_hw, d_frame_out_off, d_err, d_ws, ws_bytes, stream);
}
