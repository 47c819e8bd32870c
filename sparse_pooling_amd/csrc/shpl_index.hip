// shpl_index.hip -- device index builder of SHPL.
//
// Reference (host numpy, once per frame inside the data loader):
//   projectToImage / clip3DwithinImage      avod/avod/utils/transform.py:3-40
//   gen_sparse_pooling_input_avod           avod/avod/utils/sparse_pool_utils.py:6-20
//   produce_sparse_pooling_input            avod/avod/utils/sparse_pool_utils.py:22-58
//
// Two launches over IDX_CHUNK-point chunks of every frame (shpl_compact.h): a
// per-chunk count of the kept points, then the placement, where each thread
// evaluates one point and the kept points are ranked by wave ballots
// + an LDS prefix and written in point order (a stable compaction). A frame's
// entries start at its first input point ("capacity layout"); the tail up to
// the next frame is filled with -1 sentinels that every consumer skips, so no
// cross-frame scan is needed.
// Projection runs in f64 with the exact operation order numpy uses (an FMA
// chain over k for np.dot, dgemv's order when the product has one column,
// IEEE division, rint = round-half-even), so the integer outputs are
// bit-identical to the reference (tests/golden/index_*). The reference
// projects twice: the clip over the frame's N points (transform.py:34 via
// sparse_pool_utils.py:13), then projectToImage over the clip's survivors
// (:16) -- one column each when N == 1, resp. when one point survives.
#include "shpl_index_stage.h"

namespace shpl {
namespace {

template <typename PT, typename VT>
struct GenStage {  // gen_sparse_pooling_input_avod
    static constexpr bool HAS_BUCKETS = false;
    const void *pts;
    const void *vox;
    int64_t vstride;
    const double *P;
    double im_w, im_h;
    int64_t *bv_index;
    double *img_index;
    int64_t ld;

    struct Payload {
        double u, v;
    };
    struct In {
        double x, y, z;
    };

    __device__ void load(int64_t i, In &in) const { load_point<PT>(pts, i, in.x, in.y, in.z); }
    __device__ uint32_t eval(const Ctx &c, int f, int64_t, const In &in, Payload &pl) const {
        project(P + 12 * f, in.x, in.y, in.z, pl.u, pl.v, c.n_live == 1);
        if (!in_image(pl.u, pl.v, im_w, im_h)) return 0u;
        if (c.n_aux == 1 && c.n_live != 1) project(P + 12 * f, in.x, in.y, in.z, pl.u, pl.v, true);
        return AUX | KEEP_MULTI | KEEP_ONE;
    }
    __device__ void touch(int, int64_t, const Payload &, bool) const {}
    __device__ void emit(int, int64_t i, int64_t pos, int64_t, const Payload &pl) const {
        bv_index[2 * pos] = load_idx<VT>(vox, i * vstride);
        bv_index[2 * pos + 1] = load_idx<VT>(vox, i * vstride + 1);
        img_index[pos] = (double)(int64_t)rint(pl.u);
        img_index[ld + pos] = (double)(int64_t)rint(pl.v);
        img_index[2 * ld + pos] = 0.0;
    }
    __device__ void hole(int64_t) const {}
};

template <typename VT>
struct ProduceStage {  // produce_sparse_pooling_input (in-place img_index update)
    static constexpr bool HAS_BUCKETS = false;
    const void *bv;
    int64_t bstride;
    double *img;  // 3 rows, stride ld
    int64_t ld;
    Geometry g = {};
    int64_t *mij, *flip;
    int32_t *cell, *pix;
    uint32_t *err;

    struct Payload {
        Produced pr;
        double w;  // third row
    };
    struct In {
        double u, v, w;
        int64_t vx, vz;
    };

    __device__ void load(int64_t i, In &in) const {
        in.u = img[i];
        in.v = img[ld + i];
        in.w = img[2 * ld + i];
        in.vx = load_idx<VT>(bv, i * bstride);
        in.vz = load_idx<VT>(bv, i * bstride + 1);
    }
    __device__ uint32_t eval(const Ctx &, int, int64_t, const In &in, Payload &pl) const {
        pl.pr = produce(g, g.wq, g.hq, in.u, in.v, in.vx, in.vz);
        pl.w = in.w;
        return pl.pr.inside ? KEEP_MULTI | KEEP_ONE : 0u;
    }
    // img_index[0:2] = floor(img_index/stride), clamped -- for EVERY point
    // (sparse_pool_utils.py:30-34), after this thread has read its own value.
    __device__ void touch(int, int64_t i, const Payload &pl, bool) const {
        img[i] = pl.pr.u;
        img[ld + i] = pl.pr.v;
    }
    __device__ void emit(int, int64_t, int64_t pos, int64_t, const Payload &pl) const {
        const int64_t r = pl.pr.r;
        const int64_t vi = (int64_t)pl.pr.v, ui = (int64_t)pl.pr.u;
        const bool rok = r >= 0, pok = vi >= 0 && ui >= 0;
        if ((!rok || !pok) && err) atomicOr(err, (rok ? 0u : SHPL_EBIT_ROW) | (pok ? 0u : SHPL_EBIT_PIXEL));
        mij[2 * pos] = r;
        mij[2 * pos + 1] = pos;
        flip[3 * pos] = (int64_t)floor(pl.w);
        flip[3 * pos + 1] = vi;
        flip[3 * pos + 2] = ui;
        if (cell) cell[pos] = rok ? (int32_t)r : -1;
        if (pix) pix[pos] = pok ? (int32_t)(vi * (int64_t)g.wq + ui) : -1;
    }
    __device__ void hole(int64_t pos) const {
        if (cell) cell[pos] = -1;
        if (pix) pix[pos] = -1;
    }
};

// ------------------------------------------------- per-frame stable compaction

__global__ void k_set_pair(int64_t *o, int64_t a, int64_t b) {
    o[0] = a;
    o[1] = b;
}

}  // namespace
}  // namespace shpl

using namespace shpl;

extern "C" int shpl_build_index_workspace_bytes(int n_frames, int64_t max_points_per_frame, size_t *bytes) {
    if (!bytes || n_frames < 1 || max_points_per_frame < 0) return SHPL_ERR_ARG;
    *bytes = index_ws_bytes(n_frames, max_points_per_frame);  // [0, n] pair of the single-frame calls + chunk counts
    return SHPL_OK;
}

// shpl_build_index, optionally with the destination buckets (bk != NULL); RAGGED: every frame against its own
// image size d_im_sizes[f] (g then holds the padded map: make_geometry_ragged)
template <bool RAGGED>
static int build_index(int n_frames, const int64_t *d_point_offsets, const int64_t *d_point_counts,
                       int64_t max_points_per_frame, const void *d_points, int points_dtype, const void *d_voxels,
                       int voxels_itype, int64_t vox_stride, const double *d_P, const double *d_im_sizes,
                       const Geometry &g, const float *d_mval, int32_t *d_cell, int32_t *d_pix, float *d_val,
                       int64_t *d_mij, int64_t *d_flip, int64_t *d_frame_nnz, int64_t *d_frame_out_off,
                       uint32_t *d_err, void *d_ws, size_t ws_bytes, hipStream_t s, const Bkt *bk) {
    return by_point_types(points_dtype, voxels_itype, [&](auto pt, auto vt) {
        FrameDims<RAGGED> fd{};
        if constexpr (RAGGED) fd.im_sizes = d_im_sizes;
        FusedStage<typename decltype(pt)::T, typename decltype(vt)::T, RAGGED> st{
            fd, d_points, d_voxels, vox_stride, d_P, g, d_mval, d_cell, d_pix, d_val, d_mij, d_flip, d_err};
        return run_compaction(st, n_frames, max_points_per_frame, d_point_offsets, d_point_counts, d_frame_nnz,
                              d_frame_out_off, d_err, d_ws, ws_bytes, s, bk);
    });
}

// sizes_ok / map_ok: the ragged entries' own arguments (d_im_sizes given; img_rows, img_cols >= 1), checked
// with the pointers resp. with the shapes
static int index_args(int n_frames, const int64_t *d_point_offsets, int64_t max_points_per_frame,
                      const void *d_points, const void *d_voxels, int64_t vox_stride, const double *d_P,
                      double s_img, double s_bv, const int32_t *d_cell, const int32_t *d_pix, const float *d_val,
                      const void *d_ws, const Geometry &g, bool sizes_ok = true, bool map_ok = true) {
    if (n_frames < 1 || !d_point_offsets || !d_P || !d_ws || !sizes_ok) return SHPL_ERR_ARG;
    if (max_points_per_frame > 0 && (!d_points || !d_voxels || !d_cell || !d_pix || !d_val)) return SHPL_ERR_ARG;
    if (vox_stride < 2 || !(s_img > 0) || !(s_bv > 0) || !map_ok) return SHPL_ERR_BAD_SHAPE;
    if ((double)n_frames * (double)(g.n_cells > 0 ? g.n_cells : 0) >= 2147483647.0 ||
        (double)n_frames * (double)(g.n_pix > 0 ? g.n_pix : 0) >= 2147483647.0)
        return SHPL_ERR_BAD_SHAPE;
    return SHPL_OK;
}

extern "C" int shpl_build_index(int n_frames, const int64_t *d_point_offsets, const int64_t *d_point_counts,
                                int64_t max_points_per_frame,
                                const void *d_points, int points_dtype, const void *d_voxels,
                                int voxels_itype, int64_t vox_stride, const double *d_P, double im_w,
                                double im_h, double bv_h, double bv_w, double s_img, double s_bv,
                                const float *d_mval, int32_t *d_cell, int32_t *d_pix, float *d_val,
                                int64_t *d_mij, int64_t *d_flip, int64_t *d_frame_nnz,
                                int64_t *d_frame_out_off, uint32_t *d_err, void *d_ws, size_t ws_bytes,
                                void *stream) {
    const Geometry g = make_geometry(im_w, im_h, bv_h, bv_w, s_img, s_bv);
    const int rc = index_args(n_frames, d_point_offsets, max_points_per_frame, d_points, d_voxels, vox_stride, d_P,
                              s_img, s_bv, d_cell, d_pix, d_val, d_ws, g);
    if (rc) return rc;
    return build_index<false>(n_frames, d_point_offsets, d_point_counts, max_points_per_frame, d_points,
                              points_dtype, d_voxels, voxels_itype, vox_stride, d_P, nullptr, g, d_mval, d_cell,
                              d_pix, d_val, d_mij, d_flip, d_frame_nnz, d_frame_out_off, d_err, d_ws, ws_bytes,
                              (hipStream_t)stream, nullptr);
}

extern "C" int shpl_build_index_ragged(int n_frames, const int64_t *d_point_offsets, const int64_t *d_point_counts,
                                       int64_t max_points_per_frame, const void *d_points, int points_dtype,
                                       const void *d_voxels, int voxels_itype, int64_t vox_stride,
                                       const double *d_P, const double *d_im_sizes, int64_t img_rows,
                                       int64_t img_cols, double bv_h, double bv_w, double s_img, double s_bv,
                                       const float *d_mval, int32_t *d_cell, int32_t *d_pix, float *d_val,
                                       int64_t *d_mij, int64_t *d_flip, int64_t *d_frame_nnz,
                                       int64_t *d_frame_out_off, uint32_t *d_err, void *d_ws, size_t ws_bytes,
                                       void *stream) {
    const Geometry g = make_geometry_ragged(img_rows, img_cols, bv_h, bv_w, s_img, s_bv);
    const int rc = index_args(n_frames, d_point_offsets, max_points_per_frame, d_points, d_voxels, vox_stride, d_P,
                              s_img, s_bv, d_cell, d_pix, d_val, d_ws, g, d_im_sizes != nullptr,
                              img_rows >= 1 && img_cols >= 1);
    if (rc) return rc;
    return build_index<true>(n_frames, d_point_offsets, d_point_counts, max_points_per_frame, d_points,
                             points_dtype, d_voxels, voxels_itype, vox_stride, d_P, d_im_sizes, g, d_mval, d_cell,
                             d_pix, d_val, d_mij, d_flip, d_frame_nnz, d_frame_out_off, d_err, d_ws, ws_bytes,
                             (hipStream_t)stream, nullptr);
}

// bucket limits: 24-bit entry offsets, 512 ranges of BK_KEYS destinations per frame and key
static bool bucket_shape_ok(int64_t max_points_per_frame, int64_t nnz_cap, int64_t cells, int64_t pix) {
    return (int64_t)n_chunks_for(max_points_per_frame) * IDX_CHUNK <= ((int64_t)1 << 24) && nnz_cap >= 0 &&
           nnz_cap < ((int64_t)1 << 31) && cells <= (int64_t)BK_KEYS * BK_MAX_RANGES &&
           pix <= (int64_t)BK_KEYS * BK_MAX_RANGES;
}

extern "C" int shpl_bucket_workspace_bytes(int n_frames, int64_t max_points_per_frame, int64_t nnz_cap,
                                           int64_t cells_per_frame, int64_t pix_per_frame, size_t *bytes) {
    if (!bytes || n_frames < 1 || max_points_per_frame < 0 || cells_per_frame < 0 || pix_per_frame < 0)
        return SHPL_ERR_ARG;
    if (!bucket_shape_ok(max_points_per_frame, nnz_cap, cells_per_frame, pix_per_frame)) return SHPL_ERR_BAD_SHAPE;
    *bytes = bk_layout(n_frames, n_chunks_for(max_points_per_frame), nnz_cap, cells_per_frame, pix_per_frame).bytes;
    return SHPL_OK;
}

extern "C" int shpl_bucket_workspace_reset(int n_frames, void *d_bkt, size_t bkt_bytes, void *stream) {
    if (n_frames < 1 || !d_bkt) return SHPL_ERR_ARG;
    const BkLayout l = bk_layout(n_frames, 1, 0, 0, 0);  // the barrier words' place depends on n_frames alone
    const size_t bytes = 4 * 2 * (size_t)n_frames;
    if (bkt_bytes < l.bar + bytes) return SHPL_ERR_WORKSPACE;
    return hipMemsetAsync((char *)d_bkt + l.bar, 0, bytes, (hipStream_t)stream) == hipSuccess ? SHPL_OK
                                                                                             : SHPL_ERR_HIP;
}

// shpl_build_index_buckets (d_im_sizes NULL) and shpl_build_index_buckets_ragged over the geometry g
template <bool RAGGED>
static int build_index_buckets(int n_frames, const int64_t *d_point_offsets, const int64_t *d_point_counts,
                               int64_t max_points_per_frame, const void *d_points, int points_dtype,
                               const void *d_voxels, int voxels_itype, int64_t vox_stride, const double *d_P,
                               const double *d_im_sizes, bool map_ok, const Geometry &g, double s_img, double s_bv,
                               const float *d_mval, int32_t *d_cell, int32_t *d_pix, float *d_val,
                               int64_t *d_frame_nnz, int64_t *d_frame_out_off, uint32_t *d_err, void *d_ws,
                               size_t ws_bytes, int64_t nnz_cap, void *d_bkt, size_t bkt_bytes,
                               const shpl_pass_copy *cell_copy, const shpl_pass_copy *pixel_copy, void *stream) {
    int rc = index_args(n_frames, d_point_offsets, max_points_per_frame, d_points, d_voxels, vox_stride, d_P, s_img,
                        s_bv, d_cell, d_pix, d_val, d_ws, g, !RAGGED || d_im_sizes != nullptr, map_ok);
    if (rc) return rc;
    if (!d_bkt || !d_frame_nnz) return SHPL_ERR_ARG;
    if (!bucket_shape_ok(max_points_per_frame, nnz_cap, g.n_cells, g.n_pix)) return SHPL_ERR_BAD_SHAPE;
    const BkLayout l = bk_layout(n_frames, n_chunks_for(max_points_per_frame), nnz_cap, g.n_cells, g.n_pix);
    if (bkt_bytes < l.bytes) return SHPL_ERR_WORKSPACE;
    char *b = (char *)d_bkt;
    Bkt bk{{l.nr[0], l.nr[1]}, l.nrmax, nnz_cap, (int32_t *)(b + l.hist), (int32_t *)(b + l.ext),
           (uint32_t *)(b + l.words), {}, 0, (int32_t *)(b + l.bar)};
    const shpl_pass_copy *cps[2] = {cell_copy, pixel_copy};
    int64_t copy_bytes = 0;
    for (int k = 0; k < 2; ++k) {
        rc = make_pass_copy(cps[k], k ? g.n_pix : g.n_cells, &bk.cp[k], &copy_bytes);
        if (rc) return rc;
    }
    bk.cp_blocks = rider_blocks(n_frames, copy_bytes);
    return build_index<RAGGED>(n_frames, d_point_offsets, d_point_counts, max_points_per_frame, d_points,
                               points_dtype, d_voxels, voxels_itype, vox_stride, d_P, d_im_sizes, g, d_mval, d_cell,
                               d_pix, d_val, nullptr, nullptr, d_frame_nnz, d_frame_out_off, d_err, d_ws, ws_bytes,
                               (hipStream_t)stream, &bk);
}

extern "C" int shpl_build_index_buckets(int n_frames, const int64_t *d_point_offsets, const int64_t *d_point_counts,
                                        int64_t max_points_per_frame, const void *d_points, int points_dtype,
                                        const void *d_voxels, int voxels_itype, int64_t vox_stride, const double *d_P,
                                        double im_w, double im_h, double bv_h, double bv_w, double s_img,
                                        double s_bv, const float *d_mval, int32_t *d_cell, int32_t *d_pix,
                                        float *d_val, int64_t *d_frame_nnz, int64_t *d_frame_out_off,
                                        uint32_t *d_err, void *d_ws, size_t ws_bytes, int64_t nnz_cap, void *d_bkt,
                                        size_t bkt_bytes, const shpl_pass_copy *cell_copy,
                                        const shpl_pass_copy *pixel_copy, void *stream) {
    return build_index_buckets<false>(n_frames, d_point_offsets, d_point_counts, max_points_per_frame, d_points,
                                      points_dtype, d_voxels, voxels_itype, vox_stride, d_P, nullptr, true,
                                      make_geometry(im_w, im_h, bv_h, bv_w, s_img, s_bv), s_img, s_bv, d_mval,
                                      d_cell, d_pix, d_val, d_frame_nnz, d_frame_out_off, d_err, d_ws, ws_bytes,
                                      nnz_cap, d_bkt, bkt_bytes, cell_copy, pixel_copy, stream);
}

extern "C" int shpl_build_index_buckets_ragged(int n_frames, const int64_t *d_point_offsets,
                                               const int64_t *d_point_counts, int64_t max_points_per_frame,
                                               const void *d_points, int points_dtype, const void *d_voxels,
                                               int voxels_itype, int64_t vox_stride, const double *d_P,
                                               const double *d_im_sizes, int64_t img_rows, int64_t img_cols,
                                               double bv_h, double bv_w, double s_img, double s_bv,
                                               const float *d_mval, int32_t *d_cell, int32_t *d_pix, float *d_val,
                                               int64_t *d_frame_nnz, int64_t *d_frame_out_off, uint32_t *d_err,
                                               void *d_ws, size_t ws_bytes, int64_t nnz_cap, void *d_bkt,
                                               size_t bkt_bytes, const shpl_pass_copy *cell_copy,
                                               const shpl_pass_copy *pixel_copy, void *stream) {
    return build_index_buckets<true>(n_frames, d_point_offsets, d_point_counts, max_points_per_frame, d_points,
                                     points_dtype, d_voxels, voxels_itype, vox_stride, d_P, d_im_sizes,
                                     img_rows >= 1 && img_cols >= 1,
                                     make_geometry_ragged(img_rows, img_cols, bv_h, bv_w, s_img, s_bv), s_img, s_bv,
                                     d_mval, d_cell, d_pix, d_val, d_frame_nnz, d_frame_out_off, d_err, d_ws,
                                     ws_bytes, nnz_cap, d_bkt, bkt_bytes, cell_copy, pixel_copy, stream);
}

// Writes the device [0, n] offsets of a single frame into the workspace tail.
static int single_frame_offsets(int64_t n, void *ws, size_t ws_bytes, hipStream_t s, int64_t **off) {
    if (ws_bytes < 2 * sizeof(int64_t)) return SHPL_ERR_WORKSPACE;
    // A single frame needs device-side [0, n] offsets; they live in the workspace.
    int64_t *o = (int64_t *)ws;
    hipLaunchKernelGGL(k_set_pair, dim3(1), dim3(1), 0, s, o, (int64_t)0, n);
    SHPL_LAUNCH_CHECK();
    *off = o;
    return SHPL_OK;
}

extern "C" int shpl_gen_index(int64_t n, const void *d_points, int points_dtype, const void *d_voxels,
                              int voxels_itype, int64_t vox_stride, const double *d_P, double im_w,
                              double im_h, int64_t *d_bv_index, double *d_img_index, int64_t ld,
                              int64_t *d_nv, void *d_ws, size_t ws_bytes, void *stream) {
    if (n < 0 || !d_P || !d_bv_index || !d_img_index || !d_nv || !d_ws) return SHPL_ERR_ARG;
    if (n > 0 && (!d_points || !d_voxels)) return SHPL_ERR_ARG;
    if (vox_stride < 2 || ld < n) return SHPL_ERR_BAD_SHAPE;
    hipStream_t s = (hipStream_t)stream;
    int64_t *off;
    int rc = single_frame_offsets(n, d_ws, ws_bytes, s, &off);
    if (rc) return rc;
    return by_point_types(points_dtype, voxels_itype, [&](auto pt, auto vt) {
        GenStage<typename decltype(pt)::T, typename decltype(vt)::T> st{
            d_points, d_voxels, vox_stride, d_P, im_w, im_h, d_bv_index, d_img_index, ld};
        return run_compaction(st, 1, n, off, nullptr, d_nv, nullptr, nullptr, d_ws, ws_bytes, s);
    });
}

extern "C" int shpl_produce_index(int64_t nv, const void *d_bv_index, int bv_itype, int64_t bv_stride,
                                  double *d_img_index, int64_t ld, double im_w, double im_h, double bv_h,
                                  double bv_w, double s_img, double s_bv, int64_t *d_mij, int64_t *d_flip,
                                  int32_t *d_cell, int32_t *d_pix, int64_t *d_nk, uint32_t *d_err,
                                  void *d_ws, size_t ws_bytes, void *stream) {
    if (nv < 0 || !d_mij || !d_flip || !d_nk || !d_ws) return SHPL_ERR_ARG;
    if (nv > 0 && (!d_bv_index || !d_img_index)) return SHPL_ERR_ARG;
    if (bv_stride < 2 || ld < nv || !(s_img > 0) || !(s_bv > 0)) return SHPL_ERR_BAD_SHAPE;
    const Geometry g = make_geometry(im_w, im_h, bv_h, bv_w, s_img, s_bv);
    hipStream_t s = (hipStream_t)stream;
    int64_t *off;
    int rc = single_frame_offsets(nv, d_ws, ws_bytes, s, &off);
    if (rc) return rc;
    return by_itype(bv_itype, [&](auto vt) {
        ProduceStage<typename decltype(vt)::T> st{d_bv_index, bv_stride, d_img_index, ld, g,
                                                  d_mij, d_flip, d_cell, d_pix, d_err};
        return run_compaction(st, 1, nv, off, nullptr, d_nk, nullptr, d_err, d_ws, ws_bytes, s);
    });
}

#if SHPL_IDX1_PROBE
// probe builds only: the last k_index1 launch's per-chunk stamps (start, phase 1 done, past the frame barrier,
// aggregates read, points placed, buckets placed, holes written, end), 100 MHz ticks, chunks in launch order
extern "C" int shpl_probe_idx1(uint64_t *host, size_t n_blocks) {
    if (n_blocks > (size_t)shpl::IDX1_PROBE_BLOCKS) n_blocks = shpl::IDX1_PROBE_BLOCKS;
    return hipMemcpyFromSymbol(host, HIP_SYMBOL(shpl::g_idx1_probe), 64 * n_blocks, 0, hipMemcpyDeviceToHost) == hipSuccess
               ? SHPL_OK
               : SHPL_ERR_HIP;
}
#endif
