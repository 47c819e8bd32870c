/*
 * shpl.h -- C ABI of libshpl.so, the MI355X (gfx950) Sparse Non-homogeneous
 * Pooling Layer (SHPL).
 *
 * The reference (YeungLy/Sparse_Pooling) has no native SHPL code: its path is
 * numpy on the host plus four stock TensorFlow 1.8 ops. Each entry point
 * below replaces one piece of that path; the reference interface it stands in
 * for is cited as file:line relative to the reference checkout.
 *
 * Conventions
 *   - Every pointer named d_* is DEVICE memory (HBM), owned by the caller.
 *     The library never allocates: work buffers come from a caller-provided
 *     workspace whose size is returned by the *_workspace_bytes queries.
 *   - Feature maps are NHWC, contiguous per pixel row. A "row" is one BEV
 *     cell (b*Hb*Wb + y*Wb + x) or one image pixel (b*Hi*Wi + v*Wi + u);
 *     several frames of one batch are addressed by these global row ids.
 *   - All calls are stream-ordered on `stream` (a hipStream_t), reentrant,
 *     keep no global mutable state, and never synchronise the host.
 *   - Index errors are reported through a caller-provided device word
 *     (d_err, bit mask SHPL_EBIT_*), mirroring TF-CPU's InvalidArgumentError
 *     without a device->host sync on the hot path; kernels skip offending
 *     entries and never touch memory out of bounds.
 *   - Return value: shpl_status (launch/argument errors only).
 */
#ifndef SHPL_H
#define SHPL_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum {
    SHPL_OK = 0,
    SHPL_ERR_BAD_SHAPE = 1,  /* inconsistent sizes / strides / alignment */
    SHPL_ERR_INDEX_OOB = 2,  /* host-detectable out-of-range index */
    SHPL_ERR_HIP = 3,        /* a HIP runtime call failed */
    SHPL_ERR_WORKSPACE = 4,  /* workspace too small */
    SHPL_ERR_ARG = 5         /* null pointer / bad enum */
} shpl_status;

/* bits of the device error word */
#define SHPL_EBIT_ROW 1u     /* M row (BEV cell) outside [0, M_size[0]); shpl_bev_slices: a point's cell
                                outside the voxel grid */
#define SHPL_EBIT_COL 2u     /* M column outside [0, M_size[1]) */
#define SHPL_EBIT_PIXEL 4u   /* source index (b,v,u) outside the image */
#define SHPL_EBIT_VALUES 8u  /* len(M_val) != nnz */
#define SHPL_EBIT_CAPACITY 16u /* a frame holds more points than max_points_per_frame */
#define SHPL_EBIT_BARRIER 32u  /* shpl_build_index_buckets' one-launch form gave up waiting at a frame barrier
                                  (its chunks were not all resident: results of that call are invalid) */
#define SHPL_EBIT_GATHER 64u   /* shpl_mv3d_augment_points / shpl_mv3d_voxels_aug: a remain_index entry outside its
                                  frame (the point is skipped), or frame offsets outside the arrays (the frame is
                                  treated as empty); nothing is read through either */

typedef enum { SHPL_F32 = 0, SHPL_BF16 = 1, SHPL_F64 = 2 } shpl_dtype;
typedef enum { SHPL_I32 = 0, SHPL_I64 = 1 } shpl_itype;

/* CSR direction: which side of M the destination rows live on. */
typedef enum {
    SHPL_BY_CELL = 0,   /* destination = BEV cell (M row): img->BEV pooling, d_bev of trans */
    SHPL_BY_PIXEL = 1   /* destination = image pixel of column k: BEV->img, d_img of pooling */
} shpl_direction;

/* Order of the entries that share one destination (TF-CPU accumulation order). */
typedef enum {
    SHPL_ORDER_ENTRY = 0,    /* nnz order: SparseTensorDenseMatMul(M, .)            */
    SHPL_ORDER_COL_ROW = 1,  /* (col,row) order: matmul(sparse_transpose(M), .)     */
    SHPL_ORDER_COL_ENTRY = 2 /* (col, nnz) order: matmul(M, ., adjoint_a=True) and   */
                             /* the gradient of the transposed product              */
} shpl_order;

/* Output composition of a pull. */
typedef enum {
    SHPL_OUT_POOL = 0,    /* out = pooled                                  */
    SHPL_OUT_CONCAT = 1,  /* out = [pass || pooled]   (tf.concat axis=3)    */
    SHPL_OUT_ADD = 2      /* out = pass + pooled      (gradient add_n)      */
} shpl_out_mode;

const char *shpl_version(void);
const char *shpl_status_string(int status);

/* ---------------------------------------------------------------------------
 * Index builder
 * ------------------------------------------------------------------------- */

/* Fused, batched: points -> projection (f64, FMA chain as numpy/OpenBLAS) ->
 * image clip (strict bounds) -> round half-even -> strides -> BEV flatten ->
 * in-grid filter -> stable compaction, for n_frames frames in two launches
 * (a per-chunk count, then the placement), each with one 1024-thread
 * workgroup per 4096 points of every frame. max_points_per_frame bounds the
 * capacity off[f+1]-off[f] of every frame (SHPL_EBIT_CAPACITY otherwise).
 * Replaces gen_sparse_pooling_input_avod + produce_sparse_pooling_input
 * (avod/avod/utils/sparse_pool_utils.py:6-58; projection/clip
 * avod/avod/utils/transform.py:3-40) as called per frame by
 * KittiDataset.load_samples (avod/avod/datasets/kitti/kitti_dataset.py:374-379).
 *
 *   d_point_offsets [n_frames+1] i64 : frame f owns point slots [off[f], off[f+1])
 *   d_point_counts  optional [n_frames] i64: only the first count[f] slots are live
 *                   (the capacity layout shpl_bev_slices emits)
 *   d_points        [N,3] f64 or f32 (camera frame)
 *   d_voxels        [N, vox_stride] i32/i64, columns 0,1 = (x, z) BEV voxel index
 *   d_P             [n_frames, 3, 4] f64 camera matrices (stereo_calib.p2)
 *   im_w, im_h      image size the projection is clipped to ([W,H])
 *   bv_h, bv_w      full-resolution BEV size ((H,W))
 *   s_img, s_bv     strides (stride[0], stride[1] of the reference)
 *   d_mval          optional [N] f32 weight per INPUT point (MV3D 1/count); NULL = 1.0
 * Outputs (capacity layout: frame f's entries at [off[f], off[f] + nnz_f) in
 * point order, -1 sentinels up to off[f+1]; global ids):
 *   d_cell [N] i32  = f*Hb'*Wb' + r           (M row)
 *   d_pix  [N] i32  = f*Hi'*Wi' + v'*Wi' + u' (image pixel of column k)
 *   d_val  [N] f32
 *   d_mij  optional [N,2] i64 = reference Mij_pool rows [r, k_local]
 *   d_flip optional [N,3] i64 = reference img_index_flip_pool rows [0, v', u']
 *   d_frame_nnz     [n_frames] i64 (reference M_size[1] per frame)
 *   d_frame_out_off [n_frames+1] i64 (= d_point_offsets: entry slots of each frame)
 * The column of entry e is e itself (M's columns are arange per frame).
 * A kept entry whose flattened row is negative (the reference keeps it and TF
 * then rejects it) or whose pixel is negative gets cell/pix = -1 and sets
 * SHPL_EBIT_ROW / SHPL_EBIT_PIXEL in *d_err (nullable).
 */
int shpl_build_index_workspace_bytes(int n_frames, int64_t max_points_per_frame, size_t *bytes);
int shpl_build_index(int n_frames, const int64_t *d_point_offsets, const int64_t *d_point_counts,
                     int64_t max_points_per_frame,
                     const void *d_points, int points_dtype, const void *d_voxels, int voxels_itype,
                     int64_t vox_stride, const double *d_P, double im_w, double im_h, double bv_h,
                     double bv_w, double s_img, double s_bv, const float *d_mval,
                     int32_t *d_cell, int32_t *d_pix, float *d_val, int64_t *d_mij,
                     int64_t *d_flip, int64_t *d_frame_nnz, int64_t *d_frame_out_off,
                     uint32_t *d_err, void *d_ws, size_t ws_bytes, void *stream);

/* shpl_build_index over a batch of frames of DIFFERENT image sizes (KITTI's left colour images come as
 * 1242x375, 1224x370, 1238x374 and 1241x376; the reference hands every sample's own image_shape to
 * gen_sparse_pooling_input_avod, kitti_dataset.py:376-377). The frames share one padded image feature map
 * [n_frames, img_rows, img_cols, C]; instead of im_w, im_h:
 *   d_im_sizes [n_frames, 2] f64 : (W_f, H_f), frame f's own full-resolution image size
 *   img_rows, img_cols           : the padded map's size in strided pixels (>= 1; SHPL_ERR_BAD_SHAPE otherwise)
 * Frame f is clipped against (W_f, H_f) (so its clip survivors, and with them the order of the second
 * projection's products, are its own) and clamped against its own strided size floor(W_f / s_img),
 * floor(H_f / s_img), computed on the device with make_geometry's division. Pixel ids use the padded pitch:
 *   d_pix = f*img_rows*img_cols + v'*img_cols + u'
 * Every other output is as shpl_build_index writes it: per frame d_mij, d_flip and d_frame_nnz are the
 * reference's outputs for that frame called with its own im_size. An entry whose strided pixel lies outside the
 * padded map (u' >= img_cols or v' >= img_rows: a frame larger than the map) gets pix = -1 and sets
 * SHPL_EBIT_PIXEL, like a negative pixel. A size that is NaN, infinite, zero or negative keeps no point of its
 * frame. The 2^31 bound on global ids is taken on n_frames * img_rows * img_cols; the workspace is
 * shpl_build_index's. Arguments are checked in shpl_build_index's order (d_im_sizes with the pointers, the map
 * size with the shapes). */
int shpl_build_index_ragged(int n_frames, const int64_t *d_point_offsets, const int64_t *d_point_counts,
                            int64_t max_points_per_frame,
                            const void *d_points, int points_dtype, const void *d_voxels, int voxels_itype,
                            int64_t vox_stride, const double *d_P, const double *d_im_sizes, int64_t img_rows,
                            int64_t img_cols, double bv_h, double bv_w, double s_img, double s_bv,
                            const float *d_mval, int32_t *d_cell, int32_t *d_pix, float *d_val, int64_t *d_mij,
                            int64_t *d_flip, int64_t *d_frame_nnz, int64_t *d_frame_out_off,
                            uint32_t *d_err, void *d_ws, size_t ws_bytes, void *stream);

/* shpl_build_index for up to SHPL_MAX_INDEX_LEVELS fusion levels in ONE pass over the points. The reference's
 * AVOD RPN pools at two levels of one network (stride 1 over the BEV map, stride 8 over the BEV input padded by
 * 4 rows) and its feed code reads sparse_pooling_inputs[0] and [1] (avod/avod/core/models/rpn_model.py:841-862);
 * the dataset builds each entry by running gen_sparse_pooling_input_avod and produce_sparse_pooling_input over
 * the same points, voxel indices, calibration and image shape with that level's bv_size and stride
 * (avod/avod/datasets/kitti/kitti_dataset.py:374-389). Here every point is loaded, projected, clipped and
 * rounded once; each level then takes its own strides, BEV flatten, in-grid filter and stable compaction (the
 * kept set, the entry slots and nnz differ from level to level). Two launches, as shpl_build_index.
 *
 * `levels` is a HOST array of n_levels entries; their device pointers follow shpl_build_index's layout. Every
 * array of level l holds, over its whole capacity, the bits shpl_build_index writes when called with that
 * level's (s_img, s_bv, bv_h, bv_w) and the same other arguments (global ids per level: f*Hb'*Wb' + r and
 * f*Hi'*Wi' + v'*Wi' + u' with the level's own strided sizes). *d_err (nullable) is the OR over the levels;
 * d_frame_out_off (nullable) is shared: entry slots are the point slots at every level.
 * Status, in shpl_build_index's order: n_frames < 1 or a NULL d_point_offsets / d_P / d_ws / levels:
 * SHPL_ERR_ARG; n_levels outside [1, SHPL_MAX_INDEX_LEVELS]: SHPL_ERR_BAD_SHAPE (before levels[] is read); a
 * level's NULL frame_nnz and (max_points_per_frame > 0) a NULL d_points / d_voxels or a level's NULL cell / pix /
 * val: SHPL_ERR_ARG; vox_stride < 2, a level's stride not > 0 or BEV size negative or not finite, a level's
 * n_frames * cells or n_frames * pixels >= 2^31: SHPL_ERR_BAD_SHAPE; then the workspace (SHPL_ERR_WORKSPACE) and
 * the type codes (SHPL_ERR_ARG). A refused call writes nothing.
 * The workspace holds one count per chunk for the clip and one per level; with n_levels == 1 its size is
 * shpl_build_index's. Frames of one image size; shpl_build_index_levels_ragged (below) takes a batch of mixed
 * image sizes. */
#define SHPL_MAX_INDEX_LEVELS 4
typedef struct {
    double s_img, s_bv, bv_h, bv_w;   /* this level's stride[0], stride[1] and full-resolution BEV (H, W) */
    int32_t *cell, *pix; float *val;  /* [N] each, shpl_build_index's layout and global ids for this level */
    int64_t *mij, *flip;              /* optional [N,2], [N,3] */
    int64_t *frame_nnz;               /* [n_frames] */
} shpl_index_level;
int shpl_build_index_levels_workspace_bytes(int n_frames, int64_t max_points_per_frame, int n_levels, size_t *bytes);
int shpl_build_index_levels(int n_frames, const int64_t *d_point_offsets, const int64_t *d_point_counts,
                            int64_t max_points_per_frame, const void *d_points, int points_dtype,
                            const void *d_voxels, int voxels_itype, int64_t vox_stride, const double *d_P,
                            double im_w, double im_h, const float *d_mval, int n_levels,
                            const shpl_index_level *levels /* host array */, int64_t *d_frame_out_off,
                            uint32_t *d_err, void *d_ws, size_t ws_bytes, void *stream);

/* shpl_build_index_levels over a batch of frames of DIFFERENT image sizes: shpl_build_index_ragged for several
 * fusion levels in one pass over the points. Instead of im_w, im_h:
 *   d_im_sizes   [n_frames, 2] f64, on the device : (W_f, H_f), frame f's own full-resolution image size
 *   level_img_hw HOST array [n_levels][2] i64     : (img_rows, img_cols), the padded image feature map of each
 *                                                   level in that level's strided pixels
 * Every array of level l holds, over its whole capacity, the bits shpl_build_index_ragged writes when called
 * with that level's (s_img, s_bv, bv_h, bv_w, img_rows, img_cols) and the same other arguments. Frame f is
 * clipped ONCE against its own (W_f, H_f): its clip survivor count is its own and selects the order of the second
 * projection's products for all levels. At level l the index is clamped against floor(W_f / s_img_l),
 * floor(H_f / s_img_l) (make_geometry's division, on the device) and
 *   pix = f*img_rows_l*img_cols_l + v'*img_cols_l + u'
 * A strided pixel outside the level's padded map gets pix = -1 and sets SHPL_EBIT_PIXEL (at that level only). A
 * size that is NaN, infinite, zero or negative keeps no point of its frame at any level. *d_err is the OR over
 * the levels; d_frame_out_off is shared.
 * Status, in shpl_build_index_levels' order: d_im_sizes and level_img_hw are checked with the pointers
 * (SHPL_ERR_ARG); a level's img_rows < 1 or img_cols < 1 with that level's shapes (SHPL_ERR_BAD_SHAPE); the 2^31
 * bound is taken per level on n_frames * cells and on n_frames * img_rows * img_cols (the product saturated,
 * not wrapped). A refused call launches and writes nothing. The workspace is
 * shpl_build_index_levels_workspace_bytes'. */
int shpl_build_index_levels_ragged(int n_frames, const int64_t *d_point_offsets, const int64_t *d_point_counts,
                                   int64_t max_points_per_frame, const void *d_points, int points_dtype,
                                   const void *d_voxels, int voxels_itype, int64_t vox_stride, const double *d_P,
                                   const double *d_im_sizes, const float *d_mval, int n_levels,
                                   const shpl_index_level *levels /* host array */,
                                   const int64_t *level_img_hw /* host array */, int64_t *d_frame_out_off,
                                   uint32_t *d_err, void *d_ws, size_t ws_bytes, void *stream);

/* gen_sparse_pooling_input_avod alone (sparse_pool_utils.py:6-20), one frame:
 * outputs bv_index [nv,2] i64 and img_index 3 rows of stride ld f64 ([u;v;0]),
 * *d_nv = nv. Capacity n. */
int shpl_gen_index(int64_t n, const void *d_points, int points_dtype, const void *d_voxels,
                   int voxels_itype, int64_t vox_stride, const double *d_P, double im_w,
                   double im_h, int64_t *d_bv_index, double *d_img_index, int64_t ld,
                   int64_t *d_nv, void *d_ws, size_t ws_bytes, void *stream);

/* produce_sparse_pooling_input alone (sparse_pool_utils.py:22-58), one frame.
 * d_img_index (3 rows, stride ld, f64) is UPDATED IN PLACE like the
 * reference mutates its input dict. Outputs mij/flip (reference layout) and the
 * device map (cell, pix; val = 1). *d_nk = nk. Capacity nv. */
int shpl_produce_index(int64_t nv, const void *d_bv_index, int bv_itype, int64_t bv_stride,
                       double *d_img_index, int64_t ld, double im_w, double im_h, double bv_h,
                       double bv_w, double s_img, double s_bv, int64_t *d_mij, int64_t *d_flip,
                       int32_t *d_cell, int32_t *d_pix, int64_t *d_nk, uint32_t *d_err,
                       void *d_ws, size_t ws_bytes, void *stream);

/* ---------------------------------------------------------------------------
 * BEV slice voxelizer: the index builder's input
 * ------------------------------------------------------------------------- */

/* BevSlices.generate_bev(output_indices=True) (avod/avod/core/bev_generators/
 * bev_slices.py:33-156) with VoxelGrid2D.voxelize_2d (avod/wavedata/wavedata/
 * tools/core/voxel_grid_2d.py:43-162), for n_frames frames in one launch.
 *   d_points       [N,3] f64 camera-frame points; frame f owns [off[f], off[f+1])
 *   d_point_counts optional [n_frames] i64: only the first count[f] points are live
 *   d_planes       [n_frames,4] f64 ground planes (a, b, c, d)
 *   area_extents   host [3][2] f64 ([[xmin,xmax],[ymin,ymax],[zmin,zmax]])
 *   slice_lo/hi    host [num_slices] plane offsets of each height slice, computed
 *                  as the reference does (height_lo + s*hpd, + hpd)
 *   density_lo/hi  offsets of the density map's slice (height_lo, height_hi)
 *   density_table  host [16]: min(1, log(n+1)/norm_value), n >= 15 saturates
 * Outputs (capacity N, frame f at [off[f], off[f] + d_frame_nvox[f]); the rest
 * of the frame's slots is left untouched):
 *   d_voxel_indices [N,2] i32 = reference voxel_indices_rot rows (x, nz - z)
 *   d_pts_in_voxel  [N,3] f64 = the first point of each cell (unique_pts)
 *   d_height_maps   optional [n_frames, num_slices, nz, nx] f64 (rotated like the reference)
 *   d_density_map   optional [n_frames, nz, nx] f64
 * Slices are emitted in order and cells in (x, z) order, matching
 * np.vstack(voxel_indices_stack). Workspace: shpl_bev_workspace_bytes.
 * d_err (optional): SHPL_EBIT_ROW is set when a frame has more voxels than
 * points, and also when a point inside the extents, in a slice or in the
 * density range, floors to a cell outside the nx x nz grid (ext_max /
 * voxel_size rounding to an integer, e.g. voxel_size 0.3: the reference raises
 * ValueError there); that point is left out of every slice and of the density
 * map. A points_dtype other than SHPL_F64 is SHPL_ERR_ARG, answered behind the
 * other argument checks and before anything is written: a refused call leaves
 * the maps as they were. */
int shpl_bev_workspace_bytes(int64_t total_points, int num_slices, size_t *bytes);
int shpl_bev_slices(int n_frames, const int64_t *d_point_offsets, const int64_t *d_point_counts,
                    int64_t total_points,
                    const void *d_points, int points_dtype, const double *d_planes,
                    const double *area_extents, double voxel_size, int num_slices,
                    const double *slice_lo, const double *slice_hi, double density_lo,
                    double density_hi, double height_per_division, const double *density_table,
                    int32_t *d_voxel_indices, double *d_pts_in_voxel, int64_t *d_frame_nvox,
                    double *d_height_maps, double *d_density_map, uint32_t *d_err, void *d_ws,
                    size_t ws_bytes, void *stream);
/* The height and density maps of the last shpl_bev_slices call that used the
 * same workspace d_ws (and the same frames, points and geometry), from the
 * sorted words it left there: a caller can run the voxelizer without maps
 * (d_height_maps = d_density_map = NULL) where its outputs are on a critical
 * path, and write the maps -- ~27 MB of f64 per frame, almost all zeros --
 * later, on another stream (FramePipeline.velo_step: after the layer's
 * streaming pass). zero != 0 first zero-fills both maps (shpl_bev_slices'
 * maps arrive zero-filled; here the caller may have zeroed them itself).
 * Same values as shpl_bev_slices' maps, bit for bit. At most 4096 frames (a
 * shpl_bev_slices call over more frames keeps no per-frame word counts in the
 * workspace: SHPL_ERR_BAD_SHAPE here; its own maps are unaffected). */
int shpl_bev_maps(int n_frames, const int64_t *d_point_offsets, int64_t total_points, const void *d_points,
                  int points_dtype, const double *d_planes, const double *area_extents, double voxel_size,
                  int num_slices, const double *slice_lo, const double *slice_hi, double density_lo,
                  double density_hi, double height_per_division, const double *density_table,
                  double *d_height_maps, double *d_density_map, int zero, const void *d_ws,
                  size_t ws_bytes, void *stream);

/* The network's BEV input from the same sorted words as shpl_bev_maps: the
 * tensor KittiDataset.load_samples stacks, bev_input = np.dstack((*height_maps,
 * density_map)) (avod/avod/datasets/kitti/kitti_dataset.py:368), as the
 * tf.float32 placeholder receives it (rpn_model.py:185-186, filled at :823):
 * d_bev_input [n_frames, nz, nx, num_slices + 1] f32, element (f, y, x, v) =
 * (float) height map v (v < num_slices) or the density map (v = num_slices) of
 * shpl_bev_maps at (f, y, x), rounded to nearest once -- the feed's cast. Half
 * the bytes of the f64 maps, already in the layout the BEV feature extractor
 * reads. Zero-filled first. Same arguments as shpl_bev_maps otherwise. */
int shpl_bev_input(int n_frames, const int64_t *d_point_offsets, int64_t total_points, const void *d_points,
                   int points_dtype, const double *d_planes, const double *area_extents, double voxel_size,
                   int num_slices, const double *slice_lo, const double *slice_hi, double density_lo,
                   double density_hi, double height_per_division, const double *density_table,
                   float *d_bev_input, const void *d_ws, size_t ws_bytes, void *stream);

/* MV3D_TF's producer point_cloud_2_top_sparse
 * (MV3D_TF_release/lib/utils/construct_voxel.py:37-162), n_frames at once:
 *   d_points     [N, point_stride] f64 camera-frame points (x, y, z, ...)
 *   d_img_index2 optional [2, N] i64 rounded projections (minibatch_mv3d_img.py:88-91);
 *                NULL: computed on the device from d_P [n_frames,3,4] like the reference
 *   d_fv_aug     optional [n_frames,3] f64 (expansion_ratio, sx, sy) of augment_fv
 *                (minibatch_mv3d_img.py:191-209): u = int(u*ratio + sx), v = int(v*ratio + sy)
 *   ranges       host [6] f64: fwd (lo, hi), side (lo, hi), height (lo, hi), strict bounds
 *   res, zres, voxel_point_count  cfg.VOXEL_X_SIZE, VOXEL_Z_SIZE, VOXEL_POINT_COUNT
 * Outputs, capacity layout (frame f at [off[f], off[f] + d_frame_n[f])):
 *   d_img_index [3, ld] f64 ([u; v; 0]), d_bv_index [N,2] i64 (fwd, side),
 *   d_mval [N] f64 = 1 / points accepted by the point's voxel;
 *   d_number_buffer optional [N] i32: accepted points per voxel in voxel order,
 *   d_frame_nvox voxels per frame. */
int shpl_mv3d_workspace_bytes(int64_t total_points, size_t *bytes);
int shpl_mv3d_voxels(int n_frames, const int64_t *d_point_offsets, int64_t total_points,
                     const double *d_points, int64_t point_stride, const int64_t *d_img_index2,
                     const double *d_P, const double *d_fv_aug, const double *ranges, double res,
                     double zres, int voxel_point_count, double *d_img_index, int64_t ld, int64_t *d_bv_index,
                     double *d_mval, int64_t *d_frame_n, int32_t *d_number_buffer,
                     int64_t *d_frame_nvox, void *d_ws, size_t ws_bytes, void *stream);

/* MV3D_TF's training augmentation augment_voxel (MV3D_TF_release/lib/roi_data_layer/
 * minibatch_mv3d_img.py:132-189; cfg.TRAIN.AUGMENT_BV, on by default), the cloud half, n_frames at once.
 *   d_points     [N, point_stride] camera-frame points (x, y, z, r), point_dtype SHPL_F32 or SHPL_F64: the
 *                type T the reference's cloud is stored in -- it rounds to T after every step
 *   d_vox_aug    [n_frames, 8] f64: sx, sz, ratio, r00, r01, r10, r11, 0 -- the drawn shift and expansion
 *                ratio and rot = [[cos, sin], [-sin, cos]] of the drawn angle, formed on the host
 *   d_remain_index, d_remain_offsets  optional (both or neither), cfg.TRAIN.AUGMENT_PC: frame f's cloud becomes
 *                points[remain_index[roff[f] .. roff[f+1])] in that order, indices local to the frame, repeats
 *                allowed; total_out = roff[n_frames]. Without them total_out = total_points.
 * Per out point: (u, v) = round(project(P_f, ORIGINAL x, y, z)); x1 = T(x + sx), z1 = T(z + sz);
 * (x2, y2, z2) = T((x1, y, z1) * ratio); (x3, z3) = T(rot . (x2, z2)) in np.dot's order -- every step in f64,
 * unfused except np.dot's own chain, rounded once to T. A frame of one out point takes np.dot's one-column
 * orders, for the projection and the rotation.
 * shpl_mv3d_augment_points writes d_cloud [total_out, 4] f64 = (x3, y2, z3, r) (T's values widened; 16-byte
 * aligned; point_stride >= 4) and d_img_index2 [2, ld] i64 (ld >= total_out): shpl_mv3d_voxels' inputs.
 * shpl_mv3d_voxels_aug is shpl_mv3d_voxels over that cloud without writing it: both passes of the frame kernel
 * read the original point through the gather, augment it in registers and key the voxel on the result; the
 * image index is the ORIGINAL's (d_P, or d_img_index2 [2, total_points] indexed by the source point), and
 * d_fv_aug applies on top. Outputs and workspace are laid out by OUT point: ld >= total_out,
 * shpl_mv3d_workspace_bytes(total_out). On an f32 cloud the range tests and voxel indices run in f32 with the
 * bounds rounded to f32, as numpy runs point_cloud_2_top_sparse on an f32 array; shpl_mv3d_voxels over the widened
 * d_cloud runs them in f64, which can place a point at a voxel boundary differently.
 * Status: null or inconsistent pointers SHPL_ERR_ARG; point_dtype not SHPL_F32 / SHPL_F64, negative totals or
 * total_out != total_points without a gather SHPL_ERR_BAD_SHAPE. The offsets and remain_index live on the device
 * and are bounded there: *d_err (nullable) gets SHPL_EBIT_GATHER, see above. */
int shpl_mv3d_augment_points(int n_frames, const int64_t *d_point_offsets, int64_t total_points,
                             const void *d_points, int point_dtype, int64_t point_stride, const double *d_P,
                             const double *d_vox_aug, const int64_t *d_remain_index,
                             const int64_t *d_remain_offsets, int64_t total_out, double *d_cloud,
                             int64_t *d_img_index2, int64_t ld, uint32_t *d_err, void *stream);
int shpl_mv3d_voxels_aug(int n_frames, const int64_t *d_point_offsets, int64_t total_points,
                         const void *d_points, int point_dtype, int64_t point_stride,
                         const int64_t *d_img_index2, const double *d_P, const double *d_fv_aug,
                         const double *d_vox_aug, const int64_t *d_remain_index,
                         const int64_t *d_remain_offsets, int64_t total_out, const double *ranges, double res,
                         double zres, int voxel_point_count, double *d_img_index, int64_t ld,
                         int64_t *d_bv_index, double *d_mval, int64_t *d_frame_n, int32_t *d_number_buffer,
                         int64_t *d_frame_nvox, uint32_t *d_err, void *d_ws, size_t ws_bytes, void *stream);

/* ---------------------------------------------------------------------------
 * KITTI velodyne loader: the BEV voxelizer's input
 * ------------------------------------------------------------------------- */

/* obj_utils.get_lidar_point_cloud (avod/wavedata/wavedata/tools/obj_detection/
 * obj_utils.py:220-268) after read_lidar, for n_frames scans at once:
 * calib_utils.lidar_to_cam_frame (calib_utils.py:371-410), then with an image
 * size: z > 0, project with P2 (calib_utils.py:281-298), 0 < u < W, 0 < v < H;
 * then optionally kitti_aug.flip_point_cloud (kitti_aug.py:24-29).
 *   d_point_offsets [n_frames+1] i64: scan f is rows [off[f], off[f+1]) of d_xyzi
 *   d_xyzi      [N,4] f32 velodyne points (x, y, z, intensity), 16-byte aligned
 *   d_rect      [n_frames,3,4] f64 rows 0-2 of R0_rect4 . Tr_velo_to_cam4 (numpy's
 *               4x4 product on the host, as calib_utils.py:404 forms it)
 *   d_P, d_im_size  [n_frames,3,4] P2 and [n_frames,2] (w, h); both NULL = no filter
 *   min_intensity   NaN = none (see DESIGN.md for the reference's mask bug); any
 *               number, 0 included: keep (double)i > min_intensity (the reference's
 *               "0 means none" and f32 comparison belong to kitti.get_lidar_point_cloud)
 *   d_flip      optional [n_frames] i32, nonzero = negate x of the kept points
 * Outputs, capacity layout: d_points [N,3] f64 (frame f's kept points at
 * [off[f], off[f] + d_counts[f]) in scan order, NaN rows after). The result
 * feeds shpl_bev_slices (d_point_counts = d_counts) directly. */
int shpl_velo_workspace_bytes(int n_frames, int64_t max_points_per_frame, size_t *bytes);
int shpl_velo_to_cam(int n_frames, const int64_t *d_point_offsets, int64_t max_points_per_frame,
                     const float *d_xyzi, const double *d_rect, const double *d_P, const double *d_im_size,
                     double min_intensity, const int32_t *d_flip, double *d_points, int64_t *d_counts,
                     uint32_t *d_err, void *d_ws, size_t ws_bytes, void *stream);

/* ---------------------------------------------------------------------------
 * Correspondence matrix M: validation + device map (SURVEY a8-a10 inputs)
 * ------------------------------------------------------------------------- */

/* Pack a reference-format M = tf.SparseTensor(indices=Mij [nnz,2] i64,
 * values [n_values] f32, dense_shape=[R, ncols]) and the gather/scatter index
 * img_index_flip [ncols,3] (b,v,u) into the device map used by the pulls,
 * checking every index like TF-CPU's GatherNd / SparseTensorDenseMatMul /
 * ScatterNd kernels (rpn_model.py:328-336, retinanet_model.py:330-340,
 * network.py:243-246 build that SparseTensor from the placeholders).
 * Global ids: cell = row_base + r, col = col_base + k, pix = pix_base +
 * (b*img_h + v)*img_w + u. Invalid entries get -1 and set bits in *d_err. */
int shpl_pack_map(int64_t nnz, const int64_t *d_mij, const float *d_values, int64_t n_values,
                  int64_t n_rows, int64_t n_cols, const void *d_idx, int idx_itype,
                  int64_t img_b, int64_t img_h, int64_t img_w, int64_t row_base, int64_t col_base,
                  int64_t pix_base, int32_t *d_cell, int32_t *d_col, float *d_val,
                  int32_t *d_pix, uint32_t *d_err, void *stream);

/* ---------------------------------------------------------------------------
 * CSR keyed by destination (stable, TF accumulation order)
 * ------------------------------------------------------------------------- */

/* M's entries sorted by destination (all device arrays, caller-owned): a CSR
 * whose row segments are the runs of equal ent_dst. Layout follows the frames
 * of the map: frame f's entries occupy [frame_off[f], frame_off[f] + nnz_f)
 * sorted by (destination, TF order); its remaining capacity slots, and every
 * slot past frame_off[n_frames], hold ent_dst = -1 and are skipped. */
typedef struct {
    int32_t *ent_dst;  /* [nnz_cap] destination row of each sorted entry (-1 = empty slot) */
    int32_t *ent_src;  /* [nnz_cap] source row of each sorted entry                        */
    float *ent_val;    /* [nnz_cap] M value of each sorted entry                           */
    int32_t *ent_col;  /* [nnz_cap] column k of each sorted entry (SHPL_BY_PIXEL; else NULL). A pixel-keyed
                          CSR of shpl_build_csr_buckets may leave it NULL, marked SHPL_CSR_IDENTITY_COLS in
                          flags: every entry of the index builder's maps is a column of its own, and the pulls
                          then sum without per-column partials (bitwise the same: each partial is one product).
                          Any other pixel-keyed CSR without ent_col is SHPL_ERR_ARG for the pulls */
    int64_t n_keys;    /* destination rows (all frames)                                      */
    int64_t nnz_cap;   /* capacity of the entry arrays                                       */
    int32_t *key_range; /* optional [n_keys][2]: (first, end) sorted entry of each destination's
                           run (first == end: no entry). NULL: not built. When set,
                           shpl_build_csr fills it and shpl_pull runs one row-keyed launch. */
    /* optional, read by the sparse pass only (n_frames 0: it walks the whole capacity): the frame
       layout shpl_build_csr was given, so that it walks only the live entries -- frame f's
       [frame_off[f], frame_off[f] + min(frame_nnz[f], frame_off[f+1] - frame_off[f])) -- when
       most of the capacity is empty (raw scans: ~9 k voxel points in 120 k slots per frame).
       At most SHPL_LIVE_MAX_FRAMES frames. */
    const int64_t *frame_off; /* [n_frames + 1] */
    const int64_t *frame_nnz; /* [n_frames]     */
    int64_t n_frames;
    int64_t flags;     /* SHPL_CSR_IDENTITY_COLS: a pixel-keyed CSR whose every entry is a column of its own
                          (built by shpl_build_csr_buckets), so ent_col may be NULL; 0 otherwise */
    int32_t *heads;    /* optional [n_keys][head_k][2] run heads: (ent_src, ent_val bits) of each destination's
                          first min(run, head_k) sorted entries, filled by shpl_build_csr_buckets beside
                          key_range (the other builders take a CSR without them: SHPL_ERR_ARG otherwise). The
                          row-keyed pulls read them in the round trip of key_range instead of reading the
                          entries after it (bitwise the same). NULL: not built. */
    int64_t head_k;    /* 1 .. SHPL_CSR_MAX_HEAD when heads is set */
} shpl_csr;
#define SHPL_CSR_MAX_HEAD 32
#define SHPL_LIVE_MAX_FRAMES 1024
#define SHPL_CSR_IDENTITY_COLS 1

/* Sort the entries of every frame by destination (cell for SHPL_BY_CELL,
 * pix[col] for SHPL_BY_PIXEL) keeping `order` among equal destinations, and
 * gather the per-entry source ids so the pulls read one contiguous list:
 *   BY_CELL : ent_src = pix[col[e]] (image pixel), ent_col unused
 *   BY_PIXEL: ent_src = cell[e] (BEV row),         ent_col = col[e]
 * Frame f owns entries [d_frame_off[f], d_frame_off[f] + d_frame_nnz[f])
 * (d_frame_nnz NULL: the whole range) and destinations
 * [f*keys_per_frame, (f+1)*keys_per_frame); one workgroup sorts one frame
 * (LDS tile histogram + stable rank inside each tile). d_col NULL means
 * col[e] = e. Entries whose row, column or pixel is -1 or whose destination
 * lies outside the frame are left out.
 * With csr->key_range set (or for small batches of frames with at most 65536
 * destinations each) the sort is ONE launch of one workgroup per (frame, range
 * of 1024 destinations): each reads its frame's entries, counts its
 * destinations and the entries below them, places and ranks its own -- no
 * workgroup waits for another -- and writes key_range for its destinations. */
int shpl_csr_workspace_bytes(int64_t n_keys, int64_t nnz_cap, size_t *bytes);
int shpl_build_csr(int direction, int order, int n_frames, const int64_t *d_frame_off,
                   const int64_t *d_frame_nnz, int64_t keys_per_frame, const int32_t *d_cell,
                   const int32_t *d_col, const float *d_val, const int32_t *d_pix,
                   const shpl_csr *csr, void *d_ws, size_t ws_bytes, void *stream);
/* The same sort with the builder chosen explicitly instead of by batch shape
 * (tests and measurements; every builder yields the same entry lists):
 * SHPL_CSR_AUTO = shpl_build_csr's choice, SHPL_CSR_FRAME one workgroup per
 * frame, SHPL_CSR_SEGMENT balanced destination segments, SHPL_CSR_RANGE one
 * workgroup per (frame, destination range) reading the whole frame. Each is
 * the default of some batch shape (shpl_build_csr picks FRAME from 32 frames
 * on, SEGMENT below, RANGE for small batches of at most 65536 destinations
 * per frame); a key_range CSR always takes the range builder. Same arguments
 * and errors as shpl_build_csr otherwise. */
#define SHPL_CSR_AUTO 0
#define SHPL_CSR_FRAME 1
#define SHPL_CSR_SEGMENT 2
#define SHPL_CSR_RANGE 3
int shpl_build_csr_path(int path, int direction, int order, int n_frames, const int64_t *d_frame_off,
                        const int64_t *d_frame_nnz, int64_t keys_per_frame, const int32_t *d_cell,
                        const int32_t *d_col, const float *d_val, const int32_t *d_pix,
                        const shpl_csr *csr, void *d_ws, size_t ws_bytes, void *stream);

/* ---------------------------------------------------------------------------
 * Pull kernels: the sparse gather / scatter-add of SHPL
 * ------------------------------------------------------------------------- */

/* For every destination row d in [0, csr->n_keys):
 *   pooled[d] = sum over its CSR entries e (in CSR order) of
 *               ent_val[e] * src[ent_src[e]*src_stride + src_off + c],  c < c_pool
 *   with csr->ent_col set (SHPL_BY_PIXEL) the entries of one column k are
 *   first summed into a partial (TF's Q[k]) which is then added to pooled
 *   (ScatterNd order); every output element is written exactly once.
 *   mode SHPL_OUT_POOL  : out[d, 0:c_pool] = pooled          (0 where d is empty)
 *   mode SHPL_OUT_CONCAT: out[d, 0:c_pass] = pass[d]; out[d, c_pass:] = pooled
 *   mode SHPL_OUT_ADD   : out[d, 0:c_pool] = pass[d] + pooled
 * f32 arithmetic without FMA contraction (matches TF-CPU bit for bit);
 * SHPL_BF16 stores bf16 and accumulates in f32.
 * Two stream-ordered launches: k_dense writes every row (pass-through half
 * copied, pooled part 0 -- or pass + 0 for ADD) reading no index at all,
 * then k_sparse walks the sorted entries and overwrites the occupied rows'
 * pooled part. shpl_pull = shpl_pull_dense + shpl_pull_sparse on one stream;
 * the split entry points let a caller start the dense pass before M is built
 * (the sparse pass must follow the dense pass of the same output).
 * With csr->key_range set, shpl_pull is instead ONE launch keyed by output row
 * (k_rows: a group of lanes per row writes its pass-through chunks and walks
 * the row's run from key_range for the pooled ones) -- for small, latency-bound
 * layers (config 3), where two dependent launches and a thread per
 * (entry, chunk) cost more than the extra key_range read per row. Results are
 * bitwise the same. shpl_pull_dense / shpl_pull_sparse ignore key_range.
 * Replaces: _sparse_pool_op + concat  (sparse_pool_utils.py:96-103, :72)  -> BY_CELL, CONCAT
 *           _sparse_pool_trans_op + concat (sparse_pool_utils.py:105-117, :87) -> BY_PIXEL, CONCAT
 *           their TF autodiff gradients                       -> the other direction */
int shpl_pull(int direction, int dtype, const shpl_csr *csr, const void *d_src, int64_t src_stride,
              int64_t src_off, int64_t c_pool, const void *d_pass, int64_t pass_stride,
              int64_t pass_off, int64_t c_pass, int mode, void *d_out, int64_t out_stride,
              void *stream);
int shpl_pull_dense(int direction, int dtype, const shpl_csr *csr, const void *d_src,
                    int64_t src_stride, int64_t src_off, int64_t c_pool, const void *d_pass,
                    int64_t pass_stride, int64_t pass_off, int64_t c_pass, int mode, void *d_out,
                    int64_t out_stride, void *stream);
int shpl_pull_sparse(int direction, int dtype, const shpl_csr *csr, const void *d_src,
                     int64_t src_stride, int64_t src_off, int64_t c_pool, const void *d_pass,
                     int64_t pass_stride, int64_t pass_off, int64_t c_pass, int mode, void *d_out,
                     int64_t out_stride, void *stream);
/* The pooled part of every destination row written exactly once, with no streaming pass before it: mode
 * SHPL_OUT_POOL only (out rows' pooled columns; a concat's pass-through half is the caller's, e.g. a
 * shpl_pull_dense with c_pool = 0 beside the index build), csr->key_range required (shpl_build_csr_path(
 * SHPL_CSR_FRAME) fills it from the frame sort). Destinations whose run is empty get zeros; the others the
 * sums of shpl_pull (same order, bitwise). ONE launch: the occupied rows by a wave per 64 sorted entries
 * (cell-keyed rows of >= 32 chunks of 16 bytes; else a thread per (entry, chunk)) beside a wave per 16 rows
 * storing the empty rows' zeros. Replaces: the pooled half of sparse_pool_utils.py:96-103
 * + :72 where k_dense's zeros would be rewritten (wide channels: RetinaNet's 256). */
int shpl_pull_once(int direction, int dtype, const shpl_csr *csr, const void *d_src, int64_t src_stride,
                   int64_t src_off, int64_t c_pool, const void *d_pass, int64_t pass_stride, int64_t pass_off,
                   int64_t c_pass, int mode, void *d_out, int64_t out_stride, void *stream);
/* Zeros (+0, k_dense's bits) into the pooled columns out[d*out_stride + out_off + c], c < c_pool, of every
 * destination d that has an entry in csr -- the rows shpl_pull_sparse over the same CSR wrote -- and nothing
 * else: ONE launch over the capacity, a thread per (sorted entry, 16-byte chunk), the thread on a run's first
 * entry stores; it reads ent_dst only, and a destination outside [0, n_keys) is never stored to. For an output
 * whose pooled columns are kept zero between steps: cleared here at the previous step's cells (call it before
 * the CSR is rebuilt) they are all zero again, and the next shpl_pull_sparse over the new CSR gives the whole
 * pooled half with no k_dense zeros. 16-byte chunks when c_pool, out_stride, out_off and d_out allow them
 * (shpl_pull's rule), else one element per thread. No frame-layout (live entries) form. */
int shpl_pull_clear(int dtype, const shpl_csr *csr, int64_t c_pool, void *d_out, int64_t out_stride,
                    int64_t out_off, void *stream);

/* ---------------------------------------------------------------------------
 * Bucketed pulls: the index build hands the pulls M already cut by
 * destination (small batches, one stream, no CSR launch)
 * ------------------------------------------------------------------------- */

/* shpl_build_index, and in the same two launches the destination buckets of
 * both keys in d_bkt: per key (BEV cell, image pixel) every frame's
 * destinations are cut into ranges of 128, and each (frame, range) bucket
 * lists the frame's entries of that range in entry order -- TF's accumulation
 * order inside every destination, for both directions (the builder's columns
 * are the identity: SHPL_ORDER_ENTRY == SHPL_ORDER_COL_ROW). The count launch
 * adds per-chunk range histograms, the placement launch a stable multisplit.
 * No d_mij / d_flip outputs; nnz_cap = the point capacity (d_cell's length).
 * Limits (SHPL_ERR_BAD_SHAPE otherwise): at most 65536 cells and 65536 pixels
 * per frame, max_points_per_frame below 2^24.
 * Frames of at most 32 chunks of 1024 points run both passes in ONE launch
 * (k_index1: a frame barrier between them inside the launch) when every chunk
 * workgroup of the batch fits on the GPU at once and d_err is given (else the
 * two-launch form);
 * its barrier words live at the start of d_bkt, which must be ZEROED before
 * its first use (shpl_bucket_workspace_reset, or a memset of the whole
 * workspace) -- every call leaves them zero. SHPL_EBIT_BARRIER in *d_err: a
 * barrier gave up, or found its words not zeroed; the call's results are
 * invalid, and after a dirty start the words need shpl_bucket_workspace_reset.
 * Replaces what shpl_build_index + two shpl_build_csr calls feed the pulls
 * (kitti_dataset.py:374-379, then rpn_model.py:330-331's SparseTensor). */
/* Optional riders of shpl_build_index_buckets: the concat's pass-through half
 * of a forward pull, which needs no index -- out row r, channels [0,
 * channels) = src row r (rows: the BEV cells for cell_copy, the pixels for
 * pixel_copy, all frames). Extra workgroups of the two index launches do the
 * copies beside the latency-bound index work (one stream, no fork). Rows and
 * strides 16-byte aligned, channels * element size a multiple of 16
 * (SHPL_ERR_BAD_SHAPE otherwise). Strides in elements. */
typedef struct {
    int dtype;
    const void *src;
    int64_t src_stride;
    void *out;
    int64_t out_stride;
    int64_t channels;
} shpl_pass_copy;

int shpl_bucket_workspace_bytes(int n_frames, int64_t max_points_per_frame, int64_t nnz_cap,
                                int64_t cells_per_frame, int64_t pix_per_frame, size_t *bytes);
/* Zero the frame barrier words of a bucket workspace sized for n_frames (stream-ordered): before its first
 * shpl_build_index_buckets, and after a call that reported SHPL_EBIT_BARRIER. */
int shpl_bucket_workspace_reset(int n_frames, void *d_bkt, size_t bkt_bytes, void *stream);
int shpl_build_index_buckets(int n_frames, const int64_t *d_point_offsets, const int64_t *d_point_counts,
                             int64_t max_points_per_frame, const void *d_points, int points_dtype,
                             const void *d_voxels, int voxels_itype, int64_t vox_stride, const double *d_P,
                             double im_w, double im_h, double bv_h, double bv_w, double s_img, double s_bv,
                             const float *d_mval, int32_t *d_cell, int32_t *d_pix, float *d_val,
                             int64_t *d_frame_nnz, int64_t *d_frame_out_off, uint32_t *d_err, void *d_ws,
                             size_t ws_bytes, int64_t nnz_cap, void *d_bkt, size_t bkt_bytes,
                             const shpl_pass_copy *cell_copy, const shpl_pass_copy *pixel_copy, void *stream);
/* shpl_build_index_buckets over frames of different image sizes (shpl_build_index_ragged's d_im_sizes, img_rows,
 * img_cols in place of im_w, im_h), in all three forms (one launch, two launches, riders): the pixel key's
 * buckets, the bucket limits and shpl_bucket_workspace_bytes' pix_per_frame are those of the padded map,
 * img_rows * img_cols pixels per frame; pixel_copy copies all of them. An entry outside the padded map gets
 * no bucket. */
int shpl_build_index_buckets_ragged(int n_frames, const int64_t *d_point_offsets, const int64_t *d_point_counts,
                                    int64_t max_points_per_frame, const void *d_points, int points_dtype,
                                    const void *d_voxels, int voxels_itype, int64_t vox_stride, const double *d_P,
                                    const double *d_im_sizes, int64_t img_rows, int64_t img_cols, double bv_h,
                                    double bv_w, double s_img, double s_bv, const float *d_mval, int32_t *d_cell,
                                    int32_t *d_pix, float *d_val, int64_t *d_frame_nnz, int64_t *d_frame_out_off,
                                    uint32_t *d_err, void *d_ws, size_t ws_bytes, int64_t nnz_cap, void *d_bkt,
                                    size_t bkt_bytes, const shpl_pass_copy *cell_copy,
                                    const shpl_pass_copy *pixel_copy, void *stream);

/* The map shpl_build_index_buckets left: its frame layout, index arrays and
 * bucket workspace (the same sizes as that call). */
typedef struct {
    int n_frames;
    int64_t max_points_per_frame, nnz_cap;
    int64_t cells_per_frame, pix_per_frame;
    const int64_t *frame_off, *frame_nnz; /* [n_frames + 1], [n_frames] */
    const int32_t *cell, *pix;            /* [nnz_cap] global rows, as shpl_build_index writes them */
    const float *val;                     /* [nnz_cap] */
    void *ws;                             /* the bucket workspace */
    size_t ws_bytes;
    const uint32_t *err;                  /* the index call's d_err (NULL if it had none): after a
                                           * SHPL_EBIT_BARRIER the bucket sort reads every bucket as empty, so a
                                           * failed barrier's half-written buckets never address anything; the bit
                                           * stays until the caller clears the word (its maps stay empty until
                                           * then: FusedPipeline.check() clears it and resets the barrier words) */
} shpl_buckets;

/* One pull of shpl_pull_pair: the arguments of shpl_pull after its csr. */
typedef struct {
    int dtype;
    const void *src;
    int64_t src_stride, src_off, c_pool;
    const void *pass;
    int64_t pass_stride, pass_off, c_pass;
    int mode;
    void *out;
    int64_t out_stride;
} shpl_pull_desc;

/* Both CSRs of the map (by_cell: SHPL_BY_CELL, SHPL_ORDER_ENTRY; by_pixel:
 * SHPL_BY_PIXEL, SHPL_ORDER_COL_ROW, ent_col optional; either may be NULL) from
 * the buckets, in ONE launch: a workgroup per (key, frame, range) sorts its
 * bucket by destination, stably (the bucket is in entry order), emits the
 * sorted entries and key_range (when set) and clears the unused capacity --
 * the same lists shpl_build_csr makes of the same index arrays. No counting or
 * bucketing pass: the index build did both. */
int shpl_build_csr_buckets(const shpl_buckets *bk, const shpl_csr *by_cell, const shpl_csr *by_pixel,
                           void *stream);

/* Two row-keyed pulls in ONE launch (shpl_pull over CSRs with key_range):
 * d_cell over by_cell (SHPL_BY_CELL), d_pixel over by_pixel (SHPL_BY_PIXEL);
 * either pair may be NULL (two launches if their dtypes or vector widths
 * differ). Same results, bit for bit,
 * as the two shpl_pull calls. Replaces the forward pair
 * (sparse_pool_utils.py:96-117, with the concats of :72, :87) or, with
 * SHPL_OUT_ADD, its gradient pair. */
int shpl_pull_pair(const shpl_csr *by_cell, const shpl_pull_desc *d_cell, const shpl_csr *by_pixel,
                   const shpl_pull_desc *d_pixel, void *stream);

/* ---------------------------------------------------------------------------
 * Post-fusion 3x3 convolution
 * ------------------------------------------------------------------------- */

typedef enum { SHPL_ACT_NONE = 0, SHPL_ACT_RELU = 1 } shpl_act;

/* out[f,y,x,co] = act(round(fma(acc, scale[co], shift[co] - center[co]*scale[co])))
 *   acc = sum_{ky,kx,ci} in[f, y+ky-1, x+kx-1, ci] * W[ky,kx,ci,co]
 * i.e. (acc - center) * scale + shift with one fused rounding (the per-channel
 * shift - center*scale rounded once in f32); round = to the storage dtype;
 * act RELU = max(bits, 0) on the stored value's bit pattern as a signed
 * integer (negatives, -0 and -NaN -> +0, +NaN stays NaN). Every kernel behind
 * this call (row-streaming or tiled) applies exactly this epilogue, so the
 * same call gives the same bits whichever runs, up to the accumulation order
 * of acc (the kernels sum the MFMA products in different orders). SAME padding (zeros outside the map), stride 1, n_frames frames of h x w
 * pixels, NHWC rows of global id (f*h + y)*w + x. Input channels
 * [0, c_a) are row r of d_a (element r*a_stride + a_off + c), channels
 * [c_a, c_a + c_b) come from d_b:
 *   pool == NULL: row r of d_b (r*b_stride + b_off + c), a second dense map;
 *   pool != NULL: the img->BEV pooled map, computed in the staging from the
 *                 cell-keyed CSR (shpl_build_csr SHPL_BY_CELL, SHPL_ORDER_ENTRY,
 *                 n_keys = n_frames*h*w, entry slots of frame f from
 *                 d_frame_off[f] on) over the image map d_b, with the
 *                 arithmetic of shpl_pull: the result is the conv of
 *                 [a || shpl_pull(SHPL_BY_CELL, ...)] without writing it --
 *                 bitwise, when c_a is a multiple of the staging chunk (8 f32
 *                 / 16 bf16 channels; otherwise the K order differs).
 *                 Or the pixel-keyed CSR (shpl_build_csr SHPL_BY_PIXEL,
 *                 SHPL_ORDER_COL_ROW, with ent_col, or without it and flagged
 *                 SHPL_CSR_IDENTITY_COLS as shpl_build_csr_buckets leaves it;
 *                 a pool counts as pixel-keyed when either holds): the image
 *                 side. n_keys = n_frames*h*w then counts image pixels, d_a
 *                 is the image map, d_b the BEV map, and the result is
 *                 bitwise the conv of [a || shpl_pull(SHPL_BY_PIXEL, ...)]:
 *                 with ent_col a pixel's run is summed per column of M first
 *                 and the columns' partials then added (TF's ScatterNd order,
 *                 shpl_pull's); flagged identity columns take the plain sum,
 *                 as the pulls do. A cell-keyed CSR leaves ent_col NULL.
 * d_weights: HWIO [3][3][c_a+c_b][c_out] in the feature dtype (slim.conv2d's
 * variable). d_center / d_scale / d_shift: optional [c_out] f32 (NULL = 0 / 1
 * / 0) -- BatchNorm inference: center = moving_mean, scale = gamma /
 * sqrt(moving_var + eps), shift = beta; conv bias: shift = bias.
 * d_stats (optional, [2][c_out] f64): per-channel sum and sum of squares of
 * the pre-epilogue output, for BatchNorm in training mode (shpl_batch_norm).
 * f32: v_mfma_f32_32x32x2_f32 (exact f32 products, f32 accumulation);
 * SHPL_BF16: bf16 storage, v_mfma_f32_32x32x16_bf16, f32 accumulation, one
 * rounding at the store. Workspace: shpl_conv3x3_workspace_bytes, with
 * pool_nnz_cap = pool->nnz_cap for a pooled call and -1 without a pool.
 * bf16 inputs of at most 64 channels (c_a, c_b multiples of 8, 16-byte rows)
 * without d_stats run the row-streaming kernel; pooled, the pooled vector of
 * each occupied cell is computed once into the workspace (shpl_pull's
 * arithmetic) and gathered by the conv's staging.
 * Replaces: bv_fused = sparse_pool_layer(...) (sparse_pool_utils.py:61-92)
 *   followed by slim.conv2d(bv_fused, Ci, [3,3], normalizer_fn=slim.batch_norm)
 *   (avod/avod/core/models/rpn_model.py:338-346, scope pyramid_fusion_pooled_bev);
 *   with the pixel-keyed CSR, img_fused = [img || _sparse_pool_trans_op(M, bev)]
 *   (sparse_pool_utils.py:79-87) followed by the conv of scope
 *   pyramid_fusion_pooled_img (rpn_model.py:347-354); and
 *   slim.conv2d(bev_fused, 256, [3,3])
 *   (avod/avod/core/models/retinanet_model.py:343-348). */
int shpl_conv3x3_workspace_bytes(int dtype, int n_frames, int64_t h, int64_t w, int64_t c_a, int64_t c_b,
                                 int64_t c_out, int64_t pool_nnz_cap, int stats, size_t *bytes);
int shpl_conv3x3(int dtype, int n_frames, int64_t h, int64_t w, const void *d_a, int64_t a_stride,
                 int64_t a_off, int64_t c_a, const void *d_b, int64_t b_stride, int64_t b_off,
                 int64_t c_b, const shpl_csr *pool, const int64_t *d_frame_off, const void *d_weights,
                 int64_t c_out, const float *d_center, const float *d_scale, const float *d_shift,
                 int act, void *d_out, int64_t out_stride, double *d_stats, void *d_ws,
                 size_t ws_bytes, void *stream);

/* Whether shpl_conv3x3 with these arguments (d_ws / ws_bytes / d_center / d_scale / d_shift / stream aside;
 * stats = d_stats != NULL) runs the row-streaming form (*rows_form = 1), whose pooled call leaves the
 * occupancy maps and per-run pooled rows in its workspace that shpl_conv3x3_wgrad_reuse reads; 0 for the
 * tiled form, f32, or no pixel. The same predicate shpl_conv3x3 decides by; pool may be the pixel-keyed CSR
 * of the image side, as there. */
int shpl_conv3x3_rows_form(int dtype, int n_frames, int64_t h, int64_t w, const void *d_a, int64_t a_stride,
                           int64_t a_off, int64_t c_a, const void *d_b, int64_t b_stride, int64_t b_off, int64_t c_b,
                           const shpl_csr *pool, const int64_t *d_frame_off, const void *d_weights, int64_t c_out,
                           int act, const void *d_out, int64_t out_stride, int stats, int *rows_form);

/* Whether shpl_conv3x3 with these arguments (the same as shpl_conv3x3_rows_form's) runs the wide bf16 kernel
 * (k_conv_wide: input channels in whole chunks of 64, more than 64 of them, output channels in whole blocks
 * of 256, no statistics, 16-byte aligned rows, offsets and pointers), and on which second operand. *form:
 *   0  not the wide kernel (the row-streaming or the tiled form, f32, or no pixel);
 *   1  wide, B a dense map or absent;
 *   2  wide over the compact pooled runs (one pooled row per occupied cell, computed into the workspace);
 *   3  wide over the pooled map, materialised in the workspace by shpl_pull (a map past the occupancy
 *      table: h * ceil(w / 32) > 18432 words, or pool->nnz_cap * c_b * 2 >= 2^31 bytes).
 * The wide kernel addresses a frame's rows by signed 32-bit byte offsets: a call whose A, dense B or
 * materialised map has h * w * row stride * 2 >= 2^31 bytes answers 0 and runs the tiled form, which
 * addresses in 64 bits. The same predicate shpl_conv3x3 decides by. */
int shpl_conv3x3_wide_form(int dtype, int n_frames, int64_t h, int64_t w, const void *d_a, int64_t a_stride,
                           int64_t a_off, int64_t c_a, const void *d_b, int64_t b_stride, int64_t b_off, int64_t c_b,
                           const shpl_csr *pool, const int64_t *d_frame_off, const void *d_weights, int64_t c_out,
                           int act, const void *d_out, int64_t out_stride, int stats, int *form);

/* BatchNorm in training mode over rows x c, from d_stats of shpl_conv3x3 and
 * count = rows: mean = sum/count, var = sumsq/count - mean^2,
 * y = act((x - mean) * gamma / sqrt(var + eps) + beta), written to d_y
 * (NULL: in place over d_x); moving averages m -= (m - v) * (1 - decay) with
 * the Bessel-corrected variance (TF FusedBatchNorm, slim.batch_norm defaults
 * eps 1e-3, decay 0.999, gamma NULL = 1). d_batch_mean / d_batch_var
 * (optional) receive the batch moments (variance Bessel-corrected, as
 * FusedBatchNorm's outputs). d_ws: 2*c floats; on return it holds the mean
 * and scale = gamma / sqrt(var + eps) that shpl_batch_norm_backward takes. */
int shpl_batch_norm(int dtype, int64_t rows, void *d_x, void *d_y, int64_t stride, int64_t c,
                    const double *d_stats, double count, float eps, const float *d_gamma, const float *d_beta,
                    int act, float *d_moving_mean, float *d_moving_var, float decay, float *d_batch_mean,
                    float *d_batch_var, float *d_ws, void *stream);

/* ---------------------------------------------------------------------------
 * Post-fusion conv backward (the TF autodiff of rpn_model.py:338-354)
 * ------------------------------------------------------------------------- */

/* BatchNorm (+ ReLU) backward over rows x c. g_bn = g * [y > 0] when act is
 * SHPL_ACT_RELU (d_y = the layer output; d_y NULL: y recomputed from d_raw
 * as (raw - mean) * scale + beta with the forward's rounding -- the same mask,
 * one map less to read), xhat = (raw - mean) * scale / gamma
 * (d_raw = the conv output). Per channel (f64, fixed order):
 * dbeta = sum g_bn, dgamma = sum g_bn * xhat; then
 *   training:  g_raw = scale * (g_bn - dbeta / rows - xhat * dgamma / rows)
 *   inference: g_raw = scale * g_bn   (mean / scale from the moving statistics)
 * d_mean / d_scale NULL: 0 / 1 -- a conv bias instead of BatchNorm (dbeta is
 * then the bias gradient). Workspace: shpl_batch_norm_backward_workspace_bytes. */
int shpl_batch_norm_backward_workspace_bytes(int64_t rows, int64_t c, size_t *bytes);
int shpl_batch_norm_backward(int dtype, int64_t rows, const void *d_y, const void *d_raw, const void *d_gy,
                             int64_t stride, int64_t c, const float *d_mean, const float *d_scale,
                             const float *d_gamma, const float *d_beta, int act, int training, void *d_graw,
                             float *d_dbeta, float *d_dgamma, void *d_ws, size_t ws_bytes, void *stream);

/* Input gradient: dx = conv3x3_SAME(gy, W') with W'[ky][kx][co][ci] =
 * W[2-ky][2-kx][ci][co], the forward conv kernel on transposed packed
 * weights. d_weights: the forward's HWIO [3][3][c_dx][c_gy]. With d_dx_b
 * set, channels [0, c_split) go to d_dx and [c_split, c_dx) to d_dx_b (the
 * gradients of the conv's two sources, e.g. BEV and pooled image channels,
 * as separate dense maps); with d_dx_b NULL, c_split is ignored. Workspace:
 * shpl_conv3x3_workspace_bytes(dtype, n_frames, h, w, c_gy, 0, c_dx, -1, 0). */
int shpl_conv3x3_dgrad(int dtype, int n_frames, int64_t h, int64_t w, const void *d_gy, int64_t gy_stride,
                       int64_t c_gy, const void *d_weights, int64_t c_dx, void *d_dx, int64_t dx_stride,
                       int64_t c_split, void *d_dx_b, int64_t dx_b_stride, void *d_ws, size_t ws_bytes,
                       void *stream);

/* shpl_conv3x3_dgrad of the pooled bf16 fusion conv's two maps, d_dx_b (the pooled channels' gradient) written
 * only at the cells the pool's CSR has entries for -- the rows a pixel-keyed pull of it back to the image reads
 * (shpl_pull SHPL_BY_PIXEL); its other cells are left as they were. The occupancy comes from the forward
 * shpl_conv3x3 call over the same map, frames and shape (A = c_split channels, B = c_dx - c_split pooled
 * channels, c_gy outputs) that left it in d_fwd_ws (fwd_stats: whether that call took statistics), as
 * shpl_conv3x3_wgrad_reuse reads it: valid only for a forward for which shpl_conv3x3_rows_form reported 1;
 * what this call can check of that is SHPL_ERR_ARG when false. d_dx and the written cells of d_dx_b are
 * shpl_conv3x3_dgrad's, bit for bit. When the input gradient itself does not run the row-streaming form (f32,
 * misaligned maps) or has more than 32 gradient channels (c_gy), d_dx_b is written whole.
 * Image side (pool the pixel-keyed CSR of the forward, n_keys = n_frames*h*w image pixels): d_dx_b, the pooled
 * BEV channels' gradient over the image, is written only at the occupied pixels -- the rows a
 * shpl_pull(SHPL_BY_CELL, ...) over the SHPL_ORDER_COL_ENTRY CSR reads to carry it back to the BEV map.
 * Replaces: the image half of TF's conv2d backprop input in the rpn_model.py:338-354 fusion, which the
 * gradient of tf.gather_nd / tf.segment_sum (sparse_pool_utils.py:96-117) reads only at occupied cells. */
int shpl_conv3x3_dgrad_reuse(int dtype, int n_frames, int64_t h, int64_t w, const void *d_gy, int64_t gy_stride,
                             int64_t c_gy, const void *d_weights, int64_t c_dx, void *d_dx, int64_t dx_stride,
                             int64_t c_split, void *d_dx_b, int64_t dx_b_stride, void *d_ws, size_t ws_bytes,
                             const shpl_csr *pool, const void *d_fwd_ws, size_t fwd_ws_bytes, int fwd_stats,
                             void *stream);

/* Weight gradient: dw[ky][kx][ci][co] = sum over pixels of x[p + (ky-1, kx-1)][ci]
 * * gy[p][co], x given exactly as shpl_conv3x3's input (A channels, then B
 * channels, dense or pooled from the CSR -- recomputed, never stored). f32
 * MFMA (bf16: bf16 MFMA, exact products, f32 accumulation), per-workgroup
 * partials summed in a fixed order (f64): deterministic. d_dw: f32 HWIO
 * [3][3][c_a+c_b][c_out]. Workspace: pool_nnz_cap as shpl_conv3x3's (-1: B
 * dense or absent; with a pool, its CSR's nnz_cap, which sizes the compact
 * buffer of pooled runs of the bf16 form). pool may be the pixel-keyed CSR of
 * the image side, exactly as shpl_conv3x3 takes it (x = [img || the BEV map
 * pooled with shpl_pull(SHPL_BY_PIXEL)'s per-column sums]). */
int shpl_conv3x3_wgrad_workspace_bytes(int dtype, int n_frames, int64_t h, int64_t w, int64_t c_a, int64_t c_b,
                                       int64_t c_out, int64_t pool_nnz_cap, size_t *bytes);
int shpl_conv3x3_wgrad(int dtype, int n_frames, int64_t h, int64_t w, const void *d_a, int64_t a_stride,
                       int64_t a_off, int64_t c_a, const void *d_b, int64_t b_stride, int64_t b_off, int64_t c_b,
                       const shpl_csr *pool, const int64_t *d_frame_off, const void *d_gy, int64_t gy_stride,
                       int64_t c_out, float *d_dw, void *d_ws, size_t ws_bytes, void *stream);

/* shpl_conv3x3_wgrad of the pooled bf16 form reading the pooled operand (the cell-keyed CSR's occupancy maps
 * and per-run pooled rows) that a forward shpl_conv3x3 call over the same map, image, frames, shape and
 * channels left in its workspace, instead of preparing it again (k_occ_frame + k_pool_runs): the training
 * step's weight gradient after its forward. d_fwd_ws / fwd_ws_bytes: that call's workspace, not written since;
 * fwd_stats: whether that call took statistics (its workspace layout). Valid only for a forward call for which
 * shpl_conv3x3_rows_form reported 1 (the caller's to establish: the forward's act and output pointer are not
 * arguments here); what this call can check of that predicate and finds false is SHPL_ERR_ARG. When the
 * weight gradient itself does not run the row-streaming form the workspace is not read. Same results as
 * shpl_conv3x3_wgrad, bit for bit. Cell-keyed or pixel-keyed pool alike (the forward's). */
int shpl_conv3x3_wgrad_reuse(int dtype, int n_frames, int64_t h, int64_t w, const void *d_a, int64_t a_stride,
                             int64_t a_off, int64_t c_a, const void *d_b, int64_t b_stride, int64_t b_off,
                             int64_t c_b, const shpl_csr *pool, const int64_t *d_frame_off, const void *d_gy,
                             int64_t gy_stride, int64_t c_out, float *d_dw, void *d_ws, size_t ws_bytes,
                             const void *d_fwd_ws, size_t fwd_ws_bytes, int fwd_stats, void *stream);

/* ---------------------------------------------------------------------------
 * After-VGG upconv3: 3x3 stride-2 transposed conv over the fused conv4 map
 * ------------------------------------------------------------------------- */

/* TF's conv2d_transpose, SAME, stride 2, 3x3, over n_frames frames of h x w input pixels, 2h x 2w output pixels:
 *   out[f,oy,ox,co] = epilogue( sum over (i,ky): 2i+ky = oy, (j,kx): 2j+kx = ox, ci of
 *                               x[f,i,j,ci] * W[ky,kx,co,ci] ),   0 <= i < h, 0 <= j < w, ky, kx in 0..2
 * -- the input gradient of the SAME stride-2 conv over 2h x 2w, whose padding is pad_total = 1, pad_before =
 * pad_total // 2 = 0, pad_after = 1 (TF's conv2d_backprop_input). Even oy = 2i takes ky = 0 from row i and ky = 2
 * from row i-1, odd oy = 2i+1 takes ky = 1 from row i; columns alike: every output pixel reads the window
 * x[i-1..i, j-1..j] (zeros outside), 9 c_in c_out multiply-adds per input pixel. In torch terms:
 * conv_transpose2d(x_nchw, W.permute(3,2,0,1), stride=2)[..., :2h, :2w].
 * x = [a || b] exactly as shpl_conv3x3 takes its sources: channels [0, c_a) row r of d_a (r the input pixel
 * (f*h + i)*w + j), channels [c_a, c_a + c_b) row r of d_b (pool NULL: a second dense map; c_b = 0: none), or
 * the pooled map computed in the staging from the pool's CSR over d_b -- cell-keyed (shpl_build_csr
 * SHPL_BY_CELL, SHPL_ORDER_ENTRY: a the BEV map, b the image map) or pixel-keyed (SHPL_BY_PIXEL,
 * SHPL_ORDER_COL_ROW, with ent_col or flagged SHPL_CSR_IDENTITY_COLS: a the image map, b the BEV map; per-column
 * partial sums first under ent_col), n_keys = n_frames*h*w, entry slots of frame f from d_frame_off[f] on, with
 * shpl_pull's arithmetic: when c_a is a multiple of the staging chunk (8 f32 / 16 bf16 channels) the pooled
 * call gives bitwise the result of the same call with d_b = the dense map shpl_pull writes (the pooled values
 * are formed in the pull's order and rounded to the storage dtype once, before the MFMA).
 * d_weights: slim's conv2d_transpose variable [3][3][c_out][c_a+c_b] ("HWOI") in the feature dtype.
 * Output rows are NHWC with global id (f*2h + oy)*2w + ox, out_stride elements apart. Everything else is
 * shpl_conv3x3's contract: the epilogue (acc - center) * scale + shift with one rounding and ReLU on the bit
 * pattern; d_stats (optional, [2][c_out] f64) = per-channel sum and sum of squares of the pre-epilogue output
 * over all n_frames*2h*2w rows, deterministic, as shpl_batch_norm takes it; the argument checks, their status
 * codes and order; stream-ordered, no allocation, no host synchronisation (capturable). f32:
 * v_mfma_f32_32x32x2_f32 (exact f32 products); SHPL_BF16: v_mfma_f32_32x32x16_bf16; f32 accumulation, one
 * rounding at the store. One input tile is staged once and feeds the accumulators of all four output parities.
 * Workspace: shpl_upconv3x3_workspace_bytes, pool_nnz_cap = pool->nnz_cap for a pooled call, -1 without a pool.
 * Replaces: sparse_pool_layer over conv4 (avod/avod/core/feature_extractors/fusion_vgg_pyramid.py:53-60)
 *   followed by slim.conv2d_transpose(conv4, vgg_conv3[1], [3,3], stride=2, normalizer_fn=slim.batch_norm)
 *   (fusion_vgg_pyramid.py:198-206, scope upconv3), both sides. */
int shpl_upconv3x3_workspace_bytes(int dtype, int n_frames, int64_t h, int64_t w, int64_t c_a, int64_t c_b,
                                   int64_t c_out, int64_t pool_nnz_cap, int stats, size_t *bytes);
int shpl_upconv3x3(int dtype, int n_frames, int64_t h, int64_t w, const void *d_a, int64_t a_stride,
                   int64_t a_off, int64_t c_a, const void *d_b, int64_t b_stride, int64_t b_off, int64_t c_b,
                   const shpl_csr *pool, const int64_t *d_frame_off, const void *d_weights /* HWOI */,
                   int64_t c_out, const float *d_center, const float *d_scale, const float *d_shift, int act,
                   void *d_out, int64_t out_stride, double *d_stats, void *d_ws, size_t ws_bytes, void *stream);

/* Input gradient of shpl_upconv3x3 (its adjoint in x). h, w are the INPUT map's size; d_gy is the gradient of the
 * raw (pre-epilogue) output, 2h x 2w rows per frame of c_gy channels, gy_stride elements apart:
 *   dx[f,i,j,ci] = sum over ky, kx in 0..2 with 2i+ky < 2h, 2j+kx < 2w, and co of
 *                  gy[f,2i+ky,2j+kx,co] * W[ky,kx,co,ci]
 * (a tap whose output pixel falls outside the map contributes nothing: ky = 2 at i = h-1, kx = 2 at j = w-1).
 * d_weights is the forward's variable [3][3][c_gy][c_dx] (HWOI), unpacked and untransposed by the caller.
 * c_split, d_dx_b, dx_b_stride as in shpl_conv3x3_dgrad: channels [0, c_split) go to d_dx (dx_stride apart),
 * channels [c_split, c_dx) to d_dx_b, a dense map in the feature dtype whose every row is written -- the pooled
 * half, which shpl_pull over the side's gradient CSR then carries back to its source; with d_dx_b NULL the
 * split is ignored and all c_dx channels go to d_dx.
 * f32: v_mfma_f32_32x32x2_f32 (exact f32 products); SHPL_BF16: v_mfma_f32_32x32x16_bf16; f32 accumulation, one
 * rounding at the store; no atomics, bitwise repeatable. One staged chunk of gy feeds up to four blocks of 32 dx
 * channels. shpl_upconv3x3's argument checks, status codes and order, with gy in the place of the output
 * (gy_stride < c_gy: SHPL_ERR_BAD_SHAPE); n_frames, h or w of 0: SHPL_OK, nothing launched. Stream-ordered, no
 * allocation, no host synchronisation (capturable). Workspace: shpl_upconv3x3_dgrad_workspace_bytes. */
int shpl_upconv3x3_dgrad_workspace_bytes(int dtype, int n_frames, int64_t h, int64_t w, int64_t c_gy,
                                         int64_t c_dx, size_t *bytes);
int shpl_upconv3x3_dgrad(int dtype, int n_frames, int64_t h, int64_t w, const void *d_gy, int64_t gy_stride,
                         int64_t c_gy, const void *d_weights /* HWOI [3][3][c_gy][c_dx] */, int64_t c_dx,
                         void *d_dx, int64_t dx_stride, int64_t c_split, void *d_dx_b, int64_t dx_b_stride,
                         void *d_ws, size_t ws_bytes, void *stream);

/* Weight gradient of shpl_upconv3x3 (its adjoint in W), f32 HWOI:
 *   dW[ky,kx,co,ci] = sum over f, i, j with 2i+ky < 2h, 2j+kx < 2w of gy[f,2i+ky,2j+kx,co] * x[f,i,j,ci]
 * x = [a || b] given exactly as shpl_upconv3x3 takes its sources, in every form: dense, c_b = 0, pooled through the
 * cell-keyed CSR, pooled through the pixel-keyed CSR (ent_col groups or SHPL_CSR_IDENTITY_COLS). The pooled
 * channels are recomputed in the staging, in the pull's order, rounded once to the storage dtype and never
 * stored: when c_a is a multiple of the staging chunk (8 f32 / 16 bf16 channels) the pooled call gives bitwise
 * the dW of the same call with d_b = the dense map shpl_pull writes. d_gy as in shpl_upconv3x3_dgrad, c_out
 * channels. f32: v_mfma_f32_32x32x2_f32 (exact f32 products); SHPL_BF16: v_mfma_f32_32x32x16_bf16; f32 sums per
 * workgroup, the workgroups' partials added in a fixed order (f64): no atomics, bitwise repeatable.
 * shpl_upconv3x3's argument checks, status codes and order, with gy in the place of the output and d_dw in the
 * place of the weights; n_frames, h or w of 0: SHPL_OK, nothing launched (d_dw is left as it is). Stream-ordered,
 * no allocation, no host synchronisation (capturable). Workspace: shpl_upconv3x3_wgrad_workspace_bytes,
 * pool_nnz_cap = pool->nnz_cap for a pooled call, -1 without a pool. */
int shpl_upconv3x3_wgrad_workspace_bytes(int dtype, int n_frames, int64_t h, int64_t w, int64_t c_a, int64_t c_b,
                                         int64_t c_out, int64_t pool_nnz_cap, size_t *bytes);
int shpl_upconv3x3_wgrad(int dtype, int n_frames, int64_t h, int64_t w, const void *d_a, int64_t a_stride,
                         int64_t a_off, int64_t c_a, const void *d_b, int64_t b_stride, int64_t b_off, int64_t c_b,
                         const shpl_csr *pool, const int64_t *d_frame_off, const void *d_gy, int64_t gy_stride,
                         int64_t c_out, float *d_dw /* f32 HWOI [3][3][c_out][c_a+c_b] */, void *d_ws,
                         size_t ws_bytes, void *stream);

/* ---------------------------------------------------------------------------
 * 1x1 heads over the fused map, the SHPL applied after the projection
 * (MV3D's rpn_cls_score / rpn_bbox_pred)
 * ------------------------------------------------------------------------- */

/* out[r, co] = sum_ci [a || b'][r, ci] * W[ci, co] + bias[co], a 1x1 VALID conv with a bias and no activation
 * over `rows` rows. Channels [0, c_a) are row r of d_a (element r*a_stride + a_off + c); channels
 * [c_a, c_a + c_b) come from d_b:
 *   pool == NULL: row r of d_b (r*b_stride + b_off + c), a second dense map of rows_b == rows rows; c_b = 0
 *                 (d_b NULL, rows_b ignored) is the one-map form, the head of a materialised conv_lidar_fused;
 *   pool != NULL: the img->BEV pooled map of the image map d_b (rows_b pixels) through the cell-keyed CSR
 *                 (shpl_build_csr SHPL_BY_CELL, SHPL_ORDER_ENTRY, n_keys == rows; a pixel-keyed CSR -- ent_col
 *                 set or SHPL_CSR_IDENTITY_COLS -- is SHPL_ERR_ARG). A 1x1 conv and the SHPL are both linear,
 *                 so the head is applied before the pooling and neither the pooled map nor the concat is
 *                 ever written. The summation contract:
 *                     Z[p, :]   = b[p, :] . W[c_a:, :]                       (f32, in the workspace, no bias)
 *                     out[r, :] = a[r, :] . W[:c_a, :] + bias + sum_{k in run(r)} m_k * Z[src_k, :]
 *                 with the run of cell r walked in CSR order, one f32 multiply and one f32 add per entry
 *                 (no FMA contraction), as shpl_pull walks it; the two products are MFMA sums over the
 *                 channels. The result is the 1x1 conv of [a || shpl_pull(SHPL_BY_CELL, ...)] up to summation
 *                 order -- NOT bitwise: the pooled form sums sum_k m_k (sum_c b W) where the materialised one
 *                 sums sum_c (sum_k m_k b) W. The runs come from pool->key_range (global entry slots, so no
 *                 per-frame entry offsets are taken); a CSR without it gets one built in the workspace.
 * d_weights: [c_a + c_b][c_out] in the feature dtype (the HWIO variable of a 1x1 slim / Network.conv layer),
 * 1 <= c_out <= 32; d_bias: optional [c_out] f32. Several heads share one call with their weights joined
 * along c_out. f32: v_mfma_f32_32x32x2_f32; SHPL_BF16: bf16 maps and weights, v_mfma_f32_32x32x16_bf16, f32
 * accumulation, Z and the run sum in f32, one rounding at the store of d_out ([rows], out_stride elements
 * per row, feature dtype). Workspace: shpl_head1x1_workspace_bytes (pooled = pool != NULL), which also
 * covers shpl_head1x1_dgrad.
 * Replaces: sparse_pool (network.py:243-246), the concat and the two 1x1 convs of
 *   MV3D_TF_release/lib/networks/MV3D_voxel_train.py:144-178 (keep_prob = 1). */
int shpl_head1x1_workspace_bytes(int dtype, int64_t rows, int64_t c_a, int64_t rows_b, int64_t c_b, int64_t c_out,
                                 int pooled, size_t *bytes);
int shpl_head1x1(int dtype, int64_t rows, const void *d_a, int64_t a_stride, int64_t a_off, int64_t c_a,
                 const void *d_b, int64_t b_stride, int64_t b_off, int64_t c_b, int64_t rows_b,
                 const shpl_csr *pool, const void *d_weights, int64_t c_out, const float *d_bias, void *d_out,
                 int64_t out_stride, void *d_ws, size_t ws_bytes, void *stream);

/* Input gradients of shpl_head1x1: d_da[r, c] = sum_co gy[r, co] * W[c, co] ([rows], da_stride), and for the
 * second source d_db = G . W[c_a:, :]^T with G = gy (pool_grad NULL: dense b, rows_b == rows) or
 * G = _sparse_pool_trans_op(M, gy), the gradient pulled back to the rows_b pixels at c_out channels through
 * pool_grad, the pixel-keyed CSR of the pooled source's gradient (shpl_build_csr SHPL_BY_PIXEL,
 * SHPL_ORDER_COL_ENTRY, n_keys == rows_b; shpl_pull's sums, kept in f32 in the workspace; a cell-keyed CSR is
 * SHPL_ERR_ARG). Either output may be NULL. The sums over co are f32 fused multiply-adds in co order; one
 * rounding at the store (feature dtype). Workspace: shpl_head1x1_workspace_bytes. */
int shpl_head1x1_dgrad(int dtype, int64_t rows, const void *d_gy, int64_t gy_stride, int64_t c_out,
                       const void *d_weights, int64_t c_a, int64_t c_b, void *d_da, int64_t da_stride, void *d_db,
                       int64_t db_stride, int64_t rows_b, const shpl_csr *pool_grad, void *d_ws, size_t ws_bytes,
                       void *stream);

/* Weight and bias gradients of shpl_head1x1: d_dw f32 [c_a + c_b][c_out], dw[c, co] = sum_r x[r, c] * G[r, co]
 * over the rows of `a` with G = gy, and over the rows of `b` with G as in shpl_head1x1_dgrad (pool_grad: the
 * same pixel-keyed CSR, NULL for dense b); d_dbias (optional, [c_out] f32) = sum_r gy[r, :]. Two stages:
 * per-row-chunk f32 partials in the workspace (fused multiply-adds in row order), then the partials summed in
 * chunk order in f64 -- no floating-point atomics, bitwise the same from run to run. */
int shpl_head1x1_wgrad_workspace_bytes(int dtype, int64_t rows, int64_t c_a, int64_t rows_b, int64_t c_b,
                                       int64_t c_out, int pooled, size_t *bytes);
int shpl_head1x1_wgrad(int dtype, int64_t rows, const void *d_a, int64_t a_stride, int64_t a_off, int64_t c_a,
                       const void *d_b, int64_t b_stride, int64_t b_off, int64_t c_b, int64_t rows_b,
                       const shpl_csr *pool_grad, const void *d_gy, int64_t gy_stride, int64_t c_out, float *d_dw,
                       float *d_dbias, void *d_ws, size_t ws_bytes, void *stream);

/* ---------------------------------------------------------------------------
 * The same heads under dropout over conv_lidar_fused (MV3D's training step)
 * ------------------------------------------------------------------------- */

/* The dropout mask: a pure function of (seed, row, channel, keep_prob) -- no state, no stored tensor.
 *   T = clamp(floor(keep_prob * 65536 + 0.5), 1, 65536) in double; keep_prob outside (0, 1] (NaN included) is
 *   SHPL_ERR_ARG. The effective keep probability is T / 65536 and scale = (float)(65536.0 / T) (exact for 0.5);
 *   keep_prob = 1 gives T = 65536: everything kept, scale 1.
 *   For row r (the global row of the call: the BEV cell over all frames, int64) and concat channel c in
 *   [0, c_a + c_b) (the channels of `a` first, then the second source's): g = c >> 3, j = c & 7,
 *     (w0..w3) = Philox4x32-10(counter (r & 0xffffffff, r >> 32, g, 0), key (seed & 0xffffffff, seed >> 32)),
 *     h = (w[j >> 1] >> (16 * (j & 1))) & 0xffff, and the element is KEPT iff h < T.
 *   One Philox call covers 8 consecutive channels (one 16-byte bf16 piece, two f32 pieces).
 *   Philox4x32-10 is Random123's: multipliers M0 = 0xD2511F53, M1 = 0xCD9E8D57, key increments 0x9E3779B9,
 *   0xBB67AE85 after each round, ten rounds of
 *     (c0, c1, c2, c3) <- (hi(M1*c2) ^ c1 ^ k0, lo(M1*c2), hi(M0*c0) ^ c3 ^ k1, lo(M0*c0)).
 *   Known answer: counter 0,0,0,0 key 0,0 -> 6627e8d5 e169c58d bc57ac4c 9b00dbd8.
 * TF's tf.nn.dropout stream cannot be reproduced and nothing here tries to: parity with the reference is
 * distributional, iid Bernoulli(T / 65536) per element of the [rows, c_a + c_b] map. TF forms
 * (x / keep_prob) * mask before the conv; here the scale multiplies the f32 channel sum, which differs only by
 * where the scale is rounded (identical at 0.5). `seed` is a host scalar passed by value: a captured graph
 * replays the same mask (a device-side seed is not offered).
 *
 * shpl_dropout_mask writes the mask as an array, d_mask u8 [rows][c] (1 kept, 0 dropped) -- for checks and for
 * callers that need it elsewhere; the head calls below never read or write one. */
int shpl_dropout_mask(int64_t rows, int64_t c, double keep_prob, uint64_t seed, uint8_t *d_mask, void *stream);

/* shpl_head1x1 under that mask: with x[r, c] = a[r, c] for c < c_a and x[r, c_a + c] = the second source's
 * channel c (pool == NULL: row r of d_b, or no second source with c_b = 0, the one-map form over a materialised
 * drop_fused's input; pool != NULL: the img->BEV pooled value through the cell-keyed CSR),
 *     out[r, co] = scale * sum_c keep(r, c) * x[r, c] * W[c, co] + bias[co].
 * The mask sits between the pooling and the projection, so the projection cannot move before the pooling as
 * in shpl_head1x1; the pooling moves into the GEMM's operand staging instead. The pooled value is the f32 run
 * sum of cell r in CSR order from zero, one multiply and one add per entry (no FMA contraction), exactly as
 * shpl_pull(SHPL_BY_CELL) sums it, rounded once to the feature dtype: the MFMA operand is bit-equal to the
 * element of the materialised bv_fused. The channel sum is an f32 MFMA sum (the channels of `a`, then the
 * second source's; n = c_a + c_b terms); then one f32 multiply by scale, one add of the bias and one rounding
 * at the store. The result equals the heads of dropout([a || shpl_pull(...)]) with this mask up to the order
 * of the channel sum -- not bitwise. Neither the pooled map, the concat nor a mask is written anywhere: the
 * workspace (shpl_head1x1_drop_workspace_bytes, which also covers shpl_head1x1_drop_dgrad) holds the packed
 * weights, the f32 padded copy of gy and key ranges for a CSR that carries none -- nothing proportional to
 * rows * c_b, rows * (c_a + c_b) or nnz * c_b. Arguments and errors as shpl_head1x1, plus the keep_prob range.
 * Replaces: sparse_pool, the concat, dropout and the two 1x1 convs of
 *   MV3D_TF_release/lib/networks/MV3D_voxel_train.py:144-178 with use_dropout (keep_prob 0.5 in training). */
int shpl_head1x1_drop_workspace_bytes(int dtype, int64_t rows, int64_t c_a, int64_t rows_b, int64_t c_b,
                                      int64_t c_out, int pooled, size_t *bytes);
int shpl_head1x1_drop(int dtype, int64_t rows, const void *d_a, int64_t a_stride, int64_t a_off, int64_t c_a,
                      const void *d_b, int64_t b_stride, int64_t b_off, int64_t c_b, int64_t rows_b,
                      const shpl_csr *pool, const void *d_weights, int64_t c_out, const float *d_bias, void *d_out,
                      int64_t out_stride, double keep_prob, uint64_t seed, void *d_ws, size_t ws_bytes,
                      void *stream);

/* Input gradients of shpl_head1x1_drop, the autodiff of its expression with the mask computed again:
 *     d_da[r, c] = keep(r, c) * scale * sum_co gy[r, co] * W[c, co]      (exactly 0 where dropped)
 *     d_db[p, c] = sum over the entries k = (cell r_k, m_k) of pixel p's run of pool_grad, in CSR order from zero,
 *                  of m_k * (keep(r_k, c_a + c) * scale * sum_co gy[r_k, co] * W[c_a + c, co])
 * (pool_grad: the pixel-keyed CSR shpl_head1x1_dgrad takes, a cell-keyed one is SHPL_ERR_ARG; NULL: d_db as
 * d_da over the dense second source). The sums over co are f32 fused multiply-adds in co order (c_out terms),
 * then one multiply by scale; per kept entry one multiply by m_k and one add (a dropped entry adds nothing; no
 * per-column partials); one rounding at the store. Either output may be NULL. */
int shpl_head1x1_drop_dgrad(int dtype, int64_t rows, const void *d_gy, int64_t gy_stride, int64_t c_out,
                            const void *d_weights, int64_t c_a, int64_t c_b, void *d_da, int64_t da_stride,
                            void *d_db, int64_t db_stride, int64_t rows_b, const shpl_csr *pool_grad,
                            double keep_prob, uint64_t seed, void *d_ws, size_t ws_bytes, void *stream);

/* Weight and bias gradients of shpl_head1x1_drop: d_dw f32 [c_a + c_b][c_out],
 *     dw[c, co] = scale * sum_r keep(r, c) * x[r, c] * gy[r, co],       d_dbias[co] = sum_r gy[r, co]
 * with both halves summed over the cells r. `pool` is the forward's CELL-keyed CSR (a pixel-keyed one is
 * SHPL_ERR_ARG): x[r, c_a + c] is formed again as the forward forms it, the run sum of cell r rounded once to
 * the feature dtype. Two stages: per-row-chunk f32 partials (rows ascending, fused multiply-adds, eight waves'
 * sums added in a fixed order, then one multiply by scale) in the workspace, at most 64 chunks, then the
 * partials summed in chunk order in f64 and rounded once -- no floating-point atomics, bitwise the same from
 * run to run. Workspace: shpl_head1x1_drop_wgrad_workspace_bytes (partials and key ranges only). */
int shpl_head1x1_drop_wgrad_workspace_bytes(int dtype, int64_t rows, int64_t c_a, int64_t rows_b, int64_t c_b,
                                            int64_t c_out, int pooled, size_t *bytes);
int shpl_head1x1_drop_wgrad(int dtype, int64_t rows, const void *d_a, int64_t a_stride, int64_t a_off, int64_t c_a,
                            const void *d_b, int64_t b_stride, int64_t b_off, int64_t c_b, int64_t rows_b,
                            const shpl_csr *pool, const void *d_gy, int64_t gy_stride, int64_t c_out, float *d_dw,
                            float *d_dbias, double keep_prob, uint64_t seed, void *d_ws, size_t ws_bytes,
                            void *stream);

/* ---------------------------------------------------------------------------
 * SHPL concat with BatchNorm on both halves (the intent of use_bn=True)
 * ------------------------------------------------------------------------- */

/* out[d] = [BN(pass[d]) || BN(pooled[d])] for every destination row d of csr, C = c_pass + c_pool channels,
 * pooled[d] the f32 run sum of shpl_pull (same entry order, separate multiply and add, per-column partials for
 * a pixel-keyed CSR with ent_col) -- never stored, and in bf16 never rounded before it is normalised. Each
 * channel has its own BatchNorm: every per-channel array below is [C], the pass-through half's c_pass entries
 * first. csr must carry key_range (shpl_pull_once's requirement; SHPL_ERR_ARG without).
 *   training : per channel, in f64: s1 = sum x, s2 = sum x^2 -- over all rows for the pass-through half, over
 *              the occupied rows only for the pooled half (its other rows are 0) -- count = csr->n_keys (all
 *              rows of the batch) for both; mean = s1 / count, var = max(s2 / count - mean^2, 0),
 *              scale = gamma / sqrt(var + eps), moving averages m -= (m - v)(1 - decay) with the Bessel-
 *              corrected variance, d_batch_mean / d_batch_var optional (shpl_batch_norm's finalize).
 *              Summation order: blocks of rows (4096, at most 1024 blocks), inside a block each of its row
 *              lanes adds its rows in ascending order, the lanes are added in lane order, the blocks' partials
 *              in a fixed strided order; no floating-point atomics: two runs give the same bits.
 *   inference: mean = d_moving_mean, scale = gamma / sqrt(d_moving_var + eps) (both required, read only);
 *              one launch, no statistics pass, no workspace.
 *   y = (x - mean) * scale (+ beta), one rounded f32 operation at a time; an empty row's pooled half is the
 *   per-channel constant (0 - mean) * scale + beta, one bit pattern per channel.
 * d_gamma NULL: 1 (slim's scale=False); d_beta NULL: 0. d_save [2][C] (required in training, optional in
 * inference) receives mean and scale, which shpl_concat_bn_backward takes. Training launches: the partial
 * statistics, their reduction, the finalize, the apply; it reads the pass-through half and the gathered source
 * rows twice and writes out once. 16-byte chunks under shpl_pull's alignment rule, one element otherwise.
 * Errors: csr NULL or without key_range, c_pass or c_pool <= 0, d_out / d_src / d_pass NULL, out_stride <
 * c_pass + c_pool, a dtype or direction outside the enums, training without a workspace (or d_save) or with
 * ws_bytes below shpl_concat_bn_workspace_bytes, inference without moving statistics: SHPL_ERR_ARG, nothing
 * launched; the size limits and stride rules of shpl_pull: SHPL_ERR_BAD_SHAPE.
 * Replaces: sparse_pool_utils.py:69-70 / :84-85 with concat_bn_op :120-124, as intended -- BatchNorm on each
 * half, then concat. The reference's own code at those lines calls slim.batch_norm(x, training=...), a keyword
 * slim does not have, and raises TypeError; sparse_pool_layer(use_bn=True) of this library keeps doing that. */
int shpl_concat_bn_workspace_bytes(int64_t rows, int64_t c_pass, int64_t c_pool, size_t *bytes);
int shpl_concat_bn(int direction, int dtype, const shpl_csr *csr, const void *d_src, int64_t src_stride,
                   int64_t src_off, int64_t c_pool, const void *d_pass, int64_t pass_stride, int64_t pass_off,
                   int64_t c_pass, void *d_out, int64_t out_stride, int training, float eps, float decay,
                   const float *d_gamma, const float *d_beta, float *d_moving_mean, float *d_moving_var,
                   float *d_batch_mean, float *d_batch_var, float *d_save, void *d_ws, size_t ws_bytes,
                   void *stream);

/* The autodiff of shpl_concat_bn (no activation). d_g [rows][>= C] at g_stride; d_save the forward's mean and
 * scale; xhat = (x - mean) * scale / gamma with x the pass-through value or the run sum (0 at an empty row).
 * Per channel, in f64 and the forward's summation order: dbeta = sum g, dgamma = sum g * xhat; for the pooled
 * half sum g * xhat = xhat_empty * sum g + the sum over the occupied rows of g * (xhat - xhat_empty), with
 * xhat_empty = (0 - mean) * scale / gamma. Then
 *   training:  g_x = scale * (g - dbeta / rows - xhat * dgamma / rows)
 *   inference: g_x = scale * g
 * written for the pass-through half to d_gpass [rows][c_pass] (gpass_stride, the feature dtype), and for the
 * pooled half, at the occupied rows only, to d_gpool f32 [rows][c_pool] (contiguous rows, caller-owned scratch
 * that is never cleared and never read elsewhere). With d_gsrc set, csr_grad -- the CSR of the same map keyed by
 * the source's rows (the other direction, SHPL_ORDER_COL_ENTRY) -- carries d_gpool back: d_gsrc f32
 * [csr_grad->n_keys][c_pool] (gsrc_stride) = shpl_pull(the other direction, SHPL_F32, SHPL_OUT_POOL) of
 * d_gpool, which reads the occupied rows only. Both are f32 in either dtype: the source's gradient is summed
 * from unrounded g_x and rounded once, by the caller that wants it in bf16.
 * Every entry of the map must lie inside its frame in both CSRs. d_dbeta / d_dgamma [C], optional.
 * Errors as shpl_concat_bn's; d_g, d_gpass, d_gpool or d_save NULL, d_gsrc without csr_grad: SHPL_ERR_ARG. */
int shpl_concat_bn_backward_workspace_bytes(int64_t rows, int64_t c_pass, int64_t c_pool, size_t *bytes);
int shpl_concat_bn_backward(int direction, int dtype, const shpl_csr *csr, const shpl_csr *csr_grad,
                            const void *d_src, int64_t src_stride, int64_t src_off, int64_t c_pool,
                            const void *d_pass, int64_t pass_stride, int64_t pass_off, int64_t c_pass,
                            const void *d_g, int64_t g_stride, const float *d_save, const float *d_gamma,
                            int training, void *d_gpass, int64_t gpass_stride, void *d_gpool, void *d_gsrc,
                            int64_t gsrc_stride, float *d_dbeta, float *d_dgamma, void *d_ws, size_t ws_bytes,
                            void *stream);

#ifdef __cplusplus
}
#endif
#endif /* SHPL_H */
