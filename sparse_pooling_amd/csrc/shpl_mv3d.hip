// shpl_mv3d.hip -- MV3D_TF's SHPL producer on the device.
//
// Reference: point_cloud_2_top_sparse   MV3D_TF_release/lib/utils/construct_voxel.py:37-162
// (called per minibatch from roi_data_layer/minibatch_mv3d_img.py:88-93 with
// img_index2 = np.round(projectToImage(points, P2)).astype(int)).
// Per frame, with camera-frame points reordered to (forward, side, height):
//   keep points strictly inside the forward / side / height ranges;
//   voxel (side, fwd, height) = int((coord - range_min) / res)   [astype(int32)]
//   np.unique(axis=0) orders voxels lexicographically by (side, fwd, height);
//   walking the points in order, a voxel accepts its first VOXEL_POINT_COUNT
//   points; the accepted points, in point order, give
//     img_index = [img_index2; 0], bv_index = (fwd, side),
//     M_val = 1 / (points accepted by the point's voxel)   (MV3D's mean pooling).
// Optionally the front-view augmentation's index transform follows
// (augment_fv, MV3D_TF_release/lib/roi_data_layer/minibatch_mv3d_img.py:191-209).
// Here one workgroup per frame sorts the packed (voxel, point) words
// (shpl_tilesort.h); the thread at the start of each voxel run marks the run's
// first VOXEL_POINT_COUNT points accepted with weight 1/min(run, cap); a
// ballot compaction then emits the accepted points in point order.
//
// augment_voxel (minibatch_mv3d_img.py:132-189; cfg.TRAIN.AUGMENT_BV, the training default) sits in front of
// the producer: an optional redraw of the cloud (points[remain_index]), the projection of the ORIGINAL points
// (img_index2), then shift, scale and a rotation about the camera's y axis of the coordinates the voxels are
// keyed on. k_mv3d_augment writes that cloud and img_index2; k_mv3d_frame<T, true> does the same per point in
// registers, where it forms the voxel words and again where it emits the accepted points, and writes neither.
// T is the cloud's storage type: the reference rounds to it after every step, and on an f32 cloud numpy also
// runs the producer's range tests and voxel indices in f32 (python-float bounds do not promote an f32 array),
// so voxel_key<float> does.
#include "shpl_tilesort.h"

namespace shpl {
namespace {

struct Mv3dGeom {
    double fwd_lo, fwd_hi, side_lo, side_hi, h_lo, h_hi;  // strict ranges
    double res, zres;
    int n_side, n_fwd, n_h;  // voxel_full_size = (n_h, n_side, n_fwd)
    int cap;                 // VOXEL_POINT_COUNT
    int log_tile;
    int has_proj;            // 1: img_index2 from P2 on the device
};

// projectToImage + np.round (minibatch_mv3d_img.py:88-91)
// (gemv: the frame has one point, so np.dot has one column -- dgemv's order)
__device__ __forceinline__ void project_round(const double *P, double x, double y, double z, int64_t &u, int64_t &v,
                                              bool gemv) {
    double uf, vf;
    project(P, x, y, z, uf, vf, gemv);
    u = (int64_t)rint(uf);
    v = (int64_t)rint(vf);
}

__device__ __forceinline__ double sub_rn(double a, double b) { return __dsub_rn(a, b); }
__device__ __forceinline__ float sub_rn(float a, float b) { return __fsub_rn(a, b); }
__device__ __forceinline__ double div_rn(double a, double b) { return __ddiv_rn(a, b); }
__device__ __forceinline__ float div_rn(float a, float b) { return __fdiv_rn(a, b); }

// voxel key of camera-frame point (x, y, z) or -1 when outside the ranges, in the cloud's type T (the bounds
// and sizes rounded to it, as numpy rounds python floats beside an f32 array)
template <typename T>
__device__ __forceinline__ int64_t voxel_key(const Mv3dGeom &g, T x, T y, T z, int &si, int &fi) {
    const T fwd = z, side = x, h = y;  // points[:, [2, 0, 1, 3]]
    if (!(fwd > (T)g.fwd_lo && fwd < (T)g.fwd_hi && side > (T)g.side_lo && side < (T)g.side_hi && h > (T)g.h_lo &&
          h < (T)g.h_hi))
        return -1;
    si = (int)div_rn(sub_rn(side, (T)g.side_lo), (T)g.res);
    fi = (int)div_rn(sub_rn(fwd, (T)g.fwd_lo), (T)g.res);
    const int hi = (int)div_rn(sub_rn(h, (T)g.h_lo), (T)g.zres);
    if constexpr (!std::is_same<T, double>::value) {
        // f64 quotients are monotone below the host's f64 sizes; f32 roundings of caller-chosen ranges need
        // not be: a cell outside the grid is no voxel (the sort's tiles are sized for the grid)
        if (si >= g.n_side || fi >= g.n_fwd || hi >= g.n_h) return -1;
    }
    return ((int64_t)si * g.n_fwd + fi) * g.n_h + hi;
}

// augment_voxel's device arguments (the augmented instantiations only)
template <bool AUG>
struct Mv3dAug {};
template <>
struct Mv3dAug<true> {
    const double *vox_aug;   // [F, 8]: sx, sz, ratio, r00, r01, r10, r11, 0
    const int64_t *remain;   // optional [n_out]: frame-local source point of each out point (AUGMENT_PC)
    const int64_t *out_off;  // [F + 1] out points of each frame (the point offsets without remain)
    int64_t n_in, n_out;     // points, out points over all frames: every offset is held inside them
    uint32_t *err;           // nullable: SHPL_EBIT_GATHER
};

// Frame f's out points [p0, p1) and source points [q0, q0 + nq): offsets outside the arrays, decreasing, or
// (no remain) unequal counts make the frame empty and set SHPL_EBIT_GATHER -- nothing is read through them.
__device__ __forceinline__ void aug_frame(const Mv3dAug<true> &ag, const int64_t *pt_off, int f, int64_t &p0,
                                          int64_t &p1, int64_t &q0, int64_t &nq) {
    p0 = ag.out_off[f];
    p1 = ag.out_off[f + 1];
    q0 = pt_off[f];
    nq = pt_off[f + 1] - q0;
    if (p0 < 0 || p1 < p0 || p1 > ag.n_out || q0 < 0 || nq < 0 || nq > ag.n_in - q0 || (!ag.remain && nq != p1 - p0)) {
        if (threadIdx.x == 0 && ag.err) atomicOr(ag.err, SHPL_EBIT_GATHER);
        p0 = p1 = q0 = nq = 0;
    }
}

// Source row of out point i of a frame (aug_frame's ranges), or -1 for a remain_index entry outside the frame
// (SHPL_EBIT_GATHER; the point is skipped, never read).
__device__ __forceinline__ int64_t aug_source(const Mv3dAug<true> &ag, int64_t i, int64_t p0, int64_t q0, int64_t nq) {
    if (!ag.remain) return q0 + (i - p0);
    const int64_t r = ag.remain[i];
    if (r < 0 || r >= nq) {
        if (ag.err) atomicOr(ag.err, SHPL_EBIT_GATHER);
        return -1;
    }
    return q0 + r;
}

// augment_voxel's cloud half for one point (minibatch_mv3d_img.py:180-185), every step in f64 and rounded to
// the cloud's type T, as numpy's in-place operators do with f64 operands: += sx / sz, *= ratio, then the
// rotation np.dot(rot, [x; z]) (dot2) rounded once. gemv: the frame has one out point.
template <typename T>
__device__ __forceinline__ void augment_point(const double *a, bool gemv, T &x, T &y, T &z) {
    const T x1 = (T)__dadd_rn((double)x, a[0]), z1 = (T)__dadd_rn((double)z, a[1]);
    const T x2 = (T)__dmul_rn((double)x1, a[2]), z2 = (T)__dmul_rn((double)z1, a[2]);
    y = (T)__dmul_rn((double)y, a[2]);
    x = (T)dot2(a + 3, (double)x2, (double)z2, gemv);
    z = (T)dot2(a + 5, (double)x2, (double)z2, gemv);
}

// A frame's out point i: the coordinates the voxel is keyed on in (x, y, z), the ORIGINAL point's in (ox, oy,
// oz) -- what the image sees -- and its row in the cloud (src). false: no such point (a bad remain entry).
template <typename T, bool AUG>
__device__ __forceinline__ bool frame_point(const Mv3dAug<AUG> &ag, const T *pts, int64_t pt_stride, int f, int64_t i,
                                            int64_t p0, int64_t p1, int64_t q0, int64_t nq, T &x, T &y, T &z, T &ox,
                                            T &oy, T &oz, int64_t &src) {
    if constexpr (AUG) {
        src = aug_source(ag, i, p0, q0, nq);
        if (src < 0) return false;
    } else {
        src = i;
    }
    const T *q = pts + src * pt_stride;
    x = ox = q[0];
    y = oy = q[1];
    z = oz = q[2];
    if constexpr (AUG) augment_point(ag.vox_aug + 8 * f, p1 - p0 == 1, x, y, z);
    return true;
}

constexpr int AUG_UNROLL = 4;            // points per thread in flight while the augmented words are formed
constexpr uint64_t NO_WORD = ~0ull;      // a rejected point's word (keys are below 2^31)

// The sort word of a frame's out point i -- (voxel key, point index in the frame) -- into w; false, and w as it
// was, for a point outside the ranges or without a source.
template <typename T, bool AUG>
__device__ __forceinline__ bool point_word(const Mv3dGeom &g, const Mv3dAug<AUG> &ag, const T *pts, int64_t pt_stride,
                                           int f, int64_t i, int64_t p0, int64_t p1, int64_t q0, int64_t nq,
                                           uint64_t &w) {
    T x, y, z, ox, oy, oz;
    int64_t src;
    if (!frame_point<T, AUG>(ag, pts, pt_stride, f, i, p0, p1, q0, nq, x, y, z, ox, oy, oz, src)) return false;
    int si, fi;
    const int64_t key = voxel_key<T>(g, x, y, z, si, fi);
    if (key >= 0) w = ((uint64_t)key << 32) | (uint32_t)(i - p0);
    return key >= 0;
}

template <typename T, bool AUG>
__global__ __launch_bounds__(TS_BLOCK) void k_mv3d_frame(Mv3dGeom g, const int64_t *pt_off, const T *pts,
                                                         int64_t pt_stride, const int64_t *img2, int64_t img2_ld,
                                                         const double *P, const double *fv_aug, uint64_t *tmp,
                                                         uint64_t *srt, int32_t *acc,
                                                         double *img_index, int64_t ld, int64_t *bv_index,
                                                         double *mval, int64_t *frame_n, int32_t *vox_count,
                                                         int64_t *frame_nvox, Mv3dAug<AUG> ag) {
    __shared__ TileSortLds lds;
    const int f = blockIdx.x;
    // [p0, p1): the frame's slots in the outputs and the workspace -- its points, or (AUG) its out points,
    // read from the cloud's rows q0 + [0, nq) through the optional gather
    int64_t p0, p1, q0 = 0, nq = 0;
    if constexpr (AUG) {
        aug_frame(ag, pt_off, f, p0, p1, q0, nq);
    } else {
        p0 = pt_off[f];
        p1 = pt_off[f + 1];
    }
    const int64_t n_keys = (int64_t)g.n_side * g.n_fwd * g.n_h;
    const int n_tiles = (int)(((n_keys - 1) >> g.log_tile) + 1);
    // per point: points accepted by its voxel, 0 = rejected (outside the ranges or over the cap)
    for (int64_t i = p0 + threadIdx.x; i < p1; i += TS_BLOCK) acc[i] = 0;
    if constexpr (AUG) {
        // The sort walks the frame's words twice (count, placement). Augmenting a point costs a dependent
        // gather and a dozen f64 operations, so the words are formed ONCE, AUG_UNROLL points per thread in
        // flight, and parked in srt -- which the sort writes only after both walks -- with NO_WORD for a
        // rejected point. (tile_sort's first block_publish orders these stores before the walks' loads.)
        for (int64_t b = p0 + threadIdx.x; b < p1; b += (int64_t)AUG_UNROLL * TS_BLOCK) {
            uint64_t w[AUG_UNROLL];
#pragma unroll
            for (int u = 0; u < AUG_UNROLL; ++u) {
                const int64_t i = b + (int64_t)u * TS_BLOCK;
                w[u] = NO_WORD;
                if (i < p1) point_word<T, AUG>(g, ag, pts, pt_stride, f, i, p0, p1, q0, nq, w[u]);
            }
#pragma unroll
            for (int u = 0; u < AUG_UNROLL; ++u) {
                const int64_t i = b + (int64_t)u * TS_BLOCK;
                if (i < p1) srt[i] = w[u];
            }
        }
    }
    const int32_t n = tile_sort(
        lds, n_tiles, tmp + p0, srt + p0,
        [&](auto &&emit) {
            for (int64_t i = p0 + threadIdx.x; i < p1; i += TS_BLOCK) {
                uint64_t w;
                if constexpr (AUG) {
                    if ((w = srt[i]) != NO_WORD) emit(w);
                } else if (point_word<T, AUG>(g, ag, pts, pt_stride, f, i, p0, p1, q0, nq, w)) {
                    emit(w);
                }
            }
        },
        [&](uint64_t w) { return (int)((w >> 32) >> g.log_tile); });
    const uint64_t *words = srt + p0;
    // run starts: accept the first `cap` points of every voxel (point order = word order)
    for (int32_t s = threadIdx.x; s < n; s += TS_BLOCK) {
        if (!run_head(words, s, 32)) continue;
        const int32_t run = run_len(words, s, n, 32);
        const int32_t a = run < g.cap ? run : g.cap;
        for (int32_t u = 0; u < a; ++u) acc[p0 + (uint32_t)words[s + u]] = a;
    }
    block_publish();
    // optional VFE buffers: number_buffer per voxel in voxel order
    if (vox_count) {
        int64_t base = 0;
        for (int32_t b0 = 0; b0 < n; b0 += TS_BLOCK) {
            const int32_t s = b0 + threadIdx.x;
            const bool first = s < n && run_head(words, s, 32);
            const int32_t run = first ? run_len(words, s, n, 32) : 0;
            int32_t tot;
            const int32_t rank = block_rank(first, lds.wsum, tot);
            if (first) vox_count[p0 + base + rank] = run < g.cap ? run : g.cap;
            base += tot;
            __syncthreads();  // block_rank's second barrier
        }
        if (threadIdx.x == 0) frame_nvox[f] = base;
    }
    // emit accepted points in point order
    int64_t kept = 0;
    for (int64_t b0 = p0; b0 < p1; b0 += TS_BLOCK) {
        const int64_t i = b0 + threadIdx.x;
        const int32_t a = i < p1 ? acc[i] : 0;
        const bool keep = a > 0;
        int32_t tot;
        const int32_t rank = block_rank(keep, lds.wsum, tot);
        T x, y, z, ox, oy, oz;
        int64_t src;
        // (an accepted point was read in the key pass; AUG bounds its remain entry again before this read)
        if (keep && frame_point<T, AUG>(ag, pts, pt_stride, f, i, p0, p1, q0, nq, x, y, z, ox, oy, oz, src)) {
            const int64_t pos = p0 + kept + rank;
            int si = 0, fi = 0;
            voxel_key<T>(g, x, y, z, si, fi);
            int64_t u, v;
            if (g.has_proj) {
                project_round(P + 12 * f, (double)ox, (double)oy, (double)oz, u, v, p1 - p0 == 1);
            } else {
                u = img2[src];
                v = img2[img2_ld + src];
            }
            if (fv_aug) {
                // augment_fv (minibatch_mv3d_img.py:205-206): (img_index * ratio + shift).astype(int)
                const double *a = fv_aug + 3 * f;
                u = (int64_t)__dadd_rn(__dmul_rn((double)u, a[0]), a[1]);
                v = (int64_t)__dadd_rn(__dmul_rn((double)v, a[0]), a[2]);
            }
            img_index[pos] = (double)u;
            img_index[ld + pos] = (double)v;
            img_index[2 * ld + pos] = 0.0;
            bv_index[2 * pos] = fi;
            bv_index[2 * pos + 1] = si;
            mval[pos] = __ddiv_rn(1.0, (double)a);  // 1.0 / accepted count (construct_voxel.py:160)
        }
        kept += tot;
        __syncthreads();
    }
    if (threadIdx.x == 0) frame_n[f] = kept;
}

// augment_voxel materialised (minibatch_mv3d_img.py:170-187): out point i of frame blockIdx.y gets the
// augmented row [x, y, z, r] (T's values widened to f64, exact) and the rounded projection of the ORIGINAL
// point. A bad remain entry leaves a NaN row (the producer's range tests reject it) and pixel (0, 0).
constexpr int AUG_BLOCK = 256;

template <typename T>
__global__ __launch_bounds__(AUG_BLOCK) void k_mv3d_augment(const int64_t *pt_off, const T *pts, int64_t pt_stride,
                                                            const double *P, Mv3dAug<true> ag, double *cloud,
                                                            int64_t *img2, int64_t ld) {
    typedef double f64x2 __attribute__((ext_vector_type(2)));
    const int f = blockIdx.y;
    int64_t p0, p1, q0, nq;
    aug_frame(ag, pt_off, f, p0, p1, q0, nq);
    for (int64_t i = p0 + (int64_t)blockIdx.x * AUG_BLOCK + threadIdx.x; i < p1; i += (int64_t)gridDim.x * AUG_BLOCK) {
        const int64_t src = aug_source(ag, i, p0, q0, nq);
        const double nan = __longlong_as_double(0x7ff8000000000000ll);
        f64x2 xy = {nan, nan}, zr = {nan, nan};
        int64_t u = 0, v = 0;
        if (src >= 0) {
            const T *q = pts + src * pt_stride;
            T x = q[0], y = q[1], z = q[2];
            const T r = q[3];
            project_round(P + 12 * f, (double)x, (double)y, (double)z, u, v, p1 - p0 == 1);
            augment_point(ag.vox_aug + 8 * f, p1 - p0 == 1, x, y, z);
            xy = f64x2{(double)x, (double)y};
            zr = f64x2{(double)z, (double)r};
        }
        f64x2 *row = reinterpret_cast<f64x2 *>(cloud + 4 * i);
        row[0] = xy;
        row[1] = zr;
        img2[i] = u;
        img2[ld + i] = v;
    }
}

// Host checks shared by the two augmented entry points: SHPL_OK and *ag filled, or the status the arguments get.
int make_aug(const int64_t *d_point_offsets, int64_t total_points, const void *d_points, int point_dtype,
             const double *d_vox_aug, const int64_t *d_remain_index, const int64_t *d_remain_offsets, int64_t total_out,
             uint32_t *d_err, Mv3dAug<true> *ag) {
    if (!d_point_offsets || !d_vox_aug || (total_points > 0 && !d_points)) return SHPL_ERR_ARG;
    if (!d_remain_index != !d_remain_offsets) return SHPL_ERR_ARG;
    if (point_dtype != SHPL_F32 && point_dtype != SHPL_F64) return SHPL_ERR_BAD_SHAPE;
    if (total_points < 0 || total_out < 0 || total_points >= ((int64_t)1 << 31) || total_out >= ((int64_t)1 << 31) ||
        (!d_remain_index && total_out != total_points))
        return SHPL_ERR_BAD_SHAPE;
    *ag = Mv3dAug<true>{d_vox_aug, d_remain_index, d_remain_index ? d_remain_offsets : d_point_offsets, total_points,
                        total_out, d_err};
    return SHPL_OK;
}

// The workspace of n_slots point slots: tmp at 0, srt at `words` and acc at 2 * words bytes (a word per slot
// twice, then a count per slot). Returns its size.
size_t mv3d_ws(int64_t n_slots, size_t &words) {
    const size_t n = (size_t)(n_slots > 0 ? n_slots : 1);
    words = align_up(n * sizeof(uint64_t), 256);
    return 2 * words + align_up(n * sizeof(int32_t), 256);
}

// What shpl_mv3d_voxels and shpl_mv3d_voxels_aug check behind their own pointers, over the call's n_slots point
// slots (its points, or the augmented call's out points), in this order -- the outputs, the source of the image
// index, number_buffer's companion, the shapes, the workspace -- and then voxel_full_size and the sort's tiling
// from the ranges. SHPL_OK and g filled, or the status the arguments get.
int check_producer(int64_t n_slots, const double *d_img_index, const int64_t *d_bv_index, const double *d_mval,
                   const int64_t *d_img_index2, const double *d_P, const int32_t *d_number_buffer,
                   const int64_t *d_frame_nvox, int64_t point_stride, int64_t ld, const double *ranges, double res,
                   double zres, int voxel_point_count, size_t ws_bytes, Mv3dGeom &g) {
    if (n_slots > 0 && (!d_img_index || !d_bv_index || !d_mval)) return SHPL_ERR_ARG;
    if (!d_img_index2 && !d_P) return SHPL_ERR_ARG;
    if (d_number_buffer && !d_frame_nvox) return SHPL_ERR_ARG;
    if (point_stride < 3 || ld < n_slots || !(res > 0) || !(zres > 0) || voxel_point_count < 1 ||
        n_slots >= ((int64_t)1 << 31))
        return SHPL_ERR_BAD_SHAPE;
    size_t words;
    if (mv3d_ws(n_slots, words) > ws_bytes) return SHPL_ERR_WORKSPACE;
    g = Mv3dGeom{};
    g.fwd_lo = ranges[0];
    g.fwd_hi = ranges[1];
    g.side_lo = ranges[2];
    g.side_hi = ranges[3];
    g.h_lo = ranges[4];
    g.h_hi = ranges[5];
    g.res = res;
    g.zres = zres;
    // construct_voxel.py:77-80: x_max = int((side_hi - side_lo) / res) etc.; sizes are max + 1
    g.n_side = (int)((g.side_hi - g.side_lo) / res) + 1;
    g.n_fwd = (int)((g.fwd_hi - g.fwd_lo) / res) + 1;
    g.n_h = (int)((g.h_hi - g.h_lo) / zres) + 1;
    g.cap = voxel_point_count;
    g.has_proj = d_img_index2 ? 0 : 1;
    const int64_t n_keys = (int64_t)g.n_side * g.n_fwd * g.n_h;
    if (n_keys >= ((int64_t)1 << 31)) return SHPL_ERR_BAD_SHAPE;
    g.log_tile = ts_log_tile(n_keys);
    return SHPL_OK;
}

// One workgroup per frame over the workspace's n_slots point slots.
template <typename T, bool AUG>
int launch_frames(const Mv3dGeom &g, int n_frames, const int64_t *d_point_offsets, const void *d_points,
                  int64_t point_stride, const int64_t *d_img_index2, int64_t img2_ld, const double *d_P,
                  const double *d_fv_aug, int64_t n_slots, double *d_img_index, int64_t ld, int64_t *d_bv_index,
                  double *d_mval, int64_t *d_frame_n, int32_t *d_number_buffer, int64_t *d_frame_nvox, void *d_ws,
                  const Mv3dAug<AUG> &ag, hipStream_t stream) {
    size_t words;
    mv3d_ws(n_slots, words);
    uint64_t *tmp = (uint64_t *)d_ws;
    uint64_t *srt = (uint64_t *)((char *)d_ws + words);
    int32_t *acc = (int32_t *)((char *)d_ws + 2 * words);
    hipLaunchKernelGGL((k_mv3d_frame<T, AUG>), dim3(n_frames), dim3(TS_BLOCK), 0, stream, g, d_point_offsets,
                       (const T *)d_points, point_stride, d_img_index2, img2_ld, d_P, d_fv_aug, tmp, srt, acc,
                       d_img_index, ld, d_bv_index, d_mval, d_frame_n, d_number_buffer, d_frame_nvox, ag);
    SHPL_LAUNCH_CHECK();
    return SHPL_OK;
}

}  // namespace
}  // namespace shpl

using namespace shpl;

extern "C" int shpl_mv3d_workspace_bytes(int64_t total_points, size_t *bytes) {
    if (!bytes || total_points < 0) return SHPL_ERR_ARG;
    size_t words;
    *bytes = mv3d_ws(total_points, words);
    return SHPL_OK;
}

extern "C" int shpl_mv3d_voxels(int n_frames, const int64_t *d_point_offsets, int64_t total_points,
                                const double *d_points, int64_t point_stride, const int64_t *d_img_index2,
                                const double *d_P, const double *d_fv_aug, const double *ranges, double res,
                                double zres, int voxel_point_count, double *d_img_index, int64_t ld, int64_t *d_bv_index,
                                double *d_mval, int64_t *d_frame_n, int32_t *d_number_buffer,
                                int64_t *d_frame_nvox, void *d_ws, size_t ws_bytes, void *stream) {
    if (n_frames < 1 || !d_point_offsets || !ranges || !d_frame_n || !d_ws) return SHPL_ERR_ARG;
    if (total_points > 0 && !d_points) return SHPL_ERR_ARG;
    Mv3dGeom g;
    const int st = check_producer(total_points, d_img_index, d_bv_index, d_mval, d_img_index2, d_P, d_number_buffer,
                                  d_frame_nvox, point_stride, ld, ranges, res, zres, voxel_point_count, ws_bytes, g);
    if (st != SHPL_OK) return st;
    return launch_frames<double, false>(g, n_frames, d_point_offsets, d_points, point_stride, d_img_index2, total_points,
                                        d_P, d_fv_aug, total_points, d_img_index, ld, d_bv_index, d_mval, d_frame_n,
                                        d_number_buffer, d_frame_nvox, d_ws, Mv3dAug<false>{}, (hipStream_t)stream);
}

extern "C" int shpl_mv3d_augment_points(int n_frames, const int64_t *d_point_offsets, int64_t total_points,
                                        const void *d_points, int point_dtype, int64_t point_stride, const double *d_P,
                                        const double *d_vox_aug, const int64_t *d_remain_index,
                                        const int64_t *d_remain_offsets, int64_t total_out, double *d_cloud,
                                        int64_t *d_img_index2, int64_t ld, uint32_t *d_err, void *stream) {
    if (n_frames < 1 || !d_P) return SHPL_ERR_ARG;
    Mv3dAug<true> ag;
    const int st = make_aug(d_point_offsets, total_points, d_points, point_dtype, d_vox_aug, d_remain_index,
                            d_remain_offsets, total_out, d_err, &ag);
    if (st != SHPL_OK) return st;
    if (total_out > 0 && (!d_cloud || !d_img_index2)) return SHPL_ERR_ARG;
    if (point_stride < 4 || ld < total_out || !aligned16(d_cloud)) return SHPL_ERR_BAD_SHAPE;
    if (total_out == 0) return SHPL_OK;
    // ~16 points per thread at most 64 workgroups a frame: a streaming pass, small beside the producer
    int64_t per = (total_out / n_frames + 16 * AUG_BLOCK - 1) / (16 * AUG_BLOCK);
    per = per < 1 ? 1 : (per > 64 ? 64 : per);
    const dim3 grid((unsigned)per, (unsigned)n_frames);
    if (point_dtype == SHPL_F32)
        hipLaunchKernelGGL((k_mv3d_augment<float>), grid, dim3(AUG_BLOCK), 0, (hipStream_t)stream, d_point_offsets,
                           (const float *)d_points, point_stride, d_P, ag, d_cloud, d_img_index2, ld);
    else
        hipLaunchKernelGGL((k_mv3d_augment<double>), grid, dim3(AUG_BLOCK), 0, (hipStream_t)stream, d_point_offsets,
                           (const double *)d_points, point_stride, d_P, ag, d_cloud, d_img_index2, ld);
    SHPL_LAUNCH_CHECK();
    return SHPL_OK;
}

extern "C" int shpl_mv3d_voxels_aug(int n_frames, const int64_t *d_point_offsets, int64_t total_points,
                                    const void *d_points, int point_dtype, int64_t point_stride,
                                    const int64_t *d_img_index2, const double *d_P, const double *d_fv_aug,
                                    const double *d_vox_aug, const int64_t *d_remain_index,
                                    const int64_t *d_remain_offsets, int64_t total_out, const double *ranges, double res,
                                    double zres, int voxel_point_count, double *d_img_index, int64_t ld,
                                    int64_t *d_bv_index, double *d_mval, int64_t *d_frame_n, int32_t *d_number_buffer,
                                    int64_t *d_frame_nvox, uint32_t *d_err, void *d_ws, size_t ws_bytes, void *stream) {
    if (n_frames < 1 || !ranges || !d_frame_n || !d_ws) return SHPL_ERR_ARG;
    Mv3dAug<true> ag;
    int st = make_aug(d_point_offsets, total_points, d_points, point_dtype, d_vox_aug, d_remain_index, d_remain_offsets,
                      total_out, d_err, &ag);
    if (st != SHPL_OK) return st;
    Mv3dGeom g;
    st = check_producer(total_out, d_img_index, d_bv_index, d_mval, d_img_index2, d_P, d_number_buffer, d_frame_nvox,
                        point_stride, ld, ranges, res, zres, voxel_point_count, ws_bytes, g);
    if (st != SHPL_OK) return st;
    const auto launch = point_dtype == SHPL_F32 ? launch_frames<float, true> : launch_frames<double, true>;
    return launch(g, n_frames, d_point_offsets, d_points, point_stride, d_img_index2, total_points, d_P, d_fv_aug,
                  total_out, d_img_index, ld, d_bv_index, d_mval, d_frame_n, d_number_buffer, d_frame_nvox, d_ws, ag,
                  (hipStream_t)stream);
}
