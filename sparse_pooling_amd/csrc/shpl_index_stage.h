// shpl_index_stage.h -- the index builder's device helpers and its fused stage (FusedStage), shared by
// shpl_index.hip (the single-level entry points) and shpl_index_levels.hip (several fusion levels in one
// pass over the points).
#pragma once

#include "shpl_compact.h"

namespace shpl {
namespace {

template <typename PT>
__device__ __forceinline__ void load_point(const void *pts, int64_t i, double &x, double &y, double &z) {
    const PT *p = reinterpret_cast<const PT *>(pts) + 3 * i;
    x = (double)p[0];
    y = (double)p[1];
    z = (double)p[2];
}

template <typename IT>
__device__ __forceinline__ int64_t load_idx(const void *a, int64_t i) {
    return (int64_t)reinterpret_cast<const IT *>(a)[i];
}

// clip3DwithinImage (transform.py:28-40): 0 <= u < W-1, 0 <= v < H-1.
__device__ __forceinline__ bool in_image(double u, double v, double w, double h) {
    return (u < w - 1.0) && (u >= 0.0) && (v >= 0.0) && (v < h - 1.0);
}

struct Geometry {
    double im_w, im_h, s_img, s_bv;
    double wq, hq, bhq, bwq;  // floor(size / stride)
    int64_t n_cells;          // int(bhq*bwq)
    int64_t n_pix;            // hq*wq
    double inv_img, inv_bv;   // 1 / stride when the stride is a power of two (x / 2^k == x * 2^-k exactly), else 0
};

// 1 / s when s is a power of two (its reciprocal exact, so x * (1 / s) is bitwise x / s for every finite x that
// stays normal -- the image and voxel indices here), else 0: the division then stays a division.
inline double pow2_reciprocal(double s) {
    int e = 0;
    return (s > 0.0 && frexp(s, &e) == 0.5 && e > -1000 && e < 1000) ? ldexp(1.0, 1 - e) : 0.0;
}

// x / s (IEEE), as a multiply when the reciprocal is exact (inv != 0)
__device__ __forceinline__ double div_stride(double x, double s, double inv) {
    return inv != 0.0 ? __dmul_rn(x, inv) : __ddiv_rn(x, s);
}

Geometry make_geometry(double im_w, double im_h, double bv_h, double bv_w, double s_img, double s_bv) {
    Geometry g = {};
    g.im_w = im_w;
    g.im_h = im_h;
    g.s_img = s_img;
    g.s_bv = s_bv;
    g.wq = floor(im_w / s_img);
    g.hq = floor(im_h / s_img);
    g.bhq = floor(bv_h / s_bv);
    g.bwq = floor(bv_w / s_bv);
    g.n_cells = (int64_t)(g.bhq * g.bwq);
    g.n_pix = (int64_t)g.hq * (int64_t)g.wq;
    g.inv_img = pow2_reciprocal(s_img);
    g.inv_bv = pow2_reciprocal(s_bv);
    return g;
}

// The padded map of a ragged batch as a Geometry: wq x hq = img_cols x img_rows strided pixels (the pitch of
// the pixel ids), n_pix their product (saturated: index_args refuses it); no image size of its own (NaN).
Geometry make_geometry_ragged(int64_t img_rows, int64_t img_cols, double bv_h, double bv_w, double s_img,
                              double s_bv) {
    Geometry g = make_geometry(NAN, NAN, bv_h, bv_w, s_img, s_bv);
    g.wq = (double)img_cols;
    g.hq = (double)img_rows;
    const bool fits = img_rows >= 1 && img_cols >= 1 && (double)img_rows * (double)img_cols < 4e18;
    g.n_pix = fits ? img_rows * img_cols : (img_rows >= 1 && img_cols >= 1 ? INT64_MAX : 0);
    return g;
}

// produce_sparse_pooling_input (sparse_pool_utils.py:22-58) on one rounded
// image index (ur, vr) and one voxel index (vx, vz).
struct Produced {
    double u, v;   // strided + clamped image index (what the reference writes back)
    int64_t r;     // flattened BEV row
    bool inside;   // r < n_cells
};

// (wq, hq): the strided image size the index is clamped to -- g's, or the frame's own (ragged batches).
__device__ __forceinline__ Produced produce(const Geometry &g, double wq, double hq, double ur, double vr,
                                            int64_t vx, int64_t vz) {
    Produced o = {};
    double u = floor(div_stride(ur, g.s_img, g.inv_img));
    double v = floor(div_stride(vr, g.s_img, g.inv_img));
    if (u >= wq) u = wq - 1.0;
    if (v >= hq) v = hq - 1.0;
    o.u = u;
    o.v = v;
    const double bx = floor(div_stride((double)vx, g.s_bv, g.inv_bv));
    const double bz = floor(div_stride((double)vz, g.s_bv, g.inv_bv));
    o.r = (int64_t)__dadd_rn(__dmul_rn(bz, g.bwq), bx);
    o.inside = o.r < g.n_cells;
    return o;
}

// ------------------------------------------------------------------ stages
// Each stage: eval() decides whether point i (of frame f) is kept; emit()
// writes kept point i at global position pos (frame starts at fstart);
// touch() runs for every point in the write pass (in-place side effects).

// Ragged batches (shpl_build_index_ragged): every frame is clipped against its own image size and clamped
// against its own strided size, read from im_sizes[f] = (W_f, H_f); the frames share one padded image feature
// map of g.hq x g.wq strided pixels (the pitch of the pixel ids, g.n_pix per frame). The uniform stage carries
// none of this (an empty base: its kernel arguments are what they were).
template <bool RAGGED>
struct FrameDims {};
template <>
struct FrameDims<true> {
    const double *im_sizes;             // [n_frames, 2] f64
    const double *sz_frame = nullptr;   // k_index1: this frame's (W, H, wq, hq), staged in LDS beside P_frame
};

struct ImageDims {
    double im_w, im_h, wq, hq;
};

// A frame's own size from the device array: a NaN or +inf size becomes NaN, which fails every comparison of
// the clip (no point kept); zero, negative and -inf sizes fail `u >= 0 && u < w - 1` by themselves.
__device__ __forceinline__ double frame_size(const double *im_sizes, int f, int k) {
    const double s = im_sizes[2 * (int64_t)f + k];
    return s < HUGE_VAL ? s : __builtin_nan("");
}

template <typename PT, typename VT, bool RAGGED_ = false>
struct FusedStage : FrameDims<RAGGED_> {
    static constexpr bool HAS_BUCKETS = true;
    static constexpr bool RAGGED = RAGGED_;
    const void *pts;
    const void *vox;
    int64_t vstride;
    const double *P;
    Geometry g = {};
    const float *mval;
    int32_t *cell, *pix;
    float *val;
    int64_t *mij, *flip;
    uint32_t *err;
    const double *P_frame = nullptr;  // k_index1: this frame's P, staged in LDS at the launch's start

    struct Payload {
        Produced pr;
    };
    struct In {
        double x, y, z;
        int64_t vx, vz;
    };

    __device__ void load(int64_t i, In &in) const {
        load_point<PT>(pts, i, in.x, in.y, in.z);
        in.vx = load_idx<VT>(vox, i * vstride);
        in.vz = load_idx<VT>(vox, i * vstride + 1);
    }
    // the image frame f is clipped and clamped against: g's, or (ragged) the frame's own
    __device__ ImageDims dims(int f) const {
        if constexpr (RAGGED) {
            if (this->sz_frame) return ImageDims{this->sz_frame[0], this->sz_frame[1], this->sz_frame[2], this->sz_frame[3]};
            return ImageDims{frame_size(this->im_sizes, f, 0), frame_size(this->im_sizes, f, 1), strided_size(f, 0),
                             strided_size(f, 1)};
        } else {
            return ImageDims{g.im_w, g.im_h, g.wq, g.hq};
        }
    }
    // floor(size / s_img) of frame f's width (k = 0) or height (1): make_geometry's division
    __device__ double strided_size(int f, int k) const {
        return floor(div_stride(frame_size(this->im_sizes, f, k), g.s_img, g.inv_img));
    }
    // k_index1 (ragged): threads t = 0, 1 stage frame f's (W, H, wq, hq) into lds[4]
    __device__ void stage_dims(int f, int t, double *lds) const {
        if constexpr (RAGGED) {
            lds[t] = frame_size(this->im_sizes, f, t);
            lds[2 + t] = strided_size(f, t);
        }
    }
    // AUX = inside the clip (the columns of the second projection)
    __device__ uint32_t eval(const Ctx &c, int f, int64_t, const In &in, Payload &pl) const {
        double u, v, Pf[12];
        if (P_frame) {  // (LDS: flat loads only on this path; the global one keeps global loads)
#pragma unroll
            for (int k = 0; k < 12; ++k) Pf[k] = P_frame[k];
        } else {
#pragma unroll
            for (int k = 0; k < 12; ++k) Pf[k] = P[12 * f + k];
        }
        project(Pf, in.x, in.y, in.z, u, v, c.n_live == 1);
        const ImageDims d = dims(f);
        if (!in_image(u, v, d.im_w, d.im_h)) return 0u;
        if (c.n_aux == 1 && c.n_live != 1) project(Pf, in.x, in.y, in.z, u, v, true);
        const double ur = (double)(int64_t)rint(u);
        const double vr = (double)(int64_t)rint(v);
        pl.pr = produce(g, d.wq, d.hq, ur, vr, in.vx, in.vz);
        return AUX | (pl.pr.inside ? KEEP_MULTI | KEEP_ONE : 0u);
    }
    // (ragged) the strided pixel lies inside the padded map: a frame larger than the map has pixels that do not
    __device__ bool in_map(int64_t vi, int64_t ui) const {
        if constexpr (RAGGED) return ui < (int64_t)g.wq && vi < (int64_t)g.hq;
        return true;
    }
    __device__ void touch(int, int64_t, const Payload &, bool) const {}
    __device__ void emit(int f, int64_t i, int64_t pos, int64_t fstart, const Payload &pl) const {
        const int64_t r = pl.pr.r;
        const int64_t vi = (int64_t)pl.pr.v, ui = (int64_t)pl.pr.u;
        const bool rok = r >= 0;
        const bool pok = vi >= 0 && ui >= 0 && in_map(vi, ui);
        if ((!rok || !pok) && err) atomicOr(err, (rok ? 0u : SHPL_EBIT_ROW) | (pok ? 0u : SHPL_EBIT_PIXEL));
        cell[pos] = rok ? (int32_t)(f * g.n_cells + r) : -1;
        pix[pos] = pok ? (int32_t)(f * g.n_pix + vi * (int64_t)g.wq + ui) : -1;
        val[pos] = mval ? mval[i] : 1.0f;
        if (mij) {
            mij[2 * pos] = r;
            mij[2 * pos + 1] = pos - fstart;
        }
        if (flip) {
            flip[3 * pos] = 0;
            flip[3 * pos + 1] = vi;
            flip[3 * pos + 2] = ui;
        }
    }
    __device__ void hole(int64_t pos) const {  // capacity slot past the frame's last entry
        cell[pos] = -1;
        pix[pos] = -1;
        val[pos] = 0.0f;
    }
    // frame-local destinations of a kept entry (buckets): the cell and pixel emit() writes, unless -1
    __device__ bool bucket_keys(const Payload &pl, int32_t &kc, int32_t &kp) const {
        const int64_t r = pl.pr.r, vi = (int64_t)pl.pr.v, ui = (int64_t)pl.pr.u;
        if (r < 0 || vi < 0 || ui < 0 || !in_map(vi, ui)) return false;
        kc = (int32_t)r;
        kp = (int32_t)(vi * (int64_t)g.wq + ui);
        return true;
    }
};

}  // namespace
}  // namespace shpl
