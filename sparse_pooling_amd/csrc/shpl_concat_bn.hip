// shpl_concat_bn.hip -- the SHPL concat with BatchNorm on both halves, [BN(pass) || BN(pooled)], forward and
// backward, keyed by destination row over a CSR with key_range (include/shpl.h: the formulas, the summation
// order and the reference lines, sparse_pool_utils.py:69-70, :84-85, :120-124).
//
// The pooled half is zero outside the occupied rows, so it is never stored: its statistics are sums over the
// occupied rows with the count of all rows, every empty row's normalised pooled half is one per-channel
// constant, and the gradient's sum g * xhat is xhat_empty * sum g plus a correction at the occupied rows. A
// row's pooled value is the pull's f32 run sum (RunSum of shpl_common.h: walk_run's arithmetic bit for bit),
// formed again wherever it is needed.
//
// One thread layout for all three row passes (statistics / gradient sums, apply, gradient apply): a fused row
// is cols = cpass + cpool chunks (Chunk of shpl_chunk.h: 16 bytes under the pull's alignment rule, else one
// element); cc_n chunk lanes (the largest power of two <= min(cols, SHPL_BLOCK)) times SHPL_BLOCK / cc_n row
// lanes, so a thread keeps one chunk column and its per-channel coefficients in registers; rows wider than
// cc_n chunks take several passes over the columns. Channel ch of the fused row sits in chunk ch / VEC, for
// both halves.
#include <initializer_list>

#include "shpl_chunk.h"
#include "shpl_conv_bn.h"

namespace shpl {
namespace {

struct CbnArgs {  // strided feature rows as shpl_pull takes them, and the destination-keyed runs
    const void *pass;
    int64_t pass_stride, pass_off;
    const void *src;
    int64_t src_stride, src_off;
    const int32_t *key_range;  // NULL: every row empty (a map without entries)
    const int32_t *ent_src, *ent_col;
    const float *ent_val;
    int64_t n_rows, nnz_cap;
    uint32_t cpass, cpool;  // chunks of the two halves
};

constexpr int CBN_WALK = 4;  // gathered rows in flight per step of a run

// Row r's run [first, end), clamped to the capacity; false: empty.
__device__ __forceinline__ bool cbn_run(const CbnArgs &a, int64_t r, int32_t &first, int32_t &end) {
    if (!a.key_range) return false;
    const int2 kr = *reinterpret_cast<const int2 *>(a.key_range + 2 * r);
    first = kr.x < 0 ? 0 : kr.x;
    end = (int64_t)kr.y > a.nnz_cap ? (int32_t)a.nnz_cap : kr.y;
    return end > first;
}

// The pull's f32 sum of the run [first, end) over pooled chunk pc (RunSum: TF order, no FMA contraction).
template <typename T, int VEC, bool GROUP>
__device__ __forceinline__ void cbn_run_sum(const CbnArgs &a, int32_t first, int32_t end, uint32_t pc,
                                            float (&x)[VEC]) {
    typedef Chunk<T, VEC> C;
    const T *sc = reinterpret_cast<const T *>(a.src) + a.src_off + (int64_t)pc * VEC;
    RunSum<GROUP, VEC> rs;
    rs.init();
    for (int32_t i = first; i < end; i += CBN_WALK) {
        int32_t sr[CBN_WALK], kc[CBN_WALK];
        float w[CBN_WALK];
        typename C::raw_t raw[CBN_WALK];
#pragma unroll
        for (int u = 0; u < CBN_WALK; ++u) {
            const bool in = i + u < end;
            sr[u] = in ? a.ent_src[i + u] : 0;
            w[u] = in ? a.ent_val[i + u] : 0.0f;
            kc[u] = (GROUP && in) ? a.ent_col[i + u] : 0;
        }
#pragma unroll
        for (int u = 0; u < CBN_WALK; ++u)
            if (i + u < end) raw[u] = C::load(sc + (int64_t)sr[u] * a.src_stride);
#pragma unroll
        for (int u = 0; u < CBN_WALK; ++u) {
            if (i + u >= end) break;
            float v[VEC];
            C::to_f32(raw[u], v);
            rs.add(kc[u], w[u], v);
        }
    }
    rs.finish();
#pragma unroll
    for (int k = 0; k < VEC; ++k) x[k] = rs.acc[k];
}

__host__ __device__ __forceinline__ int cbn_chunk_lanes(int cols) {
    int cc_n = 1;
    while (cc_n * 2 <= cols && cc_n * 2 <= SHPL_BLOCK) cc_n *= 2;
    return cc_n;
}

// xhat's factor scale / gamma and the forward's rounded steps
__device__ __forceinline__ float cbn_xhat(float x, float m, float inv) { return __fmul_rn(__fsub_rn(x, m), inv); }

// ---------------------------------------------------------------- partial sums
// Per block of rows_per_block rows and per channel, f64: !BWD [sum x, sum x^2] (the pooled half over its
// occupied rows), BWD [sum g, sum g * xhat] (the pooled half's second sum without its xhat_empty * sum g term:
// over the occupied rows, g * (xhat - xhat_empty)). part [block][2][C]; k_bn_bwd_partial's scheme.
template <typename T, int VEC, bool GROUP, bool BWD>
__global__ __launch_bounds__(SHPL_BLOCK) void k_cbn_partial(const CbnArgs a, const T *__restrict__ g, int64_t g_stride,
                                                            const float *mean, const float *scale, const float *gamma,
                                                            int64_t rows_per_block, double *part) {
    typedef Chunk<T, VEC> C;
    __shared__ double red[2][SHPL_BLOCK * VEC];
    const int cols = (int)(a.cpass + a.cpool), c = cols * VEC;
    const int cc_n = cbn_chunk_lanes(cols), rl_n = SHPL_BLOCK / cc_n;
    const int rl = threadIdx.x / cc_n, cc = threadIdx.x % cc_n;
    const int64_t r0 = (int64_t)blockIdx.x * rows_per_block;
    const int64_t r1 = r0 + rows_per_block < a.n_rows ? r0 + rows_per_block : a.n_rows;
    const T *pass = reinterpret_cast<const T *>(a.pass) + a.pass_off;
    for (int c0 = 0; c0 < cols; c0 += cc_n) {
        const int col = c0 + cc;
        double s1[VEC], s2[VEC];
#pragma unroll
        for (int k = 0; k < VEC; ++k) s1[k] = s2[k] = 0.0;
        if (col < cols) {
            const bool pooled = (uint32_t)col >= a.cpass;
            float m[VEC], inv[VEC], xe[VEC];
#pragma unroll
            for (int k = 0; k < VEC; ++k) {
                const int ch = col * VEC + k;
                m[k] = BWD ? mean[ch] : 0.0f;
                inv[k] = BWD ? __fdiv_rn(scale[ch], gamma ? gamma[ch] : 1.0f) : 1.0f;
                xe[k] = cbn_xhat(0.0f, m[k], inv[k]);
            }
            for (int64_t r = r0 + rl; r < r1; r += rl_n) {
                float x[VEC];
                bool have = true;
                if (!pooled) {
                    C::to_f32(C::load_nt(pass + (r * a.pass_stride + (int64_t)col * VEC)), x);
                } else {
                    int32_t first, end;
                    have = cbn_run(a, r, first, end);
                    if (have) cbn_run_sum<T, VEC, GROUP>(a, first, end, (uint32_t)col - a.cpass, x);
                }
                if constexpr (!BWD) {
                    if (have) {
#pragma unroll
                        for (int k = 0; k < VEC; ++k) {
                            s1[k] += (double)x[k];
                            s2[k] += (double)x[k] * (double)x[k];
                        }
                    }
                } else {
                    float gv[VEC];
                    C::to_f32(C::load_nt(g + (r * g_stride + (int64_t)col * VEC)), gv);
#pragma unroll
                    for (int k = 0; k < VEC; ++k) {
                        s1[k] += (double)gv[k];
                        if (!pooled)
                            s2[k] += (double)gv[k] * (double)cbn_xhat(x[k], m[k], inv[k]);
                        else if (have)
                            s2[k] += (double)gv[k] * ((double)cbn_xhat(x[k], m[k], inv[k]) - (double)xe[k]);
                    }
                }
            }
        }
#pragma unroll
        for (int k = 0; k < VEC; ++k) {
            red[0][threadIdx.x * VEC + k] = s1[k];
            red[1][threadIdx.x * VEC + k] = s2[k];
        }
        __syncthreads();
        for (int e = threadIdx.x; e < cc_n * VEC; e += SHPL_BLOCK) {
            const int cg = e / VEC, k = e % VEC;
            if (c0 + cg >= cols) continue;
            double sa = 0.0, sb = 0.0;
            for (int q = 0; q < rl_n; ++q) {  // the row lanes in lane order
                sa += red[0][(q * cc_n + cg) * VEC + k];
                sb += red[1][(q * cc_n + cg) * VEC + k];
            }
            part[((int64_t)blockIdx.x * 2 + 0) * c + (c0 + cg) * VEC + k] = sa;
            part[((int64_t)blockIdx.x * 2 + 1) * c + (c0 + cg) * VEC + k] = sb;
        }
        __syncthreads();
    }
}

// One block per channel: the blocks' partials in a fixed order (strided_sum / block_sum of shpl_conv_bn.h).
// Forward: stats [2][c] for k_bn_finalize.
__global__ __launch_bounds__(SHPL_BLOCK) void k_cbn_stats(const double *part, int n_blocks, int c, double *stats) {
    __shared__ double red[SHPL_BLOCK / 64];
    const int ch = blockIdx.x;
    const double sa = block_sum<SHPL_BLOCK>(strided_sum<SHPL_BLOCK>(part + ch, n_blocks, 2 * c, threadIdx.x), red);
    const double sb = block_sum<SHPL_BLOCK>(strided_sum<SHPL_BLOCK>(part + c + ch, n_blocks, 2 * c, threadIdx.x), red);
    if (threadIdx.x == 0) {
        stats[ch] = sa;
        stats[c + ch] = sb;
    }
}

// Backward: dbeta, dgamma (the pooled half's with its xhat_empty * sum g term) and the mean terms of g_x.
__global__ __launch_bounds__(SHPL_BLOCK) void k_cbn_bwd_finalize(const double *part, int n_blocks, int c, int c_pass,
                                                                 double count, const float *mean, const float *scale,
                                                                 const float *gamma, float *dbeta, float *dgamma,
                                                                 float *mean_terms) {
    __shared__ double red[SHPL_BLOCK / 64];
    const int ch = blockIdx.x;
    const double sa = block_sum<SHPL_BLOCK>(strided_sum<SHPL_BLOCK>(part + ch, n_blocks, 2 * c, threadIdx.x), red);
    double sb = block_sum<SHPL_BLOCK>(strided_sum<SHPL_BLOCK>(part + c + ch, n_blocks, 2 * c, threadIdx.x), red);
    if (threadIdx.x == 0) {
        if (ch >= c_pass) {
            const float inv = __fdiv_rn(scale[ch], gamma ? gamma[ch] : 1.0f);
            sb += (double)cbn_xhat(0.0f, mean[ch], inv) * sa;
        }
        if (dbeta) dbeta[ch] = (float)sa;
        if (dgamma) dgamma[ch] = (float)sb;
        mean_terms[ch] = (float)(sa / count);
        mean_terms[c + ch] = (float)(sb / count);
    }
}

// ---------------------------------------------------------------- apply
// Forward apply and concat, one row-keyed launch. FROM_VAR (inference): `scale` holds the moving variance and
// the scale is formed here with k_bn_finalize's operations; block 0 leaves mean and scale in `save` (when set).
template <typename T, int VEC, bool GROUP, bool FROM_VAR>
__global__ __launch_bounds__(SHPL_BLOCK) void k_cbn_apply(const CbnArgs a, T *__restrict__ out, int64_t out_stride,
                                                          const float *mean, const float *scale, float eps,
                                                          const float *gamma, const float *beta, float *save) {
    typedef Chunk<T, VEC> C;
    const int cols = (int)(a.cpass + a.cpool), c = cols * VEC;
    const int cc_n = cbn_chunk_lanes(cols), rl_n = SHPL_BLOCK / cc_n;
    const int rl = threadIdx.x / cc_n, cc = threadIdx.x % cc_n;
    const T *pass = reinterpret_cast<const T *>(a.pass) + a.pass_off;
    const int64_t step = (int64_t)gridDim.x * rl_n;
    for (int c0 = 0; c0 < cols; c0 += cc_n) {
        const int col = c0 + cc;
        if (col >= cols) continue;
        const bool pooled = (uint32_t)col >= a.cpass;
        float m[VEC], sc[VEC], b[VEC], ye[VEC];
#pragma unroll
        for (int k = 0; k < VEC; ++k) {
            const int ch = col * VEC + k;
            m[k] = mean[ch];
            if constexpr (FROM_VAR)
                sc[k] = __fmul_rn(gamma ? gamma[ch] : 1.0f, __fdiv_rn(1.0f, __fsqrt_rn(__fadd_rn(scale[ch], eps))));
            else
                sc[k] = scale[ch];
            b[k] = beta ? beta[ch] : 0.0f;
            ye[k] = __fmul_rn(__fsub_rn(0.0f, m[k]), sc[k]);
            if (beta) ye[k] = __fadd_rn(ye[k], b[k]);
            if (FROM_VAR && save && blockIdx.x == 0 && rl == 0) {
                save[ch] = m[k];
                save[c + ch] = sc[k];
            }
        }
        const typename C::raw_t empty = C::from_f32(ye);  // an empty row's pooled chunk: one bit pattern
        for (int64_t r = (int64_t)blockIdx.x * rl_n + rl; r < a.n_rows; r += step) {
            T *o = out + (r * out_stride + (int64_t)col * VEC);
            float x[VEC];
            if (!pooled) {
                C::to_f32(C::load_nt(pass + (r * a.pass_stride + (int64_t)col * VEC)), x);
            } else {
                int32_t first, end;
                if (!cbn_run(a, r, first, end)) {
                    C::store_nt(o, empty);
                    continue;
                }
                cbn_run_sum<T, VEC, GROUP>(a, first, end, (uint32_t)col - a.cpass, x);
            }
#pragma unroll
            for (int k = 0; k < VEC; ++k) {
                x[k] = __fmul_rn(__fsub_rn(x[k], m[k]), sc[k]);
                if (beta) x[k] = __fadd_rn(x[k], b[k]);
            }
            C::store_nt(o, C::from_f32(x));
        }
    }
}

// Backward apply: g_x of the pass-through half into gpass, of the pooled half into gpool at the occupied rows
// (the only rows of gpool ever written, and the only ones the source's pull reads). gpool is f32 in both
// dtypes: the source's gradient is summed from unrounded values and rounded once, by its caller.
template <typename T, int VEC, bool GROUP, bool TRAIN>
__global__ __launch_bounds__(SHPL_BLOCK) void k_cbn_bwd_apply(const CbnArgs a, const T *__restrict__ g, int64_t g_stride,
                                                              const float *mean, const float *scale,
                                                              const float *gamma, const float *mean_terms,
                                                              T *__restrict__ gpass, int64_t gpass_stride,
                                                              float *__restrict__ gpool) {
    typedef Chunk<T, VEC> C;
    const int cols = (int)(a.cpass + a.cpool), c = cols * VEC;
    const int cc_n = cbn_chunk_lanes(cols), rl_n = SHPL_BLOCK / cc_n;
    const int rl = threadIdx.x / cc_n, cc = threadIdx.x % cc_n;
    const T *pass = reinterpret_cast<const T *>(a.pass) + a.pass_off;
    const int64_t step = (int64_t)gridDim.x * rl_n;
    const int64_t gpool_stride = (int64_t)a.cpool * VEC;
    for (int c0 = 0; c0 < cols; c0 += cc_n) {
        const int col = c0 + cc;
        if (col >= cols) continue;
        const bool pooled = (uint32_t)col >= a.cpass;
        float m[VEC], sc[VEC], inv[VEC], t0[VEC], t1[VEC];
#pragma unroll
        for (int k = 0; k < VEC; ++k) {
            const int ch = col * VEC + k;
            m[k] = mean[ch];
            sc[k] = scale[ch];
            inv[k] = __fdiv_rn(sc[k], gamma ? gamma[ch] : 1.0f);
            t0[k] = TRAIN ? mean_terms[ch] : 0.0f;
            t1[k] = TRAIN ? mean_terms[c + ch] : 0.0f;
        }
        for (int64_t r = (int64_t)blockIdx.x * rl_n + rl; r < a.n_rows; r += step) {
            float x[VEC];
            if (!pooled) {
                if constexpr (TRAIN) C::to_f32(C::load_nt(pass + (r * a.pass_stride + (int64_t)col * VEC)), x);
            } else {
                int32_t first, end;
                if (!cbn_run(a, r, first, end)) continue;
                if constexpr (TRAIN) cbn_run_sum<T, VEC, GROUP>(a, first, end, (uint32_t)col - a.cpass, x);
            }
            float gv[VEC];
            C::to_f32(C::load_nt(g + (r * g_stride + (int64_t)col * VEC)), gv);
#pragma unroll
            for (int k = 0; k < VEC; ++k) {
                if constexpr (TRAIN)
                    gv[k] = __fmul_rn(sc[k], __fsub_rn(__fsub_rn(gv[k], t0[k]), __fmul_rn(cbn_xhat(x[k], m[k], inv[k]), t1[k])));
                else
                    gv[k] = __fmul_rn(sc[k], gv[k]);
            }
            if (!pooled) {
                C::store_nt(gpass + (r * gpass_stride + (int64_t)col * VEC), C::from_f32(gv));
            } else {
                float *o = gpool + (r * gpool_stride + (int64_t)(col - (int)a.cpass) * VEC);
                if constexpr (VEC % 4 == 0) {  // whole 16-byte pieces (the chunk rule holds for gpool too)
#pragma unroll
                    for (int k = 0; k < VEC; k += 4) {
                        float piece[4] = {gv[k], gv[k + 1], gv[k + 2], gv[k + 3]};
                        Chunk<float, 4>::store_nt(o + k, Chunk<float, 4>::from_f32(piece));
                    }
                } else {
#pragma unroll
                    for (int k = 0; k < VEC; ++k) o[k] = gv[k];
                }
            }
        }
    }
}

// ---------------------------------------------------------------- host side
struct CbnPlan {
    CbnArgs a;
    int dtype;
    bool v16, group;
    int64_t c;
};

// The checks both entry points share (the order callers observe: tests/test_concat_bn_abi.py).
int cbn_plan(int direction, int dtype, const shpl_csr *csr, const void *d_src, int64_t src_stride, int64_t src_off,
             int64_t c_pool, const void *d_pass, int64_t pass_stride, int64_t pass_off, int64_t c_pass, CbnPlan *pl) {
    if (!csr || !csr->key_range) return SHPL_ERR_ARG;
    if (direction != SHPL_BY_CELL && direction != SHPL_BY_PIXEL) return SHPL_ERR_ARG;
    if (dtype != SHPL_F32 && dtype != SHPL_BF16) return SHPL_ERR_ARG;
    if (c_pool <= 0 || c_pass <= 0) return SHPL_ERR_ARG;
    if (!d_src || !d_pass) return SHPL_ERR_ARG;
    const int64_t n = csr->n_keys, cap = csr->nnz_cap;
    if (n < 0 || n >= 2147483647LL || cap < 0 || cap >= 2147483647LL || c_pass + c_pool > (1 << 16))
        return SHPL_ERR_BAD_SHAPE;
    if (cap > 0 && (!csr->ent_src || !csr->ent_val)) return SHPL_ERR_ARG;
    if (direction == SHPL_BY_PIXEL && cap > 0 && !csr->ent_col && !(csr->flags & SHPL_CSR_IDENTITY_COLS))
        return SHPL_ERR_ARG;
    const int64_t row_max = (int64_t)1 << 31;
    if (src_off < 0 || pass_off < 0 || src_stride < src_off + c_pool || pass_stride < pass_off + c_pass ||
        src_stride >= row_max || pass_stride >= row_max)
        return SHPL_ERR_BAD_SHAPE;
    const int64_t vec = dtype == SHPL_F32 ? 4 : 8;
    pl->v16 = c_pool % vec == 0 && c_pass % vec == 0 && src_stride % vec == 0 && src_off % vec == 0 &&
              pass_stride % vec == 0 && pass_off % vec == 0 && aligned16(d_src) && aligned16(d_pass);
    pl->dtype = dtype;
    pl->group = direction == SHPL_BY_PIXEL && csr->ent_col != nullptr;
    pl->c = c_pass + c_pool;
    // an empty map has no built CSR to walk (shpl_pull's rule): every row is empty
    pl->a = CbnArgs{d_pass, pass_stride, pass_off, d_src, src_stride, src_off, cap > 0 ? csr->key_range : nullptr,
                    csr->ent_src, csr->ent_col, csr->ent_val, n, cap, 0u, 0u};
    return SHPL_OK;
}

// 16-byte chunks need every other stream of the call on the rule too; then the chunk counts
void cbn_chunks(CbnPlan *pl, int64_t c_pass, int64_t c_pool, std::initializer_list<const void *> ptrs,
                std::initializer_list<int64_t> strides) {
    const int64_t vec = pl->dtype == SHPL_F32 ? 4 : 8;
    for (const void *p : ptrs) pl->v16 = pl->v16 && aligned16(p);
    for (int64_t s : strides) pl->v16 = pl->v16 && s % vec == 0;
    const int64_t v = pl->v16 ? vec : 1;
    pl->a.cpass = (uint32_t)(c_pass / v);
    pl->a.cpool = (uint32_t)(c_pool / v);
}

template <typename T_, int VEC_>
struct CbnElems {
    typedef T_ T;
    static constexpr int VEC = VEC_;
};
template <typename F>
void cbn_forms(const CbnPlan &pl, F &&fn) {
    by_bools([&](auto GROUP) {
        if (pl.dtype == SHPL_F32)
            pl.v16 ? fn(CbnElems<float, 4>(), GROUP) : fn(CbnElems<float, 1>(), GROUP);
        else
            pl.v16 ? fn(CbnElems<uint16_t, 8>(), GROUP) : fn(CbnElems<uint16_t, 1>(), GROUP);
    }, pl.group);
}

// Grid of the apply kernels: about four rows per thread.
int cbn_apply_grid(const CbnPlan &pl) {
    const int cc_n = cbn_chunk_lanes((int)(pl.a.cpass + pl.a.cpool));
    return grid_for(pl.a.n_rows, (int64_t)(SHPL_BLOCK / cc_n) * 4, 1 << 20);
}

size_t cbn_part_bytes(int64_t rows, int64_t c) { return align_up((size_t)bn_bwd_blocks(rows) * 2 * c * sizeof(double), 256); }

}  // namespace
}  // namespace shpl

using namespace shpl;

extern "C" int shpl_concat_bn_workspace_bytes(int64_t rows, int64_t c_pass, int64_t c_pool, size_t *bytes) {
    if (!bytes || rows < 0 || c_pass < 1 || c_pool < 1) return SHPL_ERR_ARG;
    const int64_t c = c_pass + c_pool;
    *bytes = cbn_part_bytes(rows, c) + align_up(2 * c * sizeof(double), 256);
    return SHPL_OK;
}

extern "C" int shpl_concat_bn(int direction, int dtype, const shpl_csr *csr, const void *d_src, int64_t src_stride,
                              int64_t src_off, int64_t c_pool, const void *d_pass, int64_t pass_stride,
                              int64_t pass_off, int64_t c_pass, void *d_out, int64_t out_stride, int training,
                              float eps, float decay, const float *d_gamma, const float *d_beta,
                              float *d_moving_mean, float *d_moving_var, float *d_batch_mean, float *d_batch_var,
                              float *d_save, void *d_ws, size_t ws_bytes, void *stream) {
    CbnPlan pl;
    int rc = cbn_plan(direction, dtype, csr, d_src, src_stride, src_off, c_pool, d_pass, pass_stride, pass_off, c_pass,
                      &pl);
    if (rc) return rc;
    if (!d_out || out_stride < c_pass + c_pool) return SHPL_ERR_ARG;
    if (out_stride >= ((int64_t)1 << 31)) return SHPL_ERR_BAD_SHAPE;
    size_t need = 0;
    shpl_concat_bn_workspace_bytes(pl.a.n_rows, c_pass, c_pool, &need);
    if (training && (!d_ws || ws_bytes < need || !d_save)) return SHPL_ERR_ARG;
    if (!training && (!d_moving_mean || !d_moving_var)) return SHPL_ERR_ARG;
    if (pl.a.n_rows == 0) return SHPL_OK;
    cbn_chunks(&pl, c_pass, c_pool, {d_out}, {out_stride});
    hipStream_t s = (hipStream_t)stream;
    const int c = (int)pl.c;
    const int grid = cbn_apply_grid(pl);
    if (training) {
        const int nb = bn_bwd_blocks(pl.a.n_rows);
        const int64_t rpb = (pl.a.n_rows + nb - 1) / nb;
        double *part = reinterpret_cast<double *>(d_ws);
        double *stats = reinterpret_cast<double *>((uint8_t *)d_ws + cbn_part_bytes(pl.a.n_rows, c));
        cbn_forms(pl, [&](auto el, auto GROUP) {
            typedef decltype(el) E;
            typedef typename E::T T;
            hipLaunchKernelGGL((k_cbn_partial<T, E::VEC, GROUP.value, false>), dim3(nb), dim3(SHPL_BLOCK), 0, s, pl.a,
                               (const T *)nullptr, (int64_t)0, (const float *)nullptr, (const float *)nullptr,
                               (const float *)nullptr, rpb, part);
        });
        SHPL_LAUNCH_CHECK();
        hipLaunchKernelGGL(k_cbn_stats, dim3((unsigned)c), dim3(SHPL_BLOCK), 0, s, part, nb, c, stats);
        hipLaunchKernelGGL(k_bn_finalize, dim3(1), dim3(SHPL_BLOCK), 0, s, stats, (double)pl.a.n_rows, c, eps, d_gamma,
                           d_save, d_save + c, d_moving_mean, d_moving_var, decay, d_batch_mean, d_batch_var);
        SHPL_LAUNCH_CHECK();
        cbn_forms(pl, [&](auto el, auto GROUP) {
            typedef decltype(el) E;
            typedef typename E::T T;
            hipLaunchKernelGGL((k_cbn_apply<T, E::VEC, GROUP.value, false>), dim3(grid), dim3(SHPL_BLOCK), 0, s, pl.a,
                               (T *)d_out, out_stride, (const float *)d_save, (const float *)(d_save + c), eps, d_gamma,
                               d_beta, (float *)nullptr);
        });
    } else {
        cbn_forms(pl, [&](auto el, auto GROUP) {
            typedef decltype(el) E;
            typedef typename E::T T;
            hipLaunchKernelGGL((k_cbn_apply<T, E::VEC, GROUP.value, true>), dim3(grid), dim3(SHPL_BLOCK), 0, s, pl.a,
                               (T *)d_out, out_stride, (const float *)d_moving_mean, (const float *)d_moving_var, eps,
                               d_gamma, d_beta, d_save);
        });
    }
    SHPL_LAUNCH_CHECK();
    return SHPL_OK;
}

extern "C" int shpl_concat_bn_backward_workspace_bytes(int64_t rows, int64_t c_pass, int64_t c_pool, size_t *bytes) {
    if (!bytes || rows < 0 || c_pass < 1 || c_pool < 1) return SHPL_ERR_ARG;
    const int64_t c = c_pass + c_pool;
    *bytes = cbn_part_bytes(rows, c) + align_up(2 * c * sizeof(float), 256);
    return SHPL_OK;
}

extern "C" int shpl_concat_bn_backward(int direction, int dtype, const shpl_csr *csr, const shpl_csr *csr_grad,
                                       const void *d_src, int64_t src_stride, int64_t src_off, int64_t c_pool,
                                       const void *d_pass, int64_t pass_stride, int64_t pass_off, int64_t c_pass,
                                       const void *d_g, int64_t g_stride, const float *d_save, const float *d_gamma,
                                       int training, void *d_gpass, int64_t gpass_stride, void *d_gpool, void *d_gsrc,
                                       int64_t gsrc_stride, float *d_dbeta, float *d_dgamma, void *d_ws,
                                       size_t ws_bytes, void *stream) {
    CbnPlan pl;
    int rc = cbn_plan(direction, dtype, csr, d_src, src_stride, src_off, c_pool, d_pass, pass_stride, pass_off, c_pass,
                      &pl);
    if (rc) return rc;
    if (!d_g || !d_gpass || !d_gpool || !d_save || (d_gsrc && !csr_grad)) return SHPL_ERR_ARG;
    if (g_stride < c_pass + c_pool || gpass_stride < c_pass) return SHPL_ERR_ARG;
    if (g_stride >= ((int64_t)1 << 31) || gpass_stride >= ((int64_t)1 << 31)) return SHPL_ERR_BAD_SHAPE;
    size_t need = 0;
    shpl_concat_bn_backward_workspace_bytes(pl.a.n_rows, c_pass, c_pool, &need);
    if (!d_ws || ws_bytes < need) return SHPL_ERR_ARG;
    hipStream_t s = (hipStream_t)stream;
    if (pl.a.n_rows > 0) {
        cbn_chunks(&pl, c_pass, c_pool, {d_g, d_gpass, d_gpool}, {g_stride, gpass_stride});
        const int c = (int)pl.c;
        const int nb = bn_bwd_blocks(pl.a.n_rows);
        const int64_t rpb = (pl.a.n_rows + nb - 1) / nb;
        double *part = reinterpret_cast<double *>(d_ws);
        float *mt = reinterpret_cast<float *>((uint8_t *)d_ws + cbn_part_bytes(pl.a.n_rows, c));
        const float *mean = d_save, *scale = d_save + c;
        const int grid = cbn_apply_grid(pl);
        cbn_forms(pl, [&](auto el, auto GROUP) {
            typedef decltype(el) E;
            typedef typename E::T T;
            hipLaunchKernelGGL((k_cbn_partial<T, E::VEC, GROUP.value, true>), dim3(nb), dim3(SHPL_BLOCK), 0, s, pl.a,
                               (const T *)d_g, g_stride, mean, scale, d_gamma, rpb, part);
            hipLaunchKernelGGL(k_cbn_bwd_finalize, dim3((unsigned)c), dim3(SHPL_BLOCK), 0, s, part, nb, c, (int)c_pass,
                               (double)pl.a.n_rows, mean, scale, d_gamma, d_dbeta, d_dgamma, mt);
            by_bools([&](auto TRAIN) {
                hipLaunchKernelGGL((k_cbn_bwd_apply<T, E::VEC, GROUP.value, TRAIN.value>), dim3(grid), dim3(SHPL_BLOCK),
                                   0, s, pl.a, (const T *)d_g, g_stride, mean, scale, d_gamma, (const float *)mt,
                                   (T *)d_gpass, gpass_stride, (float *)d_gpool);
            }, training != 0);
        });
        SHPL_LAUNCH_CHECK();
    }
    if (!d_gsrc) return SHPL_OK;
    // the source's gradient: the other direction's pull of g_pool (f32), which reads its occupied rows only
    return shpl_pull(direction == SHPL_BY_CELL ? SHPL_BY_PIXEL : SHPL_BY_CELL, SHPL_F32, csr_grad, d_gpool, c_pool, 0,
                     c_pool, nullptr, 0, 0, 0, SHPL_OUT_POOL, d_gsrc, gsrc_stride, stream);
}
