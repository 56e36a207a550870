// BatchNorm with batch statistics for the training step, float32 or bf16 activations (per-channel parameters, statistics and partial
// sums are float32): forward statistics (vv_bn_train_stats, or vv_bn_finalize_stats after a producer that left the partials itself),
// y = act(x * scale + shift) (vv_bn_act_fwd), and the backward through activation and normalisation with dgamma / dbeta
// (vv_bn_act_bwd; the bf16 reduction has ELU as a compile-time constant).  Every reduction is two steps: bn_reduce_kernel leaves
//     partial[(block * 2 + {0: sum, 1: sum of squares}) * C + c]        (backward: {sum du, sum du * xhat})
// per row block in the workspace, a finalise kernel adds the blocks in double in a fixed order.  Block counts: bn_blocks /
// bn_sweep_blocks below (test hooks VV_BN_NB / VV_BN_SWEEP cap them).  gfx950.
#include "common.h"

namespace {

// Column reductions over x[R][C] (C % 4 == 0, C <= 1024): workgroup = a slab of rows, lane = 4 channels.
// MODE 0: sum x, sum x^2.   MODE 1 (backward): du = dy * act'(u), u = x*scale + shift; sum du, sum du * xhat.
// Vector width of the BatchNorm sweeps: 16 bytes per lane and load (4 floats / 8 bf16).
template <typename T> struct BnVec { static constexpr int V = sizeof(T) == 2 ? 8 : 4; };
template <typename T>
__device__ __forceinline__ void ldv(const T *p, long iv, float (&o)[BnVec<T>::V]) {
    if constexpr (sizeof(T) == 4) {
        const f32x4 v = reinterpret_cast<const f32x4 *>(p)[iv];
#pragma unroll
        for (int e = 0; e < 4; ++e) o[e] = v[e];
    } else {
        const bf16x8 v = reinterpret_cast<const bf16x8 *>(p)[iv];
#pragma unroll
        for (int e = 0; e < 8; ++e) o[e] = (float)v[e];
    }
}
template <typename T>
__device__ __forceinline__ void stv(T *p, long iv, const float (&o)[BnVec<T>::V]) {
    if constexpr (sizeof(T) == 4) {
        reinterpret_cast<f32x4 *>(p)[iv] = f32x4{o[0], o[1], o[2], o[3]};
    } else {
        bf16x8 v;
#pragma unroll
        for (int e = 0; e < 8; ++e) v[e] = static_cast<__bf16>(o[e]);
        reinterpret_cast<bf16x8 *>(p)[iv] = v;
    }
}
template <int V>
__device__ __forceinline__ void ldp(const float *p, int c, float (&o)[V]) {      // V consecutive per-channel parameters
#pragma unroll
    for (int q = 0; q < V; q += 4) {
        const f32x4 v = *reinterpret_cast<const f32x4 *>(p + c + q);
#pragma unroll
        for (int e = 0; e < 4; ++e) o[q + e] = v[e];
    }
}
template <typename T>
__device__ __forceinline__ float bn_act_grad(float u, int act) {                  // act'(u)
    // ELU'(u) = 1 for u > 0, exp(u) otherwise = exp(min(u, 0)) for every u (exp(0) is exactly 1): no compare + select per element
    if (act == VV_ACT_ELU) return sizeof(T) == 4 ? expf(fminf(u, 0.f)) : __expf(fminf(u, 0.f));
    if (act == VV_ACT_RELU) return u > 0.f ? 1.f : 0.f;
    if (act == VV_ACT_LRELU) return u > 0.f ? 1.f : 0.3f;
    return 1.f;
}

// Per-block partial sums over a row range.  MODE 0: (sum x, sum x^2).  MODE 1: (sum du, sum du * xhat), du = dy * act'.
// A thread owns V consecutive channels; 256 / (C / V) rows run in parallel, four rows per thread in flight.
template <int MODE, typename T, int ACT = -1>     // ACT >= 0: the activation as a compile-time constant (the backward reduction is VALU-bound:
                                                  // 3.9 TB/s with the run-time switch per element against 5-6 TB/s for its sibling sweeps)
__global__ __launch_bounds__(256) void bn_reduce_kernel(const T *__restrict__ x, const T *__restrict__ dy,
                                                        const float *__restrict__ scale, const float *__restrict__ shift,
                                                        const float *__restrict__ mean, const float *__restrict__ rstd,
                                                        float *__restrict__ partial, long R, int C, int rows_per_block, int act) {
    constexpr int V = BnVec<T>::V;
    __shared__ float red[2][256 * V];
    const int cvn = C / V;                   // vector columns per row
    const int tid = threadIdx.x;
    const int rows_par = 256 / cvn > 0 ? 256 / cvn : 1;   // rows handled in parallel (C <= 256 V)
    const int cv = tid % cvn, rsub = tid / cvn;
    const long r0 = (long)blockIdx.x * rows_per_block;
    const long r1 = r0 + rows_per_block < R ? r0 + rows_per_block : R;
    float s0[V], s1[V], sc[V], sh[V], mu[V], rs[V];
#pragma unroll
    for (int e = 0; e < V; ++e) { s0[e] = 0.f; s1[e] = 0.f; sc[e] = 1.f; sh[e] = 0.f; mu[e] = 0.f; rs[e] = 1.f; }
    if (MODE == 1) {
        ldp<V>(scale, cv * V, sc);
        ldp<V>(shift, cv * V, sh);
        ldp<V>(mean, cv * V, mu);
        ldp<V>(rstd, cv * V, rs);
    }
    auto fold = [&](const float (&v)[V], const float (&g)[V]) {
#pragma unroll
        for (int e = 0; e < V; ++e) {
            if (MODE == 0) {
                s0[e] += v[e];
                s1[e] += v[e] * v[e];
            } else {
                const float d = g[e] * bn_act_grad<T>(v[e] * sc[e] + sh[e], ACT >= 0 ? ACT : act);
                s0[e] += d;
                s1[e] += d * ((v[e] - mu[e]) * rs[e]);
            }
        }
    };
    if (rsub < rows_par) {
        long r = r0 + rsub;
        // four rows per trip: eight independent loads in flight per thread (the sweep is HBM-bound)
        for (; r + 3L * rows_par < r1; r += 4L * rows_par) {
            float v[4][V], g[4][V];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                ldv<T>(x + (r + (long)k * rows_par) * C, cv, v[k]);
                if (MODE == 1) ldv<T>(dy + (r + (long)k * rows_par) * C, cv, g[k]);
            }
#pragma unroll
            for (int k = 0; k < 4; ++k) fold(v[k], g[k]);
        }
        for (; r < r1; r += rows_par) {
            float v[V], g[V];
            ldv<T>(x + r * C, cv, v);
            if (MODE == 1) ldv<T>(dy + r * C, cv, g);
            fold(v, g);
        }
    }
#pragma unroll
    for (int e = 0; e < V; ++e) { red[0][tid * V + e] = s0[e]; red[1][tid * V + e] = s1[e]; }
    __syncthreads();
    if (tid < cvn) {
        float a[V], b[V];
#pragma unroll
        for (int e = 0; e < V; ++e) { a[e] = 0.f; b[e] = 0.f; }
        for (int k = 0; k < rows_par && k * cvn + tid < 256; ++k)
#pragma unroll
            for (int e = 0; e < V; ++e) { a[e] += red[0][(k * cvn + tid) * V + e]; b[e] += red[1][(k * cvn + tid) * V + e]; }
#pragma unroll
        for (int e = 0; e < V; ++e) {
            partial[((size_t)blockIdx.x * 2 + 0) * C + tid * V + e] = a[e];
            partial[((size_t)blockIdx.x * 2 + 1) * C + tid * V + e] = b[e];
        }
    }
}

// Sum of the per-block partials of BN_FC channels in double, by 256 threads = 4 channels x 64 slices of the block list
// (a 1024-block list costs 16 trips of 4 independent loads, not 64 dependent ones); the 64 slice sums of a channel are
// added in slice order (deterministic).  Result valid in threads 0..3 (channel = c0 + tid).
constexpr int BN_FC = 4;
__device__ __forceinline__ void bn_partial_sums(const float *__restrict__ partial, int nblk, int C, int c0, double &s, double &ss) {
    __shared__ double red[2][64][BN_FC + 1];
    const int tid = threadIdx.x, cl = tid & (BN_FC - 1), sl = tid >> 2, c = c0 + cl;
    double a = 0.0, b = 0.0;
    if (c < C) {
        int k = sl;
        for (; k + 192 < nblk; k += 256) {
            float va[4], vb[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                va[u] = partial[((size_t)(k + 64 * u) * 2) * C + c];
                vb[u] = partial[((size_t)(k + 64 * u) * 2 + 1) * C + c];
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) { a += va[u]; b += vb[u]; }
        }
        for (; k < nblk; k += 64) { a += partial[((size_t)k * 2) * C + c]; b += partial[((size_t)k * 2 + 1) * C + c]; }
    }
    red[0][sl][cl] = a; red[1][sl][cl] = b;
    __syncthreads();
    s = 0.0; ss = 0.0;
    if (tid < BN_FC)
        for (int k = 0; k < 64; ++k) { s += red[0][k][tid]; ss += red[1][k][tid]; }
}

// Forward finalise: batch mean / biased variance -> scale, shift, rstd; moving statistics update (momentum).
__global__ __launch_bounds__(256) void bn_stats_finalize_kernel(const float *__restrict__ partial, int nblk, long R, int C, const float *gamma,
                                         const float *beta, float eps, float momentum, float *mean, float *var, float *rstd,
                                         float *scale, float *shift, float *moving_mean, float *moving_var) {
    double s, ss;
    bn_partial_sums(partial, nblk, C, blockIdx.x * BN_FC, s, ss);
    const int c = blockIdx.x * BN_FC + threadIdx.x;
    if (threadIdx.x >= BN_FC || c >= C) return;
    const double m = s / (double)R;
    double v = ss / (double)R - m * m;
    if (v < 0.0) v = 0.0;
    const float r = (float)(1.0 / sqrt(v + (double)eps));
    mean[c] = (float)m; var[c] = (float)v; rstd[c] = r;
    scale[c] = gamma[c] * r;
    shift[c] = beta[c] - (float)m * gamma[c] * r;
    if (moving_mean) moving_mean[c] = moving_mean[c] * momentum + (float)m * (1.f - momentum);
    if (moving_var) moving_var[c] = moving_var[c] * momentum + (float)v * (1.f - momentum);
}

// Backward finalise: dbeta = sum du, dgamma = sum du*xhat
__global__ __launch_bounds__(256) void bn_bwd_finalize_kernel(const float *__restrict__ partial, int nblk, int C, float *dgamma, float *dbeta) {
    double s, ss;
    bn_partial_sums(partial, nblk, C, blockIdx.x * BN_FC, s, ss);
    const int c = blockIdx.x * BN_FC + threadIdx.x;
    if (threadIdx.x >= BN_FC || c >= C) return;
    dbeta[c] = (float)s;
    dgamma[c] = (float)ss;
}

// y = act(x*scale + shift).  A thread owns V consecutive channels for the whole sweep and walks rows: the per-channel
// vectors are loaded once per thread (the element-wise form re-read them for every vector: 12 parameter loads next to the
// 2 payload loads of the backward kernel, which held it at 4.2 TB/s), four rows in flight per trip.
template <typename T>
__global__ __launch_bounds__(256) void bn_act_fwd_kernel(const T *__restrict__ x, const float *__restrict__ scale,
                                                         const float *__restrict__ shift, T *__restrict__ y, long R, int C, int act) {
    constexpr int V = BnVec<T>::V;
    const int cvn = C / V, rows_par = 256 / cvn > 0 ? 256 / cvn : 1;
    const int cv = threadIdx.x % cvn, rsub = threadIdx.x / cvn;
    if (rsub >= rows_par) return;
    float sc[V], sh[V];
    ldp<V>(scale, cv * V, sc);
    ldp<V>(shift, cv * V, sh);
    // a block sweeps one contiguous row range (DRAM pages stay local), rows_par rows per step
    const long rpb = ((R + gridDim.x - 1) / gridDim.x + rows_par - 1) / rows_par * rows_par;
    const long rend = (blockIdx.x + 1) * rpb < R ? (blockIdx.x + 1) * rpb : R;
    R = rend;
    const long stride = rows_par;
    long r = (long)blockIdx.x * rpb + rsub;
    for (; r + 3 * stride < R; r += 4 * stride) {
        float v[4][V];
#pragma unroll
        for (int k = 0; k < 4; ++k) ldv<T>(x + (r + k * stride) * C, cv, v[k]);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            float o[V];
#pragma unroll
            for (int e = 0; e < V; ++e) o[e] = vv_apply_act(v[k][e] * sc[e] + sh[e], act);
            stv<T>(y + (r + k * stride) * C, cv, o);
        }
    }
    for (; r < R; r += stride) {
        float v[V], o[V];
        ldv<T>(x + r * C, cv, v);
#pragma unroll
        for (int e = 0; e < V; ++e) o[e] = vv_apply_act(v[e] * sc[e] + sh[e], act);
        stv<T>(y + r * C, cv, o);
    }
}

// dx = gamma*rstd * (du - dbeta/R - xhat*dgamma/R),  du = dy*act'(x*scale+shift); same thread layout, with the per-channel
// constants folded to five: dx = sc * (du - k1 - (x - mu) * k2), k1 = dbeta/R, k2 = dgamma*rstd/R.
template <typename T>
__global__ __launch_bounds__(256) void bn_act_bwd_kernel(const T *__restrict__ x, const T *__restrict__ dy, const float *__restrict__ scale,
                                                         const float *__restrict__ shift, const float *__restrict__ mean,
                                                         const float *__restrict__ rstd, const float *__restrict__ dgamma,
                                                         const float *__restrict__ dbeta, T *__restrict__ dx, long R, int C, float invR, int act) {
    constexpr int V = BnVec<T>::V;
    const int cvn = C / V, rows_par = 256 / cvn > 0 ? 256 / cvn : 1;
    const int cv = threadIdx.x % cvn, rsub = threadIdx.x / cvn;
    if (rsub >= rows_par) return;
    float sc[V], sh[V], mu[V], k1[V], k2[V];
    {
        float rs[V], dg[V], db[V];
        ldp<V>(scale, cv * V, sc);
        ldp<V>(shift, cv * V, sh);
        ldp<V>(mean, cv * V, mu);
        ldp<V>(rstd, cv * V, rs);
        ldp<V>(dgamma, cv * V, dg);
        ldp<V>(dbeta, cv * V, db);
#pragma unroll
        for (int e = 0; e < V; ++e) { k1[e] = db[e] * invR; k2[e] = dg[e] * invR * rs[e]; }
    }
    auto one = [&](const float (&v)[V], const float (&g)[V], float (&o)[V]) {
#pragma unroll
        for (int e = 0; e < V; ++e) {
            const float d = g[e] * bn_act_grad<T>(v[e] * sc[e] + sh[e], act);
            o[e] = sc[e] * (d - k1[e] - (v[e] - mu[e]) * k2[e]);
        }
    };
    const long rpb = ((R + gridDim.x - 1) / gridDim.x + rows_par - 1) / rows_par * rows_par;   // contiguous row range per block
    const long rend = (blockIdx.x + 1) * rpb < R ? (blockIdx.x + 1) * rpb : R;
    R = rend;
    const long stride = rows_par;
    long r = (long)blockIdx.x * rpb + rsub;
    for (; r + stride < R; r += 2 * stride) {
        float v[2][V], g[2][V], o[V];
#pragma unroll
        for (int k = 0; k < 2; ++k) { ldv<T>(x + (r + k * stride) * C, cv, v[k]); ldv<T>(dy + (r + k * stride) * C, cv, g[k]); }
#pragma unroll
        for (int k = 0; k < 2; ++k) { one(v[k], g[k], o); stv<T>(dx + (r + k * stride) * C, cv, o); }
    }
    for (; r < R; r += stride) {
        float v[V], g[V], o[V];
        ldv<T>(x + r * C, cv, v);
        ldv<T>(dy + r * C, cv, g);
        one(v, g, o);
        stv<T>(dx + r * C, cv, o);
    }
}

// Row blocks of the two BatchNorm sweeps: 256 rows per block on the long layers (at most 1024 blocks), but never fewer
// blocks than keep ~16 rows per block -- a 2048-row x 512-channel layer is 128 blocks, not 8.
// A thread owns V consecutive channels (4 floats / 8 bf16) and a workgroup spans whole rows: C % V == 0, C / V <= 256.
// C / V need not divide 256: the 256 % (C / V) threads behind the last whole row own no row (`rsub < rows_par` in every kernel) --
// 192 channels are 24 bf16 vectors, 10 rows in parallel and 16 idle threads.
inline bool bn_shape_ok(long rows, int channels, int dtype) {
    const int V = dtype == VV_BF16 ? 8 : 4;
    return rows > 0 && channels > 0 && channels % V == 0 && channels / V <= 256;
}

// Grid of the two element-wise sweeps: a block covers 256 / (C / V) rows per step; two steps per block on the short
// layers, at most 4096 blocks (16 per CU) on the long ones
inline int bn_sweep_blocks(long R, int C, int V) {
    const int cvn = C / V;
    const int rows_par = 256 / cvn > 0 ? 256 / cvn : 1;
    long nb = (R + 2L * rows_par - 1) / (2L * rows_par);
    static const long cap = vv_hook_int(vv_hook("VV_BN_SWEEP"), 4096);
    return (int)(nb > cap ? cap : (nb < 1 ? 1 : nb));
}

inline int bn_blocks(long R, int C, int V = 4) {
    const int cvn = C / V;
    const int rows_par = 256 / cvn > 0 ? 256 / cvn : 1;
    long per = 8L * rows_par;                   // two trips of the 4-rows-in-flight loop
    if (per < 16) per = 16;
    if (per > 256) per = 256;
    long nb = (R + per - 1) / per;
    static const long cap = vv_hook_int(vv_hook("VV_BN_NB"), 1024);
    return (int)(nb > cap ? cap : (nb < 1 ? 1 : nb));
}

}  // namespace

VV_EXPORT size_t vv_bn_workspace_bytes(long rows, int channels) { return (size_t)bn_blocks(rows, channels) * 2 * channels * sizeof(float); }

VV_EXPORT int vv_bn_train_stats(const void *x, long rows, int channels, const float *gamma, const float *beta, float eps,
                                float momentum, float *mean, float *var, float *rstd, float *scale, float *shift,
                                float *moving_mean, float *moving_var, int dtype, void *workspace, size_t workspace_bytes, void *stream) {
    if (!x || !gamma || !beta || !mean || !var || !rstd || !scale || !shift) return VV_ERR_NULL;
    if (!vv_dtype_in<float, __bf16>(dtype)) return VV_ERR_DTYPE;
    if (!bn_shape_ok(rows, channels, dtype)) return VV_ERR_SHAPE;
    if (!workspace || workspace_bytes < vv_bn_workspace_bytes(rows, channels)) return VV_ERR_WORKSPACE;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const int nb = bn_blocks(rows, channels, dtype == VV_BF16 ? 8 : 4);     // <= the float32 count the workspace is sized for
    const int rpb = (int)((rows + nb - 1) / nb);
    float *part = reinterpret_cast<float *>(workspace);
    vv_with_dtype<float, __bf16>(dtype, [&](auto t) {
        using T = typename decltype(t)::type;
        VV_LAUNCH((bn_reduce_kernel<0, T>), dim3(nb), dim3(256), 0, st, reinterpret_cast<const T *>(x), nullptr, nullptr, nullptr, nullptr, nullptr, part,
                  rows, channels, rpb, 0);
    });
    VV_LAUNCH(bn_stats_finalize_kernel, dim3((channels + BN_FC - 1) / BN_FC), dim3(256), 0, st, part, nb, rows, channels, gamma, beta, eps,
              momentum, mean, var, rstd, scale, shift, moving_mean, moving_var);
    return vv_launch_status();
}

// The second half of vv_bn_train_stats for a producer that left the per-block column sums itself (vv_convT3d_k4s2_whole_stats_fwd):
// partial[(block * 2 + {0: sum, 1: sum of squares}) * channels + channel] over `nblocks` blocks that together cover `rows` rows.
VV_EXPORT int vv_bn_finalize_stats(const float *partial, int nblocks, long rows, int channels, const float *gamma, const float *beta, float eps,
                                   float momentum, float *mean, float *var, float *rstd, float *scale, float *shift, float *moving_mean,
                                   float *moving_var, void *stream) {
    if (!partial || !gamma || !beta || !mean || !var || !rstd || !scale || !shift) return VV_ERR_NULL;
    if (nblocks <= 0 || rows <= 0 || channels <= 0) return VV_ERR_SHAPE;
    VV_LAUNCH(bn_stats_finalize_kernel, dim3((channels + BN_FC - 1) / BN_FC), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), partial, nblocks,
              rows, channels, gamma, beta, eps, momentum, mean, var, rstd, scale, shift, moving_mean, moving_var);
    return vv_launch_status();
}

VV_EXPORT int vv_bn_act_fwd(const void *x, const float *scale, const float *shift, void *y, long rows, int channels, int act,
                            int dtype, void *stream) {
    if (!x || !scale || !shift || !y) return VV_ERR_NULL;
    if (!vv_dtype_in<float, __bf16>(dtype)) return VV_ERR_DTYPE;
    if (!bn_shape_ok(rows, channels, dtype)) return VV_ERR_SHAPE;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const int grid = bn_sweep_blocks(rows, channels, dtype == VV_BF16 ? 8 : 4);
    vv_with_dtype<float, __bf16>(dtype, [&](auto t) {
        using T = typename decltype(t)::type;
        VV_LAUNCH(bn_act_fwd_kernel<T>, dim3(grid), dim3(256), 0, st, reinterpret_cast<const T *>(x), scale, shift, reinterpret_cast<T *>(y), rows, channels, act);
    });
    return vv_launch_status();
}

VV_EXPORT int vv_bn_act_bwd(const void *x, const void *dy, const float *scale, const float *shift, const float *mean,
                            const float *rstd, float *dgamma, float *dbeta, void *dx, long rows, int channels, int act,
                            int dtype, void *workspace, size_t workspace_bytes, void *stream) {
    if (!x || !dy || !scale || !shift || !mean || !rstd || !dgamma || !dbeta || !dx) return VV_ERR_NULL;
    if (!vv_dtype_in<float, __bf16>(dtype)) return VV_ERR_DTYPE;
    if (!bn_shape_ok(rows, channels, dtype)) return VV_ERR_SHAPE;
    if (!workspace || workspace_bytes < vv_bn_workspace_bytes(rows, channels)) return VV_ERR_WORKSPACE;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const int nb = bn_blocks(rows, channels, dtype == VV_BF16 ? 8 : 4);     // <= the float32 count the workspace is sized for
    const int rpb = (int)((rows + nb - 1) / nb);
    float *part = reinterpret_cast<float *>(workspace);
    const int sweep = bn_sweep_blocks(rows, channels, dtype == VV_BF16 ? 8 : 4);
    vv_with_dtype<float, __bf16>(dtype, [&](auto t) {
        using T = typename decltype(t)::type;
        const T *xt = reinterpret_cast<const T *>(x), *dyt = reinterpret_cast<const T *>(dy);
        // the reduction with ELU as a compile-time constant exists for bf16 only; for float32 this is -1, the run-time switch itself
        constexpr int ELU = std::is_same<T, __bf16>::value ? (int)VV_ACT_ELU : -1;
        if (act == ELU) VV_LAUNCH((bn_reduce_kernel<1, T, ELU>), dim3(nb), dim3(256), 0, st, xt, dyt, scale, shift, mean, rstd, part, rows, channels, rpb, act);
        else VV_LAUNCH((bn_reduce_kernel<1, T>), dim3(nb), dim3(256), 0, st, xt, dyt, scale, shift, mean, rstd, part, rows, channels, rpb, act);
        VV_LAUNCH(bn_bwd_finalize_kernel, dim3((channels + BN_FC - 1) / BN_FC), dim3(256), 0, st, part, nb, channels, dgamma, dbeta);
        VV_LAUNCH(bn_act_bwd_kernel<T>, dim3(sweep), dim3(256), 0, st, xt, dyt, scale, shift, mean, rstd, dgamma, dbeta, reinterpret_cast<T *>(dx), rows,
                  channels, 1.0f / (float)rows, act);
    });
    return vv_launch_status();
}
