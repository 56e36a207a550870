// The latent stage of the multi-modal model nolboSingleObject on the device: getEval's slice | clip | sampling | mask | fill | nearest
// prototypes | correction | accuracies (src/module/nolbo.py:183-252) and fit's sampling | prior mix | KL | regulariser with its backward
// (:93-147; function.py:35-38, 40-71, 84-98).  The arithmetic and every decision are mm_latent.h, float32, shared with the host entries.
//
// Form.  A 256-thread workgroup per sample; everything between the arguments lives in LDS.
//   evaluation  launch 1: threads 0 .. Lc+Li-1 sample z (and fill the masked category elements with the prototypes' column mean, which
//               every workgroup sums for itself: C <= 256 values per column); thread c then takes prototype c of the category table and
//               instance c of the sample's own instance table, and the workgroup's first argmins come from a shuffle reduction over
//               (distance, index) pairs -- a total order, so the result is the sequential loop's.  With a mask: the masked argmin, the
//               correction, and the corrected argmin follow in the same workgroup.  Launch 2: one workgroup counts the three kinds of
//               hits (integers) and divides by B.
//   training    forward: the elements, then thread t sums the regulariser's pairs j = t, t + 256, ...; thread 0 adds the partials in
//               index order.  Backward: in pieces of 256 samples j, thread t computes the four pair weights of (i, j0 + t); then thread
//               e accumulates element e's sums over the piece in ascending j.
// No atomics, no inline assembly: a given input gives the same bits on every run, and the bits of the host entries.  gfx950 only.
#include "latent_block.h"
#include "mm_latent.h"

namespace {

static_assert(VV_LE_F32 == VV_F32 && VV_LE_BF16 == VV_BF16, "activation dtype codes");
static_assert(VV_MM_THREADS == 64 * VV_LE_WAVES, "the workgroup of vv_le_block_argmin");

__global__ __launch_bounds__(VV_MM_THREADS) void mm_eval_kernel(const VvMmEval a) {
    __shared__ float z[2 * VV_MM_MAX_L], corr[VV_MM_MAX_L], msk[VV_MM_MAX_L];
    __shared__ VvLeBest red[VV_LE_WAVES];
    const int t = threadIdx.x, b = blockIdx.x, Lc = a.Lc, Li = a.Li, L = Lc + Li;
    const bool masked = a.mask != nullptr;
    if (t < L) {
        float v = vv_mm_z(a.enc_out, a.eps, Lc, Li, b, t);
        if (masked && t < Lc) {
            const float m = a.mask[(long long)b * Lc + t];
            msk[t] = m;
            v = vv_mm_fill(v, m, vv_mm_colmean(a.prior_cat, a.C, Lc, t));
        }
        z[t] = v;
        a.z[(long long)b * L + t] = v;
        vv_le_store_act(a.z_act, a.act_dtype, (long long)b * L + t, v);
    }
    __syncthreads();
    VvLeBest cat = vv_le_best_init(), inst = vv_le_best_init(), mk = vv_le_best_init(), cor = vv_le_best_init();
    if (t < a.C) vv_le_best_take(cat, vv_le_dist(z, nullptr, a.prior_cat + (long long)t * Lc, Lc), t);
    if (t < a.I) vv_le_best_take(inst, vv_le_dist(z + Lc, nullptr, a.prior_inst + ((long long)b * a.I + t) * Li, Li), t);
    if (masked && t < a.C) vv_le_best_take(mk, vv_le_dist(z, msk, a.prior_cat + (long long)t * Lc, Lc), t);
    const int i0 = vv_le_block_argmin(cat, red), i1 = vv_le_block_argmin(inst, red);
    int i2 = i0, i3 = i0;
    if (masked) {                                       // uniform over the workgroup
        i2 = vv_le_block_argmin(mk, red);
        if (t < L) {
            const float v = t < Lc ? vv_mm_correct(msk[t], a.prior_cat[(long long)i2 * Lc + t], a.eps2[(long long)b * Lc + t], z[t]) : z[t];
            if (t < Lc) corr[t] = v;
            a.z_corr[(long long)b * L + t] = v;
            vv_le_store_act(a.z_corr_act, a.act_dtype, (long long)b * L + t, v);
        }
        __syncthreads();
        if (t < a.C) vv_le_best_take(cor, vv_le_dist(corr, nullptr, a.prior_cat + (long long)t * Lc, Lc), t);
        i3 = vv_le_block_argmin(cor, red);
    }
    if (t == 0) {
        int *ix = a.idx + (long long)b * 4;
        ix[0] = i0, ix[1] = i1, ix[2] = i2, ix[3] = i3;
    }
}

__global__ __launch_bounds__(VV_MM_THREADS) void mm_accuracy_kernel(const VvMmEval a) {
    __shared__ int red[VV_MM_THREADS / 64][3];
    const int t = threadIdx.x;
    int hits[3] = {0, 0, 0};
    for (int b = t; b < a.B; b += VV_MM_THREADS) {
        int h[3];
        vv_mm_hits(a, b, h);
#pragma unroll
        for (int k = 0; k < 3; ++k) hits[k] += h[k];
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) hits[k] += __shfl_xor(hits[k], o, 64);
        if ((t & 63) == 0) red[t >> 6][k] = hits[k];
    }
    __syncthreads();
    if (t < 3) a.acc[t] = vv_mm_accuracy(red[0][t] + red[1][t] + red[2][t] + red[3][t], a.B);
}

__global__ __launch_bounds__(VV_MM_THREADS) void mm_train_fwd_kernel(const VvMmTrain a) {
    __shared__ float term[2 * VV_MM_MAX_L], pc[VV_MM_THREADS], pi[VV_MM_THREADS];
    const int t = threadIdx.x, i = blockIdx.x, Lc = a.Lc, L = Lc + a.Li;
    if (t < L) {
        const VvLeElem v = vv_mm_elem(a, i, t);
        const float zi = vv_le_z_in(v);
        a.z_in[(long long)i * L + t] = zi;
        vv_le_store_act(a.z_in_act, a.act_dtype, (long long)i * L + t, zi);
        term[t] = vv_le_kl_term(v);
    }
    const int n = vv_mm_partials(a.B);
    if (t < n) vv_mm_reg_partial(a, i, t, pc[t], pi[t]);
    __syncthreads();
    if (t == 0) a.kl[i] = vv_le_sum(term, Lc) + vv_le_sum(term + Lc, a.Li);
    if (t == 64) a.reg[i] = vv_le_sum(pc, n) + vv_le_sum(pi, n);
}

__global__ __launch_bounds__(VV_MM_THREADS) void mm_train_bwd_kernel(const VvMmTrain a) {
    __shared__ float g[4][VV_MM_THREADS];
    const int t = threadIdx.x, i = blockIdx.x, Lc = a.Lc, L = Lc + a.Li;
    const int grp = t < Lc ? 0 : 1;
    float am = 0.0f, alv = 0.0f, mi = 0.0f, lvi = 0.0f, ei = 1.0f;
    if (t < L) {
        vv_mm_prior_at(a, i, t, mi, lvi);
        ei = vv_le_scale(lvi);
    }
    for (int j0 = 0; j0 < a.B; j0 += VV_MM_THREADS) {
        const int n = a.B - j0 < VV_MM_THREADS ? a.B - j0 : VV_MM_THREADS;
        if (t < n) {
            vv_mm_pair_grads(a, 0, i, j0 + t, g[0][t], g[1][t]);
            vv_mm_pair_grads(a, 1, i, j0 + t, g[2][t], g[3][t]);
        }
        __syncthreads();
        if (t < L) {
            for (int k = 0; k < n; ++k) {
                float mj, lvj;
                vv_mm_prior_at(a, j0 + k, t, mj, lvj);
                vv_le_pair_accumulate(am, alv, g[2 * grp][k], g[2 * grp + 1][k], mi, mj, ei, vv_le_scale(lvj));
            }
        }
        __syncthreads();
    }
    if (t < L) vv_mm_bwd_store(a, i, t, am, alv);
}

inline bool mm_dims_ok(int B, int Lc, int Li) { return vv_le_dims_ok(B, Lc, VV_MM_MAX_L) && vv_le_dims_ok(B, Li, VV_MM_MAX_L); }
inline bool mm_count_ok(int n) { return n >= 1 && n <= VV_MM_MAX_C; }

int mm_eval_check(const VvMmEval &a) {
    const void *need[] = {a.enc_out, a.eps, a.prior_cat, a.prior_inst, a.cat_onehot, a.inst_onehot, a.z, a.idx, a.acc};
    for (const void *p : need)
        if (!p) return VV_ERR_NULL;
    if ((a.mask != nullptr) != (a.eps2 != nullptr)) return VV_ERR_NULL;        // eps2 exactly when the mask is given
    if (a.mask && !a.z_corr) return VV_ERR_NULL;
    if (!mm_dims_ok(a.B, a.Lc, a.Li) || !mm_count_ok(a.C) || !mm_count_ok(a.I)) return VV_ERR_SHAPE;
    if ((a.z_act || a.z_corr_act) && !vv_dtype_in<float, __bf16>(a.act_dtype)) return VV_ERR_DTYPE;
    const void *f32s[] = {a.enc_out, a.eps, a.mask, a.eps2, a.prior_cat, a.prior_inst, a.cat_onehot, a.inst_onehot, a.z, a.z_corr, a.idx, a.acc};
    for (const void *p : f32s)
        if (vv_le_misaligned(p, 3u)) return VV_ERR_ALIGN;
    const unsigned am = a.act_dtype == VV_BF16 ? 1u : 3u;
    if (vv_le_misaligned(a.z_act, am) || vv_le_misaligned(a.z_corr_act, am)) return VV_ERR_ALIGN;
    return VV_OK;
}

int mm_train_check(const VvMmTrain &a, bool bwd) {
    const void *need[] = {a.enc_out, a.eps, a.mean_cp, a.lv_cp, a.mean_ip, a.lv_ip, a.eps_p, a.cat_onehot};
    for (const void *p : need)
        if (!p) return VV_ERR_NULL;
    if (bwd ? (!a.dz_in || !a.d_enc_out) : (!a.z_in || !a.kl || !a.reg)) return VV_ERR_NULL;
    if (!mm_dims_ok(a.B, a.Lc, a.Li) || !mm_count_ok(a.C)) return VV_ERR_SHAPE;
    if (!bwd && a.z_in_act && !vv_dtype_in<float, __bf16>(a.act_dtype)) return VV_ERR_DTYPE;
    const void *f32s[] = {a.enc_out, a.eps, a.mean_cp, a.lv_cp, a.mean_ip, a.lv_ip, a.eps_p, a.noise, a.cat_onehot, a.dz_in, a.z_in, a.kl, a.reg,
                          a.d_enc_out, a.d_mean_cp, a.d_lv_cp, a.d_mean_ip, a.d_lv_ip};
    for (const void *p : f32s)
        if (vv_le_misaligned(p, 3u)) return VV_ERR_ALIGN;
    if (vv_le_misaligned(a.z_in_act, a.act_dtype == VV_BF16 ? 1u : 3u)) return VV_ERR_ALIGN;
    return VV_OK;
}

// One body per entry pair: the arguments, the check, and then the launch (host == false) or the host's whole-batch loop.
int mm_eval(const float *enc_out, const float *eps, const float *mask, const float *eps2, const float *prior_cat, const float *prior_inst,
            const float *cat_onehot, const float *inst_onehot, float *z, float *z_corr, void *z_act, void *z_corr_act, int act_dtype, int *idx,
            float *acc, int batch, int lc, int li, int classes, int insts, bool host, void *hip_stream) {
    VvMmEval a;
    a.enc_out = enc_out, a.eps = eps, a.mask = mask, a.eps2 = eps2, a.prior_cat = prior_cat, a.prior_inst = prior_inst;
    a.cat_onehot = cat_onehot, a.inst_onehot = inst_onehot, a.z = z, a.z_corr = z_corr, a.z_act = z_act;
    a.z_corr_act = mask ? z_corr_act : nullptr, a.act_dtype = act_dtype, a.idx = idx, a.acc = acc;
    a.B = batch, a.Lc = lc, a.Li = li, a.C = classes, a.I = insts;
    const int rc = mm_eval_check(a);
    if (rc != VV_OK) return rc;
    if (host) {
        vv_mm_eval_all(a);
        return VV_OK;
    }
    hipStream_t st = reinterpret_cast<hipStream_t>(hip_stream);
    VV_LAUNCH(mm_eval_kernel, dim3((unsigned)batch), dim3(VV_MM_THREADS), 0, st, a);
    const int rl = vv_launch_status();
    if (rl != VV_OK) return rl;
    VV_LAUNCH(mm_accuracy_kernel, dim3(1), dim3(VV_MM_THREADS), 0, st, a);
    return vv_launch_status();
}

VvMmTrain mm_train_args(const float *enc_out, const float *eps, const float *mean_cp, const float *lv_cp, const float *mean_ip,
                        const float *lv_ip, const float *eps_p, const float *noise, const float *cat_onehot, int batch, int lc, int li,
                        int classes) {
    VvMmTrain a = {};
    a.enc_out = enc_out, a.eps = eps, a.mean_cp = mean_cp, a.lv_cp = lv_cp, a.mean_ip = mean_ip, a.lv_ip = lv_ip, a.eps_p = eps_p;
    a.noise = noise, a.cat_onehot = cat_onehot, a.B = batch, a.Lc = lc, a.Li = li, a.C = classes;
    return a;
}

// checks a, then runs the forward (bwd == false) or the backward as one launch or as the host's loop over the samples
int mm_train(const VvMmTrain &a, bool bwd, bool host, void *hip_stream) {
    const int rc = mm_train_check(a, bwd);
    if (rc != VV_OK) return rc;
    if (host) {
        for (int i = 0; i < a.B; ++i) bwd ? vv_mm_train_bwd_sample(a, i) : vv_mm_train_fwd_sample(a, i);
        return VV_OK;
    }
    hipStream_t st = reinterpret_cast<hipStream_t>(hip_stream);
    if (bwd) VV_LAUNCH(mm_train_bwd_kernel, dim3((unsigned)a.B), dim3(VV_MM_THREADS), 0, st, a);
    else VV_LAUNCH(mm_train_fwd_kernel, dim3((unsigned)a.B), dim3(VV_MM_THREADS), 0, st, a);
    return vv_launch_status();
}

int mm_train_fwd(const float *enc_out, const float *eps, const float *mean_cp, const float *lv_cp, const float *mean_ip, const float *lv_ip,
                 const float *eps_p, const float *noise, const float *cat_onehot, float *z_in, void *z_in_act, int act_dtype, float *kl,
                 float *reg, int batch, int lc, int li, int classes, bool host, void *hip_stream) {
    VvMmTrain a = mm_train_args(enc_out, eps, mean_cp, lv_cp, mean_ip, lv_ip, eps_p, noise, cat_onehot, batch, lc, li, classes);
    a.z_in = z_in, a.z_in_act = z_in_act, a.act_dtype = act_dtype, a.kl = kl, a.reg = reg;
    return mm_train(a, false, host, hip_stream);
}

int mm_train_bwd(const float *enc_out, const float *eps, const float *mean_cp, const float *lv_cp, const float *mean_ip, const float *lv_ip,
                 const float *eps_p, const float *noise, const float *cat_onehot, const float *dz_in, float inv_batch, float *d_enc_out,
                 float *d_mean_cp, float *d_lv_cp, float *d_mean_ip, float *d_lv_ip, int batch, int lc, int li, int classes, bool host,
                 void *hip_stream) {
    VvMmTrain a = mm_train_args(enc_out, eps, mean_cp, lv_cp, mean_ip, lv_ip, eps_p, noise, cat_onehot, batch, lc, li, classes);
    a.dz_in = dz_in, a.inv_batch = inv_batch, a.d_enc_out = d_enc_out, a.d_mean_cp = d_mean_cp, a.d_lv_cp = d_lv_cp;
    a.d_mean_ip = d_mean_ip, a.d_lv_ip = d_lv_ip;
    return mm_train(a, true, host, hip_stream);
}

}  // namespace

VV_EXPORT int vv_mm_latent_eval(const float *enc_out, const float *eps, const float *mask, const float *eps2, const float *prior_cat,
                                const float *prior_inst, const float *cat_onehot, const float *inst_onehot, float *z, float *z_corr,
                                void *z_act, void *z_corr_act, int act_dtype, int *idx, float *acc, int batch, int lc, int li, int classes,
                                int insts, void *hip_stream) {
    return mm_eval(enc_out, eps, mask, eps2, prior_cat, prior_inst, cat_onehot, inst_onehot, z, z_corr, z_act, z_corr_act, act_dtype, idx, acc,
                   batch, lc, li, classes, insts, false, hip_stream);
}

VV_EXPORT int vv_mm_latent_eval_host(const float *enc_out, const float *eps, const float *mask, const float *eps2, const float *prior_cat,
                                     const float *prior_inst, const float *cat_onehot, const float *inst_onehot, float *z, float *z_corr,
                                     void *z_act, void *z_corr_act, int act_dtype, int *idx, float *acc, int batch, int lc, int li,
                                     int classes, int insts) {
    return mm_eval(enc_out, eps, mask, eps2, prior_cat, prior_inst, cat_onehot, inst_onehot, z, z_corr, z_act, z_corr_act, act_dtype, idx, acc,
                   batch, lc, li, classes, insts, true, nullptr);
}

VV_EXPORT int vv_mm_latent_train_fwd(const float *enc_out, const float *eps, const float *mean_cp, const float *lv_cp, const float *mean_ip,
                                     const float *lv_ip, const float *eps_p, const float *noise, const float *cat_onehot, float *z_in,
                                     void *z_in_act, int act_dtype, float *kl, float *reg, int batch, int lc, int li, int classes,
                                     void *hip_stream) {
    return mm_train_fwd(enc_out, eps, mean_cp, lv_cp, mean_ip, lv_ip, eps_p, noise, cat_onehot, z_in, z_in_act, act_dtype, kl, reg, batch, lc, li,
                        classes, false, hip_stream);
}

VV_EXPORT int vv_mm_latent_train_fwd_host(const float *enc_out, const float *eps, const float *mean_cp, const float *lv_cp,
                                          const float *mean_ip, const float *lv_ip, const float *eps_p, const float *noise,
                                          const float *cat_onehot, float *z_in, void *z_in_act, int act_dtype, float *kl, float *reg,
                                          int batch, int lc, int li, int classes) {
    return mm_train_fwd(enc_out, eps, mean_cp, lv_cp, mean_ip, lv_ip, eps_p, noise, cat_onehot, z_in, z_in_act, act_dtype, kl, reg, batch, lc, li,
                        classes, true, nullptr);
}

VV_EXPORT int vv_mm_latent_train_bwd(const float *enc_out, const float *eps, const float *mean_cp, const float *lv_cp, const float *mean_ip,
                                     const float *lv_ip, const float *eps_p, const float *noise, const float *cat_onehot,
                                     const float *dz_in, float inv_batch, float *d_enc_out, float *d_mean_cp, float *d_lv_cp,
                                     float *d_mean_ip, float *d_lv_ip, int batch, int lc, int li, int classes, void *hip_stream) {
    return mm_train_bwd(enc_out, eps, mean_cp, lv_cp, mean_ip, lv_ip, eps_p, noise, cat_onehot, dz_in, inv_batch, d_enc_out, d_mean_cp, d_lv_cp,
                        d_mean_ip, d_lv_ip, batch, lc, li, classes, false, hip_stream);
}

VV_EXPORT int vv_mm_latent_train_bwd_host(const float *enc_out, const float *eps, const float *mean_cp, const float *lv_cp,
                                          const float *mean_ip, const float *lv_ip, const float *eps_p, const float *noise,
                                          const float *cat_onehot, const float *dz_in, float inv_batch, float *d_enc_out, float *d_mean_cp,
                                          float *d_lv_cp, float *d_mean_ip, float *d_lv_ip, int batch, int lc, int li, int classes) {
    return mm_train_bwd(enc_out, eps, mean_cp, lv_cp, mean_ip, lv_ip, eps_p, noise, cat_onehot, dz_in, inv_batch, d_enc_out, d_mean_cp, d_lv_cp,
                        d_mean_ip, d_lv_ip, batch, lc, li, classes, true, nullptr);
}
