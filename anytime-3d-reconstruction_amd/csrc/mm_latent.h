// The latent stage of the multi-modal model nolboSingleObject: the arithmetic and the decisions of the reference's getEval
// (src/module/nolbo.py:183-252) and of its fit (:93-147 with function.py:35-38, 40-71, 84-98) between the image encoder's head output and
// the decoder's input, as plain C++ that compiles for the host and for the device alike (mm_latent.hip deals these functions over a
// workgroup per sample and, through the *_host entries, runs the whole-batch loops at the end of this file on the CPU).  It also
// compiles without HIP (a plain C++ compiler), which is how the stand-alone sanitizer test builds it.
//
// The head output of one sample is [mean_c (Lc) | logVar_c (Lc) | mean_i (Li) | logVar_i (Li)]; every latent-shaped array
// (z, eps, noise, dz_in) is [category (Lc) | instance (Li)].
//
// Same bits on both sides.  The arithmetic of one latent element is latent_elem.h's, shared with prior_latent.h; what is added here
// keeps its rules: float32 +, -, *, the correctly rounded division and square root, comparisons and bit operations, with floating-point
// contraction switched OFF in every function, exp from detect_decode.h.  Every sum runs in one fixed order: over a latent's elements,
// over the prototypes' rows and over the classes in index order; over the batch (the regulariser's pairs) as VV_MM_THREADS strided partial sums -- partial t takes j = t, t + 256, ... in
// ascending order -- that are then added in index order; the backward's pair sums in ascending j.
//
// No inline assembly, no atomics, no memory besides the arguments.
#pragma once
#include "latent_elem.h"

#define VV_MM_HD VV_LE_HD

constexpr int VV_MM_MAX_L = 64;          // width of one latent group
constexpr int VV_MM_MAX_C = 256;         // categories, instances per category
constexpr int VV_MM_THREADS = 256;       // the workgroup, and the number of strided partial sums over the batch

// ------------------------------------------------------------------------------------------------ evaluation (nolbo.py:183-252)
struct VvMmEval {
    const float *enc_out, *eps, *mask, *eps2, *prior_cat, *prior_inst, *cat_onehot, *inst_onehot;
    float *z, *z_corr;
    void *z_act, *z_corr_act;
    int act_dtype;
    int *idx;
    float *acc;
    int B, Lc, Li, C, I;
};

// element e of [z_category | z_inst] before the mask (:185-197)
VV_MM_HD float vv_mm_z(const float *enc_out, const float *eps, int Lc, int Li, int b, int e) {
    const float *row = enc_out + (long long)b * (2 * Lc + 2 * Li);
    const float mean = e < Lc ? row[e] : row[2 * Lc + (e - Lc)];
    const float raw = e < Lc ? row[Lc + e] : row[2 * Lc + Li + (e - Lc)];
    return vv_le_sample(mean, vv_le_clip(raw), eps[(long long)b * (Lc + Li) + e]);
}
// tf.reduce_mean(mean_category_prior, axis=0)[j] (:200)
VV_MM_HD float vv_mm_colmean(const float *prior_cat, int C, int Lc, int j) {
#pragma clang fp contract(off)
    float s = 0.0f;
    for (int c = 0; c < C; ++c) s = s + prior_cat[(long long)c * Lc + j];
    return s / (float)C;
}
// z * mask, then where(z == 0, column mean, z) (:204-208): an unmasked element that is +-0 is filled too
VV_MM_HD float vv_mm_fill(float z, float m, float colmean) {
#pragma clang fp contract(off)
    const float v = z * m;
    return v == 0.0f ? colmean : v;
}
// where(mask == 0, prior[idx] + eps2, z) (:242-243; sqrt(exp(0)) = 1 exactly)
VV_MM_HD float vv_mm_correct(float m, float prior, float eps2, float z) {
#pragma clang fp contract(off)
    return m == 0.0f ? prior + eps2 : z;
}
// first argmax of a row (tf.argmax)
VV_MM_HD int vv_mm_argmax(const float *row, int n) {
    int am = 0;
    float mv = row[0];
    for (int c = 1; c < n; ++c)
        if (row[c] > mv) mv = row[c], am = c;
    return am;
}
// the three hit flags of sample b, from its idx row
VV_MM_HD void vv_mm_hits(const VvMmEval &a, int b, int hit[3]) {
    const int *ix = a.idx + (long long)b * 4;
    const int tc = vv_mm_argmax(a.cat_onehot + (long long)b * a.C, a.C), ti = vv_mm_argmax(a.inst_onehot + (long long)b * a.I, a.I);
    hit[0] = ix[0] == tc ? 1 : 0, hit[1] = ix[1] == ti ? 1 : 0, hit[2] = ix[3] == tc ? 1 : 0;
}
VV_MM_HD float vv_mm_accuracy(int hits, int B) { return (float)hits / (float)B; }

// one sample as plain loops
VV_MM_HD void vv_mm_eval_sample(const VvMmEval &a, int b) {
    const int Lc = a.Lc, Li = a.Li, L = Lc + Li;
    float z[2 * VV_MM_MAX_L], corr[VV_MM_MAX_L];
    for (int e = 0; e < L; ++e) z[e] = vv_mm_z(a.enc_out, a.eps, Lc, Li, b, e);
    const float *m = a.mask ? a.mask + (long long)b * Lc : nullptr;
    if (m)
        for (int j = 0; j < Lc; ++j) z[j] = vv_mm_fill(z[j], m[j], vv_mm_colmean(a.prior_cat, a.C, Lc, j));
    for (int e = 0; e < L; ++e) {
        a.z[(long long)b * L + e] = z[e];
        vv_le_store_act(a.z_act, a.act_dtype, (long long)b * L + e, z[e]);
    }
    VvLeBest cat = vv_le_best_init(), inst = vv_le_best_init(), msk = vv_le_best_init(), cor = vv_le_best_init();
    for (int c = 0; c < a.C; ++c) vv_le_best_take(cat, vv_le_dist(z, nullptr, a.prior_cat + (long long)c * Lc, Lc), c);
    for (int c = 0; c < a.I; ++c) vv_le_best_take(inst, vv_le_dist(z + Lc, nullptr, a.prior_inst + ((long long)b * a.I + c) * Li, Li), c);
    int *ix = a.idx + (long long)b * 4;
    ix[0] = vv_le_best_index(cat), ix[1] = vv_le_best_index(inst), ix[2] = ix[0], ix[3] = ix[0];
    if (!m) return;
    for (int c = 0; c < a.C; ++c) vv_le_best_take(msk, vv_le_dist(z, m, a.prior_cat + (long long)c * Lc, Lc), c);
    ix[2] = vv_le_best_index(msk);
    for (int j = 0; j < Lc; ++j) corr[j] = vv_mm_correct(m[j], a.prior_cat[(long long)ix[2] * Lc + j], a.eps2[(long long)b * Lc + j], z[j]);
    for (int e = 0; e < L; ++e) {
        const float v = e < Lc ? corr[e] : z[e];
        a.z_corr[(long long)b * L + e] = v;
        vv_le_store_act(a.z_corr_act, a.act_dtype, (long long)b * L + e, v);
    }
    for (int c = 0; c < a.C; ++c) vv_le_best_take(cor, vv_le_dist(corr, nullptr, a.prior_cat + (long long)c * Lc, Lc), c);
    ix[3] = vv_le_best_index(cor);
}
VV_MM_HD void vv_mm_eval_all(const VvMmEval &a) {
    for (int b = 0; b < a.B; ++b) vv_mm_eval_sample(a, b);
    int hits[3] = {0, 0, 0};
    for (int b = 0; b < a.B; ++b) {
        int h[3];
        vv_mm_hits(a, b, h);
        for (int k = 0; k < 3; ++k) hits[k] += h[k];
    }
    for (int k = 0; k < 3; ++k) a.acc[k] = vv_mm_accuracy(hits[k], a.B);
}

// ------------------------------------------------------------------------------------------------ training (nolbo.py:93-147)
struct VvMmTrain {
    const float *enc_out, *eps, *mean_cp, *lv_cp, *mean_ip, *lv_ip, *eps_p, *noise, *cat_onehot, *dz_in;
    float inv_batch;
    float *z_in;
    void *z_in_act;
    int act_dtype;
    float *kl, *reg;
    float *d_enc_out, *d_mean_cp, *d_lv_cp, *d_mean_ip, *d_lv_ip;
    int B, Lc, Li, C;
};
// what element e of sample b reads
VV_MM_HD VvLeElem vv_mm_elem(const VvMmTrain &a, int b, int e) {
    const int Lc = a.Lc, Li = a.Li;
    const float *row = a.enc_out + (long long)b * (2 * Lc + 2 * Li);
    const long long le = (long long)b * (Lc + Li) + e;
    VvLeElem v;
    if (e < Lc) {
        v.mean = row[e], v.raw = row[Lc + e];
        v.mt = a.mean_cp[(long long)b * Lc + e], v.lvt = a.lv_cp[(long long)b * Lc + e];
    } else {
        v.mean = row[2 * Lc + (e - Lc)], v.raw = row[2 * Lc + Li + (e - Lc)];
        v.mt = a.mean_ip[(long long)b * Li + (e - Lc)], v.lvt = a.lv_ip[(long long)b * Li + (e - Lc)];
    }
    v.lv = vv_le_clip(v.raw);
    v.eps = a.eps[le], v.eps_p = a.eps_p[le];
    v.from_prior = a.noise ? !(a.noise[le] == 0.0f) : false;          // tf.where(noise == 0, z, z_prior) (:123)
    v.dz = a.dz_in ? a.dz_in[le] : 0.0f;
    return v;
}
// sum_l |m_i - m_j| / exp(0.5 lv_i) in index order (function.py:49-50): the scale is row i's
VV_MM_HD float vv_mm_pair_dist(const float *mi, const float *mj, const float *lvi, int L) {
#pragma clang fp contract(off)
    float d = 0.0f;
    for (int l = 0; l < L; ++l) d = d + vv_le_abs(mi[l] - mj[l]) / vv_le_scale(lvi[l]);
    return d;
}
// 1 where the two one-hot rows are equal, else 0 (function.py:58-66)
VV_MM_HD float vv_mm_same_class(const float *cls, int C, int i, int j) {
#pragma clang fp contract(off)
    float cd = 0.0f;
    for (int c = 0; c < C; ++c) cd = cd + vv_le_abs(cls[(long long)i * C + c] - cls[(long long)j * C + c]);
    return cd > 0.0f ? 0.0f : 1.0f;
}
VV_MM_HD float vv_mm_dist_in_z(int L) { return (float)(3 * L); }
// strided partial t of row i's regulariser sums: category (every pair) and instance (equal classes only)
VV_MM_HD void vv_mm_reg_partial(const VvMmTrain &a, int i, int t, float &pc, float &pi) {
#pragma clang fp contract(off)
    const int Lc = a.Lc, Li = a.Li;
    pc = 0.0f, pi = 0.0f;
    for (int j = t; j < a.B; j += VV_MM_THREADS) {
        const float dc = vv_mm_pair_dist(a.mean_cp + (long long)i * Lc, a.mean_cp + (long long)j * Lc, a.lv_cp + (long long)i * Lc, Lc);
        const float di = vv_mm_pair_dist(a.mean_ip + (long long)i * Li, a.mean_ip + (long long)j * Li, a.lv_ip + (long long)i * Li, Li);
        pc = pc + vv_le_hinge(dc - vv_mm_dist_in_z(Lc));
        pi = pi + vv_le_hinge(di - vv_mm_dist_in_z(Li)) * vv_mm_same_class(a.cat_onehot, a.C, i, j);
    }
}
VV_MM_HD int vv_mm_partials(int B) { return B < VV_MM_THREADS ? B : VV_MM_THREADS; }

VV_MM_HD void vv_mm_train_fwd_sample(const VvMmTrain &a, int i) {
#pragma clang fp contract(off)
    const int Lc = a.Lc, Li = a.Li, L = Lc + Li;
    float term[2 * VV_MM_MAX_L], pc[VV_MM_THREADS], pi[VV_MM_THREADS];
    for (int e = 0; e < L; ++e) {
        const VvLeElem v = vv_mm_elem(a, i, e);
        const float zi = vv_le_z_in(v);
        a.z_in[(long long)i * L + e] = zi;
        vv_le_store_act(a.z_in_act, a.act_dtype, (long long)i * L + e, zi);
        term[e] = vv_le_kl_term(v);
    }
    a.kl[i] = vv_le_sum(term, Lc) + vv_le_sum(term + Lc, Li);
    const int n = vv_mm_partials(a.B);
    for (int t = 0; t < n; ++t) vv_mm_reg_partial(a, i, t, pc[t], pi[t]);
    a.reg[i] = vv_le_sum(pc, n) + vv_le_sum(pi, n);
}

// ---- backward of total = mean_b kl + mean_b reg + shape, with dz_in = d shape / d z_in.
// Pair weights of row i against row j for one group: g_ij = d reg_i / d dist_ij, g_ji = d reg_j / d dist_ji (both with the class gate).
VV_MM_HD void vv_mm_pair_grads(const VvMmTrain &a, int grp, int i, int j, float &gij, float &gji) {
#pragma clang fp contract(off)
    const int L = grp ? a.Li : a.Lc;
    const float *m = grp ? a.mean_ip : a.mean_cp, *lv = grp ? a.lv_ip : a.lv_cp;
    const float same = grp ? vv_mm_same_class(a.cat_onehot, a.C, i, j) : 1.0f;
    const float dij = vv_mm_pair_dist(m + (long long)i * L, m + (long long)j * L, lv + (long long)i * L, L);
    const float dji = vv_mm_pair_dist(m + (long long)j * L, m + (long long)i * L, lv + (long long)j * L, L);
    gij = same == 0.0f ? 0.0f : vv_le_hinge_grad(dij - vv_mm_dist_in_z(L));
    gji = same == 0.0f ? 0.0f : vv_le_hinge_grad(dji - vv_mm_dist_in_z(L));
}
// element e of sample i, given the accumulated regulariser sums: the four outputs, stored by this stage's layout
VV_MM_HD void vv_mm_bwd_store(const VvMmTrain &a, int i, int e, float am, float alv) {
    const int Lc = a.Lc, Li = a.Li;
    const VvLeGrads g = vv_le_elem_grads(vv_mm_elem(a, i, e), am, alv, 1.0f, a.inv_batch);
    float *row = a.d_enc_out + (long long)i * (2 * Lc + 2 * Li);
    if (e < Lc) {
        row[e] = g.mean, row[Lc + e] = g.lv;
        if (a.d_mean_cp) a.d_mean_cp[(long long)i * Lc + e] = g.mt;
        if (a.d_lv_cp) a.d_lv_cp[(long long)i * Lc + e] = g.lvt;
    } else {
        row[2 * Lc + (e - Lc)] = g.mean, row[2 * Lc + Li + (e - Lc)] = g.lv;
        if (a.d_mean_ip) a.d_mean_ip[(long long)i * Li + (e - Lc)] = g.mt;
        if (a.d_lv_ip) a.d_lv_ip[(long long)i * Li + (e - Lc)] = g.lvt;
    }
}
// element e's prior mean and log-variance of sample j
VV_MM_HD void vv_mm_prior_at(const VvMmTrain &a, int j, int e, float &m, float &lv) {
    if (e < a.Lc) m = a.mean_cp[(long long)j * a.Lc + e], lv = a.lv_cp[(long long)j * a.Lc + e];
    else m = a.mean_ip[(long long)j * a.Li + (e - a.Lc)], lv = a.lv_ip[(long long)j * a.Li + (e - a.Lc)];
}
VV_MM_HD void vv_mm_train_bwd_sample(const VvMmTrain &a, int i) {
    const int Lc = a.Lc, L = Lc + a.Li;
    float g[4][VV_MM_THREADS], am[2 * VV_MM_MAX_L], alv[2 * VV_MM_MAX_L];
    for (int e = 0; e < L; ++e) am[e] = 0.0f, alv[e] = 0.0f;
    for (int j0 = 0; j0 < a.B; j0 += VV_MM_THREADS) {
        const int n = a.B - j0 < VV_MM_THREADS ? a.B - j0 : VV_MM_THREADS;
        for (int t = 0; t < n; ++t) {
            vv_mm_pair_grads(a, 0, i, j0 + t, g[0][t], g[1][t]);
            vv_mm_pair_grads(a, 1, i, j0 + t, g[2][t], g[3][t]);
        }
        for (int e = 0; e < L; ++e) {
            const int grp = e < Lc ? 0 : 1;
            float mi, lvi, mj, lvj;
            vv_mm_prior_at(a, i, e, mi, lvi);
            const float ei = vv_le_scale(lvi);
            for (int t = 0; t < n; ++t) {
                vv_mm_prior_at(a, j0 + t, e, mj, lvj);
                vv_le_pair_accumulate(am[e], alv[e], g[2 * grp][t], g[2 * grp + 1][t], mi, mj, ei, vv_le_scale(lvj));
            }
        }
    }
    for (int e = 0; e < L; ++e) vv_mm_bwd_store(a, i, e, am[e], alv[e]);
}
