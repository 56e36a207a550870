// The latent stage of the models with ONE latent group and ONE learned prior -- nolboSingleObject_instOnly (reference
// src/module/nolbo.py:326-540), nolboSingleObject_category_only (:984-1204) and nolboSingleObject_modelnet_category_only (:1594-1787):
// the arithmetic and the decisions of their fit between the head output and the decoder's input (sampling, prior / posterior choice,
// kl_loss against the given prior, regulizer_loss without a class input; function.py:35-38, 40-71, 84-98) with its backward, and of
// instOnly.getEval's latent stage (:417-485), as plain C++ that compiles for the host and for the device alike.  prior_latent.hip deals
// these functions over workgroups and, through the *_host entries, runs the whole-batch loops at the end of this file on the CPU.  It
// also compiles without HIP (a plain C++ compiler), which is how the stand-alone sanitizer test builds it.
//
// The head output of one sample is [mean (L) | logVar (L)]; every other array is [B, L] (the prior table of the evaluation: [I, L]).
//
// Same bits on both sides.  The arithmetic of one latent element is latent_elem.h's, shared with mm_latent.h: float32 +, -, *, the
// correctly rounded division and square root, comparisons and bit operations, contraction OFF in every function, exp from
// detect_decode.h.  Every sum runs in ONE ascending order:
// over a latent's elements l = 0 .. L-1, over the prior table's rows, and over the batch j = 0 .. B-1 (the regulariser's pairs, forward
// and backward) -- the device walks the batch in pieces of VV_PL_PIECE rows staged in LDS and carries the running sum from piece to
// piece, so the order does not depend on the piece size.
//
// No inline assembly, no atomics, no memory besides the arguments.
#pragma once
#include "latent_elem.h"

#define VV_PL_HD VV_LE_HD

constexpr int VV_PL_MAX_L = 64;          // width of the latent
constexpr int VV_PL_MAX_I = 256;         // rows of the evaluation's prior table
constexpr int VV_PL_THREADS = 256;       // the workgroup
constexpr int VV_PL_PIECE = 64;          // rows j of the prior outputs staged per piece: one per lane of a wave
constexpr int VV_PL_ROWS = VV_PL_THREADS / 64;   // rows i per workgroup: one per wave

// ------------------------------------------------------------------------------------------------ training
struct VvPlTrain {
    const float *enc_out, *eps, *mean_p, *lv_p, *eps_p, *keep, *dz_in;
    float dist, inv_batch, reg_weight;
    float *z_in;
    unsigned short *z_in_bf16;
    float *kl, *reg;
    float *d_enc_out, *d_mean_p, *d_lv_p;
    int B, L;
};

// what element e of sample b reads
VV_PL_HD VvLeElem vv_pl_elem(const VvPlTrain &a, int b, int e) {
    const float *row = a.enc_out + (long long)b * (2 * a.L);
    const long long le = (long long)b * a.L + e;
    VvLeElem v;
    v.mean = row[e], v.raw = row[a.L + e];
    v.lv = vv_le_clip(v.raw);
    v.mt = a.mean_p[le], v.lvt = a.lv_p[le];
    v.eps = a.eps[le], v.eps_p = a.eps_p[le];
    v.from_prior = a.keep ? !(a.keep[le] == 1.0f) : false;            // tf.where(keep == 1., z, z_prior) (:1047)
    v.dz = a.dz_in ? a.dz_in[le] : 0.0f;
    return v;
}
// sum_l |m_i - m_j|_l / scale_l in index order (function.py:49-50): the scale is row i's
VV_PL_HD float vv_pl_pair_dist(const float *mi, const float *mj, const float *scale, int L) {
#pragma clang fp contract(off)
    float d = 0.0f;
    for (int l = 0; l < L; ++l) d = d + vv_le_abs(mi[l] - mj[l]) / scale[l];
    return d;
}
// element e of sample i, given the accumulated regulariser sums: d_enc_out's two entries and the prior's two
VV_PL_HD void vv_pl_bwd_store(const VvPlTrain &a, int i, int e, float am, float alv) {
    const VvLeGrads g = vv_le_elem_grads(vv_pl_elem(a, i, e), am, alv, a.reg_weight, a.inv_batch);
    float *row = a.d_enc_out + (long long)i * (2 * a.L);
    row[e] = g.mean, row[a.L + e] = g.lv;
    if (a.d_mean_p) a.d_mean_p[(long long)i * a.L + e] = g.mt;
    if (a.d_lv_p) a.d_lv_p[(long long)i * a.L + e] = g.lvt;
}

// one sample as plain loops
VV_PL_HD void vv_pl_train_fwd_sample(const VvPlTrain &a, int i) {
#pragma clang fp contract(off)
    const int L = a.L;
    float term[VV_PL_MAX_L], ei[VV_PL_MAX_L];
    for (int e = 0; e < L; ++e) {
        const VvLeElem v = vv_pl_elem(a, i, e);
        const float zi = vv_le_z_in(v);
        a.z_in[(long long)i * L + e] = zi;
        if (a.z_in_bf16) a.z_in_bf16[(long long)i * L + e] = vv_le_bf16(zi);
        term[e] = vv_le_kl_term(v);
        ei[e] = vv_le_scale(v.lvt);
    }
    a.kl[i] = vv_le_sum(term, L);
    float s = 0.0f;
    for (int j = 0; j < a.B; ++j)
        s = s + vv_le_hinge(vv_pl_pair_dist(a.mean_p + (long long)i * L, a.mean_p + (long long)j * L, ei, L) - a.dist);
    a.reg[i] = s;
}
VV_PL_HD void vv_pl_train_bwd_sample(const VvPlTrain &a, int i) {
#pragma clang fp contract(off)
    const int L = a.L;
    const float *mi = a.mean_p + (long long)i * L;
    float ei[VV_PL_MAX_L], ej[VV_PL_MAX_L], am[VV_PL_MAX_L], alv[VV_PL_MAX_L];
    for (int e = 0; e < L; ++e) ei[e] = vv_le_scale(a.lv_p[(long long)i * L + e]), am[e] = 0.0f, alv[e] = 0.0f;
    for (int j = 0; j < a.B; ++j) {
        const float *mj = a.mean_p + (long long)j * L;
        for (int e = 0; e < L; ++e) ej[e] = vv_le_scale(a.lv_p[(long long)j * L + e]);
        const float gij = vv_le_hinge_grad(vv_pl_pair_dist(mi, mj, ei, L) - a.dist);
        const float gji = vv_le_hinge_grad(vv_pl_pair_dist(mj, mi, ej, L) - a.dist);
        for (int e = 0; e < L; ++e) vv_le_pair_accumulate(am[e], alv[e], gij, gji, mi[e], mj[e], ei[e], ej[e]);
    }
    for (int e = 0; e < L; ++e) vv_pl_bwd_store(a, i, e, am[e], alv[e]);
}

// ------------------------------------------------------------------------------------------------ evaluation (nolbo.py:417-485)
struct VvPlEval {
    const float *enc_out, *eps, *mask, *fill, *prior;
    float *z, *z_corr;
    unsigned short *z_bf16, *z_corr_bf16;
    int *idx;
    int B, L, I;
};
// element e of z: sampling, then with a mask z * mask and where(z == 0, fill, z) (:429-439): an unmasked element that is +-0 is filled too
VV_PL_HD float vv_pl_eval_z(const VvPlEval &a, int b, int e) {
#pragma clang fp contract(off)
    const float *row = a.enc_out + (long long)b * (2 * a.L);
    const long long le = (long long)b * a.L + e;
    const float z = vv_le_sample(row[e], vv_le_clip(row[a.L + e]), a.eps[le]);
    if (!a.mask) return z;
    const float v = z * a.mask[le];
    return v == 0.0f ? a.fill[le] : v;
}
VV_PL_HD void vv_pl_eval_store(const VvPlEval &a, int b, int e, float z, int idx) {
    const long long le = (long long)b * a.L + e;
    const float c = a.prior[(long long)idx * a.L + e];                         // z_corrected = prior[idx], the whole row (:474)
    a.z[le] = z, a.z_corr[le] = c;
    if (a.z_bf16) a.z_bf16[le] = vv_le_bf16(z);
    if (a.z_corr_bf16) a.z_corr_bf16[le] = vv_le_bf16(c);
}
VV_PL_HD void vv_pl_eval_sample(const VvPlEval &a, int b) {
    float z[VV_PL_MAX_L];
    for (int e = 0; e < a.L; ++e) z[e] = vv_pl_eval_z(a, b, e);
    const float *m = a.mask ? a.mask + (long long)b * a.L : nullptr;
    VvLeBest best = vv_le_best_init();
    for (int c = 0; c < a.I; ++c) vv_le_best_take(best, vv_le_dist(z, m, a.prior + (long long)c * a.L, a.L), c);   // :460-462
    const int ix = vv_le_best_index(best);
    a.idx[b] = ix;
    for (int e = 0; e < a.L; ++e) vv_pl_eval_store(a, b, e, z[e], ix);
}
