// The arithmetic of ONE latent element of the learned-prior latent stages, written once for the two-prior stage (mm_latent.h) and the
// one-prior stage (prior_latent.h): sampling, the log-variance clip and its gradient gate, the KL term of an element and the four
// gradients of an element, the pairwise regulariser's hinge and one pair's share of its backward, the (distance, index) total order
// of the nearest-prior search and the masked squared distance (reference function.py:35-38, 40-71, 84-98; nolbo.py:183-252).  Plain
// C++ that compiles for the host and for the device alike, and without HIP (a plain C++ compiler).
//
// Same bits on both sides.  Everything below is float32 +, -, *, the correctly rounded division and square root, comparisons and bit
// operations, with floating-point contraction switched OFF in every function; exp is detect_decode.h's vv_det_exp (no libm / ocml
// transcendental).  Every sum runs in index order.
//
// No inline assembly, no atomics, no memory besides the arguments.
#pragma once
#include "detect_decode.h"

#define VV_LE_HD VV_DET_HD

constexpr int VV_LE_F32 = 0, VV_LE_BF16 = 1;   // = VV_F32, VV_BF16 of include/voxvae.h

VV_LE_HD float vv_le_inf() { return vv_det_float(0x7F800000u); }
VV_LE_HD float vv_le_abs(float x) { return vv_det_float(vv_det_bits(x) & 0x7FFFFFFFu); }
// tf.clip_by_value(x, -10, 10); a NaN stays
VV_LE_HD float vv_le_clip(float x) { return x != x ? x : (x < -10.0f ? -10.0f : (x > 10.0f ? 10.0f : x)); }
// where the clip lets a gradient through: the rule of vv_reparam_kl_bwd
VV_LE_HD bool vv_le_clip_passes(float raw) { return raw >= -10.0f && raw <= 10.0f; }
VV_LE_HD float vv_le_std(float lv) { return __builtin_sqrtf(vv_det_exp(lv)); }
// the scale of a prior row's distances: exp(0.5 lv) (function.py:50)
VV_LE_HD float vv_le_scale(float lv) {
#pragma clang fp contract(off)
    return vv_det_exp(0.5f * lv);
}
// sampling(mu, logVar) with the draw injected (function.py:35-38)
VV_LE_HD float vv_le_sample(float mean, float lv, float eps) {
#pragma clang fp contract(off)
    const float s = vv_le_std(lv);
    const float t = s * eps;
    return mean + t;
}
// float32 -> bfloat16, round to nearest even; a NaN keeps its sign and becomes quiet
VV_LE_HD unsigned short vv_le_bf16(float x) {
    const unsigned u = vv_det_bits(x);
    if (x != x) return (unsigned short)((u >> 16) | 0x40u);
    return (unsigned short)((u + 0x7FFFu + ((u >> 16) & 1u)) >> 16);
}
VV_LE_HD void vv_le_store_act(void *p, int dtype, long long i, float v) {
    if (!p) return;
    if (dtype == VV_LE_BF16) static_cast<unsigned short *>(p)[i] = vv_le_bf16(v);
    else static_cast<float *>(p)[i] = v;
}

// ------------------------------------------------------------------------------------------------ the nearest prior row
// sum_j [mask_j *] (z_j - p_j)^2 in index order (nolbo.py:218, :239, :460-462)
VV_LE_HD float vv_le_dist(const float *z, const float *mask, const float *p, int L) {
#pragma clang fp contract(off)
    float d = 0.0f;
    for (int j = 0; j < L; ++j) {
        const float t = z[j] - p[j];
        const float q = t * t;
        d = d + (mask ? mask[j] * q : q);
    }
    return d;
}
// first argmin among the distances below +inf; none -> 0 (the contract of vv_nearest_category).  (d, c) pairs are totally ordered, so
// the running minimum does not depend on the order in which candidates or partial results are merged.
struct VvLeBest {
    float d;
    int c;
};
VV_LE_HD VvLeBest vv_le_best_init() { return VvLeBest{vv_le_inf(), 0x7FFFFFFF}; }
VV_LE_HD void vv_le_best_take(VvLeBest &s, float d, int c) {
    if (!(d < vv_le_inf())) return;
    if (d < s.d || (d == s.d && c < s.c)) s.d = d, s.c = c;
}
VV_LE_HD int vv_le_best_index(const VvLeBest &s) { return s.d < vv_le_inf() ? s.c : 0; }

// ------------------------------------------------------------------------------------------------ one element of the training stage
// what one element reads: the posterior's mean and raw / clipped log-variance with its draw, the prior's with its draw, which of the two
// samples goes on to the decoder, and the gradient arriving at it
struct VvLeElem {
    float mean, raw, lv, eps, mt, lvt, eps_p, dz;
    bool from_prior;
};
VV_LE_HD float vv_le_z_in(const VvLeElem &v) { return v.from_prior ? vv_le_sample(v.mt, v.lvt, v.eps_p) : vv_le_sample(v.mean, v.lv, v.eps); }
// one element of kl_loss's sum (function.py:96)
VV_LE_HD float vv_le_kl_term(const VvLeElem &v) {
#pragma clang fp contract(off)
    const float a = 0.5f * (v.lvt - v.lv);
    const float d = v.mean - v.mt;
    const float num = vv_det_exp(v.lv) + d * d;
    const float den = 2.0f * vv_det_exp(v.lvt);
    return (a + num / den) - 0.5f;
}
// where(x > 0, 0, x^2) (function.py:53-54) and its derivative
VV_LE_HD float vv_le_hinge(float x) {
#pragma clang fp contract(off)
    return x > 0.0f ? 0.0f : x * x;
}
VV_LE_HD float vv_le_hinge_grad(float x) {
#pragma clang fp contract(off)
    return x > 0.0f ? 0.0f : 2.0f * x;
}
VV_LE_HD float vv_le_sum(const float *v, int n) {
#pragma clang fp contract(off)
    float s = 0.0f;
    for (int k = 0; k < n; ++k) s = s + v[k];
    return s;
}
// pair (i, j)'s share of d reg / d mean_i[l] and d reg / d lv_i[l], given the pair weights g_ij = d reg_i / d dist_ij and g_ji, the two
// means and the two scales exp(0.5 lv); the derivative of |x| at 0 is 0
VV_LE_HD void vv_le_pair_accumulate(float &am, float &alv, float gij, float gji, float mi, float mj, float ei, float ej) {
#pragma clang fp contract(off)
    const float diff = mi - mj;
    if (diff == 0.0f) return;                       // sign 0: nothing reaches the means, and |diff| = 0 nothing the scale
    const float sgn = diff > 0.0f ? 1.0f : (diff < 0.0f ? -1.0f : diff);      // a NaN stays
    am = am + (gij * sgn) / ei;
    am = am + (gji * sgn) / ej;
    alv = alv + (gij * -0.5f) * (vv_le_abs(diff) / ei);
}
// the four gradients of one element of total = inv_batch sum_b (kl + reg_weight reg) + shape, given the element's accumulated
// regulariser sums am, alv and dz = d shape / d z_in: those of the posterior's mean and raw log-variance and of the prior's two
struct VvLeGrads {
    float mean, lv, mt, lvt;
};
VV_LE_HD VvLeGrads vv_le_elem_grads(const VvLeElem &v, float am, float alv, float reg_weight, float inv_batch) {
#pragma clang fp contract(off)
    const float ex = vv_det_exp(v.lv), et = vv_det_exp(v.lvt), d = v.mean - v.mt;
    const float kl_mean = d / et;                                              // d kl / d mean; the prior mean gets the negative
    const float kl_lv = ex / (2.0f * et) - 0.5f;
    const float kl_lvt = 0.5f - (ex + d * d) / (2.0f * et);
    VvLeGrads g;
    g.mean = kl_mean * inv_batch, g.lv = kl_lv * inv_batch;
    g.mt = (reg_weight * am - kl_mean) * inv_batch, g.lvt = (kl_lvt + reg_weight * alv) * inv_batch;
    if (v.from_prior) {
        g.mt = g.mt + v.dz;
        g.lvt = g.lvt + v.dz * ((0.5f * vv_le_std(v.lvt)) * v.eps_p);
    } else {
        g.mean = g.mean + v.dz;
        g.lv = g.lv + v.dz * ((0.5f * vv_le_std(v.lv)) * v.eps);
    }
    if (!vv_le_clip_passes(v.raw)) g.lv = 0.0f;
    return g;
}
