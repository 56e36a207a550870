// The detector head's output -> the selected detections: the arithmetic and the decisions of the reference's nolbo_test.getPred
// (src/module/nolbo_test.py:81-153, :214-255) and function.nonMaximumSuppresion (src/module/function.py:117-150) for ONE frame, as plain
// C++ that compiles for the host and for the device alike (detect_decode.hip runs it in a kernel and, through vv_detect_decode_host, in
// loops on the CPU).  It also compiles without HIP (a plain C++ compiler), which is how the stand-alone sanitizer test builds it.
//
// Same bits on both sides.  Everything below is float32 +, -, *, an explicit fmaf, the correctly rounded division, comparisons and bit
// operations; floating-point contraction is switched OFF in every function, so that the host build (no FMA on a plain x86-64 target)
// and the device build round every product and sum alike.  exp, sigmoid and tanh are written here too (range reduction, a polynomial
// in fmaf, scaling through the exponent bits, clamped so that no subnormal intermediate arises): no libm / ocml transcendental is
// called.  The objectness test, the ties and the IoU test then decide alike on both sides for every input.
//
// No inline assembly, no atomics, no memory besides the arguments.
#pragma once
#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define VV_DET_HD __host__ __device__ inline
#else
#define VV_DET_HD inline
#endif

constexpr int VV_DET_MAX_P = 16;          // predictors per cell
constexpr int VV_DET_MAX_Z = 64;          // latent width
constexpr int VV_DET_MAX_SLOTS = 4096;    // candidate slots per frame: R * C * (top_1 ? 1 : P)
constexpr int VV_DET_NHWC = 0;            // head[b][r][c][channel]
constexpr int VV_DET_NCHW = 1;            // head[b][channel][r][c]

// channel offsets inside one predictor's W = 17 + 2 Z channels
constexpr int VV_DET_OBJ = 0, VV_DET_B2 = 1, VV_DET_B3 = 5, VV_DET_MEAN = 8;
VV_DET_HD int vv_det_width(int z) { return 17 + 2 * z; }
VV_DET_HD int vv_det_logvar(int z) { return 8 + z; }
VV_DET_HD int vv_det_sin(int z) { return 8 + 2 * z; }
VV_DET_HD int vv_det_cos(int z) { return 11 + 2 * z; }
VV_DET_HD int vv_det_rad(int z) { return 14 + 2 * z; }

VV_DET_HD unsigned vv_det_bits(float x) { return __builtin_bit_cast(unsigned, x); }
VV_DET_HD float vv_det_float(unsigned u) { return __builtin_bit_cast(float, u); }

// One frame of the head output: element (cell, channel) at p[cell * cell_stride + channel * channel_stride].
struct VvDetFrame {
    const float *p;
    long long cell_stride, channel_stride;
};
VV_DET_HD VvDetFrame vv_det_frame(const float *head, int layout, int b, int cells, int channels) {
    VvDetFrame f;
    f.p = head + (long long)b * cells * channels;
    f.cell_stride = layout == VV_DET_NCHW ? 1 : channels;
    f.channel_stride = layout == VV_DET_NCHW ? cells : 1;
    return f;
}
VV_DET_HD float vv_det_at(const VvDetFrame &f, int cell, int channel) { return f.p[cell * f.cell_stride + channel * f.channel_stride]; }

// e^x.  NaN -> NaN; x > 88.72283 (the largest float whose exponential is finite) -> +inf, as numpy's float32 exp; x < -87.3 -> 0 (the
// results below 1.3e-38 that numpy returns as subnormals are flushed: no subnormal arises here).  Otherwise k = round(x / ln 2) by the
// 1.5 * 2^23 trick, r = x - k ln 2 in two fmaf steps (|r| <= 0.3466), e^r by a degree-7 polynomial, the scale 2^k applied in two
// normal factors.
VV_DET_HD float vv_det_exp(float x) {
#pragma clang fp contract(off)
    if (x != x) return x;
    if (x > 88.72283f) return vv_det_float(0x7F800000u);
    if (x < -87.3f) return 0.0f;
    const float magic = 12582912.0f;
    const float kf = __builtin_fmaf(x, 1.44269504088896341f, magic) - magic;
    float r = __builtin_fmaf(kf, -0.693145751953125f, x);
    r = __builtin_fmaf(kf, -1.42860677e-06f, r);
    float p = 1.9875691500e-4f;
    p = __builtin_fmaf(p, r, 1.3981999507e-3f);
    p = __builtin_fmaf(p, r, 8.3334519073e-3f);
    p = __builtin_fmaf(p, r, 4.1665795894e-2f);
    p = __builtin_fmaf(p, r, 1.6666665459e-1f);
    p = __builtin_fmaf(p, r, 5.0000001201e-1f);
    const float r2 = r * r;
    float y = __builtin_fmaf(p, r2, r);
    y = y + 1.0f;
    const int k = (int)kf, k1 = k / 2, k2 = k - k1;                     // k in [-126, 128]; both halves in [-63, 64]
    y = y * vv_det_float((unsigned)(k1 + 127) << 23);
    return y * vv_det_float((unsigned)(k2 + 127) << 23);
}

// 1 / (1 + e^-x).  NaN -> NaN; x < -87 -> 0 (the value there is below 1.7e-38), so that neither e^-x overflows nor the quotient is
// subnormal; large x gives 1 / (1 + 0) = 1.
VV_DET_HD float vv_det_sigmoid(float x) {
#pragma clang fp contract(off)
    if (x != x) return x;
    if (x < -87.0f) return 0.0f;
    return 1.0f / (1.0f + vv_det_exp(-x));
}

// tanh x.  NaN -> NaN; |x| < 0.625: x + x^3 P(x^2); |x| <= 10: 1 - 2 / (e^(2|x|) + 1); beyond: 1 (1 - tanh 10 = 4e-9 < half a unit);
// the sign is copied in the bits, so tanh(-x) = -tanh(x) exactly and tanh(-0) = -0.
VV_DET_HD float vv_det_tanh(float x) {
#pragma clang fp contract(off)
    if (x != x) return x;
    const unsigned sign = vv_det_bits(x) & 0x80000000u;
    const float a = vv_det_float(vv_det_bits(x) & 0x7FFFFFFFu);
    float t;
    if (a < 0.625f) {
        const float z = a * a;
        float p = -5.70498872745e-3f;
        p = __builtin_fmaf(p, z, 2.06390887954e-2f);
        p = __builtin_fmaf(p, z, -5.37397155531e-2f);
        p = __builtin_fmaf(p, z, 1.33314422036e-1f);
        p = __builtin_fmaf(p, z, -3.33332819422e-1f);
        p = p * z;
        t = __builtin_fmaf(p, a, a);
    } else if (a <= 10.0f) {
        t = 1.0f - 2.0f / (vv_det_exp(a + a) + 1.0f);
    } else {
        t = 1.0f;
    }
    return vv_det_float(vv_det_bits(t) | sign);
}

VV_DET_HD float vv_det_relu(float x) { return x != x ? x : (x > 0.0f ? x : 0.0f); }       // tf.nn.relu keeps a NaN

// numpy's maximum / minimum: a NaN operand gives NaN.
VV_DET_HD float vv_det_max(float a, float b) { return a != a ? a : (b != b ? b : (a > b ? a : b)); }
VV_DET_HD float vv_det_min(float a, float b) { return a != a ? a : (b != b ? b : (a < b ? a : b)); }

// The box of predictor `pred` in cell (gr, gc): (col_min, row_min, col_max, row_max) with the reference's roundings under numpy 2
// (:114-118): t = f32(f32(gr) + y); q = f32(t / R) (the float64 division rounded to float32 = the correctly rounded float32 division);
// row_min = f32(q - f32(h / 2)).  The four box fields are (h, w, x, y): exp, exp, sigmoid, sigmoid.
VV_DET_HD void vv_det_box(const VvDetFrame &f, int cell, int pred, int width, int gr, int gc, int R, int C, float box[4]) {
#pragma clang fp contract(off)
    const int ch = pred * width + VV_DET_B2;
    const float h = vv_det_exp(vv_det_at(f, cell, ch)), w = vv_det_exp(vv_det_at(f, cell, ch + 1));
    const float x = vv_det_sigmoid(vv_det_at(f, cell, ch + 2)), y = vv_det_sigmoid(vv_det_at(f, cell, ch + 3));
    const float tr = (float)gr + y, tc = (float)gc + x;
    const float qr = tr / (float)R, qc = tc / (float)C;
    const float hh = h / 2.0f, hw = w / 2.0f;
    box[0] = qc - hw, box[1] = qr - hh, box[2] = qc + hw, box[3] = qr + hh;
}

// Does the picked box a suppress box b?  function.py:129-148 in float32 and in its operation order; strict; a NaN IoU (0/0, inf/inf,
// a NaN coordinate) suppresses nothing.
VV_DET_HD bool vv_det_suppresses(const float a[4], const float b[4], float iou_thresh) {
#pragma clang fp contract(off)
    const float area_a = (a[3] - a[1]) * (a[2] - a[0]), area_b = (b[3] - b[1]) * (b[2] - b[0]);
    const float rr_min = vv_det_max(a[1], b[1]), cc_min = vv_det_max(a[0], b[0]);
    const float rr_max = vv_det_min(a[3], b[3]), cc_max = vv_det_min(a[2], b[2]);
    const float w = vv_det_max(0.0f, cc_max - cc_min), h = vv_det_max(0.0f, rr_max - rr_min);
    const float inter = w * h;
    const float uni = (area_a + area_b) - inter;
    const float iou = inter / uni;
    return iou > iou_thresh;
}

// Inside a cell: predictors in descending objectness, ties to the lower predictor (np.argsort(-objness), stable in effect: our rule).
// -> does predictor q come before predictor p?
VV_DET_HD bool vv_det_cell_before(float sq, int q, float sp, int p) { return sq > sp || (sq == sp && q < p); }
// Among candidates: descending objectness, ties to the HIGHER candidate index (a stable ascending sort read from the end).
VV_DET_HD bool vv_det_rank_before(float sj, int j, float si, int i) { return sj > si || (sj == si && j > i); }

// One picked detection's rows except index and bbox2d: bbox3d (field 1, field 0, field 2; relu), the latents, tanh of sin / cos, the
// radian log-variances.  Value e of the F = 2 Z + 12 values of a row, in the order bbox3d, mean, log_var, sin, cos, rad.
VV_DET_HD float vv_det_row_value(const VvDetFrame &f, int cell, int pred, int z, int e) {
    const int base = pred * vv_det_width(z);
    if (e < 3) return vv_det_relu(vv_det_at(f, cell, base + VV_DET_B3 + (e == 0 ? 1 : (e == 1 ? 0 : 2))));
    e -= 3;
    if (e < 2 * z) return vv_det_at(f, cell, base + VV_DET_MEAN + e);                   // mean, then log_var
    e -= 2 * z;
    if (e < 6) return vv_det_tanh(vv_det_at(f, cell, base + vv_det_sin(z) + e));        // sin, then cos
    return vv_det_at(f, cell, base + vv_det_sin(z) + e);                                // rad_log_var
}
VV_DET_HD void vv_det_store_row_value(int z, long long row, int e, float v, float *bbox3d, float *inst_mean, float *inst_log_var,
                                      float *sn, float *cs, float *rad) {
    if (e < 3) bbox3d[row * 3 + e] = v;
    else if (e < 3 + z) inst_mean[row * z + (e - 3)] = v;
    else if (e < 3 + 2 * z) inst_log_var[row * z + (e - 3 - z)] = v;
    else if (e < 6 + 2 * z) sn[row * 3 + (e - 3 - 2 * z)] = v;
    else if (e < 9 + 2 * z) cs[row * 3 + (e - 6 - 2 * z)] = v;
    else rad[row * 3 + (e - 9 - 2 * z)] = v;
}

// ---- the whole step for one frame as plain loops (the host entry; the kernel deals the same functions over a workgroup).
// Scratch for `slots` candidates: score [slots], box [slots][4], index [slots], order [slots], live [slots].  Outputs are the frame's.
VV_DET_HD int vv_det_frame_host(const VvDetFrame &f, int R, int C, int P, int Z, float obj_thresh, float iou_thresh, int top_1, float *score,
                                float *box, int *cand, int *order, unsigned char *live, int *index, float *bbox2d, float *bbox3d,
                                float *inst_mean, float *inst_log_var, float *sn, float *cs, float *rad) {
    const int width = vv_det_width(Z);
    int n = 0;
    for (int cell = 0; cell < R * C; ++cell) {
        float s[VV_DET_MAX_P];
        for (int p = 0; p < P; ++p) s[p] = vv_det_sigmoid(vv_det_at(f, cell, p * width + VV_DET_OBJ));
        int in_cell = 0;
        for (int p = 0; p < P; ++p) in_cell += s[p] > obj_thresh ? 1 : 0;
        const int first = n;
        for (int p = 0; p < P; ++p) {
            if (!(s[p] > obj_thresh)) continue;
            int before = 0;
            for (int q = 0; q < P; ++q) before += vv_det_cell_before(s[q], q, s[p], p) ? 1 : 0;
            if (top_1 && before > 0) continue;
            const int j = first + before;
            score[j] = s[p], cand[j] = cell * P + p;
            vv_det_box(f, cell, p, width, cell / C, cell % C, R, C, box + (long long)j * 4);
        }
        n += top_1 ? (in_cell > 0 ? 1 : 0) : in_cell;
    }
    for (int i = 0; i < n; ++i) {
        int rank = 0;
        for (int j = 0; j < n; ++j) rank += vv_det_rank_before(score[j], j, score[i], i) ? 1 : 0;
        order[rank] = i, live[i] = 1;                     // live is indexed by RANK below; every rank is set here exactly once
    }
    int count = 0;
    for (int i = 0; i < n; ++i) {
        if (!live[i]) continue;
        const int a = order[i];
        for (int k = i + 1; k < n; ++k)
            if (live[k] && vv_det_suppresses(box + (long long)a * 4, box + (long long)order[k] * 4, iou_thresh)) live[k] = 0;
        const long long row = count++;
        index[row] = cand[a];
        for (int e = 0; e < 4; ++e) bbox2d[row * 5 + e] = box[(long long)a * 4 + e];
        bbox2d[row * 5 + 4] = score[a];
        for (int e = 0; e < 2 * Z + 12; ++e)
            vv_det_store_row_value(Z, row, e, vv_det_row_value(f, cand[a] / P, cand[a] % P, Z, e), bbox3d, inst_mean, inst_log_var, sn, cs, rad);
    }
    return count;
}
