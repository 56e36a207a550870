// One object's network input from a photo, after the reference's input pipeline (src/dataset_loader/pascal3D.py:216-242 calling
// src/dataset_loader/datasetUtils.py:91-152): crop the box, flip, perturb colours, cv2.warpAffine with a random scale and translation,
// cv2.resize(INTER_CUBIC) to the network size, divide by 255.  Plain C++ that compiles for the host and for the device alike (augment.hip
// runs vv_aug_warp_level over a tile's footprint in LDS and vv_aug_cubic_pixel out of it; vv_augment_images_host runs the loops at the
// end of this file) and without HIP.  No inline assembly, no atomics, no memory besides the arguments.
//
// THE FUNCTION IS DEFINED IN FLOATING POINT, every expression below written once with contraction off, so host and device give the
// same bits.  The real arithmetic of steps 2 and 3 is IEEE float64 (f64 below); the scale word and the output are float32.  Why not
// float32: with s = 0.8 or 1.2 the bilinear weights fall on multiples of 1/8, so about one warped level in 64 is a tie of v + 0.5 up to
// the rounding of s, and float32 coordinates (error 2^-19 at 50 pixels, times a gradient of 100 levels per pixel) break such ties the
// other way than exact arithmetic at 0.3 .. 0.6 % of the pixels of a random image -- measured against a float64 restatement, and each
// such level moves about one output value.  In float64 both stages agree with the restatement at every value of the test cases.
// cv2's own fixed-point tables are NOT modelled: warpAffine rounds source coordinates to 1/32 pixel and uses 2^-15 bilinear
// weights, resize rounds the cubic weights to 2^-11.  Nobody has measured the difference from cv2 (it is not a dependency of this project).
//
// params, int32 [B][16]:
//   0      image index                       5      flip bits (0 horizontal, 1 vertical)      10..12 additive value per channel, -10 .. 10
//   1..4   crop row0, col0, rows h, cols w   6      scale s as float32 bits                   13, 14 rowPad, colPad
//          (padded image's coordinates)      7, 8   dRow, dCol                                15     reserved, 0
//                                            9      invert bits, one per channel
// The padded image is the image with a border of rowPad zero rows above and below and colPad zero columns left and right.
//
// 1. source level.  Four stages on the flipped crop, in the reference's Sequential order (datasetUtils.py:64-89):
//    blur -> invert -> add -> hue/saturation.  Stages 2 and 3 are integer and exact and are all that a params row alone asks for
//    (vv_aug_source); blur and hue/saturation are opt-in per sample through the second table `colour` below.
//    Crop pixel (y, x), channel c: fx = bit 0 ? w - 1 - x : x, fy = bit 1 ? h - 1 - y : y; the padded
//    image at (row0 + fy, col0 + fx) is the image's byte, or 0 in the border (vv_aug_raw);
//    [blur, when colour asks for it: 1a below];  v = invert bit c ? 255 - v : v; v = min(max(v + add_c, 0), 255)
//    (imgaug Invert, then Add);  [hue/saturation, when colour asks for it: 1b below].  Outside the crop (y or x out of range) the
//    level is 0: warpAffine's constant border.
//
// colour, int32 [B][4], a second per-sample table (the 16-word row is unchanged and p[15] stays 0):
//   0  flags: bit 0 blur, bit 1 hue/saturation; other bits are refused       2  hue add in H units, -179 .. 179
//   1  sigma as float32 bits: finite, 0 <= sigma <= 16                         3  saturation add, -255 .. 255
//   A row of zeros (and no table at all) is the two-stage source level above, bit for bit.
//
// 1a. blur: imgaug GaussianBlur in the form that calls scipy.ndimage.gaussian_filter(mode='mirror', truncate 4), on the raw crop after
//    the flip (pad zeros are part of the crop), all three channels alike.  r = (int)(4.0f * sigma + 0.5f) in float32; r == 0 is the identity.
//        u_k = e(-0.5 * f64(k * k) / (f64(sigma) * f64(sigma))),  k = -r .. r;   S = ((u_-r + u_-r+1) + ...) left to right;   w_k = u_k / S
//    separable, axis 0 (rows) first:  t(y, x) = sum_k w_k * p(mirror(y + k, h), x),  then  v(y, x) = sum_k w_k * t(y, mirror(x + k, w)),
//    each product rounded before it is added, k ascending, the first product starting the sum, t kept as f64.  One rounding at the end:
//    level = min(max(floor(v + 0.5), 0), 255).  mirror(i, n) reflects about the edge pixels without repeating them (period 2(n - 1),
//    n == 1 gives 0); a radius above the extent reflects more than once.  Every drawn sigma is below 3 (r <= 12); a sigma above 3.125
//    (r up to 64, injected tables only) is admitted but is a SLOW path on the device ((2r + 1)^2 image reads per pixel), not measured.
//    e(x) is vv_aug_exp below, NOT libm's or OCML's exp (their bits are not guaranteed to agree): k = nearest integer to x / ln 2 by the
//    1.5 * 2^52 trick, r = x - k ln 2 in two fma steps, e^r as the degree-13 Taylor polynomial in fma (|r| <= 0.3466: truncation under
//    1e-17 relative), the scale 2^k through the exponent bits.  x in [-40, 0] (it is held there); relative error below 1e-12 (against a
//    60-digit evaluation at 110 points across the range: under 1e-15).
//    NOT modelled: scipy's symmetric-kernel summation order and its sum of the weights (differences of 1e-13 of a level before the
//    rounding), and cv2.GaussianBlur, which imgaug uses for some sigma / dtype combinations with fixed-point 8-bit weights.
// 1b. hue/saturation: imgaug AddToHueAndSaturation with per_channel false, through OpenCV's 8-bit HSV, on the three levels after add.
//    Channel 0 is taken as R (the reference hands a cv2 BGR image to imgaug, which reads it as RGB).  Forward, integers, shift 12:
//        sdiv(i) = rint((255 << 12) / i),  hdiv(i) = rint((180 << 12) / (6 i)),  sdiv(0) = hdiv(0) = 0
//        v = max, diff = v - min,  s = (diff * sdiv(v) + 2048) >> 12
//        h0 = v == r ? g - b : (v == g ? b - r + 2 diff : r - g + 4 diff);   h = (h0 * hdiv(diff) + 2048) >> 12 (arithmetic);  h < 0: h += 180
//    then h = (h + hue) mod 180 made non-negative, s = min(max(s + sat, 0), 255).  Inverse, float32, every operation rounded:
//        hf = f32(h) * (6.0f / 180.0f),  sf = f32(s) * (1.0f / 255.0f),  vf = f32(v) * (1.0f / 255.0f)
//        sector = floorf(hf),  f = hf - sector;  sector >= 6: sector = 0, f = 0
//        tab = {vf, vf * (1 - sf), vf * (1 - sf * f), vf * (1 - sf * (1 - f))}
//        (b, g, r) = tab[{1,3,0}, {1,0,2}, {3,0,1}, {0,2,1}, {0,1,3}, {2,1,0}][sector];   level = min(max(rintf(x * 255.0f), 0), 255)
//    s == 0 gives r = g = b = v.  The stage runs whenever its flag is set, at value 0 too: the 8-bit round trip is not the identity.
//    This is OpenCV's 8-bit RGB2HSV / HSV2RGB as recalled; cv2 is not a dependency of this project and the agreement with it is NOT
//    measured; cv2's own tables and its vectorised float path are NOT modelled beyond what these lines state.  The tests bind the stage
//    to a numpy restatement of these lines (exact) and to a float64 HSV chain (within 6 levels: H's quantum of 2 degrees).
// 2. warp (datasetUtils.py:137-147).  Forward matrix [[s, 0, (w/2)(1-s) + dCol], [0, s, (h/2)(1-s) + dRow]], destination w x h, integer
//    coordinates are pixel centres, dst(x, y) = src(M^-1 (x, y)).  M^-1 per axis, written about the centre so that the subtraction is exact:
//        hw = f64(w) * 0.5             (exact)                 u  = f64(x - dCol) - hw    (exact: half-integers)
//        q  = u / f64(s)               (correctly rounded)     sx = q + hw
//        x0 = floor(sx),  ax = sx - x0,  bx = 1.0 - ax         (rows likewise: hh, dRow, sy, y0, ay, by)
//    bilinear over the four source levels p00 (y0, x0), p01 (y0, x0+1), p10, p11 as f64:
//        top = bx * p00;  t = ax * p01;  top = top + t;        bot = bx * p10;  t = ax * p11;  bot = bot + t;
//        v = by * top;  t = ay * bot;  v = v + t;              level = (int)floor(v + 0.5), held to 0 .. 255 as a uint8 Mat holds it
//    A source coordinate below -1 or at or above the extent reads four zeros: the level is 0 without any arithmetic.
// 3. resize to out_cols x out_rows, INTER_CUBIC semantics, no antialiasing.  Per axis (columns shown):
//        scale = f64(w) / f64(out_cols)        f = (f64(d) + 0.5) * scale;  f = f - 0.5;      i = floor(f),  t = f - i
//    Keys weights, a = -0.75, for taps i-1, i, i+1, i+2, each product and sum one f64 operation in the order written:
//        t1 = t + 1.0:    w0 = ((a * t1 - 5a) * t1 + 8a) * t1 - 4a
//                         w1 = (((a + 2) * t - (a + 3)) * t) * t + 1.0
//        t2 = 1.0 - t:    w2 = (((a + 2) * t2 - (a + 3)) * t2) * t2 + 1.0
//                         w3 = ((1.0 - w0) - w1) - w2
//    tap indices clamped to 0 .. extent-1 (replicate).  For tap rows r = 0 .. 3 in order:
//        row_r = ((wx0 * p_r0 + wx1 * p_r1) + wx2 * p_r2) + wx3 * p_r3           (left to right, products rounded before each sum)
//        v = ((wy0 * row_0 + wy1 * row_1) + wy2 * row_2) + wy3 * row_3
//    level = min(max(floor(v + 0.5), 0), 255);  out = f32(level) / 255.0f (one correctly rounded float32 division).
// The intermediate rounding of step 2 makes the chain non-separable: it is evaluated as written.
//
// The random half (vv_augment_draw): pascal3D.py:216-241 and datasetUtils.py:98-145 on Philox4x32-10 (keep_mask.h).  Sample b owns
// blocks 8b .. 8b+7 of counter (blk, offset) under key seed; slot k below is word k & 3 of block 8b + (k >> 2), u = vv_km_uniform(word).
//   slot 0  border ratio 0.2f * u                          slot 9   scale: s = 0.8f + 0.4f * u (when gated)
//   slot 1  horizontal flip: u > 0.5                       slot 10  translation gate (transPr): u < 0.5
//   slot 2  vertical flip, only within slot 1: u > 0.5     slot 11  dRow = (int)floorf(u * f32(2m)) - m, m = (int)(0.2f * f32(h))
//   slot 3  imAugPr gate: u < 0.5                          slot 12  dCol likewise with w
//   slot 4  GaussianBlur chosen: u >= 0.5   (colour)       slot 13..15  invert channel 0..2: u < 0.05
//   slot 5  brightness (Add) chosen: u >= 0.5              slot 16  Add per_channel gate: u < 0.5
//   slot 6  hue/saturation chosen: u >= 0.5 (colour)       slot 17..19  Add value (int)floorf(u * 21.0f) - 10; without the gate slot 17's
//   slot 7  channel invert chosen: u >= 0.5                         value serves all three channels
//   slot 8  scale gate (scalePr): u < 0.5                  slot 20  blur sigma = 3.0f * u;  slot 21  hue/saturation value (colour only)
// m = 0 gives d = 0 (the reference's randint(0, 0) raises and its bare except drops the object).  The crop is the reference's:
// width = colMax - colMin;  cMin = max(0, colMin - width * border);  cMax = min(cols, colMax + width * border);  col0 = (int)cMin,
// w = (int)cMax - col0 (rows likewise), float32, products rounded before the sums.  augmentation = 0: border 0.1f, no flip, s = 1, d = 0,
// no colour change.  rowPad = colPad = 0.
// Slots 4, 6, 20 and 21 reach only the colour table (vv_aug_draw_pair, what vv_augment_draw_ex fills beside the unchanged 16-word row):
// both under the imAugPr gate of slot 3; blur chosen: flags bit 0, sigma = 3.0f * u(20); hue/saturation chosen: flags bit 1,
// value = min((int)floorf(u(21) * 41.0f) - 20, 20), sat = value, hue = (value * 180) / 255 in C integer division (imgaug's astype(int32) of
// value / 255 * 180).  augmentation = 0 and a refused sample: a row of zeros.
#pragma once
#include <math.h>

#include "keep_mask.h"

#define VV_AUG_HD VV_KM_HD
#define VV_AUG_WORDS 16

struct VvAugSample {
    const unsigned char *img;      // the image's first byte (HWC, 3 channels)
    int rows, cols;                // the image's extents
    int row0, col0, h, w, flip;
    float s;
    int d_row, d_col, inv, add[3], row_pad, col_pad;
};

VV_AUG_HD float vv_aug_bits_float(int bits) {
    union {
        int i;
        float f;
    } u;
    u.i = bits;
    return u.f;
}
VV_AUG_HD int vv_aug_float_bits(float f) {
    union {
        int i;
        float f;
    } u;
    u.f = f;
    return u.i;
}

// One params row against the image table: VV_OK (0) or the status an inadmissible row gets (-2, VV_ERR_SHAPE's value).  On success *o is
// filled.  images_bytes bounds the arena and a table row that leaves it is refused as well; negative: the arena's size is not known.
VV_AUG_HD int vv_aug_sample(const unsigned char *images, long long images_bytes, const long long *image_meta, int n_images, const int *p,
                            VvAugSample *o) {
    const int idx = p[0];
    if (idx < 0 || idx >= n_images) return -2;
    const long long off = image_meta[3 * idx], rows = image_meta[3 * idx + 1], cols = image_meta[3 * idx + 2];
    if (off < 0 || rows < 1 || cols < 1 || rows > 0x3FFF || cols > 0x3FFF) return -2;
    if (images_bytes >= 0 && off + rows * cols * 3 > images_bytes) return -2;
    const int row_pad = p[13], col_pad = p[14];
    if (row_pad < 0 || col_pad < 0 || row_pad > 0x3FFF || col_pad > 0x3FFF) return -2;
    const int row0 = p[1], col0 = p[2], h = p[3], w = p[4];
    if (h < 1 || w < 1 || row0 < 0 || col0 < 0 || h > 0x7FFF || w > 0x7FFF) return -2;
    if ((long long)row0 + h > rows + 2 * row_pad || (long long)col0 + w > cols + 2 * col_pad) return -2;
    const float s = vv_aug_bits_float(p[6]);
    if (!(s > 0.0f) || !(s <= 3.0e38f)) return -2;                     // NaN fails the first, +inf the second
    if (p[7] < -0x7FFF || p[7] > 0x7FFF || p[8] < -0x7FFF || p[8] > 0x7FFF) return -2;
    if ((p[5] & ~3) || (p[9] & ~7) || p[15] != 0) return -2;
    for (int c = 0; c < 3; ++c)
        if (p[10 + c] < -255 || p[10 + c] > 255) return -2;
    o->img = images ? images + off : images, o->rows = (int)rows, o->cols = (int)cols;
    o->row0 = row0, o->col0 = col0, o->h = h, o->w = w, o->flip = p[5], o->s = s, o->d_row = p[7], o->d_col = p[8], o->inv = p[9];
    o->add[0] = p[10], o->add[1] = p[11], o->add[2] = p[12], o->row_pad = row_pad, o->col_pad = col_pad;
    return 0;
}

// step 1: the three levels of crop pixel (y, x) as bytes 0..2 of a word; (y, x) outside the crop: 0
VV_AUG_HD unsigned vv_aug_source(const VvAugSample &a, int y, int x) {
    if (y < 0 || y >= a.h || x < 0 || x >= a.w) return 0u;
    const int fx = (a.flip & 1) ? a.w - 1 - x : x, fy = (a.flip & 2) ? a.h - 1 - y : y;
    const int r = a.row0 + fy - a.row_pad, c = a.col0 + fx - a.col_pad;
    const bool inside = r >= 0 && r < a.rows && c >= 0 && c < a.cols;
    const unsigned char *px = inside ? a.img + ((long long)r * a.cols + c) * 3 : a.img;
    unsigned out = 0u;
    for (int ch = 0; ch < 3; ++ch) {
        int v = inside ? (int)px[ch] : 0;
        v = ((a.inv >> ch) & 1) ? 255 - v : v;
        v += a.add[ch];
        v = v < 0 ? 0 : (v > 255 ? 255 : v);
        out |= (unsigned)v << (8 * ch);
    }
    return out;
}

// ---------------------------------------------------------------------------------------------------- the colour table (1a, 1b)
#define VV_AUG_COLOUR_WORDS 4
#define VV_AUG_BLUR_MAX_R 64                                               // (int)(4 * 16 + 0.5)

struct VvAugColour {
    int flags, r, hue, sat;        // r: the blur radius, 0 without the blur flag
    float sigma;
};

// One colour row: 0, or -2 for a row that is refused.  On success *o is filled.
VV_AUG_HD int vv_aug_colour(const int *c, VvAugColour *o) {
#pragma clang fp contract(off)
    if (c[0] & ~3) return -2;
    const float sigma = vv_aug_bits_float(c[1]);
    if (!(sigma >= 0.0f) || !(sigma <= 16.0f)) return -2;                 // NaN fails the first
    if (c[2] < -179 || c[2] > 179 || c[3] < -255 || c[3] > 255) return -2;
    o->flags = c[0], o->sigma = sigma, o->hue = c[2], o->sat = c[3];
    o->r = (c[0] & 1) ? (int)(4.0f * sigma + 0.5f) : 0;
    return 0;
}

// the raw level of 1.: crop pixel (y, x), 0 <= y < h, 0 <= x < w, after the flip and before any colour stage
VV_AUG_HD unsigned vv_aug_raw(const VvAugSample &a, int y, int x) {
    const int fx = (a.flip & 1) ? a.w - 1 - x : x, fy = (a.flip & 2) ? a.h - 1 - y : y;
    const int r = a.row0 + fy - a.row_pad, c = a.col0 + fx - a.col_pad;
    if (r < 0 || r >= a.rows || c < 0 || c >= a.cols) return 0u;
    const unsigned char *px = a.img + ((long long)r * a.cols + c) * 3;
    return (unsigned)px[0] | (unsigned)px[1] << 8 | (unsigned)px[2] << 16;
}

VV_AUG_HD int vv_aug_mirror(int i, int n) {
    if (n <= 1) return 0;
    const int period = 2 * (n - 1);
    i %= period;
    if (i < 0) i += period;
    return i < n ? i : period - i;
}

// e(x) of 1a
VV_AUG_HD double vv_aug_exp(double x) {
#pragma clang fp contract(off)
    if (!(x >= -40.0)) x = -40.0;
    if (x > 0.0) x = 0.0;
    const double magic = 6755399441055744.0;                              // 1.5 * 2^52
    const double kf = __builtin_fma(x, 1.4426950408889634, magic) - magic;
    double r = __builtin_fma(kf, -6.93147180369123816490e-01, x);         // ln 2, its upper 32 significant bits: k * hi is exact
    r = __builtin_fma(kf, -1.90821492927058770002e-10, r);
    double p = 1.6059043836821613e-10;                                    // 1 / 13!
    p = __builtin_fma(p, r, 2.08767569878681e-09);
    p = __builtin_fma(p, r, 2.505210838544172e-08);
    p = __builtin_fma(p, r, 2.755731922398589e-07);
    p = __builtin_fma(p, r, 2.7557319223985893e-06);
    p = __builtin_fma(p, r, 2.48015873015873e-05);
    p = __builtin_fma(p, r, 1.984126984126984e-04);
    p = __builtin_fma(p, r, 1.3888888888888889e-03);
    p = __builtin_fma(p, r, 8.333333333333333e-03);
    p = __builtin_fma(p, r, 4.1666666666666664e-02);
    p = __builtin_fma(p, r, 1.6666666666666666e-01);
    p = __builtin_fma(p, r, 0.5);
    p = __builtin_fma(p, r, 1.0);
    p = __builtin_fma(p, r, 1.0);
    union {
        unsigned long long u;
        double d;
    } s;
    s.u = (unsigned long long)((long long)kf + 1023) << 52;               // k in -58 .. 0: a normal number
    return p * s.d;
}

// the unnormalised weight u_k of 1a
VV_AUG_HD double vv_aug_blur_tap(int k, float sigma) {
#pragma clang fp contract(off)
    const double sd = (double)sigma;
    const double num = -0.5 * (double)(k * k);
    return vv_aug_exp(num / (sd * sd));
}

VV_AUG_HD unsigned vv_aug_pack_levels(const double v[3]) {
#pragma clang fp contract(off)
    unsigned out = 0u;
    for (int ch = 0; ch < 3; ++ch) {
        double l = floor(v[ch] + 0.5);
        l = l < 0.0 ? 0.0 : (l > 255.0 ? 255.0 : l);
        out |= (unsigned)(int)l << (8 * ch);
    }
    return out;
}

// 1a for one pixel from first principles: `raw(y, x)` returns the packed raw levels of an in-crop pixel, w points at the 2r+1
// normalised weights.  (2r+1)^2 reads: the form for a radius whose halo does not fit a tile's staging, and the same bits as the
// two-pass forms (the same products and sums in the same order).
template <class Raw>
VV_AUG_HD unsigned vv_aug_blur_direct(int h, int w_ext, int r, const double *w, int y, int x, Raw raw) {
#pragma clang fp contract(off)
    double v[3] = {0.0, 0.0, 0.0};
    for (int kx = -r; kx <= r; ++kx) {
        const int xx = vv_aug_mirror(x + kx, w_ext);
        double t[3] = {0.0, 0.0, 0.0};
        for (int ky = -r; ky <= r; ++ky) {
            const unsigned p = raw(vv_aug_mirror(y + ky, h), xx);
            for (int ch = 0; ch < 3; ++ch) {
                const double m = w[ky + r] * (double)((p >> (8 * ch)) & 255u);
                t[ch] = ky == -r ? m : t[ch] + m;
            }
        }
        for (int ch = 0; ch < 3; ++ch) {
            const double m = w[kx + r] * t[ch];
            v[ch] = kx == -r ? m : v[ch] + m;
        }
    }
    return vv_aug_pack_levels(v);
}

// 1b on three packed levels
VV_AUG_HD unsigned vv_aug_hue_sat(unsigned px, int hue, int sat) {
#pragma clang fp contract(off)
    const int r = (int)(px & 255u), g = (int)((px >> 8) & 255u), b = (int)((px >> 16) & 255u);
    int v = r > g ? r : g, mn = r < g ? r : g;
    v = v > b ? v : b, mn = mn < b ? mn : b;
    const int diff = v - mn;
    const int sdiv = v ? (int)rint(1044480.0 / (double)v) : 0;              // 255 << 12
    const int hdiv = diff ? (int)rint(737280.0 / (double)(6 * diff)) : 0;   // 180 << 12
    int s = (diff * sdiv + 2048) >> 12;
    const int h0 = v == r ? g - b : (v == g ? b - r + 2 * diff : r - g + 4 * diff);
    const int hn = h0 * hdiv + 2048;
    int h = hn >= 0 ? hn >> 12 : -((-hn + 4095) >> 12);                    // the arithmetic shift, spelt without shifting a negative
    if (h < 0) h += 180;
    h = (h + hue) % 180;
    if (h < 0) h += 180;
    s += sat;
    s = s < 0 ? 0 : (s > 255 ? 255 : s);
    if (s == 0) return (unsigned)v | (unsigned)v << 8 | (unsigned)v << 16;
    const float hf = (float)h * (6.0f / 180.0f), sf = (float)s * (1.0f / 255.0f), vf = (float)v * (1.0f / 255.0f);
    float sector = floorf(hf);
    float f = hf - sector;
    if (sector >= 6.0f) sector = 0.0f, f = 0.0f;
    const float tab0 = vf;
    float t = 1.0f - sf;
    const float tab1 = vf * t;
    t = sf * f;
    t = 1.0f - t;
    const float tab2 = vf * t;
    t = 1.0f - f;
    t = sf * t;
    t = 1.0f - t;
    const float tab3 = vf * t;
    // the (b, g, r) table indices of the six sectors, two bits each (b lowest), six bits per sector, sector 0 lowest
    const unsigned long long codes = 13ull | 33ull << 6 | 19ull << 12 | 24ull << 18 | 52ull << 24 | 6ull << 30;
    const unsigned cd = (unsigned)(codes >> (6 * (int)sector)) & 63u;
    unsigned out = 0u;
    for (int k = 0; k < 3; ++k) {
        const unsigned i = (cd >> (2 * k)) & 3u;
        float l = rintf((i == 0u ? tab0 : (i == 1u ? tab1 : (i == 2u ? tab2 : tab3))) * 255.0f);
        l = l < 0.0f ? 0.0f : (l > 255.0f ? 255.0f : l);
        out |= (unsigned)(int)l << (8 * (2 - k));                           // b -> channel 2, g -> 1, r -> 0
    }
    return out;
}

// stages 2 .. 4 of 1. on the packed levels that stage 1 left (the raw levels, or the blurred ones)
VV_AUG_HD unsigned vv_aug_finish(const VvAugSample &a, const VvAugColour &c, unsigned px) {
    unsigned out = 0u;
    for (int ch = 0; ch < 3; ++ch) {
        int v = (int)((px >> (8 * ch)) & 255u);
        v = ((a.inv >> ch) & 1) ? 255 - v : v;
        v += a.add[ch];
        v = v < 0 ? 0 : (v > 255 ? 255 : v);
        out |= (unsigned)v << (8 * ch);
    }
    return (c.flags & 2) ? vv_aug_hue_sat(out, c.hue, c.sat) : out;
}

// The source of step 2: the finished levels of a flagged sample out of its slab (h * w packed words, row stride w), everything else
// through vv_aug_source.  slab == nullptr is vv_aug_source.
struct VvAugSlabSource {
    const unsigned *slab;
    VV_AUG_HD unsigned operator()(const VvAugSample &a, int y, int x) const {
        if (!slab) return vv_aug_source(a, y, x);
        if (y < 0 || y >= a.h || x < 0 || x >= a.w) return 0u;
        return slab[(size_t)y * a.w + x];
    }
};

// M^-1 along one axis: destination coordinate d -> source coordinate (extent n, translation t, scale s)
VV_AUG_HD double vv_aug_inverse(int d, int n, int t, float s) {
#pragma clang fp contract(off)
    const double half = (double)n * 0.5;
    const double u = (double)(d - t) - half;
    const double q = u / (double)s;
    return q + half;
}

// step 2: the three warped levels of destination pixel (y, x) of the crop, packed as vv_aug_source packs them
// (`source(a, y, x)` is step 1: vv_aug_source, or a VvAugSlabSource)
template <class Source>
VV_AUG_HD unsigned vv_aug_warp_level(const VvAugSample &a, int y, int x, Source source) {
#pragma clang fp contract(off)
    const double sx = vv_aug_inverse(x, a.w, a.d_col, a.s), sy = vv_aug_inverse(y, a.h, a.d_row, a.s);
    if (!(sx >= -1.0) || !(sy >= -1.0) || !(sx < (double)a.w) || !(sy < (double)a.h)) return 0u;
    const double fx0 = floor(sx), fy0 = floor(sy);
    const double ax = sx - fx0, ay = sy - fy0;
    const double bx = 1.0 - ax, by = 1.0 - ay;
    const int x0 = (int)fx0, y0 = (int)fy0;                              // -1 .. extent-1
    const unsigned p00 = source(a, y0, x0), p01 = source(a, y0, x0 + 1);
    const unsigned p10 = source(a, y0 + 1, x0), p11 = source(a, y0 + 1, x0 + 1);
    unsigned out = 0u;
    for (int ch = 0; ch < 3; ++ch) {
        const int sh = 8 * ch;
        double top = bx * (double)((p00 >> sh) & 255u);
        double t = ax * (double)((p01 >> sh) & 255u);
        top = top + t;
        double bot = bx * (double)((p10 >> sh) & 255u);
        t = ax * (double)((p11 >> sh) & 255u);
        bot = bot + t;
        double v = by * top;
        t = ay * bot;
        v = v + t;
        int level = (int)floor(v + 0.5);
        level = level < 0 ? 0 : (level > 255 ? 255 : level);
        out |= (unsigned)level << sh;
    }
    return out;
}

VV_AUG_HD unsigned vv_aug_warp_level(const VvAugSample &a, int y, int x) { return vv_aug_warp_level(a, y, x, VvAugSlabSource{nullptr}); }

struct VvAugTaps {
    int i;            // floor of the source coordinate: taps i-1 .. i+2 before clamping
    double w[4];
};

VV_AUG_HD double vv_aug_scale(int src, int dst) { return (double)src / (double)dst; }

// step 3 along one axis: destination index d, scale = vv_aug_scale(src, dst)
VV_AUG_HD VvAugTaps vv_aug_taps(int d, double scale) {
#pragma clang fp contract(off)
    const double A = -0.75;
    double f = ((double)d + 0.5) * scale;
    f = f - 0.5;
    const double fi = floor(f);
    const double t = f - fi;
    VvAugTaps o;
    o.i = (int)fi;
    const double t1 = t + 1.0, t2 = 1.0 - t;
    double w0 = A * t1;
    w0 = w0 - 5.0 * A;
    w0 = w0 * t1;
    w0 = w0 + 8.0 * A;
    w0 = w0 * t1;
    w0 = w0 - 4.0 * A;
    double w1 = (A + 2.0) * t;
    w1 = w1 - (A + 3.0);
    w1 = w1 * t;
    w1 = w1 * t;
    w1 = w1 + 1.0;
    double w2 = (A + 2.0) * t2;
    w2 = w2 - (A + 3.0);
    w2 = w2 * t2;
    w2 = w2 * t2;
    w2 = w2 + 1.0;
    double w3 = 1.0 - w0;
    w3 = w3 - w1;
    w3 = w3 - w2;
    o.w[0] = w0, o.w[1] = w1, o.w[2] = w2, o.w[3] = w3;
    return o;
}

VV_AUG_HD int vv_aug_clamp(int i, int n) { return i < 0 ? 0 : (i >= n ? n - 1 : i); }

// step 3 for one output pixel: `level(r, c)` returns the packed warped levels of crop pixel (r, c), 0 <= r < h, 0 <= c < w
template <class Level>
VV_AUG_HD void vv_aug_cubic_pixel(const VvAugTaps &ty, const VvAugTaps &tx, int h, int w, Level level, float out[3]) {
#pragma clang fp contract(off)
    double v[3] = {0.0, 0.0, 0.0};
    int cc[4];
    for (int k = 0; k < 4; ++k) cc[k] = vv_aug_clamp(tx.i - 1 + k, w);
    for (int r = 0; r < 4; ++r) {
        const int rr = vv_aug_clamp(ty.i - 1 + r, h);
        const unsigned p0 = level(rr, cc[0]), p1 = level(rr, cc[1]), p2 = level(rr, cc[2]), p3 = level(rr, cc[3]);
        for (int ch = 0; ch < 3; ++ch) {
            const int sh = 8 * ch;
            double row = tx.w[0] * (double)((p0 >> sh) & 255u);
            double t = tx.w[1] * (double)((p1 >> sh) & 255u);
            row = row + t;
            t = tx.w[2] * (double)((p2 >> sh) & 255u);
            row = row + t;
            t = tx.w[3] * (double)((p3 >> sh) & 255u);
            row = row + t;
            t = ty.w[r] * row;
            v[ch] = r == 0 ? t : v[ch] + t;
        }
    }
    for (int ch = 0; ch < 3; ++ch) {
        double l = floor(v[ch] + 0.5);
        l = l < 0.0 ? 0.0 : (l > 255.0 ? 255.0 : l);
        out[ch] = (float)l / 255.0f;
    }
}

// ---------------------------------------------------------------------------------------------------------------- the random half
VV_AUG_HD unsigned vv_aug_slot(int b, int k, unsigned long long seed, unsigned long long offset) {
    const VvKmBlock r = vv_km_block(8ull * (unsigned long long)b + (unsigned long long)(k >> 2), seed, offset);
    return r.w[k & 3];
}

VV_AUG_HD int vv_aug_randint(float u, int m) {
#pragma clang fp contract(off)
    if (m < 1) return 0;
    const float t = u * (float)(2 * m);
    int d = (int)floorf(t) - m;
    return d > m - 1 ? m - 1 : d;                                        // u <= 1 - 2^-24: the product can round up to 2m only for m >= 2^23
}

// one clamped, truncated extent of the crop: [lo, hi) widened by border inside [0, n) -> *first, *count
VV_AUG_HD void vv_aug_crop_axis(float lo, float hi, float border, int n, int *first, int *count) {
#pragma clang fp contract(off)
    const float width = hi - lo;
    const float grow = width * border;
    float a = lo - grow, b = hi + grow;
    const float fn = (float)n;
    a = a > 0.0f ? a : 0.0f;                                             // a NaN becomes 0 / n: the conversions below are defined
    a = a < fn ? a : fn;
    b = b < fn ? b : fn;
    b = b > 0.0f ? b : 0.0f;
    *first = (int)a;
    *count = (int)b - (int)a;
}

// params row of sample b: -> 0, or -2 for an image index outside the table or a crop with an empty extent (the row is then all
// zero but word 0 = -1, which vv_aug_sample refuses)
// col (may be null): the colour row of the same sample, zeros for a refused one
VV_AUG_HD int vv_aug_draw_pair(const long long *image_meta, int n_images, const int *image_index, const float *boxes, int b, int augmentation,
                               unsigned long long seed, unsigned long long offset, int *p, int *col) {
#pragma clang fp contract(off)
    for (int k = 0; k < VV_AUG_WORDS; ++k) p[k] = 0;
    p[0] = -1;
    if (col)
        for (int k = 0; k < VV_AUG_COLOUR_WORDS; ++k) col[k] = 0;
    const int idx = image_index[b];
    if (idx < 0 || idx >= n_images) return -2;
    const long long rows = image_meta[3 * idx + 1], cols = image_meta[3 * idx + 2];
    if (rows < 1 || cols < 1 || rows > 0x3FFF || cols > 0x3FFF) return -2;
    VvKmBlock blk[6];
    if (augmentation)
        for (int k = 0; k < 6; ++k) blk[k] = vv_km_block(8ull * (unsigned long long)b + (unsigned long long)k, seed, offset);
    else
        for (int k = 0; k < 6; ++k) blk[k].w[0] = blk[k].w[1] = blk[k].w[2] = blk[k].w[3] = 0u;
#define VV_AUG_U(slot) vv_km_uniform(blk[(slot) >> 2].w[(slot) & 3])
    const float border = augmentation ? 0.2f * VV_AUG_U(0) : 0.1f;
    int row0, col0, h, w;
    vv_aug_crop_axis(boxes[4 * b + 0], boxes[4 * b + 2], border, (int)cols, &col0, &w);
    vv_aug_crop_axis(boxes[4 * b + 1], boxes[4 * b + 3], border, (int)rows, &row0, &h);
    if (h < 1 || w < 1) return -2;
    int flip = 0, d_row = 0, d_col = 0, inv = 0, add[3] = {0, 0, 0};
    float s = 1.0f;
    if (augmentation) {
        if (VV_AUG_U(1) > 0.5f) flip = 1 | (VV_AUG_U(2) > 0.5f ? 2 : 0);
        if (VV_AUG_U(3) < 0.5f) {
            if (VV_AUG_U(7) >= 0.5f)
                for (int c = 0; c < 3; ++c) inv |= VV_AUG_U(13 + c) < 0.05f ? 1 << c : 0;
            if (VV_AUG_U(5) >= 0.5f) {
                const bool per_channel = VV_AUG_U(16) < 0.5f;
                for (int c = 0; c < 3; ++c) {
                    int v = (int)floorf(VV_AUG_U(per_channel ? 17 + c : 17) * 21.0f) - 10;
                    add[c] = v > 10 ? 10 : v;
                }
            }
            if (col && VV_AUG_U(4) >= 0.5f) {
                col[0] |= 1;
                col[1] = vv_aug_float_bits(3.0f * VV_AUG_U(20));
            }
            if (col && VV_AUG_U(6) >= 0.5f) {
                int v = (int)floorf(VV_AUG_U(21) * 41.0f) - 20;
                v = v > 20 ? 20 : v;
                col[0] |= 2;
                col[2] = (v * 180) / 255;
                col[3] = v;
            }
        }
        if (VV_AUG_U(8) < 0.5f) {
            const float t = 0.4f * VV_AUG_U(9);
            s = 0.8f + t;
        }
        if (VV_AUG_U(10) < 0.5f) {
            d_row = vv_aug_randint(VV_AUG_U(11), (int)(0.2f * (float)h));
            d_col = vv_aug_randint(VV_AUG_U(12), (int)(0.2f * (float)w));
        }
    }
#undef VV_AUG_U
    p[0] = idx, p[1] = row0, p[2] = col0, p[3] = h, p[4] = w, p[5] = flip, p[6] = vv_aug_float_bits(s), p[7] = d_row, p[8] = d_col;
    p[9] = inv, p[10] = add[0], p[11] = add[1], p[12] = add[2];
    return 0;
}

VV_AUG_HD int vv_aug_draw_one(const long long *image_meta, int n_images, const int *image_index, const float *boxes, int b, int augmentation,
                              unsigned long long seed, unsigned long long offset, int *p) {
    return vv_aug_draw_pair(image_meta, n_images, image_index, boxes, b, augmentation, seed, offset, p, nullptr);
}

// ---------------------------------------------------------------------------------------------------------------- the host loops
#include <vector>

// every row checked before anything is written -> 0 or -2
inline int vv_aug_check_all(const unsigned char *images, long long images_bytes, const long long *image_meta, int n_images, const int *params,
                            int batch) {
    VvAugSample a;
    for (int b = 0; b < batch; ++b)
        if (vv_aug_sample(images, images_bytes, image_meta, n_images, params + (size_t)b * VV_AUG_WORDS, &a)) return -2;
    return 0;
}

// the 2r+1 normalised weights of 1a (augment.hip deals the taps over threads and sums in the same order)
inline void vv_aug_blur_weights(float sigma, int r, double *w) {
#pragma clang fp contract(off)
    for (int k = -r; k <= r; ++k) w[k + r] = vv_aug_blur_tap(k, sigma);
    double sum = w[0];
    for (int i = 1; i <= 2 * r; ++i) sum = sum + w[i];
    for (int i = 0; i <= 2 * r; ++i) w[i] = w[i] / sum;
}

// the finished source levels (stages 1 .. 4) of one sample into slab[h * w]
inline void vv_aug_colour_fill(const VvAugSample &a, const VvAugColour &c, unsigned *slab) {
#pragma clang fp contract(off)
    const int h = a.h, w = a.w, r = c.r;
    if (r == 0) {
        for (int y = 0; y < h; ++y)
            for (int x = 0; x < w; ++x) slab[(size_t)y * w + x] = vv_aug_finish(a, c, vv_aug_raw(a, y, x));
        return;
    }
    std::vector<double> wt((size_t)(2 * r + 1)), t((size_t)h * w * 3);
    vv_aug_blur_weights(c.sigma, r, wt.data());
    for (int y = 0; y < h; ++y)
        for (int x = 0; x < w; ++x) {
            double *o = &t[((size_t)y * w + x) * 3];
            for (int k = -r; k <= r; ++k) {
                const unsigned p = vv_aug_raw(a, vv_aug_mirror(y + k, h), x);
                for (int ch = 0; ch < 3; ++ch) {
                    const double m = wt[k + r] * (double)((p >> (8 * ch)) & 255u);
                    o[ch] = k == -r ? m : o[ch] + m;
                }
            }
        }
    for (int y = 0; y < h; ++y)
        for (int x = 0; x < w; ++x) {
            double v[3] = {0.0, 0.0, 0.0};
            for (int k = -r; k <= r; ++k) {
                const double *q = &t[((size_t)y * w + vv_aug_mirror(x + k, w)) * 3];
                for (int ch = 0; ch < 3; ++ch) {
                    const double m = wt[k + r] * q[ch];
                    v[ch] = k == -r ? m : v[ch] + m;
                }
            }
            slab[(size_t)y * w + x] = vv_aug_finish(a, c, vv_aug_pack_levels(v));
        }
}

// params and colour rows together (colour may be null): a flagged sample's crop must fit a slab of slab_words words -> 0 or -2
inline int vv_aug_check_all_ex(const unsigned char *images, long long images_bytes, const long long *image_meta, int n_images,
                               const int *params, const int *colour, long long slab_words, int batch) {
    VvAugSample a;
    VvAugColour c;
    for (int b = 0; b < batch; ++b) {
        if (vv_aug_sample(images, images_bytes, image_meta, n_images, params + (size_t)b * VV_AUG_WORDS, &a)) return -2;
        if (!colour) continue;
        if (vv_aug_colour(colour + (size_t)b * VV_AUG_COLOUR_WORDS, &c)) return -2;
        if (c.flags && (long long)a.h * a.w > slab_words) return -2;
    }
    return 0;
}

// out [batch][out_rows][out_cols][3]: per sample the whole warped crop once (h * w words), then the cubic stage out of it.  With a colour
// table a flagged sample b first gets its finished source levels written to slabs + b * slab_words, which the warp then reads.
inline int vv_aug_images_all_ex(const unsigned char *images, long long images_bytes, const long long *image_meta, int n_images,
                                const int *params, const int *colour, unsigned *slabs, long long slab_words, int batch, int out_rows,
                                int out_cols, float *out) {
    if (vv_aug_check_all_ex(images, images_bytes, image_meta, n_images, params, colour, slab_words, batch)) return -2;
    std::vector<unsigned> warped;
    std::vector<VvAugTaps> tx((size_t)out_cols);
    for (int b = 0; b < batch; ++b) {
        VvAugSample a;
        vv_aug_sample(images, images_bytes, image_meta, n_images, params + (size_t)b * VV_AUG_WORDS, &a);
        VvAugSlabSource source{nullptr};
        if (colour) {
            VvAugColour c;
            vv_aug_colour(colour + (size_t)b * VV_AUG_COLOUR_WORDS, &c);
            if (c.flags) {
                unsigned *slab = slabs + (size_t)b * (size_t)slab_words;
                vv_aug_colour_fill(a, c, slab);
                source.slab = slab;
            }
        }
        warped.resize((size_t)a.h * a.w);
        for (int y = 0; y < a.h; ++y)
            for (int x = 0; x < a.w; ++x) warped[(size_t)y * a.w + x] = vv_aug_warp_level(a, y, x, source);
        const double sy = vv_aug_scale(a.h, out_rows), sx = vv_aug_scale(a.w, out_cols);
        for (int ox = 0; ox < out_cols; ++ox) tx[ox] = vv_aug_taps(ox, sx);
        const unsigned *wp = warped.data();
        const int w = a.w;
        for (int oy = 0; oy < out_rows; ++oy) {
            const VvAugTaps ty = vv_aug_taps(oy, sy);
            for (int ox = 0; ox < out_cols; ++ox)
                vv_aug_cubic_pixel(ty, tx[ox], a.h, a.w, [wp, w](int r, int c) { return wp[(size_t)r * w + c]; },
                                   out + (((size_t)b * out_rows + oy) * out_cols + ox) * 3);
        }
    }
    return 0;
}

inline int vv_aug_images_all(const unsigned char *images, long long images_bytes, const long long *image_meta, int n_images, const int *params,
                             int batch, int out_rows, int out_cols, float *out) {
    return vv_aug_images_all_ex(images, images_bytes, image_meta, n_images, params, nullptr, nullptr, 0, batch, out_rows, out_cols, out);
}

// every row is written (an inadmissible one as the refused row); -> 0, or -2 when any row was inadmissible
inline int vv_aug_draw_all(const long long *image_meta, int n_images, const int *image_index, const float *boxes, int batch, int augmentation,
                           unsigned long long seed, unsigned long long offset, int *params) {
    int rc = 0;
    for (int b = 0; b < batch; ++b)
        if (vv_aug_draw_one(image_meta, n_images, image_index, boxes, b, augmentation, seed, offset, params + (size_t)b * VV_AUG_WORDS)) rc = -2;
    return rc;
}

// both tables
inline int vv_aug_draw_all_ex(const long long *image_meta, int n_images, const int *image_index, const float *boxes, int batch,
                              int augmentation, unsigned long long seed, unsigned long long offset, int *params, int *colour) {
    int rc = 0;
    for (int b = 0; b < batch; ++b)
        if (vv_aug_draw_pair(image_meta, n_images, image_index, boxes, b, augmentation, seed, offset, params + (size_t)b * VV_AUG_WORDS,
                             colour + (size_t)b * VV_AUG_COLOUR_WORDS))
            rc = -2;
    return rc;
}
