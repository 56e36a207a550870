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
// 1. source level (integer, exact).  Crop pixel (y, x), channel c: fx = bit 0 ? w - 1 - x : x, fy = bit 1 ? h - 1 - y : y; the padded
//    image at (row0 + fy, col0 + fx) is the image's byte, or 0 in the border; v = invert bit c ? 255 - v : v; v = min(max(v + add_c, 0), 255)
//    (imgaug Invert, then Add, the Sequential order of datasetUtils.py:64-89).  Outside the crop (y or x out of range) the level is 0:
//    warpAffine's constant border.
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
//   slot 4  GaussianBlur chosen: u >= 0.5   (NOT APPLIED)  slot 13..15  invert channel 0..2: u < 0.05
//   slot 5  brightness (Add) chosen: u >= 0.5              slot 16  Add per_channel gate: u < 0.5
//   slot 6  hue/saturation chosen: u >= 0.5 (NOT APPLIED)  slot 17..19  Add value (int)floorf(u * 21.0f) - 10; without the gate slot 17's
//   slot 7  channel invert chosen: u >= 0.5                         value serves all three channels
//   slot 8  scale gate (scalePr): u < 0.5                  slot 20  blur sigma, slot 21 hue/saturation value: reserved, NOT APPLIED
// m = 0 gives d = 0 (the reference's randint(0, 0) raises and its bare except drops the object).  The crop is the reference's:
// width = colMax - colMin;  cMin = max(0, colMin - width * border);  cMax = min(cols, colMax + width * border);  col0 = (int)cMin,
// w = (int)cMax - col0 (rows likewise), float32, products rounded before the sums.  augmentation = 0: border 0.1f, no flip, s = 1, d = 0,
// no colour change.  rowPad = colPad = 0.
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

// M^-1 along one axis: destination coordinate d -> source coordinate (extent n, translation t, scale s)
VV_AUG_HD double vv_aug_inverse(int d, int n, int t, float s) {
#pragma clang fp contract(off)
    const double half = (double)n * 0.5;
    const double u = (double)(d - t) - half;
    const double q = u / (double)s;
    return q + half;
}

// step 2: the three warped levels of destination pixel (y, x) of the crop, packed as vv_aug_source packs them
VV_AUG_HD unsigned vv_aug_warp_level(const VvAugSample &a, int y, int x) {
#pragma clang fp contract(off)
    const double sx = vv_aug_inverse(x, a.w, a.d_col, a.s), sy = vv_aug_inverse(y, a.h, a.d_row, a.s);
    if (!(sx >= -1.0) || !(sy >= -1.0) || !(sx < (double)a.w) || !(sy < (double)a.h)) return 0u;
    const double fx0 = floor(sx), fy0 = floor(sy);
    const double ax = sx - fx0, ay = sy - fy0;
    const double bx = 1.0 - ax, by = 1.0 - ay;
    const int x0 = (int)fx0, y0 = (int)fy0;                              // -1 .. extent-1
    const unsigned p00 = vv_aug_source(a, y0, x0), p01 = vv_aug_source(a, y0, x0 + 1);
    const unsigned p10 = vv_aug_source(a, y0 + 1, x0), p11 = vv_aug_source(a, y0 + 1, x0 + 1);
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
VV_AUG_HD int vv_aug_draw_one(const long long *image_meta, int n_images, const int *image_index, const float *boxes, int b, int augmentation,
                              unsigned long long seed, unsigned long long offset, int *p) {
#pragma clang fp contract(off)
    for (int k = 0; k < VV_AUG_WORDS; ++k) p[k] = 0;
    p[0] = -1;
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

// out [batch][out_rows][out_cols][3]: per sample the whole warped crop once (h * w words), then the cubic stage out of it
inline int vv_aug_images_all(const unsigned char *images, long long images_bytes, const long long *image_meta, int n_images, const int *params,
                             int batch, int out_rows, int out_cols, float *out) {
    if (vv_aug_check_all(images, images_bytes, image_meta, n_images, params, batch)) return -2;
    std::vector<unsigned> warped;
    std::vector<VvAugTaps> tx((size_t)out_cols);
    for (int b = 0; b < batch; ++b) {
        VvAugSample a;
        vv_aug_sample(images, images_bytes, image_meta, n_images, params + (size_t)b * VV_AUG_WORDS, &a);
        warped.resize((size_t)a.h * a.w);
        for (int y = 0; y < a.h; ++y)
            for (int x = 0; x < a.w; ++x) warped[(size_t)y * a.w + x] = vv_aug_warp_level(a, y, x);
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

// every row is written (an inadmissible one as the refused row); -> 0, or -2 when any row was inadmissible
inline int vv_aug_draw_all(const long long *image_meta, int n_images, const int *image_index, const float *boxes, int batch, int augmentation,
                           unsigned long long seed, unsigned long long offset, int *params) {
    int rc = 0;
    for (int b = 0; b < batch; ++b)
        if (vv_aug_draw_one(image_meta, n_images, image_index, boxes, b, augmentation, seed, offset, params + (size_t)b * VV_AUG_WORDS)) rc = -2;
    return rc;
}
