// Stand-alone driver for the colour stages of csrc/augment.h (1a blur, 1b hue/saturation, the colour draws) under
// -fsanitize=address,undefined (tests/test_augment_colour_host.py builds and runs it on the CPU; it is never loaded into another
// process).  Seeded images from an LCG; the image, both tables, the output and the slabs are allocated at exactly the size the
// contract names, so that a read or write one element outside is an error the sanitizer reports.  Prints a checksum per case.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "augment.h"

static uint32_t lcg_state = 13579u;
static uint32_t lcg() { return lcg_state = lcg_state * 1664525u + 1013904223u; }

struct Case {
    int rows, cols, row0, col0, h, w, flip;
    float s;
    int d_row, d_col, inv, add0, add1, add2, row_pad, col_pad, out_rows, out_cols;
    int flags;
    float sigma;
    int hue, sat;
};

static int run(const Case &c) {
    std::vector<unsigned char> img((size_t)c.rows * c.cols * 3);
    for (unsigned char &v : img) v = (unsigned char)(lcg() >> 24);
    const long long meta[3] = {0, c.rows, c.cols};
    const int p[VV_AUG_WORDS] = {0,       c.row0,  c.col0, c.h,    c.w,    c.flip,    vv_aug_float_bits(c.s), c.d_row,
                                 c.d_col, c.inv,   c.add0, c.add1, c.add2, c.row_pad, c.col_pad,              0};
    const int col[VV_AUG_COLOUR_WORDS] = {c.flags, vv_aug_float_bits(c.sigma), c.hue, c.sat};
    std::vector<float> out((size_t)c.out_rows * c.out_cols * 3);
    std::vector<unsigned> slab((size_t)c.h * c.w);                       // exactly full
    const int rc = vv_aug_images_all_ex(img.data(), (long long)img.size(), meta, 1, p, col, slab.data(), (long long)slab.size(), 1, c.out_rows,
                                        c.out_cols, out.data());
    if (rc) return 1;
    uint32_t sum = 0;
    for (float v : out) {
        if (!(v >= 0.0f && v <= 1.0f)) return 2;
        uint32_t bits;
        memcpy(&bits, &v, 4);
        sum = sum * 31u + bits;
    }
    // the direct form of the blur gives the two-pass form's bits
    VvAugSample a;
    VvAugColour cc;
    if (vv_aug_sample(img.data(), (long long)img.size(), meta, 1, p, &a) || vv_aug_colour(col, &cc)) return 3;
    if (cc.r > 0 && (long long)c.h * c.w * (2 * cc.r + 1) <= 40000) {
        std::vector<double> wt((size_t)(2 * cc.r + 1));
        vv_aug_blur_weights(cc.sigma, cc.r, wt.data());
        for (int y = 0; y < a.h; ++y)
            for (int x = 0; x < a.w; ++x) {
                const unsigned d = vv_aug_blur_direct(a.h, a.w, cc.r, wt.data(), y, x, [&a](int yy, int xx) { return vv_aug_raw(a, yy, xx); });
                if (vv_aug_finish(a, cc, d) != slab[(size_t)y * a.w + x]) return 4;
            }
    }
    printf("%dx%d crop %dx%d flags %d sigma %.3f (r %d) hue %d sat %d -> %dx%d: checksum %08x\n", c.rows, c.cols, c.h, c.w, c.flags,
           (double)c.sigma, cc.r, c.hue, c.sat, c.out_rows, c.out_cols, sum);
    return 0;
}

static int all_colours() {
    // every hue and saturation add at the ends of their ranges over a ramp of colours: the table index and every conversion stay defined
    uint32_t sum = 0;
    for (int r = 0; r < 256; r += 5)
        for (int g = 0; g < 256; g += 15)
            for (int b = 0; b < 256; b += 17) {
                const unsigned px = (unsigned)r | (unsigned)g << 8 | (unsigned)b << 16;
                const int hs[][2] = {{0, 0}, {179, 255}, {-179, -255}, {14, 20}, {-14, -20}, {90, -1}};
                for (const auto &k : hs) {
                    const unsigned o = vv_aug_hue_sat(px, k[0], k[1]);
                    if (o >> 24) return 5;
                    sum = sum * 31u + o;
                }
            }
    printf("hue/saturation over the colour ramp: checksum %08x\n", sum);
    return 0;
}

static int draws() {
    const long long meta[6] = {0, 40, 60, 7200, 7, 9};
    const int n = 257;
    std::vector<int> index(n), params((size_t)n * VV_AUG_WORDS), colour((size_t)n * VV_AUG_COLOUR_WORDS), plain((size_t)n * VV_AUG_WORDS);
    std::vector<float> boxes((size_t)n * 4);
    for (int b = 0; b < n; ++b) {
        index[b] = b & 1;
        const float cols = (float)meta[3 * index[b] + 2], rows = (float)meta[3 * index[b] + 1];
        boxes[4 * b + 0] = 0.25f * cols * (float)(lcg() >> 8) / 16777216.0f;
        boxes[4 * b + 1] = 0.25f * rows * (float)(lcg() >> 8) / 16777216.0f;
        boxes[4 * b + 2] = boxes[4 * b + 0] + 2.5f + 0.5f * cols * (float)(lcg() >> 8) / 16777216.0f;
        boxes[4 * b + 3] = boxes[4 * b + 1] + 2.5f + 0.5f * rows * (float)(lcg() >> 8) / 16777216.0f;
    }
    for (int aug = 0; aug < 2; ++aug) {
        if (vv_aug_draw_all_ex(meta, 2, index.data(), boxes.data(), n, aug, 0x123456789ABCDEFull, 7ull << 40 | 3ull, params.data(), colour.data()))
            return 6;
        if (vv_aug_draw_all(meta, 2, index.data(), boxes.data(), n, aug, 0x123456789ABCDEFull, 7ull << 40 | 3ull, plain.data())) return 7;
        if (params != plain) return 8;
        if (vv_aug_check_all_ex(nullptr, -1, meta, 2, params.data(), colour.data(), 60 * 40, n)) return 9;
        uint32_t sum = 0;
        for (int v : colour) sum = sum * 31u + (uint32_t)v;
        printf("colour draws augmentation %d: checksum %08x\n", aug, sum);
    }
    return 0;
}

int main() {
    const Case cases[] = {
        {9, 13, 0, 0, 9, 13, 0, 1.0f, 0, 0, 0, 0, 0, 0, 0, 0, 9, 13, 1, 3.0f, 0, 0},            // radius 12 on a 9 x 13 crop: reflects twice
        {1, 1, 0, 0, 1, 1, 0, 1.0f, 0, 0, 7, -3, 4, 0, 0, 0, 3, 2, 3, 1.3f, 5, -5},             // one pixel: mirror(i, 1) = 0
        {2, 5, 0, 0, 2, 5, 3, 1.2f, -1, 2, 5, 10, -10, 3, 0, 0, 8, 8, 3, 3.0f, -14, -20},
        {5, 6, 2, 4, 9, 8, 1, 0.9f, 1, 1, 2, 0, 0, 0, 3, 3, 4, 5, 3, 0.9f, 14, 20},             // a pad of 3 under the blur
        {37, 53, 0, 0, 37, 53, 2, 0.8f, 3, -5, 0, 0, 0, 0, 0, 0, 16, 24, 1, 2.1f, 0, 0},
        {37, 53, 0, 0, 37, 53, 0, 1.0f, 0, 0, 0, 0, 0, 0, 0, 0, 16, 24, 2, 0.0f, 179, 255},     // hue/saturation alone
        {7, 3, 0, 0, 7, 3, 0, 1.0f, 0, 0, 0, 0, 0, 0, 0, 0, 7, 3, 1, 16.0f, 0, 0},              // the largest sigma: radius 64
        {7, 3, 0, 0, 7, 3, 0, 1.0f, 0, 0, 0, 0, 0, 0, 0, 0, 7, 3, 1, 0.1f, 0, 0},               // radius 0 under the blur flag
        {7, 3, 0, 0, 7, 3, 0, 1.0f, 0, 0, 1, 2, 3, 4, 0, 0, 7, 3, 0, 0.0f, 0, 0},               // no flag: the slab is not touched
    };
    for (const Case &c : cases) {
        const int rc = run(c);
        if (rc) {
            printf("FAILED %d\n", rc);
            return rc;
        }
    }
    // refusals: nothing is written, neither the output nor the slab
    {
        const unsigned char img[12] = {0};
        const long long meta[3] = {0, 2, 2};
        const int p[VV_AUG_WORDS] = {0, 0, 0, 2, 2, 0, vv_aug_float_bits(1.0f), 0, 0, 0, 0, 0, 0, 0, 0, 0};
        float out[3] = {-7.0f, -7.0f, -7.0f};
        unsigned slab[4] = {9u, 9u, 9u, 9u};
        const int bad[][VV_AUG_COLOUR_WORDS] = {{4, 0, 0, 0}, {1, vv_aug_float_bits(-1.0f), 0, 0}, {1, 0x7FC00000, 0, 0},
                                                {1, vv_aug_float_bits(16.5f), 0, 0}, {2, 0, 180, 0}, {2, 0, 0, -256}};
        for (const auto &c : bad)
            if (vv_aug_images_all_ex(img, 12, meta, 1, p, c, slab, 4, 1, 1, 1, out) != -2 || out[0] != -7.0f || slab[0] != 9u) return 10;
        const int ok[VV_AUG_COLOUR_WORDS] = {3, vv_aug_float_bits(1.0f), 3, 3};
        if (vv_aug_images_all_ex(img, 12, meta, 1, p, ok, slab, 3, 1, 1, 1, out) != -2 || out[0] != -7.0f || slab[0] != 9u) return 11;   // one word short
        if (vv_aug_images_all_ex(img, 12, meta, 1, p, ok, slab, 4, 1, 1, 1, out) != 0) return 12;
    }
    int rc = all_colours();
    if (!rc) rc = draws();
    if (rc) {
        printf("FAILED %d\n", rc);
        return rc;
    }
    printf("OK\n");
    return 0;
}
