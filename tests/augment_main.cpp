// Stand-alone driver for csrc/augment.h under -fsanitize=address,undefined (tests/test_augment_host.py builds and runs it on the CPU; it
// is never loaded into another process).  Seeded images from an LCG, every buffer allocated at exactly the size the contract names, so
// that a read or write one element outside is an error the sanitizer reports.  Prints a checksum per case.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "augment.h"

static uint32_t lcg_state = 2468u;
static uint32_t lcg() { return lcg_state = lcg_state * 1664525u + 1013904223u; }

struct Case {
    int rows, cols, row0, col0, h, w, flip;
    float s;
    int d_row, d_col, inv, add0, add1, add2, row_pad, col_pad, out_rows, out_cols;
};

static int run(const Case &c) {
    std::vector<unsigned char> img((size_t)c.rows * c.cols * 3);
    for (unsigned char &v : img) v = (unsigned char)(lcg() >> 24);
    const long long meta[3] = {0, c.rows, c.cols};
    const int p[VV_AUG_WORDS] = {0,       c.row0,  c.col0, c.h,    c.w,    c.flip,    vv_aug_float_bits(c.s), c.d_row,
                                 c.d_col, c.inv,   c.add0, c.add1, c.add2, c.row_pad, c.col_pad,              0};
    std::vector<float> out((size_t)c.out_rows * c.out_cols * 3);
    const int rc = vv_aug_images_all(img.data(), (long long)img.size(), meta, 1, p, 1, c.out_rows, c.out_cols, out.data());
    if (rc) return 1;
    uint32_t sum = 0;
    for (float v : out) {
        if (!(v >= 0.0f && v <= 1.0f)) return 2;
        uint32_t bits;
        memcpy(&bits, &v, 4);
        sum = sum * 31u + bits;
    }
    printf("%dx%d crop %d,%d %dx%d pad %d,%d flip %d s %.2f d %d,%d -> %dx%d: checksum %08x\n", c.rows, c.cols, c.row0, c.col0, c.h, c.w,
           c.row_pad, c.col_pad, c.flip, (double)c.s, c.d_row, c.d_col, c.out_rows, c.out_cols, sum);
    return 0;
}

static int draws() {
    const long long meta[6] = {0, 40, 60, 7200, 7, 9};
    const int n = 257;
    std::vector<int> index(n), params((size_t)n * VV_AUG_WORDS);
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
        if (vv_aug_draw_all(meta, 2, index.data(), boxes.data(), n, aug, 0x123456789ABCDEFull, 7ull << 40 | 3ull, params.data())) return 3;
        if (vv_aug_check_all(nullptr, -1, meta, 2, params.data(), n)) return 4;
        uint32_t sum = 0;
        for (int v : params) sum = sum * 31u + (uint32_t)v;
        printf("draws augmentation %d: checksum %08x\n", aug, sum);
    }
    // hostile boxes: NaN, infinities, inverted and far outside -- every conversion stays defined, the rows are refused or inside
    const uint32_t bits[] = {0x7FC00000u, 0x7F800000u, 0xFF800000u, 0x4E6E6B28u, 0xCE6E6B28u, 0x00000000u};
    int refused = 0;
    for (int k = 0; k < 6 * 6; ++k) {
        float bx[4] = {1.0f, 1.0f, 5.0f, 5.0f};
        memcpy(&bx[k % 4], &bits[k % 6], 4);
        memcpy(&bx[(k / 6) % 4], &bits[k / 6], 4);
        const int one = 0;
        int row[VV_AUG_WORDS];
        if (vv_aug_draw_all(meta, 2, &one, bx, 1, 1, 99ull, (unsigned long long)k, row))
            ++refused;
        else if (vv_aug_check_all(nullptr, -1, meta, 2, row, 1))
            return 5;
    }
    printf("hostile boxes: %d of 36 refused\n", refused);
    return 0;
}

int main() {
    const Case cases[] = {
        {9, 13, 0, 0, 9, 13, 0, 1.0f, 0, 0, 0, 0, 0, 0, 0, 0, 9, 13},           // identity
        {5, 7, 0, 0, 5, 7, 0, 0.8f, 1, -2, 0, 0, 0, 0, 0, 0, 8, 8},             // every tap clamped
        {5, 7, 0, 0, 5, 7, 3, 1.2f, -1, 2, 5, 10, -10, 3, 0, 0, 8, 8},
        {5, 6, 0, 0, 11, 12, 0, 1.0f, 0, 0, 0, 0, 0, 0, 3, 3, 11, 12},          // a pad of 3
        {5, 6, 2, 4, 9, 8, 1, 0.9f, 1, 1, 2, 0, 0, 0, 3, 3, 4, 5},
        {37, 53, 0, 0, 37, 53, 2, 0.8f, 3, -5, 0, 0, 0, 0, 0, 0, 16, 24},
        {1, 1, 0, 0, 1, 1, 0, 1.0f, 0, 0, 7, -3, 4, 0, 0, 0, 3, 2},             // one pixel
        {4, 4, 0, 0, 4, 4, 0, 1.0e-30f, 0, 0, 0, 0, 0, 0, 0, 0, 2, 2},          // a scale whose quotient overflows: all border
        {4, 4, 0, 0, 4, 4, 0, 1.0e30f, 2, -2, 0, 0, 0, 0, 0, 0, 2, 2},
        {6, 6, 0, 0, 6, 6, 0, 1.0f, 32767, -32767, 0, 0, 0, 0, 0, 0, 3, 3},     // the largest translations
    };
    for (const Case &c : cases) {
        const int rc = run(c);
        if (rc) {
            printf("FAILED %d\n", rc);
            return rc;
        }
    }
    // refusals: nothing is written
    {
        const unsigned char img[12] = {0};
        const long long meta[3] = {0, 2, 2};
        int p[VV_AUG_WORDS] = {0, 0, 0, 3, 2, 0, vv_aug_float_bits(1.0f), 0, 0, 0, 0, 0, 0, 0, 0, 0};
        float out[3] = {-7.0f, -7.0f, -7.0f};
        if (vv_aug_images_all(img, 12, meta, 1, p, 1, 1, 1, out) != -2 || out[0] != -7.0f) return 6;
        p[3] = 2, p[0] = 1;
        if (vv_aug_images_all(img, 12, meta, 1, p, 1, 1, 1, out) != -2 || out[0] != -7.0f) return 7;
        p[0] = 0;
        if (vv_aug_images_all(img, 11, meta, 1, p, 1, 1, 1, out) != -2) return 8;       // the table leaves the arena
        if (vv_aug_images_all(img, 12, meta, 1, p, 1, 1, 1, out) != 0) return 9;
    }
    const int rc = draws();
    if (rc) {
        printf("FAILED %d\n", rc);
        return rc;
    }
    printf("OK\n");
    return 0;
}
