// Stand-alone driver for csrc/detect_decode.h under -fsanitize=address,undefined (tests/test_detect_host.py builds and runs it on the
// CPU; it is never loaded into another process).  Seeded frames from an LCG in both layouts, every buffer allocated at exactly the size
// the contract names, so that a read or write one element outside is an error the sanitizer reports.  Prints a checksum per case.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "detect_decode.h"

static uint32_t lcg_state = 12345u;
static uint32_t lcg() { return lcg_state = lcg_state * 1664525u + 1013904223u; }
static float unit() { return (float)(lcg() >> 8) * (1.0f / 16777216.0f); }     // [0, 1)

struct Case {
    int R, C, P, Z, top_1, layout, hostile;
    float obj, iou;
};

static int run(const Case &c) {
    const int W = vv_det_width(c.Z), CH = c.P * W, cells = c.R * c.C, N = cells * (c.top_1 ? 1 : c.P);
    std::vector<float> head((size_t)cells * CH);
    for (int cell = 0; cell < cells; ++cell)
        for (int ch = 0; ch < CH; ++ch) {
            const int f = ch % W;
            float v = unit() * 4.0f - 2.0f;
            if (f == 0) v = unit() < 0.3f ? unit() * 4.0f : -4.0f + unit();
            if (f == 1 || f == 2) v = -2.5f + unit();
            if (c.hostile && (lcg() & 31u) == 0u) {
                const uint32_t pick = lcg() % 5u;
                const uint32_t bits = pick == 0 ? 0x7FC00000u : pick == 1 ? 0x7F800000u : pick == 2 ? 0xFF800000u : pick == 3 ? 0x42C80000u : 0xC2C80000u;
                memcpy(&v, &bits, 4);                                            // NaN, +inf, -inf, 100, -100
            }
            const size_t at = c.layout == VV_DET_NCHW ? (size_t)ch * cells + cell : (size_t)cell * CH + ch;
            head[at] = v;
        }
    std::vector<float> score(N), box((size_t)N * 4), b2((size_t)N * 5), b3((size_t)N * 3), mean((size_t)N * c.Z), lv((size_t)N * c.Z),
        sn((size_t)N * 3), cs((size_t)N * 3), rad((size_t)N * 3);
    std::vector<int> cand(N), order(N), index(N);
    std::vector<unsigned char> live(N);
    const VvDetFrame f = vv_det_frame(head.data(), c.layout, 0, cells, CH);
    const int count = vv_det_frame_host(f, c.R, c.C, c.P, c.Z, c.obj, c.iou, c.top_1, score.data(), box.data(), cand.data(), order.data(),
                                        live.data(), index.data(), b2.data(), b3.data(), mean.data(), lv.data(), sn.data(), cs.data(),
                                        rad.data());
    if (count < 0 || count > N) return 1;
    uint32_t sum = (uint32_t)count;
    for (int r = 0; r < count; ++r) {
        if (index[r] < 0 || index[r] >= cells * c.P) return 2;
        uint32_t bits;
        memcpy(&bits, &b2[(size_t)r * 5 + 4], 4);
        sum = sum * 31u + (uint32_t)index[r] + bits;
    }
    printf("%dx%d P %d Z %d top_1 %d layout %d hostile %d: %d of %d slots, checksum %08x\n", c.R, c.C, c.P, c.Z, c.top_1, c.layout, c.hostile,
           count, N, sum);
    return 0;
}

int main() {
    const Case cases[] = {
        {1, 1, 5, 16, 1, 0, 0, 0.5f, 0.5f},  {3, 5, 5, 16, 0, 0, 0, 0.5f, 0.5f},   {3, 5, 5, 16, 0, 1, 0, 0.5f, 0.5f},
        {13, 13, 5, 16, 1, 1, 0, 0.3f, 0.4f}, {11, 38, 5, 16, 0, 0, 0, 0.5f, 0.5f}, {2, 2, 16, 64, 0, 1, 0, 0.5f, 0.5f},
        {7, 3, 1, 1, 0, 0, 0, 0.5f, 0.5f},   {6, 9, 5, 16, 0, 0, 1, 0.5f, 0.5f},   {6, 9, 5, 16, 1, 1, 1, 0.7f, 0.2f},
        {16, 16, 16, 3, 0, 0, 1, 0.0f, 0.0f},
    };
    // the activations over a sweep of bit patterns: every exponent, both signs
    uint32_t acc = 0;
    for (uint32_t u = 0; u < 0xFFFFFFFFu - 65521u; u += 65521u) {
        float x, y[3];
        memcpy(&x, &u, 4);
        y[0] = vv_det_exp(x), y[1] = vv_det_sigmoid(x), y[2] = vv_det_tanh(x);
        uint32_t b[3];
        memcpy(b, y, 12);
        acc = acc * 31u + b[0] + b[1] + b[2];
    }
    printf("activation sweep checksum %08x\n", acc);
    for (const Case &c : cases) {
        const int rc = run(c);
        if (rc) {
            printf("FAILED %d\n", rc);
            return rc;
        }
    }
    printf("OK\n");
    return 0;
}
