// Stand-alone host program over the strided part of csrc/conv2d_plan.h (built by tests/test_darknet53_host.py with
// -fsanitize=address,undefined): walks exactly-sized host buffers as conv2d.hip's loader does at stride 1 and 2 -- the row split over the
// OUTPUT grid, the per-(row, tap) predicate c2_ex_tap_valid, the pixel c2_ex_tap_pixel -- and checks the sum against a plainly indexed
// one; then the stride-1 pool's window (c2_pool1_last) the same way, and the extents the entries admit.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "conv2d_plan.h"

static int fail(const char *what, long a, long b) {
    std::printf("FAIL %s (%ld, %ld)\n", what, a, b);
    return 1;
}

static int walk(int B, int R, int C, int ksize, int stride) {
    const long Min = (long)B * R * C;
    const int Ro = c2_out_extent(R, stride), Co = c2_out_extent(C, stride);
    if (Ro != (stride == 2 ? R / 2 : R) || Co != (stride == 2 ? C / 2 : C)) return fail("output grid", Ro, Co);
    const long M = (long)B * Ro * Co;
    std::vector<double> x(Min);                    // exactly the input: a tap decided by address is an ASan report or a wrong sum
    std::vector<char> read(Min, 0);
    for (long i = 0; i < Min; ++i) x[i] = (double)((i * 2654435761u) % 1000) + 1.0;
    for (long m = 0; m < M; ++m) {
        const C2Row rc = c2_row(m, Ro, Co);
        if (rc.b < 0 || rc.b >= B || rc.r < 0 || rc.r >= Ro || rc.c < 0 || rc.c >= Co) return fail("row split range", m, 0);
        const long origin = c2_ex_tap_pixel(rc.b, rc.r, rc.c, ksize / 2, ksize / 2, ksize, stride, R, C);     // what the kernel keeps per row
        double got = 0, want = 0;
        for (int tr = 0; tr < ksize; ++tr)
            for (int tc = 0; tc < ksize; ++tc) {
                const int rr = rc.r * stride + tr - ksize / 2, cc = rc.c * stride + tc - ksize / 2;
                const bool in = rr >= 0 && rr < R && cc >= 0 && cc < C;
                if (in != c2_ex_tap_valid(rc.r, rc.c, tr, tc, ksize, stride, R, C)) return fail("tap validity", m, tr * ksize + tc);
                if (stride == 1 && in != c2_tap_valid(rc.r, rc.c, tr, tc, ksize, R, C)) return fail("stride 1 is the old predicate", m, tr * ksize + tc);
                if (!in) continue;
                const long pixel = c2_ex_tap_pixel(rc.b, rc.r, rc.c, tr, tc, ksize, stride, R, C);
                if (pixel != origin + c2_tap_offset(tr, tc, ksize, C)) return fail("origin + offset", m, tr * ksize + tc);
                if (stride == 1 && pixel != m + c2_tap_offset(tr, tc, ksize, C)) return fail("stride 1 is the old offset", m, tr * ksize + tc);
                want += x[((long)rc.b * R + rr) * C + cc] * (tr * ksize + tc + 1);
                got += x.at(pixel) * (tr * ksize + tc + 1);
                read[pixel] = 1;
            }
        if (got != want) return fail("tap sum", m, 0);
    }
    // stride 2 never reads the last row / column of an odd size, and reads everything else
    if (stride == 2 && ksize == 3)
        for (int b = 0; b < B; ++b)
            for (int r = 0; r < R; ++r)
                for (int c = 0; c < C; ++c) {
                    const bool expect = r <= 2 * Ro - 1 && c <= 2 * Co - 1;
                    if ((bool)read[((long)b * R + r) * C + c] != expect) return fail("pixels read", r, c);
                }
    return 0;
}

static int pool1(int B, int R, int C) {
    const long M = (long)B * R * C;
    std::vector<double> x(M);
    for (long i = 0; i < M; ++i) x[i] = -(double)((i * 2654435761u) % 1000) - 1.0;          // all negative: a zero pad would win
    for (long m = 0; m < M; ++m) {
        const C2Row rc = c2_row(m, R, C);
        const int r1 = c2_pool1_last(rc.r, R), c1 = c2_pool1_last(rc.c, C);
        if (r1 < rc.r || r1 > rc.r + 1 || r1 >= R || c1 < rc.c || c1 > rc.c + 1 || c1 >= C) return fail("pool window", m, 0);
        if ((r1 == rc.r) != (rc.r == R - 1) || (c1 == rc.c) != (rc.c == C - 1)) return fail("pool clip", m, 0);
        const long img = (long)rc.b * R * C;
        double got = x.at(img + (long)rc.r * C + rc.c);
        const long idx[3] = {img + (long)rc.r * C + c1, img + (long)r1 * C + rc.c, img + (long)r1 * C + c1};
        for (long i : idx) got = x.at(i) > got ? x.at(i) : got;
        double want = -1e300;
        for (int dr = 0; dr < 2; ++dr)
            for (int dc = 0; dc < 2; ++dc)
                if (rc.r + dr < R && rc.c + dc < C) {
                    const double v = x[img + (long)(rc.r + dr) * C + rc.c + dc];
                    want = v > want ? v : want;
                }
        if (got != want) return fail("pool max", m, 0);
    }
    return 0;
}

static int shapes() {
    if (!c2_ex_shape_ok(3, 2, 32, 64) || !c2_ex_shape_ok(3, 1, 3, 16) || !c2_ex_shape_ok(1, 1, 64, 40)) return fail("shape admitted", 0, 0);
    if (c2_ex_shape_ok(1, 2, 32, 64) || c2_ex_shape_ok(3, 2, 3, 32) || c2_ex_shape_ok(3, 0, 32, 32) || c2_ex_shape_ok(3, 3, 32, 32) ||
        c2_ex_shape_ok(3, 2, 16, 32) || c2_ex_shape_ok(3, 2, 48, 32) || c2_ex_shape_ok(3, -1, 32, 32))
        return fail("shape refused", 0, 0);
    if (c2_ex_extent_ok(1, 1, 8, 2, 32, 32) || c2_ex_extent_ok(1, 8, 1, 2, 32, 32) || !c2_ex_extent_ok(1, 2, 2, 2, 32, 32)) return fail("extent rows", 0, 0);
    // 65536 x 1024 x 32 = 2^31 elements: the INPUT is past the limit at either stride; at stride 2 a 2x wider output on a quarter of the
    // pixels is not
    if (c2_ex_extent_ok(1, 65536, 1024, 2, 32, 32) || c2_ex_extent_ok(1, 65536, 1024, 1, 32, 32)) return fail("extent input", 0, 0);
    if (!c2_ex_extent_ok(1, 32768, 1024, 2, 32, 64) || c2_ex_extent_ok(1, 32768, 1024, 1, 32, 64)) return fail("extent output", 0, 0);
    if (c2_ex_extent_ok(1, 1, 1, 1, 32, 32) != c2_extent_ok(1, 1, 1, 32, 32) || c2_ex_extent_ok(0, 4, 4, 2, 32, 32)) return fail("extent stride 1", 0, 0);
    return 0;
}

int main() {
    const int grids[][3] = {{1, 2, 2}, {1, 3, 5}, {2, 5, 7}, {1, 2, 9}, {2, 13, 13}, {3, 4, 6}, {2, 9, 2}};
    for (const auto &g : grids) {
        if (walk(g[0], g[1], g[2], 3, 2)) return 1;
        if (walk(g[0], g[1], g[2], 3, 1) || walk(g[0], g[1], g[2], 1, 1)) return 1;
        if (pool1(g[0], g[1], g[2])) return 1;
    }
    if (pool1(1, 1, 1) || pool1(1, 1, 9) || pool1(2, 9, 1)) return 1;
    if (shapes()) return 1;
    std::printf("OK\n");
    return 0;
}
