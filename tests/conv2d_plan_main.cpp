// Stand-alone host program over csrc/conv2d_plan.h (built by tests/test_conv2d_host.py with -fsanitize=address,undefined): walks a
// padded image in a guarded host buffer exactly as conv2d.hip's loader does -- row split, per-(row, tap) validity, tap offset -- and
// checks the sum against a plainly indexed one; then the split-K schedule: shares are non-empty, contiguous and cover every chunk once.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "conv2d_plan.h"

static int fail(const char *what, long a, long b) {
    std::printf("FAIL %s (%ld, %ld)\n", what, a, b);
    return 1;
}

static int walk(int B, int R, int C, int ksize) {
    const long M = (long)B * R * C;
    std::vector<double> x(M);                      // exactly M elements: an out-of-image tap read by address is an ASan report or a wrong sum
    for (long i = 0; i < M; ++i) x[i] = (double)((i * 2654435761u) % 1000) + 1.0;
    for (long m = 0; m < M; ++m) {
        const C2Row rc = c2_row(m, R, C);
        if (rc.b < 0 || rc.b >= B || rc.r < 0 || rc.r >= R || rc.c < 0 || rc.c >= C) return fail("row split range", m, 0);
        if (((long)rc.b * R + rc.r) * C + rc.c != m) return fail("row split inverse", m, 0);
        double got = 0, want = 0;
        for (int tr = 0; tr < ksize; ++tr)
            for (int tc = 0; tc < ksize; ++tc) {
                const int rr = rc.r + tr - ksize / 2, cc = rc.c + tc - ksize / 2;
                const bool in = rr >= 0 && rr < R && cc >= 0 && cc < C;
                if (in != c2_tap_valid(rc.r, rc.c, tr, tc, ksize, R, C)) return fail("tap validity", m, tr * ksize + tc);
                if (in) {
                    want += x[((long)rc.b * R + rr) * C + cc] * (tr * ksize + tc + 1);
                    got += x.at(m + c2_tap_offset(tr, tc, ksize, C)) * (tr * ksize + tc + 1);
                }
            }
        if (got != want) return fail("tap sum", m, 0);
    }
    return 0;
}

static int schedule() {
    for (int kchunks = 1; kchunks <= 300; ++kchunks)
        for (int splits = 1; splits <= kchunks && splits <= C2_MAX_SPLITS; ++splits) {
            int next = 0;
            for (int s = 0; s < splits; ++s) {
                int k0, k1;
                c2_split_range(kchunks, splits, s, &k0, &k1);
                if (k0 != next || k1 <= k0) return fail("split range", kchunks, splits);
                next = k1;
            }
            if (next != kchunks) return fail("split cover", kchunks, splits);
        }
    const int cins[] = {3, 32, 64, 256, 1024}, couts[] = {1, 32, 40, 245, 1024};
    for (int ksize = 1; ksize <= 3; ksize += 2)
        for (int cin : cins)
            for (int cout : couts)
                for (long M = 1; M <= 200000; M = M * 3 + 1)
                    for (long forced = 0; forced <= 40; forced += 8) {
                        const int s = c2_splits(M, ksize, cin, cout, forced), kc = c2_kchunks(ksize, cin);
                        if (s < 1 || s > C2_MAX_SPLITS || s > kc) return fail("splits range", M, s);
                        if (cin == 3 && s != 1) return fail("image layer splits", M, s);
                        if (forced == 0 && s > 1 && kc / s < C2_MIN_CHUNKS) return fail("share too small", M, s);
                    }
    if (c2_splits(169, 3, 1024, 1024, 0) != 11 || c2_splits(72 * 64, 3, 1024, 1024, 0) != 1) return fail("head layer splits", 0, 0);
    if (c2_npad(245) != 256 || c2_npad(64) != 64 || c2_npad(1) != 64 || c2_kchunks(3, 3) != 1 || c2_kchunks(3, 32) != 9) return fail("padding", 0, 0);
    if (c2_extent_ok(1, 65536, 1024, 32, 32) || !c2_extent_ok(1, 65536, 1024, 3, 31) || c2_extent_ok(1 << 20, 1 << 10, 1 << 10, 32, 32) ||
        c2_extent_ok(0, 1, 1, 32, 32) || c2_extent_ok(1, 0x7FFFFFFF, 0x7FFFFFFF, 32, 32))
        return fail("extent", 0, 0);
    return 0;
}

int main() {
    const int grids[][3] = {{2, 5, 7}, {1, 1, 1}, {1, 1, 9}, {3, 13, 13}, {2, 9, 1}, {4, 2, 2}};
    for (const auto &g : grids)
        for (int ksize = 1; ksize <= 3; ksize += 2)
            if (walk(g[0], g[1], g[2], ksize)) return 1;
    if (schedule()) return 1;
    std::printf("OK\n");
    return 0;
}
