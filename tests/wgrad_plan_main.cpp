// Stand-alone host program over csrc/wgrad_plan.h (built by tests/test_wgrad_plan_host.py with -fsanitize=address,undefined).
//   no argument:  walks dense and stride-2 shapes through the routes and checks that every chosen plan covers its rows with non-empty
//                 splits and that its slabs fit what vv_wgrad_workspace_bytes promises for the same shape; prints OK.
//   <cases file>: one case per line, one answer per line: `<form> <splits> <reduce>` or `refused`
//                 d <rows> <m> <n> <lda> <a dtype> <g dtype> <a aligned> <g aligned> <f32 only>
//                 c <batch> <side> <cin> <cout> <src dtype> <g dtype> <src aligned> <g aligned> <f32 only> <no phase>
//                 (dtype 0 = float32, 1 = bf16; the shapes are ones the entries accept)
#include <cstdio>
#include <cstdlib>

#include "wgrad_plan.h"

static const char *form_name(const WgradRoute &r, int n) {
    switch (r.form) {
    case WG_PHASE: return "PHASE";
    case WG_BF16_TAPS: return "BF16_TAPS";
    case WG_BF16_GRID: return wgrad_grid_one_tile(n) ? "BF16_GRID_ONE" : "BF16_GRID";
    case WG_BF16_DENSE: return "BF16_DENSE";
    default: return "F32";
    }
}
static const char *reduce_name(WgradReduce k) { return k == WG_REDUCE_NONE ? "none" : (k == WG_REDUCE_SLICED ? "sliced" : "plain"); }

static int fail(const char *what, long a, long b, long c) {
    std::printf("FAIL %s (%ld, %ld, %ld)\n", what, a, b, c);
    return 1;
}

static int check(const WgradRoute &r, long rows, int m, int n) {
    const long unit = r.form == WG_PHASE ? 128 : 1;                        // the phase plan counts boxes of 128 rows
    const long units = (rows + unit - 1) / unit;
    if (r.plan.splits < 1 || r.plan.rps < 1) return fail("empty plan", rows, m, n);
    if ((long)r.plan.splits * r.plan.rps < units) return fail("rows not covered", rows, m, n);
    if ((long)(r.plan.splits - 1) * r.plan.rps >= units) return fail("empty last split", rows, m, n);
    if (r.plan.ws > wgrad_workspace_bytes(rows, m, n)) return fail("slabs beyond the workspace", rows, m, n);
    if (r.plan.ws != (size_t)r.plan.splits * m * n * sizeof(float)) return fail("slab bytes", rows, m, n);
    if (r.reduce == WG_REDUCE_NONE && r.plan.splits != 1) return fail("several slabs without a reduce", rows, m, n);
    return 0;
}

static int self_check() {
    const int ms[] = {4, 36, 64, 160, 4096, 8192}, ns[] = {4, 20, 32, 64, 96, 128, 512}, cins[] = {1, 64, 128, 192, 256};
    long count = 0;
    for (long rows = 1; rows <= (1L << 20); rows = rows * 3 / 2 + 1)
        for (int m : ms)
            for (int n : ns)
                for (int dt = 0; dt < 4; ++dt)
                    for (int f32 = 0; f32 < 2; ++f32, ++count)
                        if (check(wgrad_dense_route(rows, m, n, m + 8 * (dt & 1), dt & 1, dt >> 1, true, true, f32 != 0), rows, m, n)) return 1;
    for (int side = 2; side <= 64; side *= 2)
        for (int batch = 1; (long)batch * (side / 2) * (side / 2) * (side / 2) <= (1L << 20); batch = batch * 3 / 2 + 1)
            for (int cin : cins)
                for (int cout : ns)
                    for (int dt = 0; dt < 4; ++dt)
                        for (int ov = 0; ov < 3; ++ov, ++count) {
                            if (!wgrad_conv_src_dtype_ok(cin, dt & 1)) continue;
                            const long rows = (long)batch * (side / 2) * (side / 2) * (side / 2);
                            if (check(wgrad_conv_route(batch, side, cin, cout, dt & 1, dt >> 1, true, true, ov == 1, ov == 2), rows, 64 * cin, cout))
                                return 1;
                        }
    return count > 10000 ? 0 : fail("walk too short", count, 0, 0);
}

static int answer(const char *path) {
    std::FILE *f = std::fopen(path, "r");
    if (!f) return fail("cannot open the cases file", 0, 0, 0);
    char kind;
    while (std::fscanf(f, " %c", &kind) == 1) {
        long v[10];
        const int want = kind == 'd' ? 9 : 10;
        for (int i = 0; i < want; ++i)
            if (std::fscanf(f, "%ld", &v[i]) != 1) return fail("short case", i, 0, 0);
        if (kind == 'd') {
            const WgradRoute r = wgrad_dense_route(v[0], (int)v[1], (int)v[2], (int)v[3], (int)v[4], (int)v[5], v[6] != 0, v[7] != 0, v[8] != 0);
            std::printf("%s %d %s\n", form_name(r, (int)v[2]), r.plan.splits, reduce_name(r.reduce));
        } else if (kind == 'c') {
            if (!wgrad_conv_src_dtype_ok((int)v[2], (int)v[4])) {
                std::printf("refused\n");
                continue;
            }
            const WgradRoute r = wgrad_conv_route((int)v[0], (int)v[1], (int)v[2], (int)v[3], (int)v[4], (int)v[5], v[6] != 0, v[7] != 0, v[8] != 0, v[9] != 0);
            std::printf("%s %d %s\n", form_name(r, (int)v[3]), r.plan.splits, reduce_name(r.reduce));
        } else {
            return fail("unknown case kind", kind, 0, 0);
        }
    }
    std::fclose(f);
    return 0;
}

int main(int argc, char **argv) {
    if (argc > 1) return answer(argv[1]);
    if (self_check()) return 1;
    std::printf("OK\n");
    return 0;
}
