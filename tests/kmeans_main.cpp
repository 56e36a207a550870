// Stand-alone program over csrc/kmeans_cosine.h for the sanitizer test (tests/test_kmeans_host.py): the whole-run loop and the assign loop
// on exactly sized heap arrays -- one point, one short of / exactly / one past a chunk, two chunks and three points with one centre,
// more centres than points, two identical centres, the limit k = 1024, a NULL distance -- built with -fsanitize=address,undefined.
// Prints OK.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "kmeans_cosine.h"

static unsigned long long state = 0x9E3779B97F4A7C15ull;
static double draw() {          // uniform in [0, 1)
    state = state * 6364136223846793005ull + 1442695040888963407ull;
    return (double)(state >> 11) / 9007199254740992.0;
}
static std::vector<double> rows(int n, double span) {
    std::vector<double> v((size_t)n * VV_KM_DIM);
    for (int i = 0; i < n; ++i) {
        const double e[3] = {(2.0 * draw() - 1.0) * span, 0.15 + 0.4 * (draw() - 0.5), 0.2 * (draw() - 0.5)};
        for (int j = 0; j < 3; ++j) v[(size_t)i * VV_KM_DIM + j] = std::sin(e[j]), v[(size_t)i * VV_KM_DIM + 3 + j] = std::cos(e[j]);
    }
    return v;
}

static int run(int n, int k, int max_iter, bool twins) {
    std::vector<double> x = rows(n, 3.14159), c = rows(k, 3.14159), dist(n);
    if (twins && k > 3)
        for (int j = 0; j < VV_KM_DIM; ++j) c[3 * VV_KM_DIM + j] = c[1 * VV_KM_DIM + j];
    const std::vector<double> c0 = c;
    std::vector<int> xtoc(n), seen(k, 0);
    int its = -1;
    vv_km_run_host(x.data(), n, c.data(), k, max_iter, xtoc.data(), dist.data(), &its);
    if (its < 1 || its > max_iter) return 1;
    for (int i = 0; i < n; ++i) {
        if (xtoc[i] < 0 || xtoc[i] >= k || !(dist[i] >= 0.0)) return 2;
        seen[xtoc[i]] = 1;
    }
    if (max_iter == 1)                                                          // one iteration: a cluster without a member kept its row
        for (int q = 0; q < k; ++q)
            if (!seen[q])
                for (int j = 0; j < VV_KM_DIM; ++j)
                    if (c[(size_t)q * VV_KM_DIM + j] != c0[(size_t)q * VV_KM_DIM + j]) return 3;
    if (twins && max_iter == 1 && k > 3 && seen[3]) return 4;                   // the first of two identical centres takes every tie
    std::vector<int> again(n);
    std::vector<double> d2(n);
    vv_km_assign_host(x.data(), n, c0.data(), k, again.data(), d2.data());
    vv_km_assign_host(x.data(), n, c0.data(), k, again.data(), nullptr);
    for (int i = 0; i < n; ++i)
        if (again[i] < 0 || again[i] >= k) return 5;
    return 0;
}

int main() {
    int rc = 0;
    rc |= run(1, 1, 3, false);
    rc |= run(1, 3, 1, false);
    rc |= run(VV_KM_CHUNK - 1, 7, 25, false);
    rc |= run(VV_KM_CHUNK, 7, 25, false);
    rc |= run(VV_KM_CHUNK + 1, 7, 25, false);
    rc |= run(2 * VV_KM_CHUNK + 3, 1, 4, false);
    rc |= run(5, 9, 1, false);
    rc |= run(5, 9, 12, false);
    rc |= run(300, 6, 1, true);
    rc |= run(300, 6, 1000, true);
    rc |= run(700, VV_KM_MAX_K, 2, false);
    if (rc) {
        std::printf("FAILED %d\n", rc);
        return 1;
    }
    std::printf("OK\n");
    return 0;
}
