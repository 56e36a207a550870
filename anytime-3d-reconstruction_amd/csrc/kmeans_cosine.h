// k-means over viewpoints stored as (sin a, sin e, sin i, cos a, cos e, cos i) with the reference's "cosine" distance: the arithmetic
// and the decisions of kmeans_cosine._dist_cosine / _kmeans (reference src/module/function.py:166-191), as plain C++ that compiles for
// the host and for the device alike (kmeans_cosine.hip runs it in two kernels per iteration and, through vv_kmeans_cosine_host, in
// loops on the CPU).  It also compiles without HIP (a plain C++ compiler), which is how the stand-alone sanitizer program builds it.
//
// Same bits on both sides.  Everything below is IEEE float64 +, -, *, the correctly rounded division, comparisons and integer counts;
// floating-point contraction is switched OFF in every function, so that the host build (no FMA on a plain x86-64 target) and the
// device build (v_fma_f64) round every product and sum alike: the argmin then decides the same way on both sides.
//
// Distance of a point x to a centre c, over j = 0, 1, 2 in exactly this order of operations:
//     p = x[j] * c[j];  q = x[j+3] * c[j+3];  s = p + q;  t = 1 - s;  u_j = t * t;          d = (u_0 + u_1) + u_2
// Label: the LOWEST index that minimises d -- the scan runs c = 0, 1, ... and a later centre wins only on strict `<` (np.argmin's rule).
// A NaN distance never wins, so a label is always inside [0, k).
//
// Update, THE summation order: the points are cut into chunks of VV_KM_CHUNK consecutive rows.  Inside a chunk a cluster's members
// are added in index order onto 0.0 (vv_km_chunk_sum); the chunks' partial sums are then added in chunk order onto 0.0, empty ones
// included (vv_km_fold); the centre is that total divided by the member count.  A cluster without a member keeps its row.
//
// No inline assembly, no atomics, no memory besides the arguments.
#pragma once
#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define VV_KM_HD __host__ __device__ inline
#else
#define VV_KM_HD inline
#endif

constexpr int VV_KM_DIM = 6;              // a row: three sines, then three cosines
constexpr int VV_KM_CHUNK = 256;          // points per chunk = threads of the assignment kernel's workgroup
constexpr int VV_KM_MAX_K = 1024;         // centres: 1024 * 6 * 8 bytes = 48 KiB of LDS
constexpr int VV_KM_MAX_N = 1 << 20;      // points per call: at most 4096 chunks

VV_KM_HD int vv_km_chunks(int n) { return (n + VV_KM_CHUNK - 1) / VV_KM_CHUNK; }

VV_KM_HD double vv_km_dist(const double *x, const double *c) {
#pragma clang fp contract(off)
    double u[3];
    for (int j = 0; j < 3; ++j) {
        const double p = x[j] * c[j];
        const double q = x[j + 3] * c[j + 3];
        const double s = p + q;
        const double t = 1.0 - s;
        u[j] = t * t;
    }
    return (u[0] + u[1]) + u[2];
}

// First-argmin over centres [k][6]; *dmin receives the distance to the centre returned.
VV_KM_HD int vv_km_nearest(const double *x, const double *centres, int k, double *dmin) {
#pragma clang fp contract(off)
    int best = 0;
    double bd = vv_km_dist(x, centres);
    for (int c = 1; c < k; ++c) {
        const double d = vv_km_dist(x, centres + c * VV_KM_DIM);
        if (d < bd) bd = d, best = c;
    }
    *dmin = bd;
    return best;
}

// Cluster c's partial sum over one chunk of m rows: its members in index order, added onto 0.0.  -> the number of members.
VV_KM_HD int vv_km_chunk_sum(const double *rows, const int *labels, int m, int c, double sum[VV_KM_DIM]) {
#pragma clang fp contract(off)
    int count = 0;
    for (int j = 0; j < VV_KM_DIM; ++j) sum[j] = 0.0;
    for (int i = 0; i < m; ++i) {
        if (labels[i] != c) continue;
        for (int j = 0; j < VV_KM_DIM; ++j) sum[j] = sum[j] + rows[i * VV_KM_DIM + j];
        ++count;
    }
    return count;
}

// One step of the chunk-order sum: the caller starts from 0.0 and folds chunk 0, 1, 2, ... in.
VV_KM_HD double vv_km_fold(double total, double partial) {
#pragma clang fp contract(off)
    return total + partial;
}

VV_KM_HD double vv_km_mean(double total, int count) {
#pragma clang fp contract(off)
    return total / (double)count;
}

// The whole algorithm on host pointers.  Scratch of VV_KM_MAX_K rows lives on the stack (52 KiB): nothing is allocated.
// xtoc / distance hold the last working iteration's assignment, taken BEFORE its update, as the reference returns them.
// Early exit: an iteration whose labels equal the previous iteration's has the same members in the same order, hence the same sums,
// and empty clusters keep their rows -- every later iteration would reproduce labels, centres and distances bit for bit.  So the
// loop stops after the first iteration that changes no label; *iterations is the number of iterations run.
inline void vv_km_run_host(const double *x, int n, double *centres, int k, int max_iter, int *xtoc, double *distance, int *iterations) {
#pragma clang fp contract(off)
    double total[VV_KM_MAX_K * VV_KM_DIM];
    int members[VV_KM_MAX_K];
    const int chunks = vv_km_chunks(n);
    int done = 0;
    for (int it = 1; it <= max_iter; ++it) {
        long long changed = 0;
        for (int e = 0; e < k * VV_KM_DIM; ++e) total[e] = 0.0;
        for (int c = 0; c < k; ++c) members[c] = 0;
        for (int ch = 0; ch < chunks; ++ch) {
            const int base = ch * VV_KM_CHUNK;
            const int m = n - base < VV_KM_CHUNK ? n - base : VV_KM_CHUNK;
            for (int i = base; i < base + m; ++i) {
                double d;
                const int lab = vv_km_nearest(x + (long long)i * VV_KM_DIM, centres, k, &d);
                if (it == 1 || lab != xtoc[i]) ++changed;
                xtoc[i] = lab, distance[i] = d;
            }
            for (int c = 0; c < k; ++c) {
                double s[VV_KM_DIM];
                members[c] += vv_km_chunk_sum(x + (long long)base * VV_KM_DIM, xtoc + base, m, c, s);
                for (int j = 0; j < VV_KM_DIM; ++j) total[c * VV_KM_DIM + j] = vv_km_fold(total[c * VV_KM_DIM + j], s[j]);
            }
        }
        for (int c = 0; c < k; ++c)
            if (members[c] > 0)
                for (int j = 0; j < VV_KM_DIM; ++j) centres[c * VV_KM_DIM + j] = vv_km_mean(total[c * VV_KM_DIM + j], members[c]);
        done = it;
        if (changed == 0) break;
    }
    *iterations = done;
}

inline void vv_km_assign_host(const double *x, int n, const double *centres, int k, int *xtoc, double *distance) {
#pragma clang fp contract(off)
    for (int i = 0; i < n; ++i) {
        double d;
        xtoc[i] = vv_km_nearest(x + (long long)i * VV_KM_DIM, centres, k, &d);
        if (distance) distance[i] = d;
    }
}
