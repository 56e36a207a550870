// Viewpoint clustering on the device: the reference's kmeans_cosine._kmeans (src/module/function.py:178-191) for points that are already in
// device memory.  The arithmetic, the tie rule and the summation order are kmeans_cosine.h, float64, shared with the host entries.
//
// Form.  assign:  one workgroup per chunk of VV_KM_CHUNK points, a thread per point.  The centres (k <= 1024: 48 KiB) and the chunk's rows
//                 (12 KiB) are staged in LDS; in the scan over the centres every lane reads the same address, a broadcast.  The labels go
//                 to LDS too, then thread t forms the chunk's partial sum and member count of clusters t, t + 256, ... in index order and
//                 writes them into the workspace -- every cluster's slot, an empty one as zeros -- together with the chunk's count of
//                 labels that differ from the previous iteration's (read from xtoc before it is overwritten).
//        update:  a thread per element (c, j) of the centres adds the chunks' partials in chunk order and divides by the member count;
//                 workgroup 0 also adds the chunks' change counts (integers) and settles the flag the next iteration reads.
// Early exit without a read-back: two flag words, used in turn.  Iteration t reads word (t - 1) & 1 -- written by iteration t - 1's
// update kernel, a launch earlier on the same stream -- and its update kernel writes word t & 1, so no workgroup reads a word that
// another workgroup of the SAME launch writes.  Once an iteration has changed no label the flag stays set and every remaining launch
// returns at its first instruction (kmeans_cosine.h states why that is exact).  All launches are enqueued by one call.
// No atomics, no grid-wide synchronisation, nothing read from the workspace that this call has not written.  gfx950 only.
#include "common.h"
#include "kmeans_cosine.h"

namespace {

constexpr int KM_THREADS = VV_KM_CHUNK;     // 4 waves
constexpr int KM_MAX_ITER = 1 << 16;        // launches enqueued by one call: two per iteration

struct KmWorkspace {
    double *psum;      // [chunks][k][6]
    int *pcnt;         // [chunks][k]
    int *changed;      // [chunks]
    int *flag;         // [2]
};

inline size_t km_workspace_bytes(int n, int k) {
    const size_t chunks = (size_t)vv_km_chunks(n);
    const size_t bytes = chunks * k * VV_KM_DIM * sizeof(double) + chunks * k * sizeof(int) + chunks * sizeof(int) + 2 * sizeof(int);
    return (bytes + 7u) & ~(size_t)7u;
}

inline KmWorkspace km_carve(void *workspace, int n, int k) {
    const size_t chunks = (size_t)vv_km_chunks(n);
    KmWorkspace w;
    w.psum = reinterpret_cast<double *>(workspace);
    w.pcnt = reinterpret_cast<int *>(w.psum + chunks * k * VV_KM_DIM);
    w.changed = w.pcnt + chunks * k;
    w.flag = w.changed + chunks;
    return w;
}

// TRAIN = false: labels (and distances) only, the vv_kmeans_cosine_assign entry.  `stable` is the flag word of the previous iteration
// (NULL in the first one, which compares with nothing: every label counts as changed).
template <bool TRAIN>
__global__ __launch_bounds__(KM_THREADS) void km_assign_kernel(const double *__restrict__ x, int n, const double *__restrict__ centres, int k,
                                                               int *__restrict__ xtoc, double *__restrict__ distance,
                                                               double *__restrict__ psum, int *__restrict__ pcnt, int *__restrict__ changed,
                                                               const int *__restrict__ stable) {
    __shared__ double s_centres[VV_KM_MAX_K * VV_KM_DIM];
    __shared__ double s_rows[VV_KM_CHUNK * VV_KM_DIM];
    __shared__ int s_labels[VV_KM_CHUNK];
    __shared__ int s_changed[KM_THREADS / 64];
    if (TRAIN && stable && *stable) return;                                      // uniform over the grid
    const int tid = threadIdx.x, chunk = blockIdx.x;
    const long long base = (long long)chunk * VV_KM_CHUNK;
    const int m = n - base < VV_KM_CHUNK ? (int)(n - base) : VV_KM_CHUNK;        // >= 1: the grid is vv_km_chunks(n)
    for (int e = tid; e < k * VV_KM_DIM; e += KM_THREADS) s_centres[e] = centres[e];
    for (int e = tid; e < m * VV_KM_DIM; e += KM_THREADS) s_rows[e] = x[base * VV_KM_DIM + e];
    __syncthreads();
    int label = -1;
    bool moved = false;
    if (tid < m) {
        double row[VV_KM_DIM], d;
#pragma unroll
        for (int j = 0; j < VV_KM_DIM; ++j) row[j] = s_rows[tid * VV_KM_DIM + j];
        label = vv_km_nearest(row, s_centres, k, &d);
        if (TRAIN) moved = !stable || label != xtoc[base + tid];
        xtoc[base + tid] = label;
        if (distance) distance[base + tid] = d;
    }
    if (!TRAIN) return;
    s_labels[tid] = label;
    const unsigned long long ballot = __builtin_amdgcn_ballot_w64(moved);
    if ((tid & 63) == 0) s_changed[tid >> 6] = __builtin_popcountll(ballot);
    __syncthreads();
    if (tid == 0) changed[chunk] = s_changed[0] + s_changed[1] + s_changed[2] + s_changed[3];
    for (int c = tid; c < k; c += KM_THREADS) {
        double sum[VV_KM_DIM];
        const int count = vv_km_chunk_sum(s_rows, s_labels, m, c, sum);
        const long long slot = (long long)chunk * k + c;
        pcnt[slot] = count;
#pragma unroll
        for (int j = 0; j < VV_KM_DIM; ++j) psum[slot * VV_KM_DIM + j] = sum[j];
    }
}

__global__ __launch_bounds__(KM_THREADS) void km_update_kernel(const double *__restrict__ psum, const int *__restrict__ pcnt,
                                                               const int *__restrict__ changed, int chunks, int k,
                                                               double *__restrict__ centres, int *__restrict__ flag, int it,
                                                               int *__restrict__ iterations) {
    __shared__ int s_sum[KM_THREADS];
    const int tid = threadIdx.x;
    if (it > 1 && flag[(it - 1) & 1]) {                                          // uniform over the grid
        if (blockIdx.x == 0 && tid == 0) flag[it & 1] = 1;
        return;
    }
    const int e = blockIdx.x * KM_THREADS + tid;
    if (e < k * VV_KM_DIM) {
        const int c = e / VV_KM_DIM;
        double total = 0.0;
        int count = 0;
        for (int ch = 0; ch < chunks; ++ch) {
            count += pcnt[(long long)ch * k + c];
            total = vv_km_fold(total, psum[(long long)ch * k * VV_KM_DIM + e]);
        }
        if (count > 0) centres[e] = vv_km_mean(total, count);
    }
    if (blockIdx.x != 0) return;
    int moved = 0;
    for (int ch = tid; ch < chunks; ch += KM_THREADS) moved += changed[ch];      // at most n <= 2^20 in all
    s_sum[tid] = moved;
    __syncthreads();
    for (int o = KM_THREADS / 2; o > 0; o >>= 1) {
        if (tid < o) s_sum[tid] += s_sum[tid + o];
        __syncthreads();
    }
    if (tid == 0) flag[it & 1] = s_sum[0] == 0, iterations[0] = it;
}

inline bool km_misaligned(const void *p, unsigned mask) { return (reinterpret_cast<uintptr_t>(p) & mask) != 0; }
inline bool km_shape_ok(int n, int k) { return n >= 1 && n <= VV_KM_MAX_N && k >= 1 && k <= VV_KM_MAX_K; }

}  // namespace

VV_EXPORT size_t vv_kmeans_cosine_workspace_bytes(int n, int k) { return km_shape_ok(n, k) ? km_workspace_bytes(n, k) : 0; }

VV_EXPORT int vv_kmeans_cosine(const double *x, int n, double *centres, int k, int max_iter, int *xtoc, double *distance, int *iterations,
                               void *workspace, size_t workspace_bytes, void *hip_stream) {
    if (!x || !centres || !xtoc || !distance || !iterations || !workspace) return VV_ERR_NULL;
    if (!km_shape_ok(n, k) || max_iter < 1 || max_iter > KM_MAX_ITER) return VV_ERR_SHAPE;
    if (km_misaligned(x, 7u) || km_misaligned(centres, 7u) || km_misaligned(distance, 7u) || km_misaligned(workspace, 7u) ||
        km_misaligned(xtoc, 3u) || km_misaligned(iterations, 3u))
        return VV_ERR_ALIGN;                                                     // natural alignment of the element types, no more
    if (workspace_bytes < km_workspace_bytes(n, k)) return VV_ERR_WORKSPACE;
    hipStream_t st = reinterpret_cast<hipStream_t>(hip_stream);
    const KmWorkspace w = km_carve(workspace, n, k);
    const int chunks = vv_km_chunks(n);
    const unsigned ugrid = (unsigned)((k * VV_KM_DIM + KM_THREADS - 1) / KM_THREADS);
    for (int it = 1; it <= max_iter; ++it) {
        const int *stable = it > 1 ? w.flag + ((it - 1) & 1) : nullptr;
        VV_LAUNCH(km_assign_kernel<true>, dim3((unsigned)chunks), dim3(KM_THREADS), 0, st, x, n, centres, k, xtoc, distance, w.psum, w.pcnt,
                  w.changed, stable);
        int rc = vv_launch_status();
        if (rc != VV_OK) return rc;
        VV_LAUNCH(km_update_kernel, dim3(ugrid), dim3(KM_THREADS), 0, st, w.psum, w.pcnt, w.changed, chunks, k, centres, w.flag, it, iterations);
        rc = vv_launch_status();
        if (rc != VV_OK) return rc;
    }
    return VV_OK;
}

VV_EXPORT int vv_kmeans_cosine_host(const double *x, int n, double *centres, int k, int max_iter, int *xtoc, double *distance,
                                    int *iterations) {
    if (!x || !centres || !xtoc || !distance || !iterations) return VV_ERR_NULL;
    if (!km_shape_ok(n, k) || max_iter < 1 || max_iter > KM_MAX_ITER) return VV_ERR_SHAPE;
    if (km_misaligned(x, 7u) || km_misaligned(centres, 7u) || km_misaligned(distance, 7u) || km_misaligned(xtoc, 3u) ||
        km_misaligned(iterations, 3u))
        return VV_ERR_ALIGN;
    vv_km_run_host(x, n, centres, k, max_iter, xtoc, distance, iterations);
    return VV_OK;
}

VV_EXPORT int vv_kmeans_cosine_assign(const double *x, int n, const double *centres, int k, int *xtoc, double *distance, void *hip_stream) {
    if (!x || !centres || !xtoc) return VV_ERR_NULL;
    if (!km_shape_ok(n, k)) return VV_ERR_SHAPE;
    if (km_misaligned(x, 7u) || km_misaligned(centres, 7u) || km_misaligned(distance, 7u) || km_misaligned(xtoc, 3u)) return VV_ERR_ALIGN;
    hipStream_t st = reinterpret_cast<hipStream_t>(hip_stream);
    VV_LAUNCH(km_assign_kernel<false>, dim3((unsigned)vv_km_chunks(n)), dim3(KM_THREADS), 0, st, x, n, centres, k, xtoc, distance,
              (double *)nullptr, (int *)nullptr, (int *)nullptr, (const int *)nullptr);
    return vv_launch_status();
}

VV_EXPORT int vv_kmeans_cosine_assign_host(const double *x, int n, const double *centres, int k, int *xtoc, double *distance) {
    if (!x || !centres || !xtoc) return VV_ERR_NULL;
    if (!km_shape_ok(n, k)) return VV_ERR_SHAPE;
    if (km_misaligned(x, 7u) || km_misaligned(centres, 7u) || km_misaligned(distance, 7u) || km_misaligned(xtoc, 3u)) return VV_ERR_ALIGN;
    vv_km_assign_host(x, n, centres, k, xtoc, distance);
    return VV_OK;
}
