// Precision / recall-vs-threshold counts in one streaming pass over (probabilities, target): what the reference's notebooks
// compute on the host with one numpy pass per threshold (modelnetAE3.ipynb / pascalAE3.ipynb cell 2).  For threshold i:
// TP_i = #{occupied and p > t_i}, FP_i = #{not occupied and p > t_i}; FN_i = occupied - TP_i is left to the caller.
//
// Form.  The data are extremely skewed (at a trained model almost every voxel is below every threshold or above all of them), so a
// histogram with one LDS add per voxel would put all 64 lanes of a wave on one address.  Instead the wave compares all its voxels
// with ONE threshold at a time: the compare's lane mask (a ballot) is kept by lane i of a register pair (one select per word), so after
// a chunk of 64 thresholds lane i holds the 64-bit mask of threshold i and every lane counts its own threshold with two population
// counts.  The accumulators are lane-distributed registers (lane l of chunk c <-> threshold 64 c + l): no LDS or memory traffic
// inside the loop.  With sorted thresholds the scan of a wave stops at the first threshold that none of its voxels exceeds.
//
// Everything is integer: per-(sample, 4096-voxel piece) partial counts are 32-bit and stored with plain stores; a second small launch
// adds them into the caller's int64 accumulators (integer atomics: any order gives the same bits).  No float atomics anywhere.
//
// The compare is done on an order-preserving integer image of the float32 bits, so no denormal mode can change a count:
// NaN probabilities exceed nothing, a NaN threshold is exceeded by nothing, -0 == +0.  gfx950 only.
#include "common.h"

namespace {

constexpr int PRC_THREADS = 256;     // 4 waves; also the largest threshold count (thread i finishes threshold i)
constexpr int PRC_PIECE = 4096;      // voxels of one sample per work item: a function of nothing but this constant
constexpr int PRC_MAX_GRID = 2048;

// float32 bits -> unsigned key with the order of an ordered float compare; 0 is below every key a threshold can have
__device__ __forceinline__ unsigned prc_order_key(unsigned b) {
    if (b == 0x80000000u) b = 0u;                               // -0 == +0
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);          // key(-inf) = 0x007fffff > 0
}
__device__ __forceinline__ unsigned prc_prob_key(float p) {
    const unsigned b = __float_as_uint(p);
    return (b & 0x7fffffffu) > 0x7f800000u ? 0u : prc_order_key(b);            // NaN: exceeds nothing
}
__device__ __forceinline__ unsigned prc_thr_key(float t) {
    const unsigned b = __float_as_uint(t);
    return (b & 0x7fffffffu) > 0x7f800000u ? 0xffffffffu : prc_order_key(b);   // NaN: nothing exceeds it
}

// One work item = PRC_PIECE voxels of one sample.  A lane handles slots of 4 consecutive floats that are 16-byte aligned in `pred`
// (pa = the element offset of pred inside its 16-byte line); a slot that is entirely inside the piece is one 16-byte load, a slot that
// straddles the piece's first or last voxel (rows of 27 voxels, packed rows of 513 bytes) is read element by element, so nothing
// outside [first, last) of the row is touched.  partial[e * items + item], e = 2 i: TP_i, 2 i + 1: FP_i, 2 T: occupied voxels.
template <bool PACKED>
__global__ __launch_bounds__(PRC_THREADS) void pr_curve_kernel(const float *__restrict__ pred, const void *__restrict__ target,
                                                               const float *__restrict__ thr, int T, int sorted,
                                                               unsigned *__restrict__ partial, long long items, int pieces,
                                                               long long voxels, int tvec) {
    __shared__ unsigned red[4][2][PRC_THREADS];
    __shared__ unsigned occ_red[4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    unsigned tkey[4];
#pragma unroll
    for (int c = 0; c < 4; ++c) tkey[c] = (c * 64 + lane < T) ? prc_thr_key(thr[c * 64 + lane]) : 0xffffffffu;
    const long long pa = (long long)((reinterpret_cast<uintptr_t>(pred) >> 2) & 3u);
    const float *tf = reinterpret_cast<const float *>(target);
    const unsigned char *tb = reinterpret_cast<const unsigned char *>(target);

    for (long long item = blockIdx.x; item < items; item += gridDim.x) {
        const long long b = item / pieces, v0 = (item % pieces) * PRC_PIECE;
        const long long v1 = (voxels - v0 < PRC_PIECE) ? voxels : v0 + PRC_PIECE;
        const long long e0 = b * voxels + v0, e1 = b * voxels + v1;           // flat float index range of the piece
        const long long s0 = (e0 + pa) >> 2, s1 = (e1 + pa - 1) >> 2;         // aligned slots that overlap it
        const unsigned char *row = tb + b * (voxels >> 3);
        const int niter = (int)((s1 - s0 + PRC_THREADS) / PRC_THREADS);
        unsigned tp[4] = {0u, 0u, 0u, 0u}, ab[4] = {0u, 0u, 0u, 0u}, nocc = 0u;
        for (int it = 0; it < niter; ++it) {
            const long long s = s0 + (long long)it * PRC_THREADS + tid;
            const long long E = 4 * s - pa;                                   // flat index of the slot's first element
            unsigned pk[4] = {0u, 0u, 0u, 0u}, ob = 0u;                       // keys (0 = exceeds nothing), occupied bits
            if (s <= s1) {
                if (E >= e0 && E + 4 <= e1) {
                    const f32x4 p = *reinterpret_cast<const f32x4 *>(pred + E);
#pragma unroll
                    for (int j = 0; j < 4; ++j) pk[j] = prc_prob_key(p[j]);
                    if (PACKED) {
                        const long long v = E - b * voxels;
                        const unsigned w = (unsigned)row[v >> 3] | ((unsigned)row[(v + 3) >> 3] << 8);
                        ob = (w >> (unsigned)(v & 7)) & 15u;
                    } else if (tvec) {
                        const f32x4 y = *reinterpret_cast<const f32x4 *>(tf + E);
#pragma unroll
                        for (int j = 0; j < 4; ++j) ob |= (y[j] > 0.5f ? 1u : 0u) << j;
                    } else {
#pragma unroll
                        for (int j = 0; j < 4; ++j) ob |= (tf[E + j] > 0.5f ? 1u : 0u) << j;
                    }
                } else {
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        const long long e = E + j;
                        if (e >= e0 && e < e1) {
                            pk[j] = prc_prob_key(pred[e]);
                            if (PACKED) {
                                const long long v = e - b * voxels;
                                ob |= (((unsigned)row[v >> 3] >> (unsigned)(v & 7)) & 1u) << j;
                            } else {
                                ob |= (tf[e] > 0.5f ? 1u : 0u) << j;
                            }
                        }
                    }
                }
            }
            unsigned long long occ[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                occ[j] = __builtin_amdgcn_ballot_w64(((ob >> j) & 1u) != 0u);
                nocc += (unsigned)__builtin_popcountll(occ[j]);
            }
            bool done = false;
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                if (c * 64 >= T || done) break;
                const int n = (T - c * 64 < 64) ? T - c * 64 : 64;
                unsigned mlo[4] = {0u, 0u, 0u, 0u}, mhi[4] = {0u, 0u, 0u, 0u};
                for (int i = 0; i < n; ++i) {
                    const unsigned tk = (unsigned)__builtin_amdgcn_readlane((int)tkey[c], i);
                    unsigned long long m[4];
#pragma unroll
                    for (int j = 0; j < 4; ++j) m[j] = __builtin_amdgcn_ballot_w64(pk[j] > tk);
                    if (sorted && (m[0] | m[1] | m[2] | m[3]) == 0ull) {      // non-decreasing thresholds: none of the rest is exceeded
                        done = true;
                        break;
                    }
                    const bool mine = lane == i;                              // one compare, eight selects: lane i keeps threshold i's masks
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        mlo[j] = mine ? (unsigned)m[j] : mlo[j];
                        mhi[j] = mine ? (unsigned)(m[j] >> 32) : mhi[j];
                    }
                }
#pragma unroll
                for (int j = 0; j < 4; ++j) {                                 // lane i: threshold 64 c + i
                    tp[c] += __builtin_popcount(mlo[j] & (unsigned)occ[j]) + __builtin_popcount(mhi[j] & (unsigned)(occ[j] >> 32));
                    ab[c] += __builtin_popcount(mlo[j]) + __builtin_popcount(mhi[j]);
                }
            }
        }
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            red[wave][0][c * 64 + lane] = tp[c];
            red[wave][1][c * 64 + lane] = ab[c];
        }
        if (lane == 0) occ_red[wave] = nocc;
        __syncthreads();
        if (tid < T) {
            const unsigned t = red[0][0][tid] + red[1][0][tid] + red[2][0][tid] + red[3][0][tid];
            const unsigned a = red[0][1][tid] + red[1][1][tid] + red[2][1][tid] + red[3][1][tid];
            partial[(long long)(2 * tid) * items + item] = t;
            partial[(long long)(2 * tid + 1) * items + item] = a - t;
        }
        if (tid == 0) partial[(long long)(2 * T) * items + item] = occ_red[0] + occ_red[1] + occ_red[2] + occ_red[3];
        __syncthreads();
    }
}

// Partials -> the int64 accumulators.  Block x = entry e (2 T + 1 of them), thread = sample: the sample's pieces are summed, then added
// to its group's accumulator -- one block-wide sum and one add when there is a single group, one integer atomic per sample
// otherwise.  A sample whose group is outside [0, ngroups) adds nothing and addresses nothing.
__global__ __launch_bounds__(PRC_THREADS) void pr_curve_finish_kernel(const unsigned *__restrict__ partial, long long items, int pieces,
                                                                      int T, const int *__restrict__ group, int ngroups,
                                                                      unsigned long long *__restrict__ tp_fp,
                                                                      unsigned long long *__restrict__ totals, int batch,
                                                                      long long voxels) {
    __shared__ unsigned long long red[2][4];
    const int e = blockIdx.x, tid = threadIdx.x;
    const long long b = (long long)blockIdx.y * PRC_THREADS + tid;
    unsigned long long s = 0ull, n = 0ull;
    int g = -1;
    if (b < batch) {
        g = group ? group[b] : 0;
        if (g < 0 || g >= ngroups) g = -1;
    }
    if (g >= 0) {
        const unsigned *p = partial + (long long)e * items + b * pieces;
        for (int c = 0; c < pieces; ++c) s += p[c];
        n = (unsigned long long)voxels;
    }
    if (group) {
        if (g < 0) return;
        if (e < 2 * T) {
            if (s) atomicAdd(tp_fp + (long long)g * 2 * T + e, s);
        } else {
            if (s) atomicAdd(totals + 2 * g, s);
            atomicAdd(totals + 2 * g + 1, n);
        }
        return;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        s += __shfl_xor(s, o, 64);
        n += __shfl_xor(n, o, 64);
    }
    if ((tid & 63) == 0) {
        red[0][tid >> 6] = s;
        red[1][tid >> 6] = n;
    }
    __syncthreads();
    if (tid == 0) {
        s = red[0][0] + red[0][1] + red[0][2] + red[0][3];
        n = red[1][0] + red[1][1] + red[1][2] + red[1][3];
        if (e < 2 * T) {
            if (s) atomicAdd(tp_fp + e, s);
        } else {
            if (s) atomicAdd(totals, s);
            atomicAdd(totals + 1, n);
        }
    }
}

inline long long prc_pieces(long long voxels) { return (voxels + PRC_PIECE - 1) / PRC_PIECE; }

}  // namespace

VV_EXPORT size_t vv_pr_curve_workspace_bytes(int batch, long voxels, int nthr) {
    if (batch <= 0 || voxels <= 0 || nthr < 1 || nthr > PRC_THREADS) return 0;
    return (size_t)(2 * nthr + 1) * (size_t)batch * (size_t)prc_pieces(voxels) * sizeof(unsigned);
}

VV_EXPORT int vv_pr_curve_accumulate(const float *pred, const void *target, int target_packed, const float *thresholds, int nthr,
                                     int sorted, const int *group, int ngroups, long long *tp_fp, long long *totals, void *workspace,
                                     size_t workspace_bytes, int batch, long voxels, void *stream) {
    if (!pred || !target || !thresholds || !tp_fp || !totals || !workspace) return VV_ERR_NULL;
    if (batch <= 0 || voxels <= 0 || ngroups <= 0 || nthr < 1 || nthr > PRC_THREADS) return VV_ERR_SHAPE;
    if (target_packed && (voxels & 7)) return VV_ERR_SHAPE;
    const long long pieces = prc_pieces(voxels), items = (long long)batch * pieces;
    if (pieces > 0x7fffffffLL || batch > 65535 * PRC_THREADS) return VV_ERR_SHAPE;
    if ((reinterpret_cast<uintptr_t>(pred) & 3u) || (!target_packed && (reinterpret_cast<uintptr_t>(target) & 3u)) ||
        (reinterpret_cast<uintptr_t>(tp_fp) & 7u) || (reinterpret_cast<uintptr_t>(totals) & 7u) || (reinterpret_cast<uintptr_t>(workspace) & 3u))
        return VV_ERR_ALIGN;                                    // natural alignment of the element types; rows need none beyond it
    if (workspace_bytes < vv_pr_curve_workspace_bytes(batch, voxels, nthr)) return VV_ERR_WORKSPACE;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    unsigned *partial = reinterpret_cast<unsigned *>(workspace);
    const unsigned grid = (unsigned)(items < PRC_MAX_GRID ? items : PRC_MAX_GRID);
    // the float target shares the 16-byte loads when it sits at the same offset inside its 16-byte line as pred
    const int tvec = ((reinterpret_cast<uintptr_t>(pred) ^ reinterpret_cast<uintptr_t>(target)) & 15u) == 0;
    if (target_packed)
        VV_LAUNCH((pr_curve_kernel<true>), dim3(grid), dim3(PRC_THREADS), 0, st, pred, target, thresholds, nthr, sorted, partial, items,
                  (int)pieces, (long long)voxels, 0);
    else
        VV_LAUNCH((pr_curve_kernel<false>), dim3(grid), dim3(PRC_THREADS), 0, st, pred, target, thresholds, nthr, sorted, partial, items,
                  (int)pieces, (long long)voxels, tvec);
    int rc = vv_launch_status();
    if (rc != VV_OK) return rc;
    VV_LAUNCH(pr_curve_finish_kernel, dim3(2 * nthr + 1, (batch + PRC_THREADS - 1) / PRC_THREADS), dim3(PRC_THREADS), 0, st, partial, items,
              (int)pieces, nthr, group, ngroups, reinterpret_cast<unsigned long long *>(tp_fp), reinterpret_cast<unsigned long long *>(totals),
              batch, (long long)voxels);
    return vv_launch_status();
}
