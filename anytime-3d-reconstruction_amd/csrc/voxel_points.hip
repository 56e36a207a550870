// Occupancy grids -> posed point clouds: the reference's objRescaleTransform (src/visualizer/visualizer.py:171-188: threshold, list the
// occupied cells in row-major order, shift to the bounding box, scale the largest extent to max(h, w, l), centre, apply the pose) for a
// batch of grids that are already in device memory.  A threshold, an ORDERED stream compaction, a bounding-box reduction and an affine map.
//
// Form.  One work item = one piece = VP_PIECE consecutive flat indices of one object (as in pr_curve.hip).  Inside a piece the order is
// (wave, step, lane, slot): a wave owns 1024 consecutive cells and walks them in 4 steps of 64 lanes x 4 consecutive cells, so a lane's
// float cells are one 16-byte load where the address allows and its packed cells are 4 bits of one byte.
//   count:   per piece the number of emitted cells and the box of its occupied cells -> workspace            (vp_count_kernel)
//            per object the exclusive prefix over its pieces, counts[b], bbox[b]                            (vp_object_kernel, a wave each)
//            the exclusive prefix over objects -> offsets[B + 1]                                            (vp_offsets_kernel, one block)
//   emit:    every piece recomputes its bits; a cell's row is offsets[b] + piece prefix + the totals of the earlier waves (LDS) + the
//            totals of the wave's earlier steps + the population count of the step's ballots below the lane + its own lower slots.
//            The compacted output is therefore in cell order without a sort, and neighbouring lanes write neighbouring rows.
// Integer arithmetic, ballots, population counts and plain stores: no atomics at all, the same bits on every run.  gfx950 only.
#include "common.h"

namespace {

constexpr int VP_THREADS = 256;          // 4 waves
constexpr int VP_STEPS = 4;              // steps of a wave over its run
constexpr int VP_WAVE_CELLS = VP_STEPS * 64 * 4;
constexpr int VP_PIECE = 4 * VP_WAVE_CELLS;      // 4096 cells per work item: a function of nothing but these constants
constexpr int VP_MAX_GRID = 2048;
constexpr int VP_MAX_SIDE = 128;

template <bool PACKED>
__device__ __forceinline__ bool vp_cell(const void *occ, float prob, long long b, long long voxels, long long v) {
    if (PACKED) {
        const unsigned char *row = reinterpret_cast<const unsigned char *>(occ) + b * (voxels >> 3);
        return ((row[v >> 3] >> (unsigned)(v & 7)) & 1u) != 0u;
    }
    return reinterpret_cast<const float *>(occ)[b * voxels + v] > prob;        // ordered: a NaN cell is not occupied
}

// Bit s = cell v + s of object b is occupied (v % 4 == 0; cells at or past `voxels` are absent and never read).
template <bool PACKED>
__device__ __forceinline__ unsigned vp_group(const void *occ, float prob, long long b, long long voxels, long long v) {
    if (v >= voxels) return 0u;
    if (PACKED) {                                                               // voxels % 8 == 0: the four bits sit in one byte of the row
        const unsigned char *row = reinterpret_cast<const unsigned char *>(occ) + b * (voxels >> 3);
        return ((unsigned)row[v >> 3] >> (unsigned)(v & 7)) & 15u;
    }
    const float *p = reinterpret_cast<const float *>(occ) + b * voxels + v;
    unsigned bits = 0u;
    if (v + 4 <= voxels && (reinterpret_cast<uintptr_t>(p) & 15u) == 0) {
        const f32x4 x = *reinterpret_cast<const f32x4 *>(p);
#pragma unroll
        for (int s = 0; s < 4; ++s) bits |= (x[s] > prob ? 1u : 0u) << s;
    } else {
#pragma unroll
        for (int s = 0; s < 4; ++s)
            if (v + s < voxels) bits |= (p[s] > prob ? 1u : 0u) << s;
    }
    return bits;
}

struct VpCell { int i, j, k; };
__device__ __forceinline__ VpCell vp_coords(long long v, int D) {
    const unsigned u = (unsigned)v, dd = (unsigned)(D * D);                     // v < 128^3
    VpCell c;
    c.i = (int)(u / dd);
    const unsigned r = u - (unsigned)c.i * dd;
    c.j = (int)(r / (unsigned)D);
    c.k = (int)(r - (unsigned)c.j * (unsigned)D);
    return c;
}
__device__ __forceinline__ void vp_next(VpCell &c, int D) {
    if (++c.k == D) {
        c.k = 0;
        if (++c.j == D) {
            c.j = 0;
            ++c.i;
        }
    }
}

// An occupied cell is on the surface when it lies on the grid boundary or one of its six face neighbours is not occupied.
template <bool PACKED>
__device__ __forceinline__ bool vp_surface(const void *occ, float prob, long long b, long long voxels, int D, VpCell c, long long v) {
    if (c.i == 0 || c.j == 0 || c.k == 0 || c.i == D - 1 || c.j == D - 1 || c.k == D - 1) return true;
    const long long dd = (long long)D * D;                                      // interior: all six neighbours are inside [0, voxels)
    return !(vp_cell<PACKED>(occ, prob, b, voxels, v - 1) && vp_cell<PACKED>(occ, prob, b, voxels, v + 1) &&
             vp_cell<PACKED>(occ, prob, b, voxels, v - D) && vp_cell<PACKED>(occ, prob, b, voxels, v + D) &&
             vp_cell<PACKED>(occ, prob, b, voxels, v - dd) && vp_cell<PACKED>(occ, prob, b, voxels, v + dd));
}

// The lane's four cells at v: bits of the cells that are emitted; lo / hi take in every OCCUPIED cell when BOX.
template <bool PACKED, bool BOX>
__device__ __forceinline__ unsigned vp_emitted(const void *occ, float prob, int surface, long long b, long long voxels, int D, long long v,
                                               int *lo, int *hi) {
    const unsigned ob = vp_group<PACKED>(occ, prob, b, voxels, v);
    unsigned eb = ob;
    if (ob && (BOX || surface)) {
        VpCell c = vp_coords(v, D);
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            if ((ob >> s) & 1u) {
                if (BOX) {
                    lo[0] = min(lo[0], c.i), lo[1] = min(lo[1], c.j), lo[2] = min(lo[2], c.k);
                    hi[0] = max(hi[0], c.i), hi[1] = max(hi[1], c.j), hi[2] = max(hi[2], c.k);
                }
                if (surface && !vp_surface<PACKED>(occ, prob, b, voxels, D, c, v + s)) eb &= ~(1u << s);
            }
            vp_next(c, D);
        }
    }
    return eb;
}

__device__ __forceinline__ long long vp_lane_cell(long long v0, int wave, int step, int lane) {
    return v0 + wave * VP_WAVE_CELLS + step * 256 + lane * 4;
}

// cnt[item] = emitted cells of the piece, pbox[item][6] = (lo, hi) of its occupied cells ((D, D, D, -1, -1, -1) when it has none).
template <bool PACKED>
__global__ __launch_bounds__(VP_THREADS) void vp_count_kernel(const void *__restrict__ occ, float prob, int surface, int D, long long voxels,
                                                              int pieces, long long items, int *__restrict__ cnt, int *__restrict__ pbox) {
    __shared__ int red[4][7];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    for (long long item = blockIdx.x; item < items; item += gridDim.x) {
        const long long b = item / pieces, v0 = (item % pieces) * VP_PIECE;
        int n = 0, lo[3] = {D, D, D}, hi[3] = {-1, -1, -1};
#pragma unroll
        for (int step = 0; step < VP_STEPS; ++step)
            n += __builtin_popcount(vp_emitted<PACKED, true>(occ, prob, surface, b, voxels, D, vp_lane_cell(v0, wave, step, lane), lo, hi));
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            n += __shfl_xor(n, o, 64);
#pragma unroll
            for (int a = 0; a < 3; ++a) {
                lo[a] = min(lo[a], __shfl_xor(lo[a], o, 64));
                hi[a] = max(hi[a], __shfl_xor(hi[a], o, 64));
            }
        }
        if (lane == 0) {
            red[wave][0] = n;
#pragma unroll
            for (int a = 0; a < 3; ++a) red[wave][1 + a] = lo[a], red[wave][4 + a] = hi[a];
        }
        __syncthreads();
        if (tid == 0) cnt[item] = red[0][0] + red[1][0] + red[2][0] + red[3][0];
        if (tid >= 1 && tid < 4) pbox[item * 6 + tid - 1] = min(min(red[0][tid], red[1][tid]), min(red[2][tid], red[3][tid]));
        if (tid >= 4 && tid < 7) pbox[item * 6 + tid - 1] = max(max(red[0][tid], red[1][tid]), max(red[2][tid], red[3][tid]));
        __syncthreads();
    }
}

// One wave per object: exclusive prefix of its pieces' counts (64 pieces per round, a cross-lane scan), counts[b], bbox[b].
__global__ __launch_bounds__(64) void vp_object_kernel(const int *__restrict__ cnt, const int *__restrict__ pbox, int pieces, int D,
                                                       int *__restrict__ prefix, int *__restrict__ counts, int *__restrict__ bbox) {
    const long long b = blockIdx.x;
    const int lane = threadIdx.x;
    int running = 0, lo[3] = {D, D, D}, hi[3] = {-1, -1, -1};
    for (int p0 = 0; p0 < pieces; p0 += 64) {
        const int p = p0 + lane;
        const long long item = b * pieces + p;
        const int n = p < pieces ? cnt[item] : 0;
        int incl = n;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const int up = __shfl_up(incl, o, 64);
            if (lane >= o) incl += up;
        }
        if (p < pieces) {
            prefix[item] = running + incl - n;
#pragma unroll
            for (int a = 0; a < 3; ++a) {
                lo[a] = min(lo[a], pbox[item * 6 + a]);
                hi[a] = max(hi[a], pbox[item * 6 + 3 + a]);
            }
        }
        running += __shfl(incl, 63, 64);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            lo[a] = min(lo[a], __shfl_xor(lo[a], o, 64));
            hi[a] = max(hi[a], __shfl_xor(hi[a], o, 64));
        }
    }
    if (lane == 0) {
        counts[b] = running;
#pragma unroll
        for (int a = 0; a < 3; ++a) bbox[b * 6 + a] = lo[a], bbox[b * 6 + 3 + a] = hi[a];
    }
}

// One block: offsets[b] = counts[0] + ... + counts[b - 1] in int64, offsets[batch] = the total.
__global__ __launch_bounds__(VP_THREADS) void vp_offsets_kernel(const int *__restrict__ counts, int batch, long long *__restrict__ offsets) {
    __shared__ long long wsum[4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    long long carry = 0;
    for (int b0 = 0; b0 < batch; b0 += VP_THREADS) {
        const int b = b0 + tid;
        const long long n = b < batch ? (long long)counts[b] : 0ll;
        long long incl = n;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const long long up = __shfl_up(incl, o, 64);
            if (lane >= o) incl += up;
        }
        if (lane == 63) wsum[wave] = incl;
        __syncthreads();
        long long before = carry;
        for (int w = 0; w < wave; ++w) before += wsum[w];
        if (b < batch) offsets[b] = before + incl - n;
        carry += wsum[0] + wsum[1] + wsum[2] + wsum[3];
        __syncthreads();
    }
    if (tid == 0) offsets[batch] = carry;
}

template <bool PACKED>
__global__ __launch_bounds__(VP_THREADS) void vp_emit_kernel(const void *__restrict__ occ, float prob, int surface, int D, long long voxels,
                                                             int pieces, long long items, const int *__restrict__ prefix,
                                                             const long long *__restrict__ offsets, const int *__restrict__ bbox,
                                                             const float *__restrict__ dims, const float *__restrict__ pose,
                                                             float *__restrict__ points, long long capacity) {
    __shared__ int wtot[4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    for (long long item = blockIdx.x; item < items; item += gridDim.x) {
        const long long b = item / pieces, v0 = (item % pieces) * VP_PIECE;
        unsigned eb[VP_STEPS];
        int n = 0;
#pragma unroll
        for (int step = 0; step < VP_STEPS; ++step) {
            eb[step] = vp_emitted<PACKED, false>(occ, prob, surface, b, voxels, D, vp_lane_cell(v0, wave, step, lane), nullptr, nullptr);
            n += __builtin_popcount(eb[step]);
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) n += __shfl_xor(n, o, 64);
        if (lane == 0) wtot[wave] = n;
        __syncthreads();
        long long row = offsets[b] + prefix[item];                              // of the wave's first emitted cell
        for (int w = 0; w < wave; ++w) row += wtot[w];
        if (n > 0) {                                                            // wave-uniform
            // the object's map: q = (cell - lo) scale - (ext scale) / 2, point = R q + t
            const int *bb = bbox + b * 6;
            const int lo0 = bb[0], lo1 = bb[1], lo2 = bb[2];
            const int e0 = bb[3] - lo0, e1 = bb[4] - lo1, e2 = bb[5] - lo2, E = max(e0, max(e1, e2));
            const float scale = E > 0 ? fmaxf(fmaxf(dims[b * 3], dims[b * 3 + 1]), dims[b * 3 + 2]) / (float)E : 0.f;
            const float h0 = ((float)e0 * scale) * 0.5f, h1 = ((float)e1 * scale) * 0.5f, h2 = ((float)e2 * scale) * 0.5f;
            float P[12] = {1.f, 0.f, 0.f, 0.f, 0.f, 1.f, 0.f, 0.f, 0.f, 0.f, 1.f, 0.f};
            if (pose) {
#pragma unroll
                for (int e = 0; e < 12; ++e) P[e] = pose[b * 16 + e];
            }
#pragma unroll
            for (int step = 0; step < VP_STEPS; ++step) {
                int below = 0, total = 0;                                       // emitted cells of the step in lower lanes / in the wave
#pragma unroll
                for (int s = 0; s < 4; ++s) {
                    const unsigned long long m = __builtin_amdgcn_ballot_w64(((eb[step] >> s) & 1u) != 0u);
                    below += (int)__builtin_amdgcn_mbcnt_hi((unsigned)(m >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)m, 0u));
                    total += __builtin_popcountll(m);
                }
                if (eb[step]) {
                    const long long v = vp_lane_cell(v0, wave, step, lane);
                    VpCell c = vp_coords(v, D);
                    long long g = row + below;
#pragma unroll
                    for (int s = 0; s < 4; ++s) {
                        if ((eb[step] >> s) & 1u) {
                            if (g < capacity) {
                                const float q0 = (float)(c.i - lo0) * scale - h0, q1 = (float)(c.j - lo1) * scale - h1,
                                            q2 = (float)(c.k - lo2) * scale - h2;
                                float *out = points + g * 3;
                                out[0] = P[0] * q0 + P[1] * q1 + P[2] * q2 + P[3];
                                out[1] = P[4] * q0 + P[5] * q1 + P[6] * q2 + P[7];
                                out[2] = P[8] * q0 + P[9] * q1 + P[10] * q2 + P[11];
                            }
                            ++g;
                        }
                        vp_next(c, D);
                    }
                }
                row += total;
            }
        }
        __syncthreads();
    }
}

inline long long vp_pieces(long long voxels) { return (voxels + VP_PIECE - 1) / VP_PIECE; }
inline bool vp_shape_ok(int batch, int side) {
    if (batch <= 0 || side < 1 || side > VP_MAX_SIDE) return false;
    const long long voxels = (long long)side * side * side;
    return (long long)batch * vp_pieces(voxels) <= 0x7fffffffLL;               // items, and the object kernel's grid
}
inline bool vp_misaligned(const void *p, unsigned mask) { return (reinterpret_cast<uintptr_t>(p) & mask) != 0; }

// workspace: int32 cnt[items], prefix[items], pbox[items][6]
struct VpWorkspace { int *cnt, *prefix, *pbox; };
inline VpWorkspace vp_workspace(const void *ws, long long items) {
    int *base = reinterpret_cast<int *>(const_cast<void *>(ws));
    return {base, base + items, base + 2 * items};
}

}  // namespace

VV_EXPORT size_t vv_voxel_points_workspace_bytes(int batch, int side) {
    if (!vp_shape_ok(batch, side)) return 0;
    return (size_t)batch * (size_t)vp_pieces((long long)side * side * side) * 8 * sizeof(int);
}

VV_EXPORT int vv_voxel_points_count(const void *occ, int packed, float prob, int surface_only, int batch, int side, int *counts, int *bbox,
                                    long long *offsets, void *workspace, size_t workspace_bytes, void *stream) {
    if (!occ || !counts || !bbox || !offsets || !workspace) return VV_ERR_NULL;
    if (!vp_shape_ok(batch, side)) return VV_ERR_SHAPE;
    const long long voxels = (long long)side * side * side;
    if (packed && (voxels & 7)) return VV_ERR_SHAPE;
    if ((!packed && vp_misaligned(occ, 3u)) || vp_misaligned(counts, 3u) || vp_misaligned(bbox, 3u) || vp_misaligned(offsets, 7u) ||
        vp_misaligned(workspace, 3u))
        return VV_ERR_ALIGN;                                                    // natural alignment of the element types, no more
    if (workspace_bytes < vv_voxel_points_workspace_bytes(batch, side)) return VV_ERR_WORKSPACE;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const int pieces = (int)vp_pieces(voxels);
    const long long items = (long long)batch * pieces;
    const VpWorkspace w = vp_workspace(workspace, items);
    const unsigned grid = (unsigned)(items < VP_MAX_GRID ? items : VP_MAX_GRID);
    if (packed)
        VV_LAUNCH((vp_count_kernel<true>), dim3(grid), dim3(VP_THREADS), 0, st, occ, prob, surface_only, side, voxels, pieces, items, w.cnt, w.pbox);
    else
        VV_LAUNCH((vp_count_kernel<false>), dim3(grid), dim3(VP_THREADS), 0, st, occ, prob, surface_only, side, voxels, pieces, items, w.cnt, w.pbox);
    int rc = vv_launch_status();
    if (rc != VV_OK) return rc;
    VV_LAUNCH(vp_object_kernel, dim3((unsigned)batch), dim3(64), 0, st, w.cnt, w.pbox, pieces, side, w.prefix, counts, bbox);
    rc = vv_launch_status();
    if (rc != VV_OK) return rc;
    VV_LAUNCH(vp_offsets_kernel, dim3(1), dim3(VP_THREADS), 0, st, counts, batch, offsets);
    return vv_launch_status();
}

VV_EXPORT int vv_voxel_points_emit(const void *occ, int packed, float prob, int surface_only, const float *dims, const float *pose,
                                   const long long *offsets, const int *bbox, float *points, long long capacity, const void *workspace,
                                   size_t workspace_bytes, int batch, int side, void *stream) {
    if (!occ || !dims || !offsets || !bbox || !workspace || (!points && capacity > 0)) return VV_ERR_NULL;
    if (!vp_shape_ok(batch, side) || capacity < 0) return VV_ERR_SHAPE;
    const long long voxels = (long long)side * side * side;
    if (packed && (voxels & 7)) return VV_ERR_SHAPE;
    if ((!packed && vp_misaligned(occ, 3u)) || vp_misaligned(dims, 3u) || vp_misaligned(pose, 3u) || vp_misaligned(offsets, 7u) ||
        vp_misaligned(bbox, 3u) || vp_misaligned(points, 3u) || vp_misaligned(workspace, 3u))
        return VV_ERR_ALIGN;
    if (workspace_bytes < vv_voxel_points_workspace_bytes(batch, side)) return VV_ERR_WORKSPACE;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const int pieces = (int)vp_pieces(voxels);
    const long long items = (long long)batch * pieces;
    const VpWorkspace w = vp_workspace(workspace, items);
    const unsigned grid = (unsigned)(items < VP_MAX_GRID ? items : VP_MAX_GRID);
    if (packed)
        VV_LAUNCH((vp_emit_kernel<true>), dim3(grid), dim3(VP_THREADS), 0, st, occ, prob, surface_only, side, voxels, pieces, items, w.prefix,
                  offsets, bbox, dims, pose, points, capacity);
    else
        VV_LAUNCH((vp_emit_kernel<false>), dim3(grid), dim3(VP_THREADS), 0, st, occ, prob, surface_only, side, voxels, pieces, items, w.prefix,
                  offsets, bbox, dims, pose, points, capacity);
    return vv_launch_status();
}
