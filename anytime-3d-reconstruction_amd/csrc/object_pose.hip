// Detections -> posed objects: the reference's getObjectInRealWorld (src/visualizer/visualizer.py:237-308) without its point-cloud step,
// for all detections of a frame that are already in device memory.  The arithmetic is pose_solve.h, float64, shared with the host entry.
//
// Form.  fit:      one wave per detection.  Every lane repeats the cheap prologue (scaling, rotation, ray correction: wave-uniform), then
//                  evaluates candidates lane and lane + 64 of the 128 corner-to-edge assignments (a 4x4 one-sided Jacobi each); the
//                  argmax over (iou, -k) is six xor-shuffles, the winner's translation one more shuffle; lane 0 finishes the pose, the
//                  projected corners and the filters and writes keep / candidate / iou and the detection's row into the workspace.
//        compact:  ONE workgroup walks n in pieces of 256: ballot + population-count ranks inside a wave, the waves' totals through 16
//                  bytes of LDS, a running carry across pieces -- the kept rows land in input order (as voxel_points.hip orders cells).
// No LDS in the fit, no atomics and no sort anywhere: a given input gives the same bits on every run.  gfx950 only.
#include "common.h"
#include "pose_solve.h"

namespace {

constexpr int OP_THREADS = 256;          // 4 waves
constexpr int OP_MAX_N = 65536;
constexpr int OP_ROW_WORDS = 16 + 3 + 16 + 4;      // pose, size, projected corners (float32), pixel box (int32)

__global__ __launch_bounds__(OP_THREADS) void op_fit_kernel(const float *__restrict__ bbox2d, const float *__restrict__ bbox3d,
                                                            const float *__restrict__ sn, const float *__restrict__ cs, int n,
                                                            const VvPoseCamera cam, int *__restrict__ keep, int *__restrict__ candidate,
                                                            float *__restrict__ iou, unsigned *__restrict__ rows) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long long i = (long long)blockIdx.x * (OP_THREADS / 64) + wave;
    if (i >= n) return;                                                          // wave-uniform; no barrier follows
    const float *b2 = bbox2d + i * 5, *b3 = bbox3d + i * 3;
    double box[4], R[9];
    if (!vv_pose_prepare(b2, b3, sn + i * 3, cs + i * 3, cam, box, R)) {         // wave-uniform
        if (lane == 0) keep[i] = 0, candidate[i] = -2, iou[i] = -1.f;
        return;
    }
    double best_iou = -1.0, t0 = 0.0, t1 = 0.0, t2 = 0.0;
    int best_k = -1;
#pragma unroll 1
    for (int c = 0; c < VV_POSE_CANDIDATES / 64; ++c) {
        const int k = lane + 64 * c;
        const VvPoseFit f = vv_pose_candidate(k, cam.P, R, box, (double)b3[0], (double)b3[1], (double)b3[2]);
        if (f.ok && vv_pose_better(f.iou, k, best_iou, best_k)) best_iou = f.iou, best_k = k, t0 = f.t[0], t1 = f.t[1], t2 = f.t[2];
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const double oi = __shfl_xor(best_iou, o, 64);
        const int ok = __shfl_xor(best_k, o, 64);
        if (vv_pose_better(oi, ok, best_iou, best_k)) best_iou = oi, best_k = ok;
    }
    // every lane now names the same winner; its translation sits in the lane that evaluated it (that lane's own best is the winner:
    // the order is total).  No winner: lane 0 is read, whose translation is still zero unless it holds a candidate -- so select.
    const int src = best_k >= 0 ? (best_k & 63) : lane;
    t0 = __shfl(t0, src, 64), t1 = __shfl(t1, src, 64), t2 = __shfl(t2, src, 64);
    if (lane != 0) return;
    VvPoseObject o;
    o.candidate = best_k, o.iou = best_iou;
    o.X[0] = best_k >= 0 ? t0 : 0.0, o.X[1] = best_k >= 0 ? t1 : 0.0, o.X[2] = best_k >= 0 ? t2 : 0.0;
    vv_pose_finish(b3, cam, box, R, o);
    keep[i] = o.keep, candidate[i] = o.candidate, iou[i] = (float)o.iou;
    unsigned *row = rows + i * OP_ROW_WORDS;
#pragma unroll
    for (int e = 0; e < 16; ++e) row[e] = __float_as_uint(o.pose[e]);
#pragma unroll
    for (int e = 0; e < 3; ++e) row[16 + e] = __float_as_uint(o.size[e]);
#pragma unroll
    for (int e = 0; e < 16; ++e) row[19 + e] = __float_as_uint(o.proj[e]);
#pragma unroll
    for (int e = 0; e < 4; ++e) row[35 + e] = (unsigned)o.box2d[e];
}

// One workgroup.  Kept detection i goes to row (kept detections before i): rows at or past the count are not written.
__global__ __launch_bounds__(OP_THREADS) void op_compact_kernel(const int *__restrict__ keep, const unsigned *__restrict__ rows, int n,
                                                                int *__restrict__ count, int *__restrict__ index, float *__restrict__ pose,
                                                                float *__restrict__ size, int *__restrict__ box2d,
                                                                float *__restrict__ box3d_proj) {
    __shared__ int wtot[OP_THREADS / 64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int carry = 0;
    for (int i0 = 0; i0 < n; i0 += OP_THREADS) {
        const int i = i0 + tid;
        const bool k = i < n && keep[i] != 0;
        const unsigned long long m = __builtin_amdgcn_ballot_w64(k);
        const int below = (int)__builtin_amdgcn_mbcnt_hi((unsigned)(m >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)m, 0u));
        if (lane == 0) wtot[wave] = __builtin_popcountll(m);
        __syncthreads();
        int before = carry;
        for (int w = 0; w < wave; ++w) before += wtot[w];
        if (k) {
            const long long r = before + below;                                  // <= i < n
            const unsigned *row = rows + (long long)i * OP_ROW_WORDS;
            index[r] = i;
#pragma unroll
            for (int e = 0; e < 16; ++e) pose[r * 16 + e] = __uint_as_float(row[e]);
#pragma unroll
            for (int e = 0; e < 3; ++e) size[r * 3 + e] = __uint_as_float(row[16 + e]);
#pragma unroll
            for (int e = 0; e < 16; ++e) box3d_proj[r * 16 + e] = __uint_as_float(row[19 + e]);
#pragma unroll
            for (int e = 0; e < 4; ++e) box2d[r * 4 + e] = (int)row[35 + e];
        }
        carry += wtot[0] + wtot[1] + wtot[2] + wtot[3];
        __syncthreads();
    }
    if (tid == 0) count[0] = carry;
}

inline bool op_shape_ok(int n, double image_col, double image_row) {
    return n >= 1 && n <= OP_MAX_N && image_col > 0.0 && image_row > 0.0 && image_col < 1e9 && image_row < 1e9;   // (a NaN size fails)
}
inline bool op_misaligned(const void *p, unsigned mask) { return (reinterpret_cast<uintptr_t>(p) & mask) != 0; }

inline VvPoseCamera op_camera(const double *proj, const double *proj_inv, double image_col, double image_row) {
    VvPoseCamera cam;
    for (int e = 0; e < 16; ++e) cam.P[e] = proj[e], cam.Pinv[e] = proj_inv[e];
    cam.col = image_col, cam.row = image_row;
    return cam;
}

}  // namespace

VV_EXPORT size_t vv_object_pose_workspace_bytes(int n) {
    if (n < 1 || n > OP_MAX_N) return 0;
    return (size_t)n * OP_ROW_WORDS * sizeof(unsigned);
}

VV_EXPORT int vv_object_pose(const float *bbox2d, const float *bbox3d, const float *sin_aei, const float *cos_aei, int n, double image_col,
                             double image_row, const double *proj, const double *proj_inv, int *keep, int *candidate, float *iou,
                             int *count, int *index, float *pose, float *size, int *box2d, float *box3d_proj, void *workspace,
                             size_t workspace_bytes, void *stream) {
    if (!bbox2d || !bbox3d || !sin_aei || !cos_aei || !proj || !proj_inv || !keep || !candidate || !iou || !count || !index || !pose ||
        !size || !box2d || !box3d_proj || !workspace)
        return VV_ERR_NULL;
    if (!op_shape_ok(n, image_col, image_row)) return VV_ERR_SHAPE;
    if (op_misaligned(bbox2d, 3u) || op_misaligned(bbox3d, 3u) || op_misaligned(sin_aei, 3u) || op_misaligned(cos_aei, 3u) ||
        op_misaligned(proj, 7u) || op_misaligned(proj_inv, 7u) || op_misaligned(keep, 3u) || op_misaligned(candidate, 3u) ||
        op_misaligned(iou, 3u) || op_misaligned(count, 3u) || op_misaligned(index, 3u) || op_misaligned(pose, 3u) ||
        op_misaligned(size, 3u) || op_misaligned(box2d, 3u) || op_misaligned(box3d_proj, 3u) || op_misaligned(workspace, 3u))
        return VV_ERR_ALIGN;                                                     // natural alignment of the element types, no more
    if (workspace_bytes < vv_object_pose_workspace_bytes(n)) return VV_ERR_WORKSPACE;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const VvPoseCamera cam = op_camera(proj, proj_inv, image_col, image_row);    // read now: the caller's arrays may change after the call
    unsigned *rows = reinterpret_cast<unsigned *>(workspace);
    const unsigned grid = (unsigned)((n + OP_THREADS / 64 - 1) / (OP_THREADS / 64));
    VV_LAUNCH(op_fit_kernel, dim3(grid), dim3(OP_THREADS), 0, st, bbox2d, bbox3d, sin_aei, cos_aei, n, cam, keep, candidate, iou, rows);
    const int rc = vv_launch_status();
    if (rc != VV_OK) return rc;
    VV_LAUNCH(op_compact_kernel, dim3(1), dim3(OP_THREADS), 0, st, keep, rows, n, count, index, pose, size, box2d, box3d_proj);
    return vv_launch_status();
}

VV_EXPORT int vv_object_pose_host(const float *bbox2d, const float *bbox3d, const float *sin_aei, const float *cos_aei, int n,
                                  double image_col, double image_row, const double *proj, const double *proj_inv, int *keep, int *candidate,
                                  float *iou, int *count, int *index, float *pose, float *size, int *box2d, float *box3d_proj,
                                  double *translation, int sweeps) {
    if (!bbox2d || !bbox3d || !sin_aei || !cos_aei || !proj || !proj_inv || !keep || !candidate || !iou || !count || !index || !pose ||
        !size || !box2d || !box3d_proj)
        return VV_ERR_NULL;
    if (!op_shape_ok(n, image_col, image_row) || sweeps > 64) return VV_ERR_SHAPE;
    if (op_misaligned(bbox2d, 3u) || op_misaligned(bbox3d, 3u) || op_misaligned(sin_aei, 3u) || op_misaligned(cos_aei, 3u) ||
        op_misaligned(proj, 7u) || op_misaligned(proj_inv, 7u) || op_misaligned(keep, 3u) || op_misaligned(candidate, 3u) ||
        op_misaligned(iou, 3u) || op_misaligned(count, 3u) || op_misaligned(index, 3u) || op_misaligned(pose, 3u) ||
        op_misaligned(size, 3u) || op_misaligned(box2d, 3u) || op_misaligned(box3d_proj, 3u) || op_misaligned(translation, 7u))
        return VV_ERR_ALIGN;
    const VvPoseCamera cam = op_camera(proj, proj_inv, image_col, image_row);
    int kept = 0;
    for (int i = 0; i < n; ++i) {
        VvPoseObject o;
        vv_pose_object(bbox2d + (size_t)i * 5, bbox3d + (size_t)i * 3, sin_aei + (size_t)i * 3, cos_aei + (size_t)i * 3, cam,
                       sweeps > 0 ? sweeps : VV_POSE_SWEEPS, o);
        keep[i] = o.keep, candidate[i] = o.candidate, iou[i] = (float)o.iou;
        if (translation)
            for (int e = 0; e < 3; ++e) translation[(size_t)i * 3 + e] = o.X[e];
        if (!o.keep) continue;
        const size_t r = (size_t)kept++;
        index[r] = i;
        for (int e = 0; e < 16; ++e) pose[r * 16 + e] = o.pose[e], box3d_proj[r * 16 + e] = o.proj[e];
        for (int e = 0; e < 3; ++e) size[r * 3 + e] = o.size[e];
        for (int e = 0; e < 4; ++e) box2d[r * 4 + e] = o.box2d[e];
    }
    count[0] = kept;
    return VV_OK;
}

// ---- the reference's single-object helpers on the host (src/visualizer/visualizer.py drop-ins): float64 in, float64 out
VV_EXPORT int vv_pose_translation_host(const double *proj, const double *rotation, const double *box2d, const double *whl, double *translation,
                                       int *candidate, double *iou) {
    if (!proj || !rotation || !box2d || !whl || !translation) return VV_ERR_NULL;
    if (op_misaligned(proj, 7u) || op_misaligned(rotation, 7u) || op_misaligned(box2d, 7u) || op_misaligned(whl, 7u) ||
        op_misaligned(translation, 7u) || op_misaligned(candidate, 3u) || op_misaligned(iou, 7u))
        return VV_ERR_ALIGN;
    double best;
    const int k = vv_pose_fit(proj, rotation, box2d, whl[0], whl[1], whl[2], VV_POSE_SWEEPS, &best, translation);
    if (candidate) *candidate = k;
    if (iou) *iou = best;
    return VV_OK;
}

VV_EXPORT int vv_pose_ray_host(const double *proj_inv, double px, double py, double *ray) {
    if (!proj_inv || !ray) return VV_ERR_NULL;
    if (op_misaligned(proj_inv, 7u) || op_misaligned(ray, 7u)) return VV_ERR_ALIGN;
    vv_pose_ray(proj_inv, px, py, ray);
    return VV_OK;
}

VV_EXPORT int vv_pose_ray_rotation_host(const double *ray, double *rotation) {
    if (!ray || !rotation) return VV_ERR_NULL;
    if (op_misaligned(ray, 7u) || op_misaligned(rotation, 7u)) return VV_ERR_ALIGN;
    vv_pose_ray_rotation(ray, rotation);
    return VV_OK;
}

VV_EXPORT int vv_pose_box_projection_host(const double *proj, const double *rotation, const double *translation, double w, double h, double l,
                                          double *corners) {
    if (!proj || !rotation || !translation || !corners) return VV_ERR_NULL;
    if (op_misaligned(proj, 7u) || op_misaligned(rotation, 7u) || op_misaligned(translation, 7u) || op_misaligned(corners, 7u))
        return VV_ERR_ALIGN;
    vv_pose_box_projection(proj, rotation, translation, w, h, l, corners);
    return VV_OK;
}
