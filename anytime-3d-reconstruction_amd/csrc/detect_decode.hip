// The detector head's output -> the selected detections of B frames: the reference's nolbo_test.getPred up to its NMS
// (src/module/nolbo_test.py:81-153, :214-255; src/module/function.py:117-150), for head outputs that are already in device memory.  The
// arithmetic and every decision are detect_decode.h, float32, shared with the host entry.
//
// Form.  ONE launch, one 256-thread workgroup per frame; everything between the head output and the output rows lives in LDS.
//   decode   threads stride over the cells in pieces of 256.  A thread takes the sigmoid of its cell's P objectness logits, counts the
//            candidates (0 .. P, or 0 .. 1 with top_1) and places them: the exclusive prefix of the counts inside a wave is five ballots
//            and population counts (one per bit of the count), the waves' totals go through 16 bytes of LDS, a running carry crosses
//            the pieces -- candidates land in cell order, inside a cell in descending objectness (object_pose.hip and voxel_points.hip
//            order their rows the same way).  Score and flat index of a candidate: 8 bytes of LDS.
//   rank     by counting: rank_i = #{j : s_j > s_i or (s_j == s_i and j > i)}, order[rank_i] = i; the thread that ranked a candidate
//            computes its box and stores it AT THE RANK (16 bytes of LDS), so the scan reads boxes and flags in its own order.
//   scan     in rank order; for each live candidate every thread tests its share of the later live ones; one barrier per pick, dead
//            candidates are skipped four flags at a time without one (the skip reads only flags up to the next pick, the tests
//            write only above it).
//   gather   the survivors (live after the scan) are numbered by ballot and population count again; the picked rows' fields are read
//            from the head output, activated and written in pick order.
// No sort, no atomics, no inline assembly: a given input gives the same bits on every run.  gfx950 only.
#include "common.h"
#include "detect_decode.h"

#include <vector>

namespace {

constexpr int DD_THREADS = 256;          // 4 waves
// dynamic LDS for `slots` candidate slots: box 16 + score 4 + flat index 4 + order 2 + pick 2 + live 1 bytes per slot, the piece's
// objectness values [16][256], the waves' totals
constexpr int DD_FIXED_BYTES = VV_DET_MAX_P * DD_THREADS * 4 + 64;
inline int dd_lds_bytes(int slots) { return ((slots + 3) & ~3) * 29 + DD_FIXED_BYTES; }
constexpr int DD_MAX_LDS = VV_DET_MAX_SLOTS * 29 + DD_FIXED_BYTES;          // 135232 of the CU's 163840

struct DdArgs {
    const float *head;
    int layout, R, C, P, Z, top_1, slots;
    float obj_thresh, iou_thresh;
    int *count, *index;
    float *bbox2d, *bbox3d, *inst_mean, *inst_log_var, *sn, *cs, *rad;
};

// Exclusive prefix of v (0 .. 31) over the lanes of a wave, and the wave's total: a ballot and a population count per bit of v.
__device__ __forceinline__ int dd_wave_prefix(int v, int &total) {
    int below = 0;
    total = 0;
#pragma unroll
    for (int k = 0; k < 5; ++k) {
        const unsigned long long m = __builtin_amdgcn_ballot_w64(((v >> k) & 1) != 0);
        below += (int)__builtin_amdgcn_mbcnt_hi((unsigned)(m >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)m, 0u)) << k;
        total += __builtin_popcountll(m) << k;
    }
    return below;
}

__global__ __launch_bounds__(DD_THREADS) void dd_frame_kernel(const DdArgs a) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int S = (a.slots + 3) & ~3;
    float *box = reinterpret_cast<float *>(smem);                          // [S][4] by RANK
    float *score = box + (size_t)S * 4;                                    // [S]
    int *cand = reinterpret_cast<int *>(score + S);                        // [S]   cell * P + predictor
    unsigned short *order = reinterpret_cast<unsigned short *>(cand + S);  // [S]   order[rank] = candidate
    unsigned short *pick = order + S;                                      // [S]   pick[row] = rank
    unsigned char *live = reinterpret_cast<unsigned char *>(pick + S);     // [S]   by RANK
    float *cell_s = reinterpret_cast<float *>(live + S);                   // [16][256]
    int *wtot = reinterpret_cast<int *>(cell_s + VV_DET_MAX_P * DD_THREADS);   // [4]

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int b = blockIdx.x, cells = a.R * a.C, P = a.P, Z = a.Z, width = vv_det_width(Z);
    const VvDetFrame f = vv_det_frame(a.head, a.layout, b, cells, P * width);
    const float thr = a.obj_thresh;

    // ---- decode
    int carry = 0;
    for (int c0 = 0; c0 < cells; c0 += DD_THREADS) {
        const int cell = c0 + tid;
        int cnt = 0;
        if (cell < cells) {
            for (int p = 0; p < P; ++p) {
                const float s = vv_det_sigmoid(vv_det_at(f, cell, p * width + VV_DET_OBJ));
                cell_s[p * DD_THREADS + tid] = s;                          // this thread's column: read back by this thread only
                cnt += s > thr ? 1 : 0;
            }
            if (a.top_1 && cnt > 1) cnt = 1;
        }
        int total;
        const int below = dd_wave_prefix(cnt, total);
        if (lane == 0) wtot[wave] = total;
        __syncthreads();
        int first = carry + below;
        for (int w = 0; w < wave; ++w) first += wtot[w];
        if (cnt > 0) {
            for (int p = 0; p < P; ++p) {
                const float sp = cell_s[p * DD_THREADS + tid];
                if (!(sp > thr)) continue;
                int before = 0;
                for (int q = 0; q < P; ++q) before += vv_det_cell_before(cell_s[q * DD_THREADS + tid], q, sp, p) ? 1 : 0;
                if (a.top_1 && before > 0) continue;
                const int j = first + before;                              // < the frame's candidate total <= slots
                score[j] = sp, cand[j] = cell * P + p;
            }
        }
        carry += wtot[0] + wtot[1] + wtot[2] + wtot[3];
        __syncthreads();
    }
    const int n = carry;                                                   // uniform: every thread summed the same totals

    // ---- rank; a candidate's box is computed here and lands at its RANK, so that the scan reads boxes and flags in its own order
    for (int i = tid; i < n; i += DD_THREADS) {
        const float si = score[i];
        int rank = 0;
        for (int j = 0; j < n; ++j) rank += vv_det_rank_before(score[j], j, si, i) ? 1 : 0;
        order[rank] = (unsigned short)i;                                   // a permutation: the order is total
        live[i] = 1;
        const int c = cand[i], cell = c / P, gr = cell / a.C;
        vv_det_box(f, cell, c - cell * P, width, gr, cell - gr * a.C, a.R, a.C, box + (size_t)rank * 4);
    }
    for (int i = n + tid; i < ((n + 3) & ~3); i += DD_THREADS) live[i] = 0;   // the scan reads the flags four at a time (<= S)
    __syncthreads();

    // ---- greedy scan.  Dead candidates are skipped four flags at a time and without a barrier: a wave that is ahead writes flags
    // above the next pick only, and the first live flag at or after i + 1 IS the next pick, whatever the flags above it hold.
    const unsigned *live4 = reinterpret_cast<const unsigned *>(live);
    for (int i = 0; i < n; ++i) {
        const unsigned w = __builtin_amdgcn_readfirstlane(live4[i >> 2]) >> ((i & 3) * 8);
        if (w == 0) {
            i |= 3;
            continue;
        }
        i += __builtin_ctz(w) >> 3;                                        // < n: the flags at and past n are zero
        float ba[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) ba[e] = box[(size_t)i * 4 + e];
        for (int k = i + 1 + tid; k < n; k += DD_THREADS)
            if (live[k] && vv_det_suppresses(ba, box + (size_t)k * 4, a.iou_thresh)) live[k] = 0;
        __syncthreads();
    }
    __syncthreads();

    // ---- number the survivors in rank order
    carry = 0;
    for (int i0 = 0; i0 < n; i0 += DD_THREADS) {
        const int i = i0 + tid;
        const bool k = i < n && live[i] != 0;
        int total;
        const int below = dd_wave_prefix(k ? 1 : 0, total);
        if (lane == 0) wtot[wave] = total;
        __syncthreads();
        int row = carry + below;
        for (int w = 0; w < wave; ++w) row += wtot[w];
        if (k) pick[row] = (unsigned short)i;                              // row <= i < n
        carry += wtot[0] + wtot[1] + wtot[2] + wtot[3];
        __syncthreads();
    }
    const int count = carry;
    if (tid == 0) a.count[b] = count;

    // ---- gather: rows below count only
    const long long out0 = (long long)b * a.slots;
    for (int row = tid; row < count; row += DD_THREADS) {
        const int rk = pick[row], pa = order[rk];
        a.index[out0 + row] = cand[pa];
        float *o = a.bbox2d + (out0 + row) * 5;
#pragma unroll
        for (int e = 0; e < 4; ++e) o[e] = box[(size_t)rk * 4 + e];
        o[4] = score[pa];
    }
    const int F = 2 * Z + 12;
    for (int t = tid; t < count * F; t += DD_THREADS) {                     // <= 4096 * 140
        const int row = t / F, e = t - row * F;
        const int c = cand[order[pick[row]]];
        const int cell = c / P, p = c - cell * P;
        vv_det_store_row_value(Z, out0 + row, e, vv_det_row_value(f, cell, p, Z, e), a.bbox3d, a.inst_mean, a.inst_log_var, a.sn, a.cs,
                               a.rad);
    }
}

inline bool dd_misaligned(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 3u) != 0; }

// -> VV_OK, or the status an inadmissible call gets; *slots = R * C * (top_1 ? 1 : P)
inline int dd_check(const void *head, int layout, int batch, int R, int C, int P, int Z, int channels, const void *count, const void *index,
                    const void *bbox2d, const void *bbox3d, const void *inst_mean, const void *inst_log_var, const void *sn, const void *cs,
                    const void *rad, int top_1, int *slots) {
    const void *ptrs[] = {head, count, index, bbox2d, bbox3d, inst_mean, inst_log_var, sn, cs, rad};
    for (const void *p : ptrs)
        if (!p) return VV_ERR_NULL;
    if (batch < 1 || R < 1 || C < 1 || P < 1 || P > VV_DET_MAX_P || Z < 1 || Z > VV_DET_MAX_Z) return VV_ERR_SHAPE;
    if (layout != VV_DET_NHWC && layout != VV_DET_NCHW) return VV_ERR_SHAPE;
    if (channels != P * vv_det_width(Z)) return VV_ERR_SHAPE;
    const long long n = (long long)R * C * (top_1 ? 1 : P);
    if (n > VV_DET_MAX_SLOTS) return VV_ERR_SHAPE;
    for (const void *p : ptrs)
        if (dd_misaligned(p)) return VV_ERR_ALIGN;                          // natural alignment of the element types, no more
    *slots = (int)n;
    return VV_OK;
}

}  // namespace

VV_EXPORT int vv_detect_decode(const float *head, int layout, int batch, int grid_row, int grid_col, int predictor_num, int z_dim,
                               int channels, float obj_thresh, float iou_thresh, int top_1, int *count, int *index, float *bbox2d,
                               float *bbox3d, float *inst_mean, float *inst_log_var, float *sin_aei, float *cos_aei, float *rad_log_var,
                               void *hip_stream) {
    int slots = 0;
    const int rc = dd_check(head, layout, batch, grid_row, grid_col, predictor_num, z_dim, channels, count, index, bbox2d, bbox3d, inst_mean,
                            inst_log_var, sin_aei, cos_aei, rad_log_var, top_1, &slots);
    if (rc != VV_OK) return rc;
    DdArgs a;
    a.head = head, a.layout = layout, a.R = grid_row, a.C = grid_col, a.P = predictor_num, a.Z = z_dim, a.top_1 = top_1 ? 1 : 0;
    a.slots = slots, a.obj_thresh = obj_thresh, a.iou_thresh = iou_thresh, a.count = count, a.index = index, a.bbox2d = bbox2d;
    a.bbox3d = bbox3d, a.inst_mean = inst_mean, a.inst_log_var = inst_log_var, a.sn = sin_aei, a.cs = cos_aei, a.rad = rad_log_var;
    vv_allow_lds<&dd_frame_kernel>(DD_MAX_LDS);
    VV_LAUNCH(dd_frame_kernel, dim3((unsigned)batch), dim3(DD_THREADS), (size_t)dd_lds_bytes(slots), reinterpret_cast<hipStream_t>(hip_stream), a);
    return vv_launch_status();
}

VV_EXPORT int vv_detect_decode_host(const float *head, int layout, int batch, int grid_row, int grid_col, int predictor_num, int z_dim,
                                    int channels, float obj_thresh, float iou_thresh, int top_1, int *count, int *index, float *bbox2d,
                                    float *bbox3d, float *inst_mean, float *inst_log_var, float *sin_aei, float *cos_aei,
                                    float *rad_log_var) {
    int slots = 0;
    const int rc = dd_check(head, layout, batch, grid_row, grid_col, predictor_num, z_dim, channels, count, index, bbox2d, bbox3d, inst_mean,
                            inst_log_var, sin_aei, cos_aei, rad_log_var, top_1, &slots);
    if (rc != VV_OK) return rc;
    const size_t N = (size_t)slots, Z = (size_t)z_dim;
    std::vector<float> score(N), box(N * 4);
    std::vector<int> cand(N), order(N);
    std::vector<unsigned char> live(N);
    for (int b = 0; b < batch; ++b) {
        const VvDetFrame f = vv_det_frame(head, layout, b, grid_row * grid_col, channels);
        const size_t o = (size_t)b * N;
        count[b] = vv_det_frame_host(f, grid_row, grid_col, predictor_num, z_dim, obj_thresh, iou_thresh, top_1 ? 1 : 0, score.data(),
                                     box.data(), cand.data(), order.data(), live.data(), index + o, bbox2d + o * 5, bbox3d + o * 3,
                                     inst_mean + o * Z, inst_log_var + o * Z, sin_aei + o * 3, cos_aei + o * 3, rad_log_var + o * 3);
    }
    return VV_OK;
}

// The header's activations alone, on the host: which = 0 exp, 1 sigmoid, 2 tanh.
VV_EXPORT int vv_detect_activation_host(const float *x, float *y, long n, int which) {
    if (!x || !y) return VV_ERR_NULL;
    if (n < 0 || which < 0 || which > 2) return VV_ERR_SHAPE;
    if (dd_misaligned(x) || dd_misaligned(y)) return VV_ERR_ALIGN;
    for (long i = 0; i < n; ++i) y[i] = which == 0 ? vv_det_exp(x[i]) : (which == 1 ? vv_det_sigmoid(x[i]) : vv_det_tanh(x[i]));
    return VV_OK;
}
