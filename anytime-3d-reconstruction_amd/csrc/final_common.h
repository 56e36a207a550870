// What the last decoder layer's kernels share (Conv3DTranspose k4 s2 SAME 64 -> 1, sigmoid, weighted BCE, TP / FP / FN):
//   final_bce.hip      final_bce_kernel<T>, final_bce_mfma_kernel (box forms), final_bce_sweep_kernel (P form), final_bce_sweepw_kernel (Q form)
//   final_bce_fp8.hip  final_bce_sweep_fp8_kernel (P form, e4m3fn input)
//   final_mean.hip     final_mean_box_kernel<T>, final_mean_sweep_kernel (Q form over K samples), final_mean_finish_kernel
// Here, once: the geometry constants, the workgroup-to-tile order, the box and sweep lane roles with their output index, the box
// staging, the per-voxel loss in its three arithmetic forms, the block reduction to one partial, and every piece of the Q form that
// the single-sample and the sampled-mean sweep have in common (staging lane offsets, weight operand, operand slots, qkey, the
// MFMAs of a plane, Q publish, Q gather).  Stage lambdas, loops, target loads and counted waits stay in the kernels, and so do the
// P-form gathers: the bf16 one reads swizzled 16-byte quads, the fp8 one unswizzled dwords from two PH buffers.
// Plain __forceinline__ functions wherever they leave final_bce_sweepw_kernel's generated code alone; FL_BLOCK_STATS and the FL_Q_*
// body pieces are macros because as functions they do not (see FL_BLOCK_STATS).
#pragma once
#include "common.h"

constexpr int FL_CIN = 64;                  // input channels
constexpr int FL_BOX_ROW = FL_CIN + 4;      // box forms: floats per staged voxel row (+16 B pad against bank conflicts)
constexpr int FL_ROWS = 100;                // sweep forms: 10 x 10 halo rows of an 8 x 8 cell tile
#ifndef VV_SW_DEPTH
#define VV_SW_DEPTH 1            // input planes in flight ahead of the one being multiplied (ring = depth + 1 slots)
#endif
constexpr int FL_DEPTH = VV_SW_DEPTH;
constexpr int FL_XB = 13 * 1024, FL_NX = FL_DEPTH + 1;   // bf16 plane slot (104 rows x 128 B), ring depth
constexpr int FL_QB = 80 * 128;             // Q_d [80 centre cells][td 4][th 4][pw 2] float32

// final_bce.hip: per-sample (bce, TP, FP, FN) from the partial blocks, lanes over blocks b, b + 64, ... then the wave sum
void vv_final_reduce_launch(const float *partials, float *stats, int nblk, int batch, hipStream_t st);
// final_bce_fp8.hip: sweep-form last layer with an e4m3fn input; returns the partial blocks per sample.
int vv_final_bce_sweep_fp8_launch(const void *x, const float *w_keras, const float *target, float *probs, float *logits, float *partials,
                                  int batch, int side, float gamma, float epsilon, hipStream_t st);

// XCD-aware order (workgroups are dealt round-robin over 8 XCDs): block g takes item (g % 8) * (T / 8) + g / 8 of the sample-major
// list, so the halo tiles of neighbouring blocks of one sample are re-read from ONE XCD's L2.
__device__ __forceinline__ int fl_work_item() {
    const int T = gridDim.x;
    return (T & 7) ? (int)blockIdx.x : (int)(blockIdx.x & 7) * (T >> 3) + (int)(blockIdx.x >> 3);
}

// index of output voxel (od, oh, ow) of sample b; lo = log2 of the output side
__device__ __forceinline__ size_t fl_out_index(int b, int od, int oh, int ow, int lo) {
    return ((((((size_t)b << lo) + od) << lo) + oh) << lo) + ow;
}

// ---------------------------------------------------------------------------------------------------------------
// Box forms: one workgroup = a 4x4x4 block of input-grid cells (-> 8x8x8 outputs); wave w owns output parity (pd, ph) = (w >> 1, w & 1),
// a lane one cell (md, mh, mw) with both pw parities.
struct FlBox {
    int m0d, m0h, m0w;          // first cell of the block
    int pd, ph, md, mh, mw;
    __device__ __forceinline__ size_t out(int b, int li) const {     // the lane's output pair
        return fl_out_index(b, 2 * (m0d + md) + pd, 2 * (m0h + mh) + ph, 2 * (m0w + mw), li + 1);
    }
};
__device__ __forceinline__ FlBox fl_box(int blk, int nb, int wv, int lane) {   // nb = blocks per axis
    FlBox g;
    g.m0w = (blk % nb) * 4; g.m0h = ((blk / nb) % nb) * 4; g.m0d = (blk / (nb * nb)) * 4;
    g.pd = wv >> 1; g.ph = wv & 1;
    g.mw = lane & 3; g.mh = (lane >> 2) & 3; g.md = lane >> 4;
    return g;
}

// stage the 6^3 halo tile of a block as float32 rows: 216 voxels x 64 channels, 16 B (= 4 f32 / 8 bf16 -> split) per lane per step
template <typename T>
__device__ __forceinline__ void fl_box_stage(const T *xb, float *tile, const FlBox &g, int li) {
    const int n = 1 << li;
    constexpr int EPL = 16 / sizeof(T);          // elements per 16-byte load
    constexpr int LPV = FL_CIN / EPL;            // loads per voxel
    for (int i = threadIdx.x; i < 216 * LPV; i += 256) {
        const int vox = i / LPV, part = i % LPV;
        const int zw = vox % 6, zh = (vox / 6) % 6, zd = vox / 36;
        const int id = g.m0d - 1 + zd, ih = g.m0h - 1 + zh, iw = g.m0w - 1 + zw;
        float vals[EPL];
        if ((unsigned)id < (unsigned)n && (unsigned)ih < (unsigned)n && (unsigned)iw < (unsigned)n) {
            const T *src = xb + ((((size_t)id << li) + ih << li) + iw) * FL_CIN + part * EPL;
            const uint4 raw = *reinterpret_cast<const uint4 *>(src);
            const T *rv = reinterpret_cast<const T *>(&raw);
#pragma unroll
            for (int e = 0; e < EPL; ++e) vals[e] = static_cast<float>(rv[e]);
        } else {
#pragma unroll
            for (int e = 0; e < EPL; ++e) vals[e] = 0.f;
        }
        float *dst = tile + vox * FL_BOX_ROW + part * EPL;
#pragma unroll
        for (int e = 0; e < EPL; e += 4) *reinterpret_cast<f32x4 *>(dst + e) = f32x4{vals[e], vals[e + 1], vals[e + 2], vals[e + 3]};
    }
}

// ---------------------------------------------------------------------------------------------------------------
// Sweep forms: one workgroup = an 8 x 8 tile of cells in (h, w) swept through the depth; a step finishes two output planes of 16 x 16
// voxels.  Gather role of a thread: sl = od parity slot, ohh = output row inside the tile, mw = cell column (both pw per lane).
struct FlRole {
    int mw, ohh, sl, mh, ph;
    __device__ __forceinline__ int oh(int h0) const { return 2 * h0 + ohh; }        // output row / first output column, tile at (h0, w0)
    __device__ __forceinline__ int ow(int w0) const { return 2 * (w0 + mw); }
};
__device__ __forceinline__ FlRole fl_role(int tid) {
    FlRole r;
    r.mw = tid & 7; r.ohh = (tid >> 3) & 15; r.sl = tid >> 7;
    r.mh = r.ohh >> 1; r.ph = r.ohh & 1;
    return r;
}

// ---------------------------------------------------------------------------------------------------------------
// binary_loss / voxelPrecisionRecall of one voxel (function.py:79-80, 110) in the three arithmetic forms the kernels use.  They are
// NOT interchangeable: each kernel's sums are pinned bit for bit to its form.
//   FL_PRECISE  expf / logf, threshold on p >= 0.5                  (box kernels, mean finish)
//   FL_HW       hardware rcp / exp / log (relative error ~1e-7, far below the bf16 operand rounding), threshold on the logit
//               (sigmoid(l) >= 0.5 <=> l >= 0)                      (P-form sweeps)
//   FL_HW01     FL_HW with one logarithm per voxel when every target of the wave is 0 or 1: then exactly one of the two terms has a
//               non-zero factor and the other is +-0 -- the same sum.  Any other target value in the wave (`soft`) takes the
//               general form.                                        (Q-form sweep)
enum { FL_PRECISE, FL_HW, FL_HW01 };

template <int FORM>
__device__ __forceinline__ float fl_sigmoid(float l) {               // tf.sigmoid, autoencoder3D.py:136
    return FORM == FL_PRECISE ? 1.0f / (1.0f + expf(-l)) : __builtin_amdgcn_rcpf(1.0f + __expf(-l));
}

// p = the probability, l = its logit (read by the hardware forms only), hi = 1 - epsilon (0.99999988 in float32, function.py:79; formed
// by the kernel in front of its loop), soft: FL_HW01 only
template <int FORM>
__device__ __forceinline__ void fl_voxel_stats(float p, float l, float y, float gamma, float epsilon, float hi, bool soft, float &bce,
                                               float &tp, float &fp, float &fn) {
    const float q = fminf(fmaxf(p, epsilon), hi);
    if (FORM == FL_PRECISE) bce -= gamma * y * logf(q) + (1.0f - gamma) * (1.0f - y) * logf(1.0f - q);
    else if (FORM == FL_HW || soft) bce -= gamma * y * __logf(q) + (1.0f - gamma) * (1.0f - y) * __logf(1.0f - q);
    else bce -= (y != 0.f ? gamma : 1.0f - gamma) * __logf(y != 0.f ? q : 1.0f - q);
    const float yh = (FORM == FL_PRECISE ? p >= 0.5f : l >= 0.f) ? 1.f : 0.f;
    tp += y * yh; fp += (1.f - y) * yh; fn += y * (1.f - yh);
}

// the output pair (pw 0, pw 1) of a lane of a single-sample kernel: logits -> probabilities, loss terms added
template <int FORM>
__device__ __forceinline__ float2 fl_pair_stats(float l0, float l1, float2 y, float gamma, float epsilon, float hi, float &bce, float &tp,
                                                float &fp, float &fn) {
    const bool soft = FORM == FL_HW01 && __builtin_amdgcn_ballot_w64((y.x != 0.f && y.x != 1.f) || (y.y != 0.f && y.y != 1.f)) != 0;
    const float l[2] = {l0, l1}, yy[2] = {y.x, y.y};
    float p[2];
#pragma unroll
    for (int e = 0; e < 2; ++e) {
        p[e] = fl_sigmoid<FORM>(l[e]);
        fl_voxel_stats<FORM>(p[e], l[e], yy[e], gamma, epsilon, hi, soft, bce, tp, fp, fn);
    }
    return make_float2(p[0], p[1]);
}

// Wave shuffles, then the four waves in order: partial `blk` of `partials` = this workgroup's (bce, TP, FP, FN).  `red` = float[4][4] in
// LDS, tid = threadIdx.x, wv = the wave (tid >> 6, as the kernel holds it).  A macro, like the Q pieces marked so below: a
// __forceinline__ function is optimised on its own before it is inlined, and final_bce_sweepw_kernel -- whose generated code is
// pinned -- then comes out with other register assignments and another instruction order.  As text in the kernel body it is the
// code the kernel had.
#define FL_BLOCK_STATS(bce, tp, fp, fn, tid, wv, red, partials, blk)                                                                   \
    do {                                                                                                                               \
        bce = vv_wave_sum(bce); tp = vv_wave_sum(tp); fp = vv_wave_sum(fp); fn = vv_wave_sum(fn);                                      \
        if (((tid) & 63) == 0) { red[wv][0] = bce; red[wv][1] = tp; red[wv][2] = fp; red[wv][3] = fn; }                                \
        __syncthreads();                                                                                                               \
        if ((tid) < 4) (partials)[(size_t)(blk) * 4 + (tid)] = red[0][tid] + red[1][tid] + red[2][tid] + red[3][tid];                  \
    } while (0)

// ---------------------------------------------------------------------------------------------------------------
// Q form (final_bce_sweepw_kernel, final_mean_sweep_kernel): the w direction summed INSIDE the MFMA.  The two w terms of an output
// column share their centre cell: out[2i] = x_i w[tw 1] + x_{i-1} w[tw 3], out[2i+1] = x_{i+1} w[tw 0] + x_i w[tw 2].  With K = 128 =
// (centre | left) resp. (right | centre) channels and the 16 (td, th) pairs as the MFMA's rows (v_mfma_f32_16x16x32_bf16), the matrix
// pipe delivers Q[centre cell][td][th][pw], and an output pair reads ONE 8-byte granule per (ah, td).
// The pieces that sit in the kernel BODY are macros for the reason given at FL_BLOCK_STATS (each was tried as a __forceinline__
// function and moved final_bce_sweepw_kernel); they name the kernels' locals li, n, h0, w0, wv, lane and declare the ones listed.
// fl_qkey and fl_q_mfma_plane are functions: the kernels always had those as lambdas, which the compiler treats the same way.

// Staging of a plane: 13 pieces of 8 rows; every wave issues 4 (the 3 surplus ones go to the sink behind the ring so that the
// vector-memory counter advances uniformly).  Declares sv[4], sdst[4]: the lane part of a piece's source offset (sample B0, halo row,
// swizzled slot; out-of-range if the row is outside the grid or past the 100 halo rows) and its place in a ring slot, prepared
// once; what changes from plane to plane rides in the kernel's soffset.
#define FL_Q_STAGE_LANES(B0)                                                                                                           \
    unsigned sv[4], sdst[4];                                                                                                           \
    _Pragma("unroll") for (int i = 0; i < 4; ++i) {                                                                                    \
        const int piece = wv * 4 + i, row = piece * 8 + (lane >> 3);                                                                   \
        const int zh = row / 10, zw = row - zh * 10;                                                                                   \
        const int ih = h0 - 1 + zh, iw = w0 - 1 + zw;                                                                                  \
        const bool ok = row < FL_ROWS && (unsigned)ih < (unsigned)n && (unsigned)iw < (unsigned)n;                                     \
        const int g = (lane & 7) ^ (zw & 7); /* slot key zw & 7: conflict-free for the 16x16x32 operand reads of centre / left / right cells (d5w_swz.py) */ \
        sv[i] = ok ? (unsigned)((((((B0) << li) << li) + ih) << li) + iw) * (FL_CIN * 2) + g * 16 : 0xFFFFFFF0u;                        \
        sdst[i] = piece < 13 ? (unsigned)(piece * 1024) : (unsigned)(FL_NX * FL_XB); /* surplus pieces: the sink (ring-slot independent) */ \
    }

// Declares c16, kq, wf, ntl, xo.
// wf: weights as the first MFMA operand (16 rows n = td * 4 + th, K = 128): for output-column parity pw the K halves are the taps
// (tw 1 | tw 3) of (centre | left) for pw = 0 and (tw 0 | tw 2) of (right | centre) for pw = 1; lane (n = lane & 15, kq = lane >> 4)
// holds 8 input channels of k-step ks, straight from the Keras array W = [64 taps][64 ci].
// Row tiles: tile T = 16 centre cells (zh = 2T, 2T + 1; zw = 1 .. 8); wave w owns tile w, wave 0 tile 4 as well (ntl tiles).
// xo[centre, left, right][channel half] = byte offset of this lane's operand slot inside a plane slot, tile wv (tile 4: + 80 rows).
#define FL_Q_OPERANDS(W)                                                                                                               \
    const int c16 = lane & 15, kq = lane >> 4;                                                                                         \
    uint4 wf[2][4];                                                                                                                    \
    _Pragma("unroll") for (int pw = 0; pw < 2; ++pw)                                                                                   \
        _Pragma("unroll") for (int kk = 0; kk < 4; ++kk) {                                                                             \
            const int tw = pw == 0 ? (kk < 2 ? 1 : 3) : (kk < 2 ? 0 : 2);                                                              \
            const float *wr = (W) + (c16 * 4 + tw) * FL_CIN + (kk & 1) * 32 + kq * 8;                                                  \
            const f32x4 w0v = *reinterpret_cast<const f32x4 *>(wr), w1v = *reinterpret_cast<const f32x4 *>(wr + 4);                    \
            bf16x8 o;                                                                                                                  \
            _Pragma("unroll") for (int e = 0; e < 4; ++e) { o[e] = static_cast<__bf16>(w0v[e]); o[4 + e] = static_cast<__bf16>(w1v[e]); } \
            wf[pw][kk] = *reinterpret_cast<const uint4 *>(&o);                                                                         \
        }                                                                                                                              \
    const int ntl = wv == 0 ? 2 : 1;                                                                                                   \
    const int rowC = (2 * wv + (c16 >> 3)) * 10 + 1 + (c16 & 7); /* halo row of this lane's centre cell */                             \
    unsigned xo[3][2];                                                                                                                 \
    _Pragma("unroll") for (int s3 = 0; s3 < 3; ++s3)                                                                                   \
        _Pragma("unroll") for (int hf = 0; hf < 2; ++hf) {                                                                             \
            const int sh = s3 == 0 ? 0 : s3 == 1 ? -1 : 1, zwc = 1 + (c16 & 7) + sh;                                                   \
            xo[s3][hf] = (unsigned)((rowC + sh) * 128 + (((hf * 4 + kq) ^ (zwc & 7)) << 4));                                           \
        }

// Q row of a centre cell pr = zh * 8 + (zw - 1): 16 granules of 8 B = (pw 0, pw 1) of n = td * 4 + th, granule g stored at g ^ key,
// key = ((zh + zw - 1) & 7) << 1 (bit 0 clear: the th pair of a 16-byte store stays adjacent): every ds_write_b128 lane group of the
// publish and both 32-lane passes of every ds_read_b64 of the gather are conflict-free (profiles/microbench/d5w_swz.py: exhaustive over
// linear keys under the guide's lane-group / bank model; the first key tried was 2-way on the stores)
__device__ __forceinline__ int fl_qkey(int pr) { return (((pr & 7) + (pr >> 3)) & 7) << 1; }

// Q_d[n][cell][pw] for this wave's tiles from the plane slot Xd: D[n][cell], weights first, K = (centre | left) / (right | centre)
// channels; acc[tile][pw].  The kernels call it through a one-line lambda mfma_plane(ring slot, acc), as they always did.
__device__ __forceinline__ void fl_q_mfma_plane(const char *Xd, int ntl, const unsigned (&xo)[3][2], const uint4 (&wf)[2][4], f32x4 (&acc)[2][2]) {
#pragma unroll
    for (int t = 0; t < 2; ++t) {
        acc[t][0] = f32x4{0.f, 0.f, 0.f, 0.f};
        acc[t][1] = f32x4{0.f, 0.f, 0.f, 0.f};
        if (t < ntl) {
            const char *Xt = Xd + t * (80 * 128);             // tile 4 = tile 0 + 8 halo rows of 10 cells: same zw, same slot keys
            uint4 fc[2], fl[2], fr2[2];
#pragma unroll
            for (int hf = 0; hf < 2; ++hf) {
                fc[hf] = *reinterpret_cast<const uint4 *>(Xt + xo[0][hf]);
                fl[hf] = *reinterpret_cast<const uint4 *>(Xt + xo[1][hf]);
                fr2[hf] = *reinterpret_cast<const uint4 *>(Xt + xo[2][hf]);
            }
#pragma unroll
            for (int ks = 0; ks < 4; ++ks) {                  // the two accumulators alternate: no chain of dependent MFMAs
                const uint4 &a0 = ks < 2 ? fc[ks] : fl[ks - 2], &a1 = ks < 2 ? fr2[ks] : fc[ks - 2];
                acc[t][0] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(*reinterpret_cast<const bf16x8 *>(&wf[0][ks]),
                                                                    *reinterpret_cast<const bf16x8 *>(&a0), acc[t][0], 0, 0, 0);
                acc[t][1] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(*reinterpret_cast<const bf16x8 *>(&wf[1][ks]),
                                                                    *reinterpret_cast<const bf16x8 *>(&a1), acc[t][1], 0, 0, 0);
            }
        }
    }
}

// publish ACC = Q_d into PQ: lane = centre cell (lane & 15), td = lane >> 4, registers walk th: (th 0, th 1) and (th 2, th 3) with both
// pw are two 16-byte stores per tile
#define FL_Q_PUBLISH(PQ, ACC)                                                                                                          \
    _Pragma("unroll") for (int t = 0; t < 2; ++t)                                                                                      \
        if (t < ntl) {                                                                                                                 \
            const int pr = (wv + 4 * t) * 16 + c16, key = fl_qkey(pr);                                                                 \
            char *row = (PQ) + pr * 128;                                                                                               \
            *reinterpret_cast<f32x4 *>(row + (((4 * kq) ^ key) << 3)) = f32x4{ACC[t][0][0], ACC[t][1][0], ACC[t][0][1], ACC[t][1][1]}; \
            *reinterpret_cast<f32x4 *>(row + (((4 * kq + 2) ^ key) << 3)) = f32x4{ACC[t][0][2], ACC[t][1][2], ACC[t][0][3], ACC[t][1][3]}; \
        }

// gather for the thread of role R (FlRole): the w direction is already summed inside Q, so an output pair (pw 0, pw 1) takes ONE
// 8-byte read per (ah, td): the td = sl entries are added to (L0, L1) and complete the output planes od = 2d - 1 + sl; the td = 2 + sl
// entries are added to (LO0, LO1), this plane's contribution to the next step's outputs.  Q is read in the step that publishes it,
// so one buffer holds it.
#define FL_Q_GATHER(PQ, R, L0, L1, LO0, LO1)                                                                                           \
    _Pragma("unroll") for (int ah = 0; ah < 2; ++ah) {                                                                                 \
        const int zh = (R).mh + (R).ph - ah + 1, th = 1 - (R).ph + 2 * ah;                                                             \
        const int pr = zh * 8 + (R).mw, key = fl_qkey(pr);                                                                             \
        const char *row = (PQ) + pr * 128;                                                                                             \
        const float2 qa = *reinterpret_cast<const float2 *>(row + ((((R).sl * 4 + th) ^ key) << 3));                                   \
        const float2 qb = *reinterpret_cast<const float2 *>(row + ((((2 + (R).sl) * 4 + th) ^ key) << 3));                             \
        L0 += qa.x; L1 += qa.y;                                                                                                        \
        LO0 += qb.x; LO1 += qb.y;                                                                                                      \
    }
