// The HBM-bound tail of the path (gfx950):
//   final_bce  : Conv3DTranspose k4 s2 SAME -> 1 channel, sigmoid, weighted BCE and TP/FP/FN, fused
//                (autoencoder3D.py:129-136; function.py:73-82, 100-115)
// Four kernels (VALU box, MFMA box, P-form sweep, Q-form sweep) and the reduction of their partials.  Geometry, lane roles, voxel
// loss, block reduction and the Q-form pieces shared with final_mean.hip live in final_common.h.
#include <string.h>

#include "final_common.h"

namespace {

// ---------------------------------------------------------------------------------------------------------------
// final_bce.  One workgroup = a 4x4x4 block of input-grid cells (-> 8x8x8 logits) of one sample.  The 6x6x6 input
// halo tile is staged in LDS as float32 rows (padded by 16 B against bank conflicts); wave w owns output parity
// (pd,ph) = (w>>1, w&1) and each lane both pw parities of its cell, so the 16 weight vectors a wave needs are
// wave-uniform and come through the scalar cache.  Loss terms are reduced by wave shuffles, then across the 4
// waves in LDS, and written as one partial per workgroup; final_reduce sums a sample's partials in block order.
template <typename T>
__global__ __launch_bounds__(256) void final_bce_kernel(const T *__restrict__ x, const float *__restrict__ w,
                                                        const float *__restrict__ target, float *__restrict__ probs,
                                                        float *__restrict__ logits, float *__restrict__ partials,
                                                        int din_log2, float gamma, float epsilon) {
    __shared__ __attribute__((aligned(16))) float tile[216 * FL_BOX_ROW];
    __shared__ float red[4][4];
    const int li = din_log2, nb = (1 << li) >> 2;  // blocks per axis
    const int blk = blockIdx.x, b = blockIdx.y;
    const int lane = threadIdx.x & 63;
    const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const FlBox g = fl_box(blk, nb, wv, lane);
    const int pd = g.pd, ph = g.ph, mw = g.mw, mh = g.mh, md = g.md;
    fl_box_stage(x + ((size_t)b << (3 * li)) * FL_CIN, tile, g, li);
    __syncthreads();

    float acc0 = 0.f, acc1 = 0.f;
#pragma unroll
    for (int ad = 0; ad < 2; ++ad) {
#pragma unroll
        for (int ah = 0; ah < 2; ++ah) {
            const int zd = md + pd - ad + 1, zh = mh + ph - ah + 1;
            const int td = 1 - pd + 2 * ad, th = 1 - ph + 2 * ah;
            const float *r0 = tile + ((zd * 6 + zh) * 6 + mw) * FL_BOX_ROW;  // zw = mw, mw+1, mw+2
            const float *wt = w + (size_t)((td * 4 + th) * 4) * FL_CIN;  // [tw][ci], wave-uniform
#pragma unroll 4
            for (int c = 0; c < FL_CIN; c += 4) {
                const f32x4 x0 = *reinterpret_cast<const f32x4 *>(r0 + c);
                const f32x4 x1 = *reinterpret_cast<const f32x4 *>(r0 + FL_BOX_ROW + c);
                const f32x4 x2 = *reinterpret_cast<const f32x4 *>(r0 + 2 * FL_BOX_ROW + c);
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    // pw = 0: i = mw (tw 1), mw-1 (tw 3);  pw = 1: i = mw+1 (tw 0), mw (tw 2)
                    acc0 = fmaf(x1[e], wt[1 * FL_CIN + c + e], acc0);
                    acc0 = fmaf(x0[e], wt[3 * FL_CIN + c + e], acc0);
                    acc1 = fmaf(x2[e], wt[0 * FL_CIN + c + e], acc1);
                    acc1 = fmaf(x1[e], wt[2 * FL_CIN + c + e], acc1);
                }
            }
        }
    }
    const size_t o = g.out(b, li);
    float bce = 0.f, tp = 0.f, fp = 0.f, fn = 0.f;
    const float2 p = fl_pair_stats<FL_PRECISE>(acc0, acc1, *reinterpret_cast<const float2 *>(target + o), gamma, epsilon, 1.0f - epsilon, bce, tp, fp, fn);
    if (probs) *reinterpret_cast<float2 *>(probs + o) = p;
    if (logits) *reinterpret_cast<float2 *>(logits + o) = make_float2(acc0, acc1);
    FL_BLOCK_STATS(bce, tp, fp, fn, (int)threadIdx.x, wv, red, partials, (size_t)b * gridDim.x + blk);
}

// ---------------------------------------------------------------------------------------------------------------
// final_bce on MFMA (bf16 activations), scatter form.  A transposed conv with one output channel is
//   P[i][t] = sum_ci x[i][ci] * w[t][ci]      (a [voxels x 64] x [64 x 64 taps] GEMM: v_mfma_f32_32x32x16_bf16)
//   logit[o] = sum_{(i,t) : o = 2i + t - 1} P[i][t]   (8 terms per output voxel)
// One workgroup = 4x4x4 input cells (+1 halo: 216 rows, padded to 224) -> P in LDS (f32, aliased over the
// staged operands) -> every lane gathers its 2 x 8 terms, then sigmoid / BCE / TP / FP / FN as in the VALU kernel.
constexpr int FM_ROWS = 224;            // 216 halo voxels padded to 7 MFMA row tiles
constexpr int FM_PPITCH = 33;           // floats per P row (32 taps of one half + 1: consecutive voxels on consecutive banks)

__global__ __launch_bounds__(256) void final_bce_mfma_kernel(const __bf16 *__restrict__ x, const float *__restrict__ w,
                                                             const float *__restrict__ target, float *__restrict__ probs,
                                                             float *__restrict__ logits, float *__restrict__ partials,
                                                             int din_log2, unsigned x_bytes, float gamma, float epsilon) {
    // LDS: staged operands (36 KiB), later overwritten by ONE 32-tap half of P at a time (28 KiB): 4 workgroups per CU.
    extern __shared__ __attribute__((aligned(16))) char smem[];
    char *As = smem;                                   // [224][128 B] bf16 rows, slot-swizzled (source side)
    char *Ws = smem + FM_ROWS * 128;                   // [64 taps][128 B]
    float *P = reinterpret_cast<float *>(smem);        // [216][33] f32
    __shared__ float red[4][4];
    const int li = din_log2, n = 1 << li, nb = n >> 2, nblk = nb * nb * nb;
    const int wi = fl_work_item();
    const int blk = wi % nblk, b = wi / nblk;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
    const FlBox g = fl_box(blk, nb, wv, lane);
    const int m0d = g.m0d, m0h = g.m0h, m0w = g.m0w;

    // stage A by LDS-DMA: 224 rows x 8 slots = 28 wave instructions (8 rows each); rows >= 216 and halo voxels outside
    // the grid come back as zeros (out-of-range buffer offsets)
    {
        const u32x4 rs = vv_make_rsrc(x, x_bytes);
        const unsigned lds0 = (unsigned)(unsigned long long)(lptr_t)As;
        const int pos = lane & 7, rsub = lane >> 3;
        for (int it = wv; it < FM_ROWS / 8; it += 4) {
            const int row = it * 8 + rsub;
            const int zw = row % 6, zh = (row / 6) % 6, zd = row / 36;
            const int id = m0d - 1 + zd, ih = m0h - 1 + zh, iw = m0w - 1 + zw;
            const bool ok = row < 216 && (unsigned)id < (unsigned)n && (unsigned)ih < (unsigned)n && (unsigned)iw < (unsigned)n;
            const int g = pos ^ ((row >> 1) & 7);
            const unsigned vo = ok ? (unsigned)((((((b << li) + id) << li) + ih) << li) + iw) * (FL_CIN * 2) + g * 16 : 0xFFFFFFF0u;
            vv_dma16(rs, vo, lds0 + it * 1024);
        }
    }
#pragma unroll
    for (int it = 0; it < 2; ++it) {
        const int idx = tid + 256 * it, row = idx >> 3, slot = idx & 7;
        const f32x4 w0 = *reinterpret_cast<const f32x4 *>(w + row * FL_CIN + slot * 8);
        const f32x4 w1 = *reinterpret_cast<const f32x4 *>(w + row * FL_CIN + slot * 8 + 4);
        bf16x8 o;
#pragma unroll
        for (int e = 0; e < 4; ++e) { o[e] = static_cast<__bf16>(w0[e]); o[4 + e] = static_cast<__bf16>(w1[e]); }
        *reinterpret_cast<bf16x8 *>(Ws + vv_swz_off(row, slot)) = o;
    }
    vv_wait_vm<0>();
    __syncthreads();

    // MFMA: wave -> tap half nt = wv & 1, row tiles mt = (wv >> 1) + 2 j
    const int fr = lane & 31, fh = lane >> 5;
    const int nt = wv & 1, mt0 = wv >> 1;
    uint4 fb[4];
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) fb[ks] = *reinterpret_cast<const uint4 *>(Ws + vv_swz_off(nt * 32 + fr, ks * 2 + fh));
    f32x16 acc[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
#pragma unroll
        for (int q = 0; q < 16; ++q) acc[j][q] = 0.f;
        const int mt = mt0 + 2 * j;
        if (mt < 7) {
#pragma unroll
            for (int ks = 0; ks < 4; ++ks) {
                const uint4 fa = *reinterpret_cast<const uint4 *>(As + vv_swz_off(mt * 32 + fr, ks * 2 + fh));
                acc[j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(*reinterpret_cast<const bf16x8 *>(&fa),
                                                                 *reinterpret_cast<const bf16x8 *>(&fb[ks]), acc[j], 0, 0, 0);
            }
        }
    }

    // wave -> output parity (pd, ph); lane -> cell; both pw parities per lane.  Tap half h holds td = 2h, 2h+1, i.e. the
    // terms with ad = h of every output: two passes of {waves of that half publish P, everyone gathers its 4 terms}.
    const int pd = g.pd, ph = g.ph, mw = g.mw, mh = g.mh, md = g.md;
    float acc0 = 0.f, acc1 = 0.f;
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        __syncthreads();   // operands (h = 0) / previous half (h = 1) no longer read by anyone
        if (nt == h) {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int mt = mt0 + 2 * j;
                if (mt < 7) {
#pragma unroll
                    for (int q = 0; q < 16; ++q) {
                        const int row = mt * 32 + (q & 3) + 8 * (q >> 2) + 4 * fh;
                        if (row < 216) P[row * FM_PPITCH + fr] = acc[j][q];
                    }
                }
            }
        }
        __syncthreads();
        const int ad = h, td = 1 - pd + 2 * ad - 2 * h;          // tap row inside this half (0 or 1)
#pragma unroll
        for (int ah = 0; ah < 2; ++ah) {
            const int zd = md + pd - ad + 1, zh = mh + ph - ah + 1;
            const int th = 1 - ph + 2 * ah;
            const float *r = P + ((zd * 6 + zh) * 6 + mw) * FM_PPITCH + (td * 4 + th) * 4;
            acc0 += r[FM_PPITCH + 1] + r[3];                    // pw = 0: i = mw (tw 1), mw-1 (tw 3)
            acc1 += r[2 * FM_PPITCH + 0] + r[FM_PPITCH + 2];    // pw = 1: i = mw+1 (tw 0), mw (tw 2)
        }
    }
    const size_t o = g.out(b, li);
    float bce = 0.f, tp = 0.f, fp = 0.f, fn = 0.f;
    const float2 p = fl_pair_stats<FL_PRECISE>(acc0, acc1, *reinterpret_cast<const float2 *>(target + o), gamma, epsilon, 1.0f - epsilon, bce, tp, fp, fn);
    if (probs) *reinterpret_cast<float2 *>(probs + o) = p;
    if (logits) *reinterpret_cast<float2 *>(logits + o) = make_float2(acc0, acc1);
    FL_BLOCK_STATS(bce, tp, fp, fn, tid, wv, red, partials, (size_t)b * nblk + blk);
}

// ---------------------------------------------------------------------------------------------------------------
// final_bce, sweep form (bf16): the box kernel above stages a 6^3 halo for 4^3 cells, so it loads, multiplies and
// publishes every input voxel 3.4 times.  Here one workgroup owns an 8 x 8 tile of cells in (h, w) and sweeps the whole
// depth: per plane d it stages the 10 x 10 halo rows ONCE (LDS-DMA, double buffered), forms P_d = X_d W^T on MFMA, keeps
// the td in {2,3} half of P_d for the next step and combines the td in {0,1} half with the kept half of P_{d-1}:
//   od = 2d - 1 + s  <-  P_d[td = s] + P_{d-1}[td = 2 + s]            (s = 0, 1; 2 x 2 terms in h, w each)
// so a step finishes two output planes of 16 x 16 voxels (256 threads x one pw pair).  Amplification 1.56 (h, w halo
// only), P is published once per cell, and the four BCE / TP / FP / FN sums stay in registers for the whole sweep.
// The voxel math uses the hardware exp / log / rcp (relative error ~1e-7, far below the bf16 operand rounding) and
// thresholds on the logit (sigmoid(l) >= 0.5 <=> l >= 0, function.py:110).
// P rows are dense (32 taps = 8 quads of 16 B); quad q of the row of halo cell (zh, zw) sits at slot q ^ (zw & 7): the gather reads
// whole quads with ds_read_b128 and this slot key makes every one of its lane groups conflict-free (exhaustive search over
// a*zh + b*zw keys and pitches 32 / 36 / 40: profiles/microbench/d5_swz.py; the dword gathers of rounds 1-2 at pitch 36 were 4-way).
constexpr int SW_PP = 32, SW_PSZ = FL_ROWS * SW_PP;   // P row pitch / buffer floats
// LDS: 2 plane slots + 1 KiB sink + PL + PH = 53,248 B (+ 64 B of static sums): THREE workgroups per CU (rounds 1-2: 73.6 KB, two).
// The 4th MFMA row tile reads 24 rows past a plane slot (into the next slot / the sink and the head of PL): whatever it finds only
// reaches accumulator rows >= 104, which are never published.
constexpr int SW_LDS = FL_NX * FL_XB + 1024 + 2 * SW_PSZ * 4;

__global__ __launch_bounds__(256, FL_DEPTH == 1 ? 3 : 2) void final_bce_sweep_kernel(const __bf16 *__restrict__ x, const float *__restrict__ w,
                                                                 const float *__restrict__ target, float *__restrict__ probs,
                                                                 float *__restrict__ logits, float *__restrict__ partials,
                                                                 int din_log2, unsigned x_bytes, float gamma, float epsilon) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    char *Xs = smem;                                             // ring of FL_NX planes x [104 rows][128 B], slot-swizzled; 1 KiB sink
    float *PL = reinterpret_cast<float *>(smem + FL_NX * FL_XB + 1024);   // P_d[td 0,1]  [100][32]
    float *PH = PL + SW_PSZ;                                     // P_d[td 2,3]  [100][32]: read in step d for the outputs of step d+1
    __shared__ float red[4][4];
    const int li = din_log2, n = 1 << li, nt8 = n >> 3, ntile = nt8 * nt8;
    const int wi = fl_work_item();
    const int tile = wi % ntile, b = wi / ntile;
    const int h0 = (tile / nt8) * 8, w0 = (tile % nt8) * 8;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int fr = lane & 31, fh = lane >> 5;

    const u32x4 rs = vv_make_rsrc(x, x_bytes);
    const unsigned ldsx = (unsigned)(unsigned long long)(lptr_t)Xs;
    // plane d -> ring slot d % 3: 13 pieces of 8 rows; every wave issues 4 (the 3 surplus ones go to the sink so that the
    // vector-memory counter advances uniformly); rows >= 100, voxels outside the grid and planes outside [0, n) arrive
    // as zeros (the virtual plane d = n closes the sweep).  The 4th MFMA row tile reads rows 96..127, i.e. 24 rows past
    // the slot: whatever it finds there only reaches accumulator rows >= 104, which are never published.
    // The lane part of a piece's source offset (sample, halo row, swizzled slot; out-of-range if the row is outside the grid
    // or past the 100 halo rows) is prepared once; the plane rides in soffset.
    unsigned sv[4], sdst[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int piece = wv * 4 + i, row = piece * 8 + (lane >> 3);
        const int zh = row / 10, zw = row - zh * 10;
        const int ih = h0 - 1 + zh, iw = w0 - 1 + zw;
        const bool ok = row < FL_ROWS && (unsigned)ih < (unsigned)n && (unsigned)iw < (unsigned)n;
        const int g = (lane & 7) ^ ((row >> 1) & 7);
        sv[i] = ok ? (unsigned)(((((b << li) << li) + ih) << li) + iw) * (FL_CIN * 2) + g * 16 : 0xFFFFFFF0u;
        sdst[i] = piece < 13 ? (unsigned)(piece * 1024) : (unsigned)(FL_NX * FL_XB);     // surplus pieces: the sink (ring-slot independent)
    }
    auto stage = [&](int d, int sp) {              // sp = d % FL_NX, passed so that the unrolled steps see a constant
        // a plane outside [0, n): every lane out of range by its OFFSET.  (A descriptor of zero records is not a substitute: the
        // zero-fill of the virtual plane d = n then went missing now and then and od = 2n - 1 read the stale slot -- found by the
        // B = 256 cross-check against the box form, profiles/microbench/chk_e1_d5.py.)
        const bool din = (unsigned)d < (unsigned)n;
        const unsigned soff = (unsigned)__builtin_amdgcn_readfirstlane(din ? (d << (2 * li)) * (FL_CIN * 2) : 0);
        const unsigned slot = ldsx + sp * FL_XB;
#pragma unroll
        for (int i = 0; i < 4; ++i) vv_dma16(rs, din ? sv[i] : 0xFFFFFFF0u, soff, wv * 4 + i < 13 ? slot + sdst[i] : ldsx + sdst[i]);
    };
    stage(0, 0);

    // weights of this wave's tap half as B fragments (lane: tap nt*32 + fr, k = ks*16 + 8 fh + j), straight from the
    // Keras array [64 taps][64 ci]
    const int nt = wv & 1, mt0 = wv >> 1;
    uint4 fb[4];
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) {
        const float *wr = w + (nt * 32 + fr) * FL_CIN + ks * 16 + 8 * fh;
        const f32x4 w0v = *reinterpret_cast<const f32x4 *>(wr), w1v = *reinterpret_cast<const f32x4 *>(wr + 4);
        bf16x8 o;
#pragma unroll
        for (int e = 0; e < 4; ++e) { o[e] = static_cast<__bf16>(w0v[e]); o[4 + e] = static_cast<__bf16>(w1v[e]); }
        fb[ks] = *reinterpret_cast<const uint4 *>(&o);
    }

    const FlRole r = fl_role(tid);
    const int mw = r.mw, sl = r.sl, mh = r.mh, ph = r.ph;
    const int lo = li + 1, n2 = 2 * n;
    const int oh = r.oh(h0), ow = r.ow(w0);
    const float hi = 1.0f - epsilon;
    float bce = 0.f, tp = 0.f, fp = 0.f, fn = 0.f;
    float lo0 = 0.f, lo1 = 0.f;                                  // td in {2,3} contributions of P_{d-1} to this step's outputs (P_{-1} = 0)

    // P_d = X_d W^T for this wave's two row tiles and its tap half: D[tap][cell], weights-first
    auto mfma_plane = [&](int sp, f32x16 (&acc)[2]) {             // sp = ring slot of the plane
        const char *Xd = Xs + sp * FL_XB;
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int q = 0; q < 16; ++q) acc[j][q] = 0.f;
        // k-step outer, row tile inner: consecutive MFMAs go to different accumulators (the other order is two chains of four
        // dependent MFMAs)
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) {
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                const int mt = mt0 + 2 * j;
                const uint4 fa = *reinterpret_cast<const uint4 *>(Xd + vv_swz_off(mt * 32 + fr, ks * 2 + fh));
                acc[j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(*reinterpret_cast<const bf16x8 *>(&fb[ks]),
                                                                 *reinterpret_cast<const bf16x8 *>(&fa), acc[j], 0, 0, 0);
            }
        }
    };

    // Software pipeline: step d publishes P_d (computed during step d-1) and then runs the MFMAs of plane d+1 in the same
    // instruction stream as the gather / loss math of plane d (matrix pipe under the VALU and LDS work).
    vv_wait_vm<0>();                                             // plane 0
    __syncthreads();                                             // ... for every wave
    f32x16 acc[2];
    mfma_plane(0, acc);
#pragma unroll
    for (int k = 1; k <= FL_DEPTH; ++k) stage(k, k);
    __syncthreads();                                             // slot 0 may be refilled from the first step on

    // (Unrolling this loop by two with the step parity as a compile-time constant -- ring slot and P buffer addresses folded
    // into the instructions -- is worth 2 % (53.5 vs 54.7 us) in the clean kernel; with the ablation switches still compiled in
    // it returned a low loss sum at B = 256 with exact logits and counts, which is not understood: not used.)
    int oldh = 0;                                                // ring slot of plane d
#pragma unroll 1
    for (int d = 0; d <= n; ++d) {
        // weights-first: lane = cell row, registers walk the taps of the half; quad g = taps 8g + 4fh .. +3 = the four tw
        // of one (td, th): one 16-byte store per quad
        float *Pw = nt == 0 ? PL : PH;
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int row = (mt0 + 2 * j) * 32 + fr;
            if (row < FL_ROWS) {
                const int zwk = (row - (row / 10) * 10) & 7;              // slot key of this halo cell
#pragma unroll
                for (int g = 0; g < 4; ++g)
                    *reinterpret_cast<f32x4 *>(Pw + row * SW_PP + (((2 * g + fh) ^ zwk) << 2)) =
                        f32x4{acc[j][4 * g], acc[j][4 * g + 1], acc[j][4 * g + 2], acc[j][4 * g + 3]};
            }
        }
        const int od = 2 * d - 1 + sl;
        const bool ovalid = (unsigned)od < (unsigned)n2;
        const size_t o = fl_out_index(b, ovalid ? od : 0, oh, ow, lo);
        // The target pair is loaded by inline asm so that its wait can be counted: the vector-memory counter retires in
        // order, and a compiler-placed wait for this load would be vmcnt(0), i.e. it would also wait for the 4 pieces of
        // plane d+2 issued right after it -- the look-ahead.  In flight, oldest first:
        //   [plane d+1 x4][stores d-1] [y d][plane d+2 x4]
        // so "all but the newest 5" covers plane d+1 whatever the number of stores (more stores only wait for more).
        // An asm output is a READY value to the compiler: nothing in the language stops it from copying y or re-using its
        // registers while the load is in flight.  tests/test_isa_lint.py checks on the generated code that no instruction
        // names the pair between this load and the counted wait below that lands it ("+v"(y)); round 2's dead ends came from
        // exactly that (a look-ahead load whose last instance was DEAD: its registers went to the logit accumulators of the
        // last plane while it was in flight -- DESIGN.md section 4d).  The two compiler-managed alternatives were built in round 3
        // and are worse: a plain load of the noalias argument is moved by the compiler across the asm statements into the
        // `ovalid` branch (behind the counted wait, whose count then no longer holds: wrong logits), a volatile load becomes a
        // system-scope flat load with an immediate vmcnt(0).
        float2 y;
        asm volatile("global_load_dwordx2 %0, %1, off" : "=v"(y) : "v"(target + o) : "memory");
        stage(d + 1 + FL_DEPTH, oldh);
        // depth 1: [plane d+1 x4][stores d-1][y d][plane d+2 x4] -> all but the newest 5.  depth 2: plane d+1 is followed by
        // stores d-2 (0..2), y d-1, plane d+2 x4, stores d-1 (0..2), y d, plane d+3 x4 = 10..14 operations -> all but the newest 10
        vv_wait_vm<FL_DEPTH == 1 ? 5 : 10>();                                                 // plane d+1 has landed
        __syncthreads();                                         // ... for every wave; P_d is published

        f32x16 acc_next[2];
        const int nexth = oldh + 1 == FL_NX ? 0 : oldh + 1;      // ring slot of plane d+1
        mfma_plane(nexth, acc_next);

        // gather: per ah the tap quads (tw 0..3) of the three cells mw, mw+1, mw+2 -- ds_read_b128, conflict-free.  The td in {0,1}
        // half of P_d (PL) completes the output planes od = 2d - 1 + sl together with the td in {2,3} half of P_{d-1}, which was
        // gathered a step ago into (lo0, lo1): PH is read in the step that publishes it, so ONE buffer holds it.
        float l0 = lo0, l1 = lo1;
        lo0 = 0.f; lo1 = 0.f;
#pragma unroll
        for (int ah = 0; ah < 2; ++ah) {
            const int zh = mh + ph - ah + 1, th = 1 - ph + 2 * ah;
            const int q = sl * 4 + th, rowb = (zh * 10 + mw) * SW_PP;
            const int o0 = rowb + ((q ^ (mw & 7)) << 2), o1 = rowb + SW_PP + ((q ^ ((mw + 1) & 7)) << 2),
                      o2 = rowb + 2 * SW_PP + ((q ^ ((mw + 2) & 7)) << 2);
            const f32x4 a0 = *reinterpret_cast<const f32x4 *>(PL + o0), a1 = *reinterpret_cast<const f32x4 *>(PL + o1),
                        a2 = *reinterpret_cast<const f32x4 *>(PL + o2);
            const f32x4 b0 = *reinterpret_cast<const f32x4 *>(PH + o0), b1 = *reinterpret_cast<const f32x4 *>(PH + o1),
                        b2 = *reinterpret_cast<const f32x4 *>(PH + o2);
            l0 += a1[1] + a0[3];                                         // pw = 0: cell mw+1 (tw 1), cell mw (tw 3)
            l1 += a2[0] + a1[2];                                         // pw = 1: cell mw+2 (tw 0), cell mw+1 (tw 2)
            lo0 += b1[1] + b0[3];
            lo1 += b2[0] + b1[2];
        }
        asm volatile("s_waitcnt vmcnt(4)" : "+v"(y) : : "memory");   // y has landed; plane d+2 may still be in flight
        if (ovalid) {
            const float2 p = fl_pair_stats<FL_HW>(l0, l1, y, gamma, epsilon, hi, bce, tp, fp, fn);
            if (probs) *reinterpret_cast<float2 *>(probs + o) = p;
            if (logits) *reinterpret_cast<float2 *>(logits + o) = make_float2(l0, l1);
        }
        acc[0] = acc_next[0];
        acc[1] = acc_next[1];
        oldh = nexth;
        __syncthreads();      // every gather of P_d / P_{d-1} and every read of plane d+1 is done: publish d+1, refill its slot
    }
    vv_wait_vm<0>();                                             // the last (all-zero) look-ahead planes
    FL_BLOCK_STATS(bce, tp, fp, fn, tid, wv, red, partials, (size_t)b * ntile + tile);
}

// ---------------------------------------------------------------------------------------------------------------
// final_bce, sweep form with the w direction summed INSIDE the MFMA (bf16, round 3; the Q form of final_common.h).  The sweep kernel above
// publishes P[halo cell][64 taps] (25.6 KB of float32 per plane) and every output gathers 8 terms from it; its ablations
// put the memory side of the layer at 31 us and the float32 round trip of P through LDS (written at the LDS write rate, gathered as whole tap
// quads) at most of the other 20.  Q[centre cell][td][th][pw] is the same FLOPs and the same float32 sums, but 80 cells x 32 values = 10 KB per
// plane instead of 100 x 64, and an output pair reads ONE 8-byte granule per (ah, td) instead of three 16-byte quads: LDS written / 2.5,
// gathered / 6, 38 KB of LDS and <= 128 VGPRs = four workgroups per CU.  The counted waits are the sweep kernel's, unchanged.
// final_mean.hip's final_mean_sweep_kernel runs the same Q pieces over the samples of an object (its loop differs: samples chained, no target
// load, sums in LDS); tests/test_gpu_sampled.py compares the two kernels' outputs bit for bit at K = 1.
constexpr int SWW_LDS = FL_NX * FL_XB + 1024 + FL_QB;
__global__ __launch_bounds__(256, 4) void final_bce_sweepw_kernel(const __bf16 *__restrict__ x, const float *__restrict__ w,
                                                                 const float *__restrict__ target, float *__restrict__ probs,
                                                                 float *__restrict__ logits, float *__restrict__ partials,
                                                                 int din_log2, unsigned x_bytes, float gamma, float epsilon) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    char *Xs = smem;                                             // ring of FL_NX planes x [104 rows][128 B], slot-swizzled; 1 KiB sink
    char *Pq = smem + FL_NX * FL_XB + 1024;                      // Q_d [80 centre cells][td 4][th 4][pw 2] float32, 8-byte granule g at g ^ key(cell)
    __shared__ float red[4][4];
    const int li = din_log2, n = 1 << li, nt8 = n >> 3, ntile = nt8 * nt8;
    const int wi = fl_work_item();
    const int tile = wi % ntile, b = wi / ntile;
    const int h0 = (tile / nt8) * 8, w0 = (tile % nt8) * 8;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);

    const u32x4 rs = vv_make_rsrc(x, x_bytes);
    const unsigned ldsx = (unsigned)(unsigned long long)(lptr_t)Xs;
    // plane d -> ring slot d % 2; rows >= 100, voxels outside the grid and planes outside [0, n) arrive as zeros (the virtual plane
    // d = n closes the sweep).  The operand reads stay inside rows 0 .. 99 (centre cells zw = 1 .. 8 and their left / right neighbours).
    // The sample is part of the lane offset; the plane rides in soffset.
    FL_Q_STAGE_LANES(b)
    auto stage = [&](int d, int sp) {              // sp = d % FL_NX, passed so that the unrolled steps see a constant
        // a plane outside [0, n): every lane out of range by its OFFSET.  (A descriptor of zero records is not a substitute: the
        // zero-fill of the virtual plane d = n then went missing now and then and od = 2n - 1 read the stale slot -- found by the
        // B = 256 cross-check against the box form, profiles/microbench/chk_e1_d5.py.)
        const bool din = (unsigned)d < (unsigned)n;
        const unsigned soff = (unsigned)__builtin_amdgcn_readfirstlane(din ? (d << (2 * li)) * (FL_CIN * 2) : 0);
        const unsigned slot = ldsx + sp * FL_XB;
#pragma unroll
        for (int i = 0; i < 4; ++i) vv_dma16(rs, din ? sv[i] : 0xFFFFFFF0u, soff, wv * 4 + i < 13 ? slot + sdst[i] : ldsx + sdst[i]);
    };
    stage(0, 0);

    FL_Q_OPERANDS(w)
    const FlRole r = fl_role(tid);
    const int lo = li + 1, n2 = 2 * n;
    const int oh = r.oh(h0), ow = r.ow(w0);
    const float hi = 1.0f - epsilon;
    float bce = 0.f, tp = 0.f, fp = 0.f, fn = 0.f;
    float lo0 = 0.f, lo1 = 0.f;                                  // td in {2,3} contributions of Q_{d-1} to this step's outputs (Q_{-1} = 0)
    auto mfma_plane = [&](int sp, f32x4 (&acc)[2][2]) { fl_q_mfma_plane(Xs + sp * FL_XB, ntl, xo, wf, acc); };   // sp = ring slot of the plane

    // Software pipeline: step d publishes Q_d (computed during step d-1) and then runs the MFMAs of plane d+1 in the same
    // instruction stream as the gather / loss math of plane d (matrix pipe under the VALU and LDS work).
    vv_wait_vm<0>();                                             // plane 0
    __syncthreads();                                             // ... for every wave
    f32x4 acc[2][2];
    mfma_plane(0, acc);
#pragma unroll
    for (int k = 1; k <= FL_DEPTH; ++k) stage(k, k);
    __syncthreads();                                             // slot 0 may be refilled from the first step on

    int oldh = 0;                                                // ring slot of plane d
#pragma unroll 1
    for (int d = 0; d <= n; ++d) {
        FL_Q_PUBLISH(Pq, acc)
        const int od = 2 * d - 1 + r.sl;
        const bool ovalid = (unsigned)od < (unsigned)n2;
        const size_t o = fl_out_index(b, ovalid ? od : 0, oh, ow, lo);
        // The target pair is loaded by inline asm so that its wait can be counted (see final_bce_sweep_kernel for the history and the
        // compiler-managed forms that fail).  In flight, oldest first: [plane d+1 x4][stores d-1] [y d][plane d+2 x4]: "all but the newest
        // 5" covers plane d+1 whatever the number of stores.  tests/test_isa_lint.py checks on the generated code that no instruction
        // names the pair between this load and the counted wait below that lands it ("+v"(y)).
        float2 y;
        asm volatile("global_load_dwordx2 %0, %1, off" : "=v"(y) : "v"(target + o) : "memory");
        stage(d + 1 + FL_DEPTH, oldh);
        // depth 1: [plane d+1 x4][stores d-1][y d][plane d+2 x4] -> all but the newest 5.  depth 2: plane d+1 is followed by
        // stores d-2 (0..2), y d-1, plane d+2 x4, stores d-1 (0..2), y d, plane d+3 x4 = 10..14 operations -> all but the newest 10
        vv_wait_vm<FL_DEPTH == 1 ? 5 : 10>();                                                 // plane d+1 has landed
        __syncthreads();                                         // ... for every wave; Q_d is published

        f32x4 acc_next[2][2];
        const int nexth = oldh + 1 == FL_NX ? 0 : oldh + 1;      // ring slot of plane d+1
        mfma_plane(nexth, acc_next);

        float l0 = lo0, l1 = lo1;
        lo0 = 0.f; lo1 = 0.f;
        FL_Q_GATHER(Pq, r, l0, l1, lo0, lo1)
        asm volatile("s_waitcnt vmcnt(4)" : "+v"(y) : : "memory");   // y has landed; plane d+2 may still be in flight
        if (ovalid) {
            const float2 p = fl_pair_stats<FL_HW01>(l0, l1, y, gamma, epsilon, hi, bce, tp, fp, fn);
            if (probs) *reinterpret_cast<float2 *>(probs + o) = p;
            if (logits) *reinterpret_cast<float2 *>(logits + o) = make_float2(l0, l1);
        }
#pragma unroll
        for (int t = 0; t < 2; ++t) { acc[t][0] = acc_next[t][0]; acc[t][1] = acc_next[t][1]; }
        oldh = nexth;
        __syncthreads();      // every gather of Q_d and every read of plane d+1 is done: publish d+1, refill its slot
    }
    vv_wait_vm<0>();                                             // the last (all-zero) look-ahead planes
    FL_BLOCK_STATS(bce, tp, fp, fn, tid, wv, red, partials, (size_t)b * ntile + tile);
}

// stats[b] = sum of sample b's partials: lanes take blocks b, b + 64, ..., then the wave sum
__global__ __launch_bounds__(64) void final_reduce_kernel(const float *__restrict__ partials, float *__restrict__ stats, int nblk) {
    const int b = blockIdx.x, lane = threadIdx.x;
    float s[4] = {0.f, 0.f, 0.f, 0.f};
    for (int i = lane; i < nblk; i += 64) {
        const f32x4 v = *reinterpret_cast<const f32x4 *>(partials + ((size_t)b * nblk + i) * 4);
        s[0] += v[0]; s[1] += v[1]; s[2] += v[2]; s[3] += v[3];
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) s[k] = vv_wave_sum(s[k]);
    if (lane == 0) *reinterpret_cast<f32x4 *>(stats + (size_t)b * 4) = f32x4{s[0], s[1], s[2], s[3]};
}

// final_reduce + shape_metrics (nolbo.py:1498-1501) in ONE launch for the usual case of a few partial blocks per sample: thread
// b sums its sample's partials in block order, keeps the sample's metrics terms (vv_add_shape_metrics), and the batch means are
// formed by a fixed tree (wave shuffles, then the waves in order): deterministic, independent of timing.
__global__ __launch_bounds__(256) void final_reduce_metrics_kernel(const float *__restrict__ partials, float *__restrict__ stats,
                                                                   float *__restrict__ out4, int nblk, int batch) {
    __shared__ float red[4][4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    float m[4] = {0.f, 0.f, 0.f, 0.f};
    for (int b = tid; b < batch; b += 256) {
        f32x4 s = {0.f, 0.f, 0.f, 0.f};
        for (int i = 0; i < nblk; ++i) s += *reinterpret_cast<const f32x4 *>(partials + ((size_t)b * nblk + i) * 4);
        *reinterpret_cast<f32x4 *>(stats + (size_t)b * 4) = s;
        vv_add_shape_metrics(s[0], s[1], s[2], s[3], m[0], m[1], m[2], m[3]);
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) m[k] = vv_wave_sum(m[k]);
    if (lane == 0) { red[wave][0] = m[0]; red[wave][1] = m[1]; red[wave][2] = m[2]; red[wave][3] = m[3]; }
    __syncthreads();
    if (tid < 4) out4[tid] = (red[0][tid] + red[1][tid] + red[2][tid] + red[3][tid]) / (float)batch;
}

// per-sample sums from the partial blocks, and the batch metrics when the caller wants them
void finish_stats(const float *partials, float *stats, float *metrics4, int nblk, int batch, hipStream_t st) {
    if (metrics4 && nblk <= 64) {
        VV_LAUNCH(final_reduce_metrics_kernel, dim3(1), dim3(256), 0, st, partials, stats, metrics4, nblk, batch);
        return;
    }
    vv_final_reduce_launch(partials, stats, nblk, batch, st);
    if (metrics4) vv_shape_metrics_launch(stats, metrics4, batch, st);
}

int final_bce_impl(const void *x, const float *w_keras, const float *target, float *probs, float *logits, float *stats, float *metrics4,
                   int batch, int side, int cin, float gamma, float epsilon, int dtype, void *workspace, size_t workspace_bytes, void *stream) {
    if (!x || !w_keras || !target || !stats) return VV_ERR_NULL;
    if (!vv_dtype_in<float, __bf16, vv_fp8>(dtype)) return VV_ERR_DTYPE;
    if (batch <= 0 || batch > 65535 || side < 4 || !vv_is_pow2(side) || cin != FL_CIN) return VV_ERR_SHAPE;
    if (dtype == VV_FP8 && side < 8) return VV_ERR_SHAPE;                  // the e4m3fn input exists in sweep form only
    if (!vv_aligned16(x) || !vv_aligned16(target) || (probs && !vv_aligned16(probs)) || (logits && !vv_aligned16(logits)))
        return VV_ERR_ALIGN;
    if (!workspace || workspace_bytes < vv_convT3d_final_bce_workspace_bytes(batch, side) || !vv_aligned16(workspace))
        return VV_ERR_WORKSPACE;
    const int nb = side / 4, nblk = nb * nb * nb;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    float *partials = reinterpret_cast<float *>(workspace);
    const int ntile = (side / 8) * (side / 8);
    if (dtype == VV_FP8) {
        const int nt8 = vv_final_bce_sweep_fp8_launch(x, w_keras, target, probs, logits, partials, batch, side, gamma, epsilon, st);
        finish_stats(partials, stats, metrics4, nt8, batch, st);
        return vv_launch_status();
    }
    const char *force = vv_hook("VV_FINAL_BCE");                  // "sweep" / "sweepp" / "box": override the batch heuristic (tests)
    const bool sweep = dtype == VV_BF16 && side >= 8 &&
                       (force ? force[0] == 's' : (long)batch * ntile >= 128);   // enough workgroups to fill the chip
    // "sweep" = the form with the w direction summed inside the MFMA (round 3); "sweepp" = the form that publishes P[halo cell][64 taps]
    const bool form_p = force && !strcmp(force, "sweepp");
    if (sweep) {
        vv_allow_lds<&final_bce_sweep_kernel>(SW_LDS);
        // 32-bit buffer offsets: <= 2 GiB of input per launch; every per-sample tensor moves on by the same sample range
        const size_t in_per = (size_t)side * side * side * FL_CIN * 2, vox = (size_t)8 * side * side * side;
        const int per = vv_chunk_samples(in_per, batch);
        if (per < 1) return VV_ERR_SHAPE;
        for (int b0 = 0; b0 < batch; b0 += per) {
            const int nbt = batch - b0 < per ? batch - b0 : per;
            const auto launch = [&](auto kernel, size_t lds) {    // both forms take the same arguments
                VV_LAUNCH(kernel, dim3(ntile * nbt), dim3(256), lds, st,
                          reinterpret_cast<const __bf16 *>(reinterpret_cast<const char *>(x) + (size_t)b0 * in_per), w_keras, target + (size_t)b0 * vox,
                          probs ? probs + (size_t)b0 * vox : nullptr, logits ? logits + (size_t)b0 * vox : nullptr, partials + (size_t)b0 * ntile * 4,
                          vv_log2(side), (unsigned)((size_t)nbt * in_per), gamma, epsilon);
            };
            if (form_p) launch(final_bce_sweep_kernel, SW_LDS);
            else launch(final_bce_sweepw_kernel, SWW_LDS);
        }
        finish_stats(partials, stats, metrics4, ntile, batch, st);
        return vv_launch_status();
    }
    if (dtype == VV_BF16)
        VV_LAUNCH(final_bce_mfma_kernel, dim3(nblk * batch), dim3(256), (size_t)FM_ROWS * 128 + 64 * 128, st,
                  reinterpret_cast<const __bf16 *>(x), w_keras, target, probs, logits, partials, vv_log2(side),
                  (unsigned)((size_t)batch * side * side * side * FL_CIN * 2), gamma, epsilon);
    else
        VV_LAUNCH((final_bce_kernel<float>), dim3(nblk, batch), dim3(256), 0, st, reinterpret_cast<const float *>(x),
                           w_keras, target, probs, logits, partials, vv_log2(side), gamma, epsilon);
    finish_stats(partials, stats, metrics4, nblk, batch, st);
    return vv_launch_status();
}

}  // namespace

void vv_final_reduce_launch(const float *partials, float *stats, int nblk, int batch, hipStream_t st) {
    VV_LAUNCH(final_reduce_kernel, dim3(batch), dim3(64), 0, st, partials, stats, nblk);
}

VV_EXPORT size_t vv_convT3d_final_bce_workspace_bytes(int batch, int side) {
    const size_t nb = side / 4;
    return (size_t)batch * nb * nb * nb * 4 * sizeof(float);
}

VV_EXPORT int vv_convT3d_final_bce_fwd(const void *x, const float *w_keras, const float *target, float *probs,
                                       float *logits, float *stats, int batch, int side, int cin, float gamma,
                                       float epsilon, int dtype, void *workspace, size_t workspace_bytes, void *stream) {
    return final_bce_impl(x, w_keras, target, probs, logits, stats, nullptr, batch, side, cin, gamma, epsilon, dtype, workspace,
                          workspace_bytes, stream);
}

VV_EXPORT int vv_convT3d_final_bce_metrics_fwd(const void *x, const float *w_keras, const float *target, float *probs,
                                               float *logits, float *stats, float *metrics4, int batch, int side, int cin, float gamma,
                                               float epsilon, int dtype, void *workspace, size_t workspace_bytes, void *stream) {
    if (!metrics4) return VV_ERR_NULL;
    return final_bce_impl(x, w_keras, target, probs, logits, stats, metrics4, batch, side, cin, gamma, epsilon, dtype, workspace,
                          workspace_bytes, stream);
}
