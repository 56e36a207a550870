// Sampled-mean reconstruction (gfx950): the last decoder layer over the K latent samples of one object, averaged in the kernel.
//   sample_latents : z[b*K + k] = mean[b] + sqrt(exp(logvar[b])) * eps[b][k]          (function.py:35-38; nolbo_test.py:169-173)
//   final_mean     : Conv3DTranspose k4 s2 SAME -> 1 channel, sigmoid, MEAN over the K samples of an object, and the weighted BCE /
//                    TP / FP / FN of that mean  (nolbo_test.py:174-177: tf.reduce_mean(decoder(latents), axis=0);
//                    autoencoder3D.py:129-136; function.py:73-82, 100-115)
// A workgroup owns a piece of ONE object's output grid and a slice of that object's samples and loops over them; the probabilities of a
// sample exist in registers only, their float32 sum in registers (box form) or LDS (sweep form).  The slice sums go to the workspace
// (<= 8 float32 grids per object) and final_mean_finish_kernel forms the mean and scores it.  Every sum runs in a fixed order that depends
// on (K, side) only -- k ascending inside a slice, slices ascending, 1,024-voxel stats blocks in order -- and not on the number of objects
// in the call: no float atomics, two runs are bit-identical, and an object's result does not depend on what it is batched with.
// The box geometry and staging, the Q-form sweep pieces, the voxel loss and the block reduction are the single-sample layer's
// (final_common.h): a sample's probability is the same expression here and there.
#include "final_common.h"

namespace {

// Where the sums go: the float32 probability sums of K slice s to part + s * slice_stride; the finish kernel adds the slices in order,
// stores the mean and (with a target) one stats partial per 1,024 voxels.
struct FmOut {
    const float *target;      // [B, vox] or NULL
    float *mean_probs;        // [B, vox]
    float *part;              // [nslices][B, vox] float32 sums
    float *partials;          // [B][nfin][4]
    size_t slice_stride;
    int nslices, samples;
    float gamma, epsilon, inv_k;
};

// ---------------------------------------------------------------------------------------------------------------
// Box form (float32 and bf16 activations, any side): the workgroup of final_bce.hip's final_bce_kernel -- a 4x4x4 block of input
// cells -> 8x8x8 outputs, wave = output parity (pd, ph), lane = cell with both pw -- looped over the samples [k0, k1) of its object
// with the two probability sums in registers.  The weights sit in LDS; with bf16 activations they are rounded to bf16 first, as the
// MFMA forms of the single-sample layer do, so that a sample's logit is the same product sum here and there.
constexpr int FMB_LDS = (216 * FL_BOX_ROW + 64 * FL_CIN) * 4;

template <typename T>
__global__ __launch_bounds__(256) void final_mean_box_kernel(const T *__restrict__ x, const float *__restrict__ w, FmOut a, int din_log2) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    float *tile = reinterpret_cast<float *>(smem);                // [216][FL_BOX_ROW]
    float *wl = tile + 216 * FL_BOX_ROW;                              // [64 taps][64 ci]
    const int li = din_log2, nb = (1 << li) >> 2;
    const int blk = blockIdx.x, b = blockIdx.y / a.nslices, s = blockIdx.y % a.nslices;
    const int k0 = (s * a.samples) / a.nslices, k1 = ((s + 1) * a.samples) / a.nslices;

    for (int i = threadIdx.x; i < 64 * FL_CIN; i += 256) {
        const float v = w[i];
        wl[i] = sizeof(T) == 2 ? static_cast<float>(static_cast<__bf16>(v)) : v;
    }

    const int lane = threadIdx.x & 63;
    const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const FlBox g = fl_box(blk, nb, wv, lane);
    const int pd = g.pd, ph = g.ph, mw = g.mw, mh = g.mh, md = g.md;
    float sum0 = 0.f, sum1 = 0.f;
    for (int k = k0; k < k1; ++k) {
        __syncthreads();                          // the previous sample's tile is no longer read
        fl_box_stage(x + (((size_t)b * a.samples + k) << (3 * li)) * FL_CIN, tile, g, li);
        __syncthreads();
        float acc0 = 0.f, acc1 = 0.f;
#pragma unroll
        for (int ad = 0; ad < 2; ++ad) {
#pragma unroll
            for (int ah = 0; ah < 2; ++ah) {
                const int zd = md + pd - ad + 1, zh = mh + ph - ah + 1;
                const int td = 1 - pd + 2 * ad, th = 1 - ph + 2 * ah;
                const float *r0 = tile + ((zd * 6 + zh) * 6 + mw) * FL_BOX_ROW;   // zw = mw, mw+1, mw+2
                const float *wt = wl + ((td * 4 + th) * 4) * FL_CIN;          // [tw][ci], wave-uniform: LDS broadcast reads
#pragma unroll 4
                for (int c = 0; c < FL_CIN; c += 4) {
                    const f32x4 x0 = *reinterpret_cast<const f32x4 *>(r0 + c);
                    const f32x4 x1 = *reinterpret_cast<const f32x4 *>(r0 + FL_BOX_ROW + c);
                    const f32x4 x2 = *reinterpret_cast<const f32x4 *>(r0 + 2 * FL_BOX_ROW + c);
                    const f32x4 w0 = *reinterpret_cast<const f32x4 *>(wt + 0 * FL_CIN + c), w1 = *reinterpret_cast<const f32x4 *>(wt + 1 * FL_CIN + c);
                    const f32x4 w2 = *reinterpret_cast<const f32x4 *>(wt + 2 * FL_CIN + c), w3 = *reinterpret_cast<const f32x4 *>(wt + 3 * FL_CIN + c);
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        // pw = 0: i = mw (tw 1), mw-1 (tw 3);  pw = 1: i = mw+1 (tw 0), mw (tw 2)
                        acc0 = fmaf(x1[e], w1[e], acc0);
                        acc0 = fmaf(x0[e], w3[e], acc0);
                        acc1 = fmaf(x2[e], w0[e], acc1);
                        acc1 = fmaf(x1[e], w2[e], acc1);
                    }
                }
            }
        }
        sum0 += fl_sigmoid<FL_PRECISE>(acc0);                     // the mean is over probabilities
        sum1 += fl_sigmoid<FL_PRECISE>(acc1);
    }
    *reinterpret_cast<float2 *>(a.part + (size_t)s * a.slice_stride + g.out(b, li)) = make_float2(sum0, sum1);
}

// ---------------------------------------------------------------------------------------------------------------
// Sweep form (bf16 activations, side >= 8): final_bce.hip's final_bce_sweepw_kernel (the Q form of final_common.h) -- an 8 x 8 tile of cells in (h, w) swept through
// the depth, the 10 x 10 halo rows of a plane staged once by LDS-DMA into a two-slot ring, Q_d[centre cell][td][th][pw] formed on
// v_mfma_f32_16x16x32_bf16 with the w direction summed inside the MFMA, od = 2d - 1 + s <- Q_d[td = s] + Q_{d-1}[td = 2 + s] -- run
// over the (sample, plane) sequence of one object as ONE software pipeline: the plane after a sample's last one is the next sample's
// first, so the look-ahead never drains between samples.  A workgroup owns the depth range [r * rng, (r + 1) * rng) of its tile, i.e.
// the output planes [2 r rng, 2 (r + 1) rng), and walks the input planes d_first = max(r * rng - 1, 0) .. d_last = (r + 1) * rng of
// every sample (one halo plane in front: its Q only feeds the carry; plane n is the all-zero plane that closes a sweep).  Each thread
// keeps the float32 probability sums of ITS output pairs in LDS (rng * 2 KB, thread-private slots: no barrier protects them, none is
// needed).  Nothing but the LDS-DMA touches the vector-memory counter inside the loop, so "all but the newest 4" is plane t + 1.
static_assert(FL_NX == 2, "final_mean_sweep_kernel counts its waits and flips its ring for two plane slots");
constexpr int MS_BASE = FL_NX * FL_XB + 1024 + FL_QB;          // plane ring + sink + Q
static inline size_t ms_lds(int rng) { return (size_t)MS_BASE + (size_t)rng * 2048; }

__global__ __launch_bounds__(256, 2) void final_mean_sweep_kernel(const __bf16 *__restrict__ x, const float *__restrict__ w, FmOut a, int din_log2,
                                                                  int rng_log2, unsigned x_bytes) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    char *Xs = smem;                                             // ring of FL_NX planes x [104 rows][128 B], slot-swizzled; 1 KiB sink
    char *Pq = smem + FL_NX * FL_XB + 1024;                      // Q_d [80 centre cells][td 4][th 4][pw 2] float32, 8-byte granule g at g ^ key(cell)
    char *Acc = smem + MS_BASE;                                  // [2 rng output planes][16 oh][8 cells] float2 sums
    const int li = din_log2, n = 1 << li, nt8 = n >> 3, ntile = nt8 * nt8;
    const int rng = 1 << rng_log2, nranges = n >> rng_log2;
    const int wi = fl_work_item();
    const int tile = wi % ntile, r = (wi / ntile) % nranges, s = (wi / (ntile * nranges)) % a.nslices, b = wi / (ntile * nranges * a.nslices);
    const int k0 = (s * a.samples) / a.nslices, k1 = ((s + 1) * a.samples) / a.nslices;
    const int d_first = r == 0 ? 0 : r * rng - 1, d_last = (r + 1) * rng;
    const int od_lo = 2 * r * rng, od_hi = od_lo + 2 * rng;
    const int h0 = (tile / nt8) * 8, w0 = (tile % nt8) * 8;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);

    const u32x4 rs = vv_make_rsrc(x, x_bytes);
    const unsigned ldsx = (unsigned)(unsigned long long)(lptr_t)Xs;
    // rows >= 100, voxels outside the grid, planes outside [0, n) and everything past the last sample arrive as zeros (every lane out
    // of range by its OFFSET, as in final_bce_sweepw_kernel).  The lane offsets are those of sample 0: sample and plane ride in soffset.
    FL_Q_STAGE_LANES(0)
    int ks = k0, ds = d_first;                                   // the (sample, plane) the next stage() fetches; FM_NEXT_PLANE moves it on
#define FM_NEXT_PLANE() do { const bool wrap_ = ds == d_last; ks += wrap_ ? 1 : 0; ds = wrap_ ? d_first : ds + 1; } while (0)
    auto stage = [&](int sp, int ks, int ds) {
        const bool din = ks < k1 && (unsigned)ds < (unsigned)n;
        const unsigned soff = (unsigned)__builtin_amdgcn_readfirstlane(din ? ((((b * a.samples + ks) << li) + ds) << (2 * li)) * (FL_CIN * 2) : 0);
        const unsigned slot = ldsx + sp * FL_XB;
#pragma unroll
        for (int i = 0; i < 4; ++i) vv_dma16(rs, din ? sv[i] : 0xFFFFFFF0u, soff, wv * 4 + i < 13 ? slot + sdst[i] : ldsx + sdst[i]);
    };
    stage(0, ks, ds);
    FM_NEXT_PLANE();

    FL_Q_OPERANDS(w)
    const FlRole gr = fl_role(tid);
    const int sl = gr.sl, lo = li + 1;
    const int oh = gr.oh(h0), ow = gr.ow(w0);
    float2 *mine = reinterpret_cast<float2 *>(Acc) + (tid & 127);   // slot of local output plane q: mine[q * 128]; this thread owns q = 2j + 1 - sl
    for (int j = 0; j < rng; ++j) mine[(2 * j + 1 - sl) * 128] = make_float2(0.f, 0.f);
    float lo0 = 0.f, lo1 = 0.f;

    auto mfma_plane = [&](int sp, f32x4 (&acc)[2][2]) { fl_q_mfma_plane(Xs + sp * FL_XB, ntl, xo, wf, acc); };   // sp = ring slot of the plane

    vv_wait_vm<0>();                                             // step 0's plane
    __syncthreads();
    f32x4 acc[2][2];
    mfma_plane(0, acc);
    stage(1, ks, ds);
    FM_NEXT_PLANE();
    __syncthreads();                                             // slot 0 may be refilled from the first step on

    const int nsteps = (k1 - k0) * (d_last - d_first + 1);
    int oldh = 0, d = d_first;
#pragma unroll 1
    for (int t = 0; t < nsteps; ++t) {
        FL_Q_PUBLISH(Pq, acc)
        stage(oldh, ks, ds);                                     // step t + 2 into the slot step t's MFMAs have left
        FM_NEXT_PLANE();
        vv_wait_vm<4>();                                         // in flight: [step t+1 x4][step t+2 x4] -> step t + 1 has landed
        __syncthreads();                                         // ... for every wave; Q of step t is published

        f32x4 acc_next[2][2];
        const int nexth = oldh ^ 1;
        mfma_plane(nexth, acc_next);

        const bool first = d == d_first;                         // a sample starts: nothing is carried over from the previous one
        float l0 = first ? 0.f : lo0, l1 = first ? 0.f : lo1;
        lo0 = 0.f; lo1 = 0.f;
        FL_Q_GATHER(Pq, gr, l0, l1, lo0, lo1)
        const int od = 2 * d - 1 + sl;
        if (od >= od_lo && od < od_hi) {
            float2 *slot = mine + (od - od_lo) * 128;
            float2 v = *slot;
            v.x += fl_sigmoid<FL_HW>(l0);                        // the single-sample sweep form's sigmoid; the mean is over probabilities
            v.y += fl_sigmoid<FL_HW>(l1);
            *slot = v;
        }
#pragma unroll
        for (int u = 0; u < 2; ++u) { acc[u][0] = acc_next[u][0]; acc[u][1] = acc_next[u][1]; }
        oldh = nexth;
        d = d == d_last ? d_first : d + 1;
        __syncthreads();      // every gather of Q and every read of the next plane is done: publish the next Q, refill its slot
    }
#undef FM_NEXT_PLANE
    vv_wait_vm<0>();                                             // the two (all-zero) look-ahead planes past the end

    float *dst = a.part + (size_t)s * a.slice_stride;
    for (int j = 0; j < rng; ++j) {
        const int q = 2 * j + 1 - sl;
        const size_t o = ((((((size_t)b << lo) + (od_lo + q)) << lo) + oh) << lo) + ow;   // not fl_out_index: as a call it reorders this epilogue
        *reinterpret_cast<float2 *>(dst + o) = mine[q * 128];
    }
}

// slice sums -> mean and stats partials: 1,024 voxels of one object per workgroup, slices added in ascending order
__global__ __launch_bounds__(256) void final_mean_finish_kernel(FmOut a, int vox) {
    __shared__ float red[4][4];
    const int b = blockIdx.y, i = blockIdx.x * 1024 + threadIdx.x * 4;
    float bce = 0.f, tp = 0.f, fp = 0.f, fn = 0.f;
    if (i < vox) {
        const size_t o = (size_t)b * vox + i;
        f32x4 sum = *reinterpret_cast<const f32x4 *>(a.part + o);
        for (int s = 1; s < a.nslices; ++s) sum += *reinterpret_cast<const f32x4 *>(a.part + (size_t)s * a.slice_stride + o);
        const f32x4 p = sum * a.inv_k;
        *reinterpret_cast<f32x4 *>(a.mean_probs + o) = p;
        if (a.target) {
            const f32x4 y = *reinterpret_cast<const f32x4 *>(a.target + o);
#pragma unroll
            for (int e = 0; e < 4; ++e) fl_voxel_stats<FL_PRECISE>(p[e], 0.f, y[e], a.gamma, a.epsilon, 1.0f - a.epsilon, false, bce, tp, fp, fn);
        }
    }
    if (a.target) FL_BLOCK_STATS(bce, tp, fp, fn, (int)threadIdx.x, (int)(threadIdx.x >> 6), red, a.partials, (size_t)b * gridDim.x + blockIdx.x);
}

template <typename TA>
__global__ void sample_latents_kernel(const float *__restrict__ mean, const float *__restrict__ logvar, const float *__restrict__ eps,
                                      float *__restrict__ z, TA *__restrict__ z_act, int samples, int latent, long total) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total) return;
    const long row = i / latent;
    const size_t m = (size_t)(row / samples) * latent + (size_t)(i - row * latent);
    const float v = mean[m] + sqrtf(expf(logvar[m])) * eps[i];    // function.py:37
    if (z) z[i] = v;
    if (z_act) vv_store(z_act, (size_t)i, v);
}

// How a call is cut into workgroups.
//   K slices: a function of K alone (an object's sums must not depend on the batch it arrives in): the largest power of two <= K / 4,
//             at most 8 -- a slice holds >= 4 samples, so the slice traffic stays below an eighth of the input's, and the one-object call
//             with K = 32 (nolbo_test.py's shape) gets 8 times the workgroups.
//   sweep (bf16, side >= 8): rng = input planes per depth range (<= 16: the LDS sums), halved down to 4 while the grid is short of two
//             workgroups per CU.  A depth split changes no sum: an output voxel is the same expression in every range.
struct FmPlan { bool sweep; int rng, nslices, nfin; };
constexpr long FM_FILL = 512;
int fm_slices(int samples) { return samples >= 32 ? 8 : samples >= 16 ? 4 : samples >= 8 ? 2 : 1; }
FmPlan fm_plan(int objects, int samples, int side, int dtype) {
    FmPlan p;
    p.sweep = dtype == VV_BF16 && side >= 8;
    p.nslices = fm_slices(samples);
    p.rng = 0;
    if (p.sweep) {
        p.rng = side < 16 ? side : 16;
        long wgs = (long)objects * p.nslices * (side / 8) * (side / 8) * (side / p.rng);
        while (wgs < FM_FILL && p.rng > 4) { p.rng >>= 1; wgs *= 2; }
    }
    p.nfin = (8 * side * side * side + 1023) / 1024;
    return p;
}
size_t fm_partials_bytes(int objects, int side) { return (size_t)objects * ((8 * side * side * side + 1023) / 1024) * 4 * sizeof(float); }

}  // namespace

VV_EXPORT int vv_sample_latents(const float *mean, const float *logvar, const float *eps, float *z, void *z_act, int act_dtype, int objects,
                                int samples, int latent, void *stream) {
    if (!mean || !logvar || !eps || (!z && !z_act)) return VV_ERR_NULL;
    if (z_act && !vv_dtype_in<float, __bf16>(act_dtype)) return VV_ERR_DTYPE;
    if (objects <= 0 || samples <= 0 || latent <= 0) return VV_ERR_SHAPE;
    const long total = (long)objects * samples * latent;
    const dim3 grid((unsigned)((total + 255) / 256));
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    // without z_act act_dtype is not checked and nothing is stored as it: any code but VV_BF16 takes the float instantiation
    vv_with_dtype<float, __bf16>(act_dtype == VV_BF16 ? VV_BF16 : VV_F32, [&](auto t) {
        using T = typename decltype(t)::type;
        VV_LAUNCH(sample_latents_kernel<T>, grid, dim3(256), 0, st, mean, logvar, eps, z, reinterpret_cast<T *>(z_act), samples, latent, total);
    });
    return vv_launch_status();
}

VV_EXPORT size_t vv_convT3d_final_mean_workspace_bytes(int objects, int samples, int side) {
    if (objects <= 0 || samples <= 0 || side < 4) return 0;
    // the stats partials, then the slice grids: 8 of them for every K >= 8 (K < 32 uses the first 2 or 4), one below
    return fm_partials_bytes(objects, side) + (size_t)(samples >= 8 ? 8 : 1) * objects * 8 * side * side * side * sizeof(float);
}

VV_EXPORT int vv_convT3d_final_mean_fwd(const void *x, const float *w_keras, const float *target, float *mean_probs, float *stats, int objects,
                                        int samples, int side, int cin, float gamma, float epsilon, int dtype, void *workspace,
                                        size_t workspace_bytes, void *stream) {
    if (!x || !w_keras || !mean_probs || (target != nullptr) != (stats != nullptr)) return VV_ERR_NULL;
    if (!vv_dtype_in<float, __bf16>(dtype)) return VV_ERR_DTYPE;
    if (objects <= 0 || samples < 1 || samples > 1024 || (long)objects * samples > 65535 || side < 4 || !vv_is_pow2(side) || cin != FL_CIN)
        return VV_ERR_SHAPE;
    if (!vv_aligned16(x) || (target && !vv_aligned16(target)) || !vv_aligned16(mean_probs)) return VV_ERR_ALIGN;
    if (!workspace || workspace_bytes < vv_convT3d_final_mean_workspace_bytes(objects, samples, side) || !vv_aligned16(workspace))
        return VV_ERR_WORKSPACE;
    const FmPlan p = fm_plan(objects, samples, side, dtype);
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const size_t vox = (size_t)8 * side * side * side;
    FmOut a;
    a.target = target; a.mean_probs = mean_probs;
    a.partials = reinterpret_cast<float *>(workspace);
    a.part = reinterpret_cast<float *>(reinterpret_cast<char *>(workspace) + fm_partials_bytes(objects, side));
    a.slice_stride = (size_t)objects * vox;
    a.nslices = p.nslices; a.samples = samples;
    a.gamma = gamma; a.epsilon = epsilon; a.inv_k = 1.0f / (float)samples;
    if (p.sweep) {
        vv_allow_lds<&final_mean_sweep_kernel>((int)ms_lds(16));
        // 32-bit buffer offsets: <= 2 GiB of input per launch, cut by whole objects; every per-object tensor moves on by the same range
        const size_t in_per = (size_t)side * side * side * FL_CIN * 2 * samples;
        const int per = vv_chunk_samples(in_per, objects);
        if (per < 1) return VV_ERR_SHAPE;
        const int ntile = (side / 8) * (side / 8), nranges = side / p.rng;
        for (int b0 = 0; b0 < objects; b0 += per) {
            const int nb = objects - b0 < per ? objects - b0 : per;
            FmOut c = a;
            if (target) c.target = target + (size_t)b0 * vox;
            c.mean_probs = mean_probs + (size_t)b0 * vox;
            c.part = a.part + (size_t)b0 * vox;
            VV_LAUNCH(final_mean_sweep_kernel, dim3((unsigned)(nb * p.nslices * nranges * ntile)), dim3(256), ms_lds(p.rng), st,
                      reinterpret_cast<const __bf16 *>(reinterpret_cast<const char *>(x) + (size_t)b0 * in_per), w_keras, c, vv_log2(side),
                      vv_log2(p.rng), (unsigned)((size_t)nb * in_per));
        }
    } else {
        const dim3 grid((unsigned)((side / 4) * (side / 4) * (side / 4)), (unsigned)(objects * p.nslices));
        vv_with_dtype<float, __bf16>(dtype, [&](auto t) {
            using T = typename decltype(t)::type;
            vv_allow_lds<&final_mean_box_kernel<T>>(FMB_LDS);
            VV_LAUNCH(final_mean_box_kernel<T>, grid, dim3(256), FMB_LDS, st, reinterpret_cast<const T *>(x), w_keras, a, vv_log2(side));
        });
    }
    VV_LAUNCH(final_mean_finish_kernel, dim3((unsigned)p.nfin, (unsigned)objects), dim3(256), 0, st, a, (int)vox);
    if (target) vv_final_reduce_launch(a.partials, stats, p.nfin, objects, st);
    return vv_launch_status();
}
