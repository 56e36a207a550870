// The one-group, one-prior latent stage on the device: fit's sampling | prior / posterior choice | KL | pairwise regulariser with its
// backward for nolboSingleObject_instOnly, nolboSingleObject_category_only and nolboSingleObject_modelnet_category_only, and
// instOnly.getEval's sampling | mask | fill | nearest prior row.  The arithmetic and every decision are prior_latent.h, float32, shared
// with the host entries.
//
// Form.  Training: a 256-thread workgroup takes VV_PL_ROWS = 4 rows i, one per wave; lane e of a wave owns element e of its row.  The
//   pair sums walk the batch in pieces of VV_PL_PIECE = 64 rows j: the whole workgroup copies the piece's prior means (the backward: and
//   the scales exp(0.5 lv_j)) into LDS with coalesced loads -- rows padded to 65 words, so lane j reading column l and lane l reading
//   row k are both conflict-free -- and all four waves use it.  Forward: lane j forms the hinge term of pair (i, j0 + j); lane 0 adds
//   the piece's terms to the row's running sum in ascending j.  Backward: lane j forms the two pair weights of (i, j0 + j) and
//   (j0 + j, i); lane e then accumulates element e's sums over the piece in ascending j.  Any B: the running sums pass from piece to
//   piece in registers.
//   Evaluation: a workgroup per sample; lanes 0 .. L-1 sample (mask, fill) z into LDS, thread c takes prior row c, and the first argmin
//   comes from a shuffle reduction over (distance, index) pairs -- a total order, so the result is the sequential loop's.
// No atomics, no inline assembly: a given input gives the same bits on every run, and the bits of the host entries.  gfx950 only.
#include "latent_block.h"
#include "prior_latent.h"

namespace {

static_assert(VV_PL_THREADS == 64 * VV_LE_WAVES, "the workgroup of vv_le_block_argmin");
constexpr int PL_PAD = VV_PL_MAX_L + 1;

// the piece's rows j0 .. j0 + n - 1 of a [B, L] array into LDS rows of PL_PAD words, optionally as scales
template <bool SCALE>
__device__ __forceinline__ void pl_stage(float (*dst)[PL_PAD], const float *src, int j0, int n, int L) {
    const float *p = src + (long long)j0 * L;
    for (int k = threadIdx.x; k < n * L; k += VV_PL_THREADS) {
        const int r = k / L, c = k - r * L;
        dst[r][c] = SCALE ? vv_le_scale(p[k]) : p[k];
    }
}

__global__ __launch_bounds__(VV_PL_THREADS) void pl_train_fwd_kernel(const VvPlTrain a) {
    __shared__ float mp[VV_PL_PIECE][PL_PAD];
    __shared__ float mi[VV_PL_ROWS][VV_PL_MAX_L], ei[VV_PL_ROWS][VV_PL_MAX_L], term[VV_PL_ROWS][VV_PL_MAX_L], hv[VV_PL_ROWS][VV_PL_PIECE];
    const int t = threadIdx.x, w = t >> 6, lane = t & 63, L = a.L;
    const long long row = (long long)blockIdx.x * VV_PL_ROWS + w;
    const bool live = row < a.B;
    const int i = live ? (int)row : 0;
    if (live && lane < L) {
        const VvLeElem v = vv_pl_elem(a, i, lane);
        const float zi = vv_le_z_in(v);
        a.z_in[(long long)i * L + lane] = zi;
        if (a.z_in_bf16) a.z_in_bf16[(long long)i * L + lane] = vv_le_bf16(zi);
        term[w][lane] = vv_le_kl_term(v);
        mi[w][lane] = v.mt, ei[w][lane] = vv_le_scale(v.lvt);
    }
    float s = 0.0f;
    for (int j0 = 0; j0 < a.B; j0 += VV_PL_PIECE) {                 // uniform over the workgroup
        const int n = a.B - j0 < VV_PL_PIECE ? a.B - j0 : VV_PL_PIECE;
        pl_stage<false>(mp, a.mean_p, j0, n, L);
        __syncthreads();                                             // the piece (first time: and mi, ei, term) is in LDS
        if (live && lane < n) hv[w][lane] = vv_le_hinge(vv_pl_pair_dist(mi[w], mp[lane], ei[w], L) - a.dist);
        __syncthreads();                                             // every wave has read the piece; the wave's terms are in LDS
        if (live && lane == 0) {
#pragma clang fp contract(off)
            for (int k = 0; k < n; ++k) s = s + hv[w][k];
        }
    }
    if (live && lane == 0) a.kl[i] = vv_le_sum(term[w], L), a.reg[i] = s;
}

__global__ __launch_bounds__(VV_PL_THREADS) void pl_train_bwd_kernel(const VvPlTrain a) {
    __shared__ float mp[VV_PL_PIECE][PL_PAD], ep[VV_PL_PIECE][PL_PAD];
    __shared__ float mi[VV_PL_ROWS][VV_PL_MAX_L], ei[VV_PL_ROWS][VV_PL_MAX_L], g[VV_PL_ROWS][2][VV_PL_PIECE];
    const int t = threadIdx.x, w = t >> 6, lane = t & 63, L = a.L;
    const long long row = (long long)blockIdx.x * VV_PL_ROWS + w;
    const bool live = row < a.B;
    const int i = live ? (int)row : 0;
    float am = 0.0f, alv = 0.0f, m_e = 0.0f, e_e = 1.0f;
    if (live && lane < L) {
        m_e = a.mean_p[(long long)i * L + lane], e_e = vv_le_scale(a.lv_p[(long long)i * L + lane]);
        mi[w][lane] = m_e, ei[w][lane] = e_e;
    }
    for (int j0 = 0; j0 < a.B; j0 += VV_PL_PIECE) {                 // uniform over the workgroup
        const int n = a.B - j0 < VV_PL_PIECE ? a.B - j0 : VV_PL_PIECE;
        pl_stage<false>(mp, a.mean_p, j0, n, L);
        pl_stage<true>(ep, a.lv_p, j0, n, L);
        __syncthreads();
        if (live && lane < n) {
            g[w][0][lane] = vv_le_hinge_grad(vv_pl_pair_dist(mi[w], mp[lane], ei[w], L) - a.dist);
            g[w][1][lane] = vv_le_hinge_grad(vv_pl_pair_dist(mp[lane], mi[w], ep[lane], L) - a.dist);
        }
        __syncthreads();
        if (live && lane < L)
            for (int k = 0; k < n; ++k) vv_le_pair_accumulate(am, alv, g[w][0][k], g[w][1][k], m_e, mp[k][lane], e_e, ep[k][lane]);
        __syncthreads();                                             // the piece is read: the next one may overwrite it
    }
    if (live && lane < L) vv_pl_bwd_store(a, i, lane, am, alv);
}

__global__ __launch_bounds__(VV_PL_THREADS) void pl_eval_kernel(const VvPlEval a) {
    __shared__ float z[VV_PL_MAX_L], msk[VV_PL_MAX_L];
    __shared__ VvLeBest red[VV_LE_WAVES];
    const int t = threadIdx.x, b = blockIdx.x, L = a.L;
    const bool masked = a.mask != nullptr;
    float v = 0.0f;
    if (t < L) {
        v = vv_pl_eval_z(a, b, t);
        z[t] = v;
        if (masked) msk[t] = a.mask[(long long)b * L + t];
    }
    __syncthreads();
    VvLeBest best = vv_le_best_init();
    if (t < a.I) vv_le_best_take(best, vv_le_dist(z, masked ? msk : nullptr, a.prior + (long long)t * L, L), t);
    const int ix = vv_le_block_argmin(best, red);
    if (t < L) vv_pl_eval_store(a, b, t, v, ix);
    if (t == 0) a.idx[b] = ix;
}

int pl_train_check(const VvPlTrain &a, bool bwd) {
    const void *need[] = {a.enc_out, a.eps, a.mean_p, a.lv_p, a.eps_p};
    for (const void *p : need)
        if (!p) return VV_ERR_NULL;
    if (bwd ? (!a.dz_in || !a.d_enc_out) : (!a.z_in || !a.kl || !a.reg)) return VV_ERR_NULL;
    if (!vv_le_dims_ok(a.B, a.L, VV_PL_MAX_L)) return VV_ERR_SHAPE;
    const void *f32s[] = {a.enc_out, a.eps, a.mean_p, a.lv_p, a.eps_p, a.keep, a.dz_in, a.z_in, a.kl, a.reg, a.d_enc_out, a.d_mean_p, a.d_lv_p};
    for (const void *p : f32s)
        if (vv_le_misaligned(p, 3u)) return VV_ERR_ALIGN;
    if (vv_le_misaligned(a.z_in_bf16, 1u)) return VV_ERR_ALIGN;
    return VV_OK;
}

int pl_eval_check(const VvPlEval &a) {
    const void *need[] = {a.enc_out, a.eps, a.prior, a.z, a.z_corr, a.idx};
    for (const void *p : need)
        if (!p) return VV_ERR_NULL;
    if ((a.mask != nullptr) != (a.fill != nullptr)) return VV_ERR_NULL;        // fill exactly when the mask is given
    if (!vv_le_dims_ok(a.B, a.L, VV_PL_MAX_L) || a.I < 1 || a.I > VV_PL_MAX_I) return VV_ERR_SHAPE;
    const void *f32s[] = {a.enc_out, a.eps, a.mask, a.fill, a.prior, a.z, a.z_corr, a.idx};
    for (const void *p : f32s)
        if (vv_le_misaligned(p, 3u)) return VV_ERR_ALIGN;
    if (vv_le_misaligned(a.z_bf16, 1u) || vv_le_misaligned(a.z_corr_bf16, 1u)) return VV_ERR_ALIGN;
    return VV_OK;
}

VvPlTrain pl_train_args(const float *enc_out, const float *eps, const float *mean_p, const float *lv_p, const float *eps_p, const float *keep,
                        float dist, int batch, int latent) {
    VvPlTrain a = {};
    a.enc_out = enc_out, a.eps = eps, a.mean_p = mean_p, a.lv_p = lv_p, a.eps_p = eps_p, a.keep = keep, a.dist = dist;
    a.B = batch, a.L = latent;
    return a;
}

inline dim3 pl_train_grid(int batch) { return dim3((unsigned)(((long long)batch + VV_PL_ROWS - 1) / VV_PL_ROWS)); }

// One body per entry pair: the arguments, the check, and then the launch (host == false) or the host's loop over the samples.
int pl_train(const VvPlTrain &a, bool bwd, bool host, void *hip_stream) {
    const int rc = pl_train_check(a, bwd);
    if (rc != VV_OK) return rc;
    if (host) {
        for (int i = 0; i < a.B; ++i) bwd ? vv_pl_train_bwd_sample(a, i) : vv_pl_train_fwd_sample(a, i);
        return VV_OK;
    }
    hipStream_t st = reinterpret_cast<hipStream_t>(hip_stream);
    if (bwd) VV_LAUNCH(pl_train_bwd_kernel, pl_train_grid(a.B), dim3(VV_PL_THREADS), 0, st, a);
    else VV_LAUNCH(pl_train_fwd_kernel, pl_train_grid(a.B), dim3(VV_PL_THREADS), 0, st, a);
    return vv_launch_status();
}

int pl_train_fwd(const float *enc_out, const float *eps, const float *mean_p, const float *lv_p, const float *eps_p, const float *keep,
                 float dist, float *z_in, void *z_in_bf16, float *kl, float *reg, int batch, int latent, bool host, void *hip_stream) {
    VvPlTrain a = pl_train_args(enc_out, eps, mean_p, lv_p, eps_p, keep, dist, batch, latent);
    a.z_in = z_in, a.z_in_bf16 = static_cast<unsigned short *>(z_in_bf16), a.kl = kl, a.reg = reg;
    return pl_train(a, false, host, hip_stream);
}

int pl_train_bwd(const float *enc_out, const float *eps, const float *mean_p, const float *lv_p, const float *eps_p, const float *keep,
                 float dist, const float *dz_in, float inv_batch, float reg_weight, float *d_enc_out, float *d_mean_p, float *d_lv_p, int batch,
                 int latent, bool host, void *hip_stream) {
    VvPlTrain a = pl_train_args(enc_out, eps, mean_p, lv_p, eps_p, keep, dist, batch, latent);
    a.dz_in = dz_in, a.inv_batch = inv_batch, a.reg_weight = reg_weight, a.d_enc_out = d_enc_out, a.d_mean_p = d_mean_p, a.d_lv_p = d_lv_p;
    return pl_train(a, true, host, hip_stream);
}

int pl_eval(const float *enc_out, const float *eps, const float *mask, const float *fill, const float *prior, float *z, float *z_corr,
            void *z_bf16, void *z_corr_bf16, int *idx, int batch, int latent, int insts, bool host, void *hip_stream) {
    VvPlEval a = {};
    a.enc_out = enc_out, a.eps = eps, a.mask = mask, a.fill = fill, a.prior = prior, a.z = z, a.z_corr = z_corr;
    a.z_bf16 = static_cast<unsigned short *>(z_bf16), a.z_corr_bf16 = static_cast<unsigned short *>(z_corr_bf16), a.idx = idx;
    a.B = batch, a.L = latent, a.I = insts;
    const int rc = pl_eval_check(a);
    if (rc != VV_OK) return rc;
    if (host) {
        for (int b = 0; b < batch; ++b) vv_pl_eval_sample(a, b);
        return VV_OK;
    }
    VV_LAUNCH(pl_eval_kernel, dim3((unsigned)batch), dim3(VV_PL_THREADS), 0, reinterpret_cast<hipStream_t>(hip_stream), a);
    return vv_launch_status();
}

}  // namespace

VV_EXPORT int vv_prior_latent_train_fwd(const float *enc_out, const float *eps, const float *mean_p, const float *lv_p, const float *eps_p,
                                        const float *keep, float dist, float *z_in, void *z_in_bf16, float *kl, float *reg, int batch,
                                        int latent, void *hip_stream) {
    return pl_train_fwd(enc_out, eps, mean_p, lv_p, eps_p, keep, dist, z_in, z_in_bf16, kl, reg, batch, latent, false, hip_stream);
}

VV_EXPORT int vv_prior_latent_train_fwd_host(const float *enc_out, const float *eps, const float *mean_p, const float *lv_p,
                                             const float *eps_p, const float *keep, float dist, float *z_in, void *z_in_bf16, float *kl,
                                             float *reg, int batch, int latent) {
    return pl_train_fwd(enc_out, eps, mean_p, lv_p, eps_p, keep, dist, z_in, z_in_bf16, kl, reg, batch, latent, true, nullptr);
}

VV_EXPORT int vv_prior_latent_train_bwd(const float *enc_out, const float *eps, const float *mean_p, const float *lv_p, const float *eps_p,
                                        const float *keep, float dist, const float *dz_in, float inv_batch, float reg_weight,
                                        float *d_enc_out, float *d_mean_p, float *d_lv_p, int batch, int latent, void *hip_stream) {
    return pl_train_bwd(enc_out, eps, mean_p, lv_p, eps_p, keep, dist, dz_in, inv_batch, reg_weight, d_enc_out, d_mean_p, d_lv_p, batch, latent,
                        false, hip_stream);
}

VV_EXPORT int vv_prior_latent_train_bwd_host(const float *enc_out, const float *eps, const float *mean_p, const float *lv_p,
                                             const float *eps_p, const float *keep, float dist, const float *dz_in, float inv_batch,
                                             float reg_weight, float *d_enc_out, float *d_mean_p, float *d_lv_p, int batch, int latent) {
    return pl_train_bwd(enc_out, eps, mean_p, lv_p, eps_p, keep, dist, dz_in, inv_batch, reg_weight, d_enc_out, d_mean_p, d_lv_p, batch, latent,
                        true, nullptr);
}

VV_EXPORT int vv_inst_latent_eval(const float *enc_out, const float *eps, const float *mask, const float *fill, const float *prior, float *z,
                                  float *z_corr, void *z_bf16, void *z_corr_bf16, int *idx, int batch, int latent, int insts,
                                  void *hip_stream) {
    return pl_eval(enc_out, eps, mask, fill, prior, z, z_corr, z_bf16, z_corr_bf16, idx, batch, latent, insts, false, hip_stream);
}

VV_EXPORT int vv_inst_latent_eval_host(const float *enc_out, const float *eps, const float *mask, const float *fill, const float *prior,
                                       float *z, float *z_corr, void *z_bf16, void *z_corr_bf16, int *idx, int batch, int latent,
                                       int insts) {
    return pl_eval(enc_out, eps, mask, fill, prior, z, z_corr, z_bf16, z_corr_bf16, idx, batch, latent, insts, true, nullptr);
}
