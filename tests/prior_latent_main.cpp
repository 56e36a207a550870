// Stand-alone program over csrc/prior_latent.h for the sanitizer test (tests/test_prior_latent_host.py): the whole-batch loops of the
// training forward, the training backward and the evaluation on exactly sized heap arrays -- small and odd shapes, the limits (L = 64,
// I = 256, B = 257 = past four pieces of the pair sums), non-finite inputs, NULL optional outputs -- built with
// -fsanitize=address,undefined.  Prints OK.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "prior_latent.h"

static unsigned long long state = 0x9E3779B97F4A7C15ull;
static float draw() {          // uniform in [-2, 2)
    state = state * 6364136223846793005ull + 1442695040888963407ull;
    return (float)((state >> 40) & 0xFFFF) / 16384.0f - 2.0f;
}
static std::vector<float> vec(size_t n) {
    std::vector<float> v(n);
    for (float &x : v) x = draw();
    return v;
}

static int run(int B, int L, int I, bool masked, bool hostile, bool twins) {
    const size_t n = (size_t)B * L;
    std::vector<float> enc = vec(2 * n), eps = vec(n), mp = vec(n), lp = vec(n), epsp = vec(n), keep(n), dz = vec(n);
    for (float &m : keep) m = draw() > 0.0f ? 1.0f : 0.0f;
    if (B > 1)
        for (int l = 0; l < L; ++l) mp[(size_t)L + l] = mp[l];                 // two samples with identical prior means
    if (hostile) {
        enc[0] = vv_det_float(0x7FC00000u), enc[(size_t)L] = 1e30f;
        if (n > 1) enc[1] = vv_le_inf();
        lp[0] = -1e30f;
    }
    std::vector<float> zin(n), kl(B), reg(B), de(2 * n), dm(n), dlv(n);
    std::vector<unsigned short> zb(n);
    VvPlTrain t = {};
    t.enc_out = enc.data(), t.eps = eps.data(), t.mean_p = mp.data(), t.lv_p = lp.data(), t.eps_p = epsp.data();
    t.keep = masked ? keep.data() : nullptr, t.dz_in = dz.data(), t.dist = 3.0f * (float)L, t.inv_batch = 1.0f / (float)B, t.reg_weight = 0.01f;
    t.z_in = zin.data(), t.z_in_bf16 = twins ? zb.data() : nullptr, t.kl = kl.data(), t.reg = reg.data();
    t.d_enc_out = de.data(), t.d_mean_p = hostile ? nullptr : dm.data(), t.d_lv_p = twins ? dlv.data() : nullptr, t.B = B, t.L = L;
    for (int i = 0; i < B; ++i) vv_pl_train_fwd_sample(t, i);
    for (int i = 0; i < B; ++i) vv_pl_train_bwd_sample(t, i);
    if (!hostile)
        for (int l = 0; l < L; ++l)
            if (dm[l] != dm[l]) return 2;                                       // |a - b| at a == b: gradient 0, not NaN

    std::vector<float> prior = vec((size_t)I * L), fill = vec(n), mask(n), z(n), zc(n);
    std::vector<unsigned short> zcb(n);
    std::vector<int> idx(B);
    for (float &m : mask) m = draw() > 0.0f ? 1.0f : 0.0f;
    if (hostile) prior[0] = vv_det_float(0x7FC00000u);
    VvPlEval e = {};
    e.enc_out = enc.data(), e.eps = eps.data(), e.mask = masked ? mask.data() : nullptr, e.fill = masked ? fill.data() : nullptr;
    e.prior = prior.data(), e.z = z.data(), e.z_corr = zc.data(), e.z_bf16 = twins ? zb.data() : nullptr;
    e.z_corr_bf16 = twins ? zcb.data() : nullptr, e.idx = idx.data(), e.B = B, e.L = L, e.I = I;
    for (int b = 0; b < B; ++b) vv_pl_eval_sample(e, b);
    for (int b = 0; b < B; ++b)
        if (idx[b] < 0 || idx[b] >= I) return 1;
    return 0;
}

int main() {
    int rc = 0;
    rc |= run(1, 1, 1, true, false, false);
    rc |= run(2, 16, 10, false, false, true);
    rc |= run(5, 3, 1, true, true, true);
    rc |= run(65, 1, 7, true, false, false);
    rc |= run(257, 64, 256, true, false, true);
    rc |= run(130, 5, 256, false, true, false);
    if (rc) {
        std::printf("FAILED %d\n", rc);
        return 1;
    }
    std::printf("OK\n");
    return 0;
}
