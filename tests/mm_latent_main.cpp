// Stand-alone program over csrc/mm_latent.h for the sanitizer test (tests/test_mm_latent_host.py): the whole-batch loops of the evaluation,
// the training forward and the training backward on exactly sized heap arrays -- small and odd shapes, the limits (Lc = Li = 64,
// C = I = 256, B = 257 = a second piece of the pair sums), non-finite inputs -- built with -fsanitize=address,undefined.  Prints OK.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "mm_latent.h"

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

static int run(int B, int Lc, int Li, int C, int I, bool masked, bool hostile, int act_dtype) {
    const size_t L = (size_t)Lc + Li;
    std::vector<float> enc = vec((size_t)B * 2 * L), eps = vec(B * L), eps2 = vec((size_t)B * Lc), pc = vec((size_t)C * Lc);
    std::vector<float> pi = vec((size_t)B * I * Li), mask((size_t)B * Lc), co((size_t)B * C, 0.0f), io((size_t)B * I, 0.0f);
    for (float &m : mask) m = draw() > 0.0f ? 1.0f : 0.0f;
    for (int b = 0; b < B; ++b) co[(size_t)b * C + b % C] = 1.0f, io[(size_t)b * I + (b * 7) % I] = 1.0f;
    if (hostile) {
        enc[0] = vv_det_float(0x7FC00000u), enc[1] = vv_le_inf(), enc[(size_t)Lc] = 1e30f, enc[(size_t)Lc + 1] = -1e30f;
        pc[0] = vv_det_float(0x7FC00000u);
    }
    std::vector<float> z(B * L), zc(B * L), acc(3);
    std::vector<unsigned short> za(B * L * 2), zca(B * L * 2);
    std::vector<int> idx((size_t)B * 4);
    VvMmEval e = {};
    e.enc_out = enc.data(), e.eps = eps.data(), e.mask = masked ? mask.data() : nullptr, e.eps2 = masked ? eps2.data() : nullptr;
    e.prior_cat = pc.data(), e.prior_inst = pi.data(), e.cat_onehot = co.data(), e.inst_onehot = io.data(), e.z = z.data();
    e.z_corr = zc.data(), e.z_act = za.data(), e.z_corr_act = masked ? zca.data() : nullptr, e.act_dtype = act_dtype, e.idx = idx.data();
    e.acc = acc.data(), e.B = B, e.Lc = Lc, e.Li = Li, e.C = C, e.I = I;
    vv_mm_eval_all(e);
    for (int b = 0; b < B; ++b)
        if (idx[(size_t)b * 4] < 0 || idx[(size_t)b * 4] >= C || idx[(size_t)b * 4 + 1] < 0 || idx[(size_t)b * 4 + 1] >= I ||
            idx[(size_t)b * 4 + 2] < 0 || idx[(size_t)b * 4 + 2] >= C || idx[(size_t)b * 4 + 3] < 0 || idx[(size_t)b * 4 + 3] >= C)
            return 1;

    std::vector<float> mcp = vec((size_t)B * Lc), lcp = vec((size_t)B * Lc), mip = vec((size_t)B * Li), lip = vec((size_t)B * Li);
    std::vector<float> epsp = vec(B * L), noise(B * L), dz = vec(B * L), zin(B * L), kl(B), reg(B);
    std::vector<float> de((size_t)B * 2 * L), dmc((size_t)B * Lc), dlc((size_t)B * Lc), dmi((size_t)B * Li), dli((size_t)B * Li);
    for (float &m : noise) m = draw() > 0.0f ? 1.0f : 0.0f;
    if (B > 1)
        for (int l = 0; l < Lc; ++l) mcp[(size_t)Lc + l] = mcp[l];          // two samples with identical prior means
    VvMmTrain t = {};
    t.enc_out = enc.data(), t.eps = eps.data(), t.mean_cp = mcp.data(), t.lv_cp = lcp.data(), t.mean_ip = mip.data(), t.lv_ip = lip.data();
    t.eps_p = epsp.data(), t.noise = masked ? noise.data() : nullptr, t.cat_onehot = co.data(), t.dz_in = dz.data(), t.inv_batch = 1.0f / (float)B;
    t.z_in = zin.data(), t.z_in_act = za.data(), t.act_dtype = act_dtype, t.kl = kl.data(), t.reg = reg.data(), t.d_enc_out = de.data();
    t.d_mean_cp = dmc.data(), t.d_lv_cp = hostile ? nullptr : dlc.data(), t.d_mean_ip = dmi.data(), t.d_lv_ip = hostile ? nullptr : dli.data();
    t.B = B, t.Lc = Lc, t.Li = Li, t.C = C;
    for (int i = 0; i < B; ++i) vv_mm_train_fwd_sample(t, i);
    for (int i = 0; i < B; ++i) vv_mm_train_bwd_sample(t, i);
    if (!hostile)
        for (int l = 0; l < Lc; ++l)
            if (dmc[l] != dmc[l]) return 2;                                   // |a - b| at a == b: gradient 0, not NaN
    return 0;
}

int main() {
    int rc = 0;
    rc |= run(1, 1, 1, 1, 1, true, false, VV_LE_F32);
    rc |= run(1, 7, 12, 12, 10, false, false, VV_LE_BF16);
    rc |= run(5, 3, 9, 12, 1, true, true, VV_LE_BF16);
    rc |= run(72, 8, 8, 12, 10, true, false, VV_LE_F32);
    rc |= run(257, 64, 64, 256, 256, true, false, VV_LE_BF16);
    rc |= run(300, 5, 64, 3, 256, false, true, VV_LE_F32);
    if (rc) {
        std::printf("FAILED %d\n", rc);
        return 1;
    }
    std::printf("OK\n");
    return 0;
}
