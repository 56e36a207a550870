"""CPU tests of the oracle itself: three independent statements must agree
(numpy definition / C fp32 restatement / torch-CPU functional ops), plus the committed golden
fixtures and the loss edge cases of SURVEY.md §8(c).  No GPU."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import c_oracle as co
from oracle import numpy_oracle as no
from voxvae import synthetic as syn

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')


def _torch_conv_same(x, w, s):
    # Keras [kd,kh,kw,Ci,Co] -> torch [Co,Ci,kd,kh,kw]; TF SAME for k=4: s=2 pads (1,1), s=1 pads (1,2)
    xt = torch.from_numpy(x).permute(0, 4, 1, 2, 3)
    wt = torch.from_numpy(w).permute(4, 3, 0, 1, 2)
    pad = (1, 1) * 3 if s == 2 else (1, 2) * 3
    return F.conv3d(F.pad(xt, pad), wt, stride=s).permute(0, 2, 3, 4, 1).numpy()


def _torch_convT_same(x, w, s):
    # Keras [kd,kh,kw,Co,Ci] -> torch conv_transpose weight [Ci,Co,kd,kh,kw]; padding=1, crop to n*s
    xt = torch.from_numpy(x).permute(0, 4, 1, 2, 3)
    wt = torch.from_numpy(w).permute(4, 3, 0, 1, 2)
    y = F.conv_transpose3d(xt, wt, stride=s, padding=1)
    n = x.shape[1] * s
    return y[:, :, :n, :n, :n].permute(0, 2, 3, 4, 1).numpy()


@pytest.mark.parametrize('D,Ci,Co,s', [(8, 3, 5, 2), (4, 4, 6, 1), (2, 8, 4, 1), (6, 1, 7, 2), (7, 2, 3, 2), (5, 2, 3, 1)])
def test_conv3d_same_three_statements(D, Ci, Co, s):
    rng = np.random.default_rng(D * 100 + Ci)
    x = rng.standard_normal((2, D, D, D, Ci))
    w = rng.standard_normal((4, 4, 4, Ci, Co))
    y_np = no.conv3d_same(x, w, s)
    assert y_np.shape[1] == -(-D // s)
    if D % s == 0:                                  # torch statement uses the fixed pads of even sizes
        np.testing.assert_allclose(y_np, _torch_conv_same(x, w, s), rtol=0, atol=1e-11)
    y_c = co.conv3d_same(x, w, s)
    np.testing.assert_allclose(y_c, y_np, rtol=0, atol=2e-4)


@pytest.mark.parametrize('D,Ci,Co,s', [(4, 3, 5, 2), (2, 8, 6, 1), (4, 8, 4, 1), (3, 2, 1, 2), (8, 4, 1, 2)])
def test_conv3d_transpose_same_three_statements(D, Ci, Co, s):
    rng = np.random.default_rng(D * 10 + Co)
    x = rng.standard_normal((2, D, D, D, Ci))
    w = rng.standard_normal((4, 4, 4, Co, Ci))
    y_np = no.conv3d_transpose_same(x, w, s)
    assert y_np.shape == (2, D * s, D * s, D * s, Co)
    np.testing.assert_allclose(y_np, _torch_convT_same(x, w, s), rtol=0, atol=1e-11)
    np.testing.assert_allclose(co.conv3d_transpose_same(x, w, s), y_np, rtol=0, atol=2e-4)


@pytest.mark.parametrize('D,Ci,Co,s', [(8, 2, 3, 2), (6, 1, 2, 2), (4, 3, 2, 1), (7, 2, 2, 2)])
def test_conv_and_transpose_against_scipy_correlate(D, Ci, Co, s):
    """A fourth, independent statement (round 4): scipy.signal.correlate / convolve, an N-D routine that shares no code with numpy_oracle's
    tap loops, the C restatement or torch's oneDNN path.  Conv3D SAME = 'valid' cross-correlation of the TF-padded input, strided by
    slicing; Conv3DTranspose SAME = full convolution of the zero-stuffed input with the kernel, cropped by pad_before (the gradient-of-conv
    definition TensorFlow documents)."""
    from scipy import signal
    rng = np.random.default_rng(D * 7 + Ci)
    x = rng.standard_normal((2, D, D, D, Ci))
    w = rng.standard_normal((4, 4, 4, Ci, Co))
    out_n = -(-D // s)
    pad_total = max((out_n - 1) * s + 4 - D, 0)
    pb = pad_total // 2
    xp = np.pad(x, ((0, 0),) + ((pb, pad_total - pb),) * 3 + ((0, 0),))
    y = np.zeros((2, out_n, out_n, out_n, Co))
    for b in range(2):
        for co in range(Co):
            acc = sum(signal.correlate(xp[b, ..., ci], w[..., ci, co], mode='valid') for ci in range(Ci))
            y[b, ..., co] = acc[::s, ::s, ::s][:out_n, :out_n, :out_n]
    np.testing.assert_allclose(no.conv3d_same(x, w, s), y, rtol=0, atol=1e-10)
    # transposed: Keras kernel [k,k,k,Cout_T,Cin_T]; input z [2,n,n,n,Cin_T] -> [2,n*s,n*s,n*s,Cout_T]
    n = out_n
    z = rng.standard_normal((2, n, n, n, Co))
    wt = rng.standard_normal((4, 4, 4, Ci, Co))                     # Cout_T = Ci, Cin_T = Co
    N = n * s
    pt = max((n - 1) * s + 4 - N, 0)
    ptb = pt // 2
    yt = np.zeros((2, N, N, N, Ci))
    for b in range(2):
        for co in range(Ci):
            acc = 0.0
            for ci in range(Co):
                up = np.zeros(((n - 1) * s + 1,) * 3)
                up[::s, ::s, ::s] = z[b, ..., ci]
                acc = acc + signal.convolve(up, wt[..., co, ci], mode='full')
            yt[b, ..., co] = acc[ptb:ptb + N, ptb:ptb + N, ptb:ptb + N]
    np.testing.assert_allclose(no.conv3d_transpose_same(z, wt, s), yt, rtol=0, atol=1e-10)


def test_transpose_is_adjoint_of_conv():
    """<conv(x), y> == <x, convT(y)> for the same kernel: the defining property of Conv3DTranspose."""
    rng = np.random.default_rng(3)
    for s, D in ((2, 8), (1, 4)):
        x = rng.standard_normal((1, D, D, D, 3))
        w = rng.standard_normal((4, 4, 4, 3, 5))         # forward kernel Ci=3 -> Co=5
        y = rng.standard_normal((1, D // s, D // s, D // s, 5))
        lhs = np.sum(no.conv3d_same(x, w, s) * y)
        rhs = np.sum(x * no.conv3d_transpose_same(y, w, s))   # same array read as [k,k,k,Co_T=3,Ci_T=5]
        assert abs(lhs - rhs) < 1e-9 * max(1.0, abs(lhs))


def test_bn_act_and_dense_c_vs_numpy():
    rng = np.random.default_rng(0)
    x = rng.standard_normal((3, 2, 2, 2, 16)).astype(np.float32)
    p = {'bn/gamma': rng.uniform(0.5, 1.5, 16).astype(np.float32), 'bn/beta': rng.normal(0, 0.1, 16).astype(np.float32),
         'bn/moving_mean': rng.normal(0, 0.1, 16).astype(np.float32),
         'bn/moving_variance': rng.uniform(0.5, 1.5, 16).astype(np.float32)}
    for act in ('elu', 'relu', 'lrelu', 'None'):
        ref = no.activation(no.batchnorm_inference(x.astype(np.float64), p['bn/gamma'], p['bn/beta'], p['bn/moving_mean'],
                                                   p['bn/moving_variance']), act)
        got = co.bn_act_(x.copy(), p, 'bn', act)
        np.testing.assert_allclose(got, ref, rtol=0, atol=2e-6)


@pytest.mark.parametrize('name', ['vae_d32_l64_b2', 'ae_d32_l64_b2', 'vae_d16_l64_b3'])
def test_c_oracle_matches_golden(name):
    g = np.load(os.path.join(GOLDEN, name + '.npz'))
    D, L, var, B, C = [int(v) for v in g['meta'][:5]]
    cfg = syn.make_config(D, L, bool(var))
    ep, dp = syn.make_encoder_params(cfg['encoder']), syn.make_decoder_params(cfg['decoder'])
    x, eps = syn.make_voxels(B, D), syn.make_eps(B, L)
    c = co.vae_eval_forward(cfg, ep, dp, x, x, eps, variational=bool(var))
    np.testing.assert_allclose(c['enc_out'], g['p0_enc_out'], rtol=0, atol=2e-6)
    np.testing.assert_allclose(c['z'], g['p0_z'], rtol=0, atol=5e-6)
    if var:
        np.testing.assert_allclose(c['kl'], g['p0_kl'], rtol=1e-5, atol=1e-6)
    lg = g['p0_logits']
    np.testing.assert_allclose(c['logits'], lg, rtol=0, atol=1e-4)       # well inside the 1e-3 bar
    safe = np.abs(lg) > 1e-4                                              # occupancy exact away from the threshold
    assert np.array_equal((c['logits'] >= 0)[safe], (lg >= 0)[safe])
    np.testing.assert_allclose(c['bce'], g['p0_bce'], rtol=2e-6)
    for k in ('tp', 'fp', 'fn'):
        assert np.abs(c[k] - g['p0_' + k]).max() <= np.sum(~safe)


def test_numpy_oracle_reproduces_golden_fp64():
    """The fixture generator is deterministic (seeded numpy Generators)."""
    import importlib.util
    spec = importlib.util.spec_from_file_location('make_golden', os.path.join(GOLDEN, 'make_golden.py'))
    mg = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mg)
    new = mg.make_case('vae_d16_l64_b3')
    g = np.load(os.path.join(GOLDEN, 'vae_d16_l64_b3.npz'))
    for k in g.files:
        np.testing.assert_array_equal(new[k], g[k])


def test_binary_loss_edge_cases():
    """SURVEY.md hard part 6: in float32 the upper clip 1-1e-7 is 0.99999988, i.e. logits saturate at
    +-15.9424; all-empty / all-full grids; TP+FP == 0 -> precision 0 through the 1e-10 guard."""
    assert np.float32(1.0) - np.float32(1e-7) == np.float32(0.99999988)
    lg = np.array([[-40.0, -16.0, -15.9, 0.0, 15.9, 16.0, 40.0, -1e-9]], np.float32)
    y = np.array([[1, 0, 1, 1, 0, 1, 0, 1]], np.float32)
    p32 = no.sigmoid(lg.astype(np.float32))
    ref = no.binary_loss(p32, y, gamma=0.6)
    probs, bce, tp, fp, fn = co.sigmoid_bce_counts(lg, y)
    np.testing.assert_allclose(bce, ref, rtol=1e-6)
    # saturated positives cost -0.6*log(1e-7), saturated negatives -0.4*log(1-0.99999988)
    assert abs(float(no.binary_loss(np.array([[0.0]], np.float32), np.array([[1.0]], np.float32), gamma=0.6)[0])
               - 0.6 * 16.118095) < 1e-4
    t_tp, t_fp, t_fn = no.voxel_precision_recall(y, p32)
    assert (tp[0], fp[0], fn[0]) == (t_tp[0], t_fp[0], t_fn[0])
    # threshold is >= on the float32 probability: sigmoid(-1e-9) rounds to 0.5 -> occupied
    assert probs[0, -1] == np.float32(0.5) and t_tp[0] == 3
    empty = np.zeros((1, 64), np.float32)
    tp0, fp0, fn0 = no.voxel_precision_recall(empty, np.full((1, 64), 0.1, np.float32))
    pr, rc = no.pr_rc(tp0, fp0, fn0)
    assert pr == 0.0 and rc == 0.0
    full = np.ones((1, 64), np.float32)
    tp1, fp1, fn1 = no.voxel_precision_recall(full, np.full((1, 64), 0.9, np.float32))
    assert no.pr_rc(tp1, fp1, fn1) == (pytest.approx(1.0), pytest.approx(1.0))


def test_kl_and_sampling_formulas():
    rng = np.random.default_rng(1)
    e = rng.standard_normal((4, 32)).astype(np.float32) * 6
    eps = rng.standard_normal((4, 16)).astype(np.float32)
    mu, lv = no.split_mean_logvar(e.astype(np.float64), 16)
    assert lv.min() >= -10 and lv.max() <= 10
    z, kl = co.reparam_kl(e, eps, 16)
    np.testing.assert_allclose(z, no.sampling(mu, lv, eps), rtol=1e-5, atol=1e-5)
    np.testing.assert_allclose(kl, no.kl_loss(mu, lv, 0 * mu, 0 * lv), rtol=2e-5)
    # closed form against torch.distributions
    q = torch.distributions.Normal(torch.from_numpy(mu), torch.from_numpy(np.exp(0.5 * lv)))
    pr = torch.distributions.Normal(torch.zeros_like(q.loc), torch.ones_like(q.scale))
    np.testing.assert_allclose(torch.distributions.kl_divergence(q, pr).sum(-1).numpy(),
                               no.kl_loss(mu, lv, 0 * mu, 0 * lv), rtol=1e-10)


def test_missing_latent_quirks():
    """where(z == 0) also rewrites genuine zeros (nolbo.py:1481-1482); masked entries are replaced by
    the prior sample in the corrected latent (nolbo.py:1510)."""
    g = np.load(os.path.join(GOLDEN, 'vae_d16_l64_b3.npz'))
    mask = syn.make_mask(3, 64, 0.5)
    cats = syn.make_category_vectors(40, 64)
    z = g['p5_z']
    np.testing.assert_allclose(z[mask == 0], np.broadcast_to(cats.astype(np.float64).mean(0), z.shape)[mask == 0])
    zc = g['p5_z_corr']
    np.testing.assert_array_equal(zc[mask == 1], z[mask == 1])
    eps2 = syn.make_eps(3, 64, seed=8)
    idx = g['p5_argmin_masked'].astype(int)
    np.testing.assert_allclose(zc[mask == 0], (cats[idx].astype(np.float64) + eps2)[mask == 0])


def test_torch_cpu_f32_bracket_matches_c_oracle():
    """bench.py's secondary CPU leg (torch float32 ops) and the C oracle are two statements of the same forward."""
    from oracle import c_oracle as co
    from oracle import torch_oracle as to
    cfg = syn.make_config(16, 64, True)
    ep, dp = syn.make_encoder_params(cfg['encoder']), syn.make_decoder_params(cfg['decoder'])
    x, eps = syn.make_voxels(3, 16), syn.make_eps(3, 64)
    co.build()
    r = co.vae_eval_forward(cfg, ep, dp, x, x, eps)
    lg, bce, tp, fp, fn = to.eval_forward_f32(cfg, ep, dp, x, eps)
    assert np.abs(lg - r['logits']).max() < 2e-4
    np.testing.assert_allclose(bce, r['bce'], rtol=1e-4)
    np.testing.assert_array_equal([tp, fp, fn], [r['tp'], r['fp'], r['fn']])


def test_c_oracle_under_asan():
    """The C restatement under AddressSanitizer + UBSan (oracle/Makefile `asan`: every exported routine on small odd shapes
    with exactly-sized heap buffers).  GPU ASan does not exist on this pool; the sanitizers run on the CPU build."""
    import subprocess
    here = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'oracle')
    p = subprocess.run(['make', '-C', here, '-B', 'asan'], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    assert p.returncode == 0 and 'asan driver: ok' in p.stdout, p.stdout[-3000:]


@pytest.mark.parametrize('name', ['vae_d32_l64_b2', 'vae_d16_l64_b3'])
def test_c_oracle_two_pass_get_eval_matches_golden(name):
    """c_oracle.vae_get_eval (fp32 C conv stacks + float32 latent algebra; the checker of the trained-weights parity test)
    against the float64 definition-level fixtures of the missing-latent path (nolbo.py:1472-1528)."""
    g = np.load(os.path.join(GOLDEN, name + '.npz'))
    D, L, var, B, C = [int(v) for v in g['meta'][:5]]
    cfg = syn.make_config(D, L, True)
    ep, dp = syn.make_encoder_params(cfg['encoder']), syn.make_decoder_params(cfg['decoder'])
    x, eps, eps2 = syn.make_voxels(B, D), syn.make_eps(B, L), syn.make_eps(B, L, seed=8)
    oh, cats, mask = syn.make_onehot(B, C), syn.make_category_vectors(C, L), syn.make_mask(B, L, 0.5)
    r = co.vae_get_eval(cfg, ep, dp, x, x, oh, cats, eps, 0.5, mask, eps2)
    np.testing.assert_allclose(r['z'], g['p5_z'], rtol=0, atol=5e-6)
    np.testing.assert_allclose(r['z_c'], g['p5_z_corr'], rtol=0, atol=5e-6)
    assert np.array_equal(r['argmin_masked'], g['p5_argmin_masked'].astype(np.int64))
    np.testing.assert_allclose(r['logits'], g['p5_logits'], rtol=0, atol=1e-4)
    np.testing.assert_allclose(r['logits_c'], g['p5_logits_c'], rtol=0, atol=1e-4)
    np.testing.assert_allclose(r['bce'], g['p5_bce'], rtol=2e-6)
    np.testing.assert_allclose(r['bce_c'], g['p5_bce_c'], rtol=2e-6)
    assert abs(r['acc'] - g['p5_scalars'][3]) < 1e-12 and abs(r['acc_c'] - g['p5_scalars'][7]) < 1e-12


def test_max_pool_encoder_c_vs_numpy():
    """final_pool = 'max' (reference autoencoder3D.py:92-93): the fp32 C composition against the float64 definition."""
    cfg = syn.make_config(32, 8, True)                   # last feature map 2^3: the two pools differ
    cfg['encoder']['final_pool'] = 'max'
    cfg['encoder']['filter_num_list'] = [8, 8, 16, 16, 16]
    ep = syn.make_encoder_params(cfg['encoder'])
    x = syn.make_voxels(2, 32, seed=5)
    ref = no.encoder3D_forward(cfg['encoder'], ep, x.astype(np.float64))
    got = co.encoder3D_forward(cfg['encoder'], ep, x)
    np.testing.assert_allclose(got, ref, rtol=0, atol=5e-6)
    cfg['encoder']['final_pool'] = 'average'
    assert np.abs(no.encoder3D_forward(cfg['encoder'], ep, x.astype(np.float64)) - ref).max() > 1e-3     # the two pools differ


def test_fit_step_adam_chain_matches_torch_optim_adam():
    """oracle.torch_oracle.fit_step carries its own Adam in numpy (Keras' rule: lr_t m / (sqrt(v) + eps), lr_t = lr sqrt(1 - b2^t) / (1 - b1^t)),
    and the multi-step GPU tests lean on it at t > 1.  Three chained steps on the 16^3 model; from the returned gradients the updates of
    two tensors are replayed through torch.optim.Adam in float64 with eps set before every step to 1e-7 / sqrt(1 - b2^t), which is
    algebraically the same rule (torch divides by sqrt(v / (1 - b2^t)) + eps).  On random data the two agree to 2.2e-16 over seven steps."""
    import torch
    from oracle import torch_oracle as to
    from voxvae import synthetic as syn
    cfg = syn.make_config(16, 64, True)
    ep = syn.make_encoder_params(cfg['encoder'], seed=42, nontrivial_affine=True)
    dp = syn.make_decoder_params(cfg['decoder'], seed=43, nontrivial_affine=True, final_gain=2.0)
    names = ['enc/conv0/kernel', 'dec/bnT1/gamma']
    start = {'enc/conv0/kernel': ep['conv0/kernel'], 'dec/bnT1/gamma': dp['bnT1/gamma']}
    P = {n: torch.tensor(np.asarray(start[n], np.float64), requires_grad=True) for n in names}
    opt = torch.optim.Adam([P[n] for n in names], lr=1e-3, betas=(0.9, 0.999), eps=1e-7)
    adam = None
    for t in range(1, 4):
        x, eps = syn.make_voxels(2, 16, seed=100 + t), syn.make_eps(2, 64, seed=200 + t)
        ref = to.fit_step(cfg, ep, dp, x, x, eps, adam_state=adam, lr=1e-3, variational=True)
        adam = ref['adam']
        assert adam['t'] == t
        ep = {n[4:]: v for n, v in ref['params'].items() if n.startswith('enc/')}
        dp = {n[4:]: v for n, v in ref['params'].items() if n.startswith('dec/')}
        opt.param_groups[0]['eps'] = 1e-7 / np.sqrt(1.0 - 0.999 ** t)
        for n in names:
            assert np.abs(ref['grads'][n]).max() > 0
            P[n].grad = torch.tensor(ref['grads'][n], dtype=torch.float64)
        opt.step()
        for n in names:
            assert np.abs(P[n].detach().numpy() - ref['params'][n]).max() <= 1e-12, (n, t)
            assert np.abs(ref['params'][n] - start[n]).max() > 1e-4 * t       # the weights did move, by about lr per step


def test_adam_float32_rounding_and_the_units_it_is_measured_in():
    """Reference only (numpy): Keras Adam evaluated in float32 in the kernels' expression order, with and without contracted multiply-adds,
    against the float64 rule on the same float32-rounded constants -- what ANY float32 Adam can reach, and so what the GPU tests may ask.
    State of a second step (m = (1-b1) g1, v = (1-b2) g1^2, a fresh gradient g2 of the same scale, scales over ten decades):
      * m and v stay within 4 of their units (2^-24 (|b1 m| + |(1-b1) g|), 2^-24 v);
      * weights away from 0 (+-10^U(-2, 0), tests/test_gpu_train_ops.py): the parameter stays within 4 units of 2^-24 (|p| + |step|);
      * weights of a real layer (N(0, 0.05), some arbitrarily close to 0): that unit is exceeded several times over (measured 78 / 166),
        because m's rounding error does not shrink when b1 m and (1-b1) g cancel; measured against the step's size before the
        cancellation (adam_units(..., uncancelled=True)) the error is 3.84 units.  The GPU tests' bound of 8 units is twice what this emulation reaches, so everything here is held to 4."""
    from _train_ref import adam_float32_emulation, adam_units, lr_t_of
    rng = np.random.default_rng(0)
    n = 2_000_000
    scale = 10.0 ** rng.uniform(-8, 2, n)
    g1 = scale * rng.standard_normal(n)
    m, v = (0.1 * g1).astype(np.float32), (0.001 * g1 * g1).astype(np.float32)
    g = (scale * rng.standard_normal(n)).astype(np.float32)
    away = (10.0 ** rng.uniform(-2, 0, n) * rng.choice([-1.0, 1.0], n)).astype(np.float32)
    layer = (0.05 * rng.standard_normal(n)).astype(np.float32)
    lr_t = lr_t_of(2)
    for contract in (False, True):
        out = adam_float32_emulation(away, g, m, v, lr_t, contract)
        um, uv, up = adam_units(*out, away, g, m, v, lr_t)
        assert um <= 4 and uv <= 4 and up <= 4, (contract, um, uv, up)
        out = adam_float32_emulation(layer, g, m, v, lr_t, contract)
        plain, fixed = adam_units(*out, layer, g, m, v, lr_t)[2], adam_units(*out, layer, g, m, v, lr_t, uncancelled=True)[2]
        print('\n[adam float32 emulation, contract=%d] parameter error on N(0, 0.05) weights: %.1f plain units, %.2f uncancelled' % (contract, plain, fixed))
        assert plain > 8 and fixed <= 4, (contract, plain, fixed)


@pytest.mark.parametrize('name', ['vae_d32_l64_b2', 'ae_d32_l64_b2', 'vae_d16_l64_b3', 'vae_d64_l16_b1'])
def test_latent_ops_reproduce_golden_details(name):
    """The public latent ops (latent_mask_fill / nearest_category / latent_correct / category_accuracy), applied to the details
    vae_get_eval stored in the fixtures, give the fixtures' z, argmin_masked, z_corr and accuracies bit for bit: vae_get_eval is
    written on top of them, and the committed goldens pin that rewrite."""
    g = np.load(os.path.join(GOLDEN, name + '.npz'))
    D, L, var, B, C = [int(v) for v in g['meta'][:5]]
    oh, cats = syn.make_onehot(B, C), syn.make_category_vectors(C, L).astype(np.float64)
    eps, eps2, mask = syn.make_eps(B, L), syn.make_eps(B, L, seed=8), syn.make_mask(B, L, 0.5).astype(np.float64)
    enc = g['p5_enc_out']
    z0 = no.sampling(*no.split_mean_logvar(enc, L), eps) if var else enc
    z = no.latent_mask_fill(z0, mask, cats)
    np.testing.assert_array_equal(z, g['p5_z'])
    idx = no.nearest_category(z, cats, mask)
    np.testing.assert_array_equal(idx, g['p5_argmin_masked'].astype(np.int64))
    zc = no.latent_correct(z, mask, cats, idx, eps2)
    np.testing.assert_array_equal(zc, g['p5_z_corr'])
    assert no.category_accuracy(no.nearest_category(z, cats), oh) == g['p5_scalars'][3]
    assert no.category_accuracy(no.nearest_category(zc, cats), oh) == g['p5_scalars'][7]
    assert no.category_accuracy(no.nearest_category(g['p0_z'], cats), oh) == g['p0_scalars'][3]


def test_latent_op_quirks():
    """Each quirk of the missing-modality algebra, stated once on numbers small enough to read."""
    P = np.array([[1.0, 2.0, 4.0], [3.0, 2.0, 0.0], [1.0, 2.0, 4.0], [-9.0, 6.0, 4.0]])       # rows 0 and 2 are the same prototype
    mean = P.mean(0)                                                                          # [-1, 3, 3]
    # -0.0 and a genuine zero under a mask of 1 are replaced by the prototype mean, exactly like a masked entry
    z = np.array([[5.0, -0.0, 0.0], [7.0, 8.0, 9.0]])
    mask = np.array([[1.0, 1.0, 1.0], [0.0, 1.0, -0.0]])
    np.testing.assert_array_equal(no.latent_mask_fill(z, mask, P), [[5.0, mean[1], mean[2]], [mean[0], 8.0, mean[2]]])
    # a fully masked row has distance 0 to every class: index 0
    zz = np.array([[1.1, 2.0, 3.9], [3.0, 2.1, 0.2], [50.0, 60.0, 70.0]])
    mm = np.array([[1.0, 1.0, 1.0], [1.0, 1.0, 1.0], [0.0, 0.0, 0.0]])
    assert np.all(no.nearest_category_distances(zz, P, mm)[2] == 0)
    np.testing.assert_array_equal(no.nearest_category(zz, P, mm), [0, 1, 0])        # row 0: prototypes 0 and 2 tie, the first wins
    np.testing.assert_array_equal(no.nearest_category(zz[:, ::-1], P[::-1, ::-1]), [1, 2, 1])   # ... also when the pair sits at 1 and 3
    # a non-finite latent cannot push the index out of [0, C): NaN and +inf distances never compete, a row without any other gets 0
    bad = np.array([[np.inf, 2.0, 4.0], [np.nan, 2.0, 0.0], [3.0, 2.0, 0.1]])
    np.testing.assert_array_equal(no.nearest_category(bad, P), [0, 0, 1])
    np.testing.assert_array_equal(no.nearest_category(bad, P, np.array([[0.0, 1.0, 1.0]] * 3)), [0, 0, 1])    # inf * 0 = NaN
    Pbad = P.copy()
    Pbad[1, 0] = np.inf
    np.testing.assert_array_equal(no.nearest_category(bad, Pbad), [0, 0, 0])        # class 1 is out of the race: the next nearest wins
    # the corrected latent keeps z where mask != 0 (0.5 and 2.0 are not 0) and takes P[idx] + eps2 where it is 0 or -0.0
    e2 = np.full((2, 3), 0.25)
    got = no.latent_correct(z, np.array([[0.5, 0.0, 2.0], [-0.0, 1.0, 1.0]]), P, np.array([3, 1]), e2)
    np.testing.assert_array_equal(got, [[5.0, 6.25, 0.0], [3.25, 8.0, 9.0]])
    # argmax of an all-zero one-hot row is 0, of a row with two maxima the first
    oh = np.array([[0.0, 0.0, 0.0], [0.0, 1.0, 1.0], [0.0, 0.0, 1.0], [1.0, 0.0, 0.0]])
    assert no.category_accuracy([0, 1, 1, 2], oh) == 0.5


def test_binary_loss_f32clip_reference():
    """The loss reference for float32 kernels: float32 clip and float32 1 - q, float64 from there on.  On probabilities away from
    saturation it is binary_loss in float64 to rounding; at saturation it follows the float32 constants; the terms sum to the loss."""
    rng = np.random.default_rng(4)
    p = rng.uniform(0.05, 0.95, (3, 50)).astype(np.float32)
    y = (rng.random((3, 50)) < 0.4).astype(np.float32)
    for gamma, br in ((0.5, False), (0.6, False), (1.0, True)):
        loss, terms = no.binary_loss_f32clip(p, y, gamma=gamma, b_range=br)
        assert terms.shape == (3, 50) and terms.dtype == np.float64
        np.testing.assert_array_equal(loss, -terms.sum(-1))
        np.testing.assert_allclose(loss, no.binary_loss(p.astype(np.float64), y, gamma=gamma, b_range=br), rtol=2e-6)
    edge = np.array([[0.0, 1.0, 1e-8, np.float32(1 - 1e-7), 0.5]], np.float32)
    hi = float(np.float32(1.0) - np.float32(1e-7))
    lo = float(np.float32(1e-7))
    loss, terms = no.binary_loss_f32clip(edge, np.array([[1.0, 1.0, 0.0, 0.0, 1.0]]), gamma=1.0)
    np.testing.assert_array_equal(terms[0], [np.log(lo), np.log(hi), 0.0, 0.0, np.log(0.5)])
    loss, terms = no.binary_loss_f32clip(edge, np.array([[0.0, 0.0, 0.0, 0.0, 0.0]]), gamma=0.0)
    one_minus_hi = float(np.float32(1.0) - np.float32(hi))                           # 1.1920929e-07, not 1e-7
    np.testing.assert_array_equal(terms[0], [np.log(float(np.float32(1.0) - np.float32(lo))), np.log(one_minus_hi), np.log(float(np.float32(1.0) - np.float32(1e-7))),
                                             np.log(one_minus_hi), np.log(0.5)])
