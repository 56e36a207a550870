"""GPU tests of the sampled-mean reconstruction (the reference's nolbo_test.py:167-180: K latents per object from the posterior, every one
decoded, the occupancy probabilities averaged), from the kernel (final_mean.hip) through DecoderEngine.forward_mean up to
getSampledShape / getSampledEval and the entry script.  Expected values come from the oracle; the tolerances are derived, not tuned:

  mean_probs   atol 1.5e-5: the single-sample last layer is held to 1e-5 per probability (test_gpu_ops.py), a mean of K terms inherits
               that, and a float32 sum of K <= 64 terms in [0, 1] adds at most 64 * 2^-24 ~ 4e-6
  counts       exact outside the band |mean_ref - 0.5| < 2e-5 (capped at 2e-3 of the voxels so that it cannot hide a failure)
"""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from oracle import numpy_oracle as no

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, 'anytime-3d-reconstruction_amd')
ATOL_MEAN = 1.5e-5


@pytest.fixture(scope='module')
def L():
    from voxvae import lib
    lib.load()
    assert torch.cuda.is_available()
    return lib


def _st():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _dev(a, dt=torch.float32):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(DEV).to(dt).contiguous()


def _bf16_round(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(torch.bfloat16).to(torch.float32).numpy()


def _final_mean(L, xd, wd, yd, B, K, side, dt):
    """-> (mean_probs [B,D,D,D,1] float32 numpy, stats [B,4] float64 numpy or None)"""
    D = 2 * side
    ws = torch.empty(max(L.load().vv_convT3d_final_mean_workspace_bytes(B, K, side), 16), dtype=torch.uint8, device=DEV)
    mean = torch.full((B, D, D, D, 1), -1.0, dtype=torch.float32, device=DEV)
    stats = torch.full((B, 4), -1.0, dtype=torch.float32, device=DEV) if yd is not None else None
    L.call('vv_convT3d_final_mean_fwd', L.ptr(xd), L.ptr(wd), L.ptr(yd), L.ptr(mean), L.ptr(stats), B, K, side, 64, 0.6, 1e-7, dt,
           L.ptr(ws), ws.numel(), _st())
    torch.cuda.synchronize()
    return mean.cpu().numpy(), (stats.cpu().numpy().astype(np.float64) if stats is not None else None)


def _op_inputs(dtname, B, K, side):
    rng = np.random.default_rng(1000 * side + K)
    x = rng.standard_normal((B * K, side, side, side, 64)).astype(np.float32)
    w = (rng.standard_normal((4, 4, 4, 1, 64)) * 0.3).astype(np.float32)
    if dtname == 'bf16':
        x, w = _bf16_round(x), _bf16_round(w)   # the bf16 path feeds MFMA: both operands are bf16
    D = 2 * side
    y = (rng.random((B, D, D, D, 1)) < 0.3).astype(np.float32)
    return x, w, y


def _check_against_oracle(L, dtname, B, K, side):
    """One call of vv_convT3d_final_mean_fwd on the seeded inputs of (B, K, side) against the float64 oracle: mean, counts, loss.
    -> what the bit-identity checks need: (device inputs, mean, stats)"""
    dt, tdt = L.DTYPES[dtname], (torch.float32 if dtname == 'f32' else torch.bfloat16)
    x, w, y = _op_inputs(dtname, B, K, side)
    D = 2 * side
    w64 = w.astype(np.float64)           # object by object: the float64 oracle's intermediates stay small at the larger shapes
    pbar = np.stack([no.sigmoid(no.conv3d_transpose_same(x[b * K:(b + 1) * K].astype(np.float64), w64, 2)).mean(axis=0) for b in range(B)])
    xd, wd, yd = _dev(x, tdt), _dev(w), _dev(y)
    got, s = _final_mean(L, xd, wd, yd, B, K, side, dt)
    err = np.abs(got.astype(np.float64) - pbar).max()
    print('\n[final_mean %s B %d K %d side %d] max |d mean| %.2e' % (dtname, B, K, side, err))
    assert err <= ATOL_MEAN, err
    # counts: exact outside a band around the threshold, and the band is small
    band = np.abs(pbar - 0.5) < 2e-5
    print('[final_mean] band share %.2e' % band.mean())
    assert band.mean() <= 2e-3
    assert np.array_equal((got >= 0.5)[~band], (pbar >= 0.5)[~band])           # the AVERAGED prediction is what is thresholded
    tp, fp, fn = no.voxel_precision_recall(y, pbar)
    slack = band.reshape(B, -1).sum(-1)
    for k, r in ((1, tp), (2, fp), (3, fn)):
        assert np.all(np.abs(s[:, k] - r) <= slack), (k, s[:, k], r, slack)
    # the loss formula on the kernel's own float32 mean (the clip makes log(1 - p) ill-conditioned near p -> 1), then the oracle's loss
    q = np.clip(got, np.float32(1e-7), np.float32(1.0) - np.float32(1e-7))
    om = (np.float32(1.0) - q).astype(np.float64)
    bce_self = -(0.6 * y * np.log(q.astype(np.float64)) + 0.4 * (1 - y) * np.log(om)).reshape(B, -1).sum(-1)
    np.testing.assert_allclose(s[:, 0], bce_self, rtol=2e-5)
    np.testing.assert_allclose(s[:, 0], no.binary_loss(pbar.astype(np.float32), y, gamma=0.6), rtol=2e-3)
    return (xd, wd, yd), got, s


@pytest.mark.parametrize('dtname', ['f32', 'bf16'])
@pytest.mark.parametrize('B,K,side', [(3, 8, 8), (2, 4, 16), (1, 32, 8), (5, 3, 4)])
def test_convT3d_final_mean(L, dtname, B, K, side, monkeypatch):
    dt = L.DTYPES[dtname]
    (xd, wd, yd), got, s = _check_against_oracle(L, dtname, B, K, side)
    # no target: the same mean bit for bit; a second run: bit-identical mean and stats; cut into launches of one object: the same again
    got_nt, s_nt = _final_mean(L, xd, wd, None, B, K, side, dt)
    assert s_nt is None and np.array_equal(got_nt, got)
    got2, s2 = _final_mean(L, xd, wd, yd, B, K, side, dt)
    assert np.array_equal(got2, got) and np.array_equal(s2, s)
    monkeypatch.setenv('VV_CHUNK_SAMPLES', '1')
    got3, s3 = _final_mean(L, xd, wd, yd, B, K, side, dt)
    assert np.array_equal(got3, got) and np.array_equal(s3, s)


@pytest.mark.parametrize('B,K,side,planes', [(64, 3, 16, 8), (16, 3, 32, 16)])
def test_convT3d_final_mean_sweep_at_full_depth_ranges(L, B, K, side, planes):
    """The bf16 sweep form halves its depth range (16 input planes, the 32 KB of LDS sums) down to 4 while the grid is short of two
    workgroups per CU, which every small shape above is.  These two calls are large enough to keep `planes` = 8 and 16 planes per
    workgroup (objects x K-slices x tiles x ranges >= 512 at that range, < 512 at twice it) -- 16 at side 32 is the one-plane-halo
    split with 70 KB of LDS, the form of large 64^3 calls -- and are held to the same oracle bounds.
    K is odd on purpose: these logits (sigma ~ 7) mostly saturate the sigmoid, and with K = 2 one sample at 1 and one at 0 average to 0.5
    to within the band in 1.1-1.3 % of the voxels (measured on the first version of this test, kernel error 4e-7): the band cap, which
    exists so that the band cannot hide a failure, then refuses the INPUTS.  With K = 3 saturated samples average to 0, 1/3, 2/3 or 1."""
    ntile = (side // 8) ** 2
    assert B * ntile * (side // planes) >= 512 and (planes == 16 or B * ntile * (side // (2 * planes)) < 512)     # K = 3: one K slice
    _check_against_oracle(L, 'bf16', B, K, side)


@pytest.mark.parametrize('dtname', ['f32', 'bf16'])
def test_an_object_does_not_depend_on_its_batch(L, dtname):
    """The summation order is a function of (K, side) only: object 1 of a batch of 3 alone gives the same bits."""
    B, K, side = 3, 8, 8
    dt, tdt = L.DTYPES[dtname], (torch.float32 if dtname == 'f32' else torch.bfloat16)
    x, w, y = _op_inputs(dtname, B, K, side)
    got, s = _final_mean(L, _dev(x, tdt), _dev(w), _dev(y), B, K, side, dt)
    one, s1 = _final_mean(L, _dev(x[K:2 * K], tdt), _dev(w), _dev(y[1:2]), 1, K, side, dt)
    assert np.array_equal(one[0], got[1]) and np.array_equal(s1[0], s[1])


@pytest.mark.parametrize('dtname', ['f32', 'bf16'])
@pytest.mark.parametrize('B,side', [(3, 8), (2, 16), (4, 4)])
def test_one_sample_is_the_single_sample_layer(L, dtname, B, side):
    dt, tdt = L.DTYPES[dtname], (torch.float32 if dtname == 'f32' else torch.bfloat16)
    x, w, y = _op_inputs(dtname, B, 1, side)
    D = 2 * side
    xd, wd, yd = _dev(x, tdt), _dev(w), _dev(y)
    got, s = _final_mean(L, xd, wd, yd, B, 1, side, dt)
    ws = torch.empty(max(L.load().vv_convT3d_final_bce_workspace_bytes(B, side), 16), dtype=torch.uint8, device=DEV)
    probs = torch.empty(B, D, D, D, 1, dtype=torch.float32, device=DEV)
    stats = torch.empty(B, 4, dtype=torch.float32, device=DEV)
    L.call('vv_convT3d_final_bce_fwd', L.ptr(xd), L.ptr(wd), L.ptr(yd), L.ptr(probs), None, L.ptr(stats), B, side, 64, 0.6, 1e-7, dt,
           L.ptr(ws), ws.numel(), _st())
    torch.cuda.synchronize()
    p1, s1 = probs.cpu().numpy(), stats.cpu().numpy().astype(np.float64)
    np.testing.assert_allclose(got, p1, rtol=0, atol=1e-5)
    band = np.abs(p1.astype(np.float64) - 0.5) < 2e-5
    assert np.array_equal((got >= 0.5)[~band], (p1 >= 0.5)[~band])
    slack = band.reshape(B, -1).sum(-1)
    for k in (1, 2, 3):
        assert np.all(np.abs(s[:, k] - s1[:, k]) <= slack)


@pytest.mark.parametrize('B,side', [(3, 8), (2, 16)])
def test_one_sample_sweep_is_the_single_sample_sweep_bit_for_bit(L, B, side, monkeypatch):
    """bf16, K = 1, both layers in their Q-form sweep (final_mean takes it for every bf16 call at side >= 8; the single-sample layer
    is forced to it, small batches go to its box form otherwise): staging, operands, MFMAs, publish, gather and sigmoid are one text
    in final_common.h, so the mean of one sample IS the single-sample probability, bit for bit."""
    monkeypatch.setenv('VV_FINAL_BCE', 'sweep')
    x, w, y = _op_inputs('bf16', B, 1, side)
    D = 2 * side
    xd, wd, yd = _dev(x, torch.bfloat16), _dev(w), _dev(y)
    got, _ = _final_mean(L, xd, wd, yd, B, 1, side, L.VV_BF16)
    ws = torch.empty(max(L.load().vv_convT3d_final_bce_workspace_bytes(B, side), 16), dtype=torch.uint8, device=DEV)
    probs = torch.full((B, D, D, D, 1), -1.0, dtype=torch.float32, device=DEV)
    stats = torch.empty(B, 4, dtype=torch.float32, device=DEV)
    L.call('vv_convT3d_final_bce_fwd', L.ptr(xd), L.ptr(wd), L.ptr(yd), L.ptr(probs), None, L.ptr(stats), B, side, 64, 0.6, 1e-7, L.VV_BF16,
           L.ptr(ws), ws.numel(), _st())
    torch.cuda.synchronize()
    assert np.array_equal(got, probs.cpu().numpy())


@pytest.mark.parametrize('B,K,Lz', [(3, 5, 64), (1, 32, 16), (7, 1, 64)])
def test_sample_latents(L, B, K, Lz):
    rng = np.random.default_rng(B * 100 + K)
    mean = rng.standard_normal((B, Lz)).astype(np.float32)
    logvar = rng.uniform(-10, 3, (B, Lz)).astype(np.float32)
    eps = rng.standard_normal((B, K, Lz)).astype(np.float32)
    ref = no.sampling(np.broadcast_to(mean[:, None, :], eps.shape).astype(np.float64), np.broadcast_to(logvar[:, None, :], eps.shape).astype(np.float64),
                      eps.astype(np.float64)).reshape(B * K, Lz)
    from voxvae import engine as E
    z, z_act = E.sample_latents(_dev(mean), _dev(logvar), _dev(eps), L.VV_BF16)
    torch.cuda.synchronize()
    assert z.shape == (B * K, Lz) and z_act.dtype == torch.bfloat16
    np.testing.assert_allclose(z.cpu().numpy(), ref, rtol=2e-5, atol=2e-5)
    assert torch.equal(z_act, z.to(torch.bfloat16))                            # the same values, rounded once
    zf, zf_act = E.sample_latents(_dev(mean), _dev(logvar), _dev(eps), L.VV_F32)
    assert zf_act is zf and torch.equal(zf, z)
    only_act = torch.empty(B * K, Lz, dtype=torch.bfloat16, device=DEV)
    md, ld, ed = _dev(mean), _dev(logvar), _dev(eps)
    L.call('vv_sample_latents', L.ptr(md), L.ptr(ld), L.ptr(ed), None, L.ptr(only_act), L.VV_BF16, B, K, Lz, _st())
    torch.cuda.synchronize()
    assert torch.equal(only_act, z_act)


# ---------------------------------------------------------------------------------------------- engine level, trained 32^3 operating point
@pytest.fixture(scope='module')
def trained():
    from voxvae import synthetic as syn
    from voxvae import trained as tr
    cfg, ep, dp, info = tr.train_operating_point(device=DEV)
    assert info['reached'], info
    x = np.concatenate([syn.make_voxels(256, 32, seed=4321)[:48], syn.make_voxels(16, 32, seed=777)], axis=0)
    return dict(cfg=cfg, ep=ep, dp=dp, x=x)


def _model(t, dtype, cls='VAE'):
    import voxvae
    voxvae.set_default_dtype(dtype)
    voxvae.set_default_device(DEV)
    import src.module.nolbo as nolbo
    m = getattr(nolbo, 'nolboSingleObject_modelnet_category_' + cls)(nolbo_structure=t['cfg'])
    m._encoder.set_weights_dict(t['ep'])
    m._decoder.set_weights_dict(t['dp'])
    return m


def _latents(m, t, B, K, seed=5):
    """(mean, logvar, eps, z float32, z_act): K posterior samples of the first B evaluation shapes"""
    from voxvae import engine as E
    from voxvae import synthetic as syn
    x = torch.from_numpy(t['x'][:B]).to(DEV)
    mean, logvar = m._posterior(x)
    eps = torch.from_numpy(syn.make_eps(B * K, mean.shape[1], seed=seed).reshape(B, K, -1)).to(DEV)
    z, z_act = E.sample_latents(mean, logvar, eps, m._act_dt)
    return x, mean, logvar, eps, z, z_act


def _unfused_mean(m, z_act, B, K):
    probs, _, _ = m._dec_eng.forward(z_act)
    torch.cuda.synchronize()
    return probs.double().cpu().numpy().reshape((B, K) + tuple(probs.shape[1:])).mean(axis=1)


def _form_gap(m, z_act, monkeypatch):
    """Largest logit difference between the two EXISTING bf16 forms of the single-sample last layer (sweep / box) on the hidden
    activations of these latents: what a different float32 summation order costs on this data."""
    from voxvae import lib as L
    dec = m._dec_eng
    h, hdt, side, n = dec._hidden(z_act, None, False)
    D = 2 * side
    y = torch.zeros(n, D, D, D, 1, dtype=torch.float32, device=DEV)
    out = []
    for form in ('sweep', 'box'):
        monkeypatch.setenv('VV_FINAL_BCE', form)
        ws = torch.empty(max(L.load().vv_convT3d_final_bce_workspace_bytes(n, side), 16), dtype=torch.uint8, device=DEV)
        logits = torch.empty(n, D, D, D, 1, dtype=torch.float32, device=DEV)
        stats = torch.empty(n, 4, dtype=torch.float32, device=DEV)
        L.call('vv_convT3d_final_bce_fwd', L.ptr(h), L.ptr(dec.params['convT%d/kernel' % (len(dec.filters) - 1)]), L.ptr(y), None, L.ptr(logits),
               L.ptr(stats), n, side, dec.filters[-2], 0.6, 1e-7, hdt, L.ptr(ws), ws.numel(), _st())
        torch.cuda.synchronize()
        out.append(logits.double().cpu().numpy())
    monkeypatch.delenv('VV_FINAL_BCE')
    return float(np.abs(out[0] - out[1]).max())


def test_forward_mean_f32_against_the_unfused_composition_and_the_c_oracle(trained):
    from oracle import c_oracle as co
    t, B, K = trained, 4, 8
    m = _model(t, 'f32')
    x, mean, logvar, eps, z, z_act = _latents(m, t, B, K)
    got, stats, metrics = m._dec_eng.forward_mean(z_act, K, x)
    torch.cuda.synchronize()
    got = got.cpu().numpy()
    ref_own = _unfused_mean(m, z_act, B, K)
    d_own = np.abs(got - ref_own).max()
    lg = co.decoder3D_logits(t['cfg']['decoder'], t['dp'], z.cpu().numpy())
    pbar = no.sigmoid(lg.astype(np.float64)).reshape((B, K) + got.shape[1:]).mean(axis=1)
    d_or = np.abs(got - pbar).max()
    print('\n[forward_mean f32] max |d mean| vs unfused %.2e, vs C oracle %.2e' % (d_own, d_or))
    assert d_own <= ATOL_MEAN
    assert d_or <= 2.5e-4                                                      # the logit bar 1e-3 times the sigmoid's slope bound 1/4
    safe = np.abs(pbar - 0.5) >= 1e-4
    assert np.array_equal((got >= 0.5)[safe], (pbar >= 0.5)[safe])
    # stats and metrics describe the averaged prediction
    s = stats.double().cpu().numpy()
    tp, fp, fn = no.voxel_precision_recall(t['x'][:B], pbar)
    slack = (~safe).reshape(B, -1).sum(-1)
    for k, r in ((1, tp), (2, fp), (3, fn)):
        assert np.all(np.abs(s[:, k] - r) <= slack)
    mm = metrics.cpu().numpy()
    prr, rcc = no.pr_rc(s[:, 1], s[:, 2], s[:, 3])
    np.testing.assert_allclose(mm[:3], [s[:, 0].mean(), prr, rcc], rtol=1e-5)


def test_forward_mean_bf16_against_the_unfused_composition(trained, monkeypatch):
    """Both sides read the same bf16 hidden activations and differ in float32 summation order only.  The allowance is a quarter (the
    sigmoid's slope bound) of the largest logit difference the two EXISTING forms of the last layer show between each other on these
    activations, plus 4e-6 for the float32 sum over K.  Measured on MI355X: see the printed line; 3.8e-6 between the forms -> allowance 5.0e-6, 8.9e-8 observed
    (DESIGN.md section 4d)."""
    t, B, K = trained, 4, 8
    m = _model(t, 'bf16')
    x, mean, logvar, eps, z, z_act = _latents(m, t, B, K)
    gap = _form_gap(m, z_act, monkeypatch)
    got, stats, _ = m._dec_eng.forward_mean(z_act, K, x)
    torch.cuda.synchronize()
    d = np.abs(got.cpu().numpy() - _unfused_mean(m, z_act, B, K)).max()
    print('\n[forward_mean bf16] existing sweep vs box forms: max |d logit| %.3e -> allowance %.3e; fused vs unfused max |d mean| %.3e'
          % (gap, 0.25 * gap + 4e-6, d))
    assert d <= 0.25 * gap + 4e-6


def test_forward_mean_needs_sigmoid_and_whole_objects(trained):
    import copy
    from voxvae import engine as E
    t = trained
    m = _model(t, 'f32')
    z = torch.zeros(6, 64, dtype=torch.float32, device=DEV)
    with pytest.raises(ValueError):
        m._dec_eng.forward_mean(z, 4)
    st = copy.deepcopy(t['cfg']['decoder'])
    st['final_activation'] = 'None'
    dec = E.DecoderEngine(st, 'f32', DEV)
    with pytest.raises(NotImplementedError):
        dec.forward_mean(z, 3)


# ---------------------------------------------------------------------------------------------- API level
def test_getSampledEval_is_getSampledShape_on_the_posterior(trained):
    from voxvae import synthetic as syn
    t, B, K = trained, 6, 8
    m = _model(t, 'bf16')
    x = t['x'][:B]
    eps = syn.make_eps(B * K, 64, seed=11).reshape(B, K, 64)
    a = m.getSampledEval((x, x), K, _eps=eps)
    mean, logvar = m._posterior(torch.from_numpy(x).to(DEV))
    b = m.getSampledShape(mean, logvar, K, target=x, _eps=eps)
    assert len(a) == 4 and len(b) == 4
    assert np.array_equal(np.array(a[0]), np.array(b[0]))
    assert [float(v) for v in a[1:]] == [float(v) for v in b[1:]]
    # no target: the prediction alone, the same bits
    p = m.getSampledShape(mean.cpu().numpy(), logvar.cpu().numpy(), K, _eps=eps)
    assert np.array_equal(np.array(p), np.array(a[0]))
    assert np.array(p).shape == (B, 32, 32, 32, 1)
    # chunking must not change results
    for mdb in (8, 64, 256):
        c = m.getSampledShape(mean, logvar, K, target=x, _eps=eps, max_decode_batch=mdb)
        assert np.array_equal(np.array(c[0]), np.array(a[0])), mdb
        assert [float(v) for v in c[1:]] == [float(v) for v in a[1:]], mdb
    # a drawn eps: another prediction, still a probability grid
    r = np.array(m.getSampledEval((x, x), K)[0])
    assert r.min() >= 0 and r.max() <= 1 and not np.array_equal(r, np.array(a[0]))


@pytest.mark.parametrize('dtype', ['f32', 'bf16'])
def test_one_zero_sample_reproduces_getEval(trained, dtype, monkeypatch):
    t, B = trained, 6
    m = _model(t, dtype)
    x = t['x'][:B]
    pred = np.array(m.getEval(inputs=(x, x), _eps=np.zeros((B, 64), np.float32))[0])
    got = np.array(m.getSampledEval((x, x), 1, _eps=np.zeros((B, 1, 64), np.float32))[0])
    d = np.abs(got - pred).max()
    if dtype == 'f32':
        tol = ATOL_MEAN
    else:
        mean, logvar = m._posterior(torch.from_numpy(x).to(DEV))
        tol = 0.25 * _form_gap(m, mean.to(torch.bfloat16).contiguous(), monkeypatch) + 4e-6
    print('\n[K = 1, eps = 0, %s] max |d pred| vs getEval %.3e (allowed %.3e)' % (dtype, d, tol))
    assert d <= tol


def test_autoencoder_has_no_posterior(trained):
    import voxvae
    from voxvae import synthetic as syn
    import src.module.nolbo as nolbo
    voxvae.set_default_dtype('bf16')
    voxvae.set_default_device(DEV)
    cfg = syn.make_config(32, 64, False)
    m = nolbo.nolboSingleObject_modelnet_category_AE(nolbo_structure=cfg)
    m._encoder.set_weights_dict(syn.make_encoder_params(cfg['encoder']))
    m._decoder.set_weights_dict(syn.make_decoder_params(cfg['decoder']))
    x = trained['x'][:2]
    with pytest.raises(ValueError):
        m.getSampledEval((x, x), 4)
    # the latent-level form serves every class that owns a decoder
    z = np.array(m.getLatent(x))
    p = np.array(m.getSampledShape(z, np.full_like(z, -6.0), 4))
    assert p.shape == (2, 32, 32, 32, 1) and p.min() >= 0 and p.max() <= 1


def test_fp8_engine_runs_and_stays_with_its_single_sample_path(trained):
    """An fp8-policy engine: its fp8 layers run, the last hidden layer is stored as bf16 for the sampled-mean kernel.  With eps = 0 every one
    of the K samples is the posterior mean, so the averaged prediction is the engine's own single-sample prediction up to the element
    type of the last hidden layer: mean IoU within 1e-3."""
    t, B, K = trained, 64, 4
    m = _model(t, 'fp8')
    x = t['x'][:B]
    single = np.array(m.getEval(inputs=(x, x), _eps=np.zeros((B, 64), np.float32))[0])
    got = np.array(m.getSampledEval((x, x), K, _eps=np.zeros((B, K, 64), np.float32))[0])
    yt = x.reshape(B, -1) > 0.5

    def iou(p):
        yh = p.reshape(B, -1) >= 0.5
        return ((yh & yt).sum(1) / np.maximum((yh | yt).sum(1), 1)).mean()
    print('\n[fp8 engine] IoU single-sample %.4f, sampled mean (K = %d, eps = 0) %.4f' % (iou(single), K, iou(got)))
    assert iou(single) > 0.4
    assert abs(iou(got) - iou(single)) <= 1e-3


def test_64_cubed_model(monkeypatch):
    """The reference's native grid at B = 2, K = 4: the last layer runs at side 32, where the sweep form splits the depth; against the
    unfused composition with the allowance of the bf16 engine-level test."""
    import voxvae
    from voxvae import synthetic as syn
    import src.module.nolbo as nolbo
    voxvae.set_default_dtype('bf16')
    voxvae.set_default_device(DEV)
    cfg = syn.make_config(64, 64, True)
    m = nolbo.nolboSingleObject_modelnet_category_VAE(nolbo_structure=cfg)
    m._encoder.set_weights_dict(syn.make_encoder_params(cfg['encoder']))
    m._decoder.set_weights_dict(syn.make_decoder_params(cfg['decoder']))
    B, K = 2, 4
    x = syn.make_voxels(B, 64, seed=3)
    eps = syn.make_eps(B * K, 64, seed=4).reshape(B, K, 64)
    pred, loss, pr, rc = m.getSampledEval((x, x), K, _eps=eps)
    p = np.array(pred)
    assert p.shape == (B, 64, 64, 64, 1) and np.isfinite(p).all() and p.min() >= 0 and p.max() <= 1
    assert np.isfinite([float(loss), float(pr), float(rc)]).all()
    from voxvae import engine as E
    mean, logvar = m._posterior(torch.from_numpy(x).to(DEV))
    _, z_act = E.sample_latents(mean, logvar, torch.from_numpy(eps).to(DEV), m._act_dt)
    gap = _form_gap(m, z_act, monkeypatch)
    d = np.abs(p - _unfused_mean(m, z_act, B, K)).max()
    print('\n[64^3 B 2 K 4] sweep vs box max |d logit| %.3e; fused vs unfused max |d mean| %.3e' % (gap, d))
    assert d <= 0.25 * gap + 4e-6


def test_entry_script_prints_the_sampled_mean_numbers():
    env = dict(os.environ)
    env.pop('VV_FINAL_BCE', None)
    p = subprocess.run([sys.executable, 'test_modelnet_VAE.py', '--voxel', '32', '--batch', '8', '--sampling', '4', '--max-iter', '2'],
                       cwd=PKG, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-2000:]
    assert 'sloss:' in p.stdout and 'spr:' in p.stdout and 'src:' in p.stdout, p.stdout[-1000:]
