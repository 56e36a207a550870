"""GPU tests of the multi-modal model classes at side 16, latent 4 + 4, batch 8, a tiny torch module as image encoder:
nolboSingleObject.getEval against the numpy statement composed with the decoder engine called directly (both missing_prob forms, both
activation dtypes, training=True); the sampled-shape methods on the concatenated latent; one fit step with latent='hip' against
latent='torch' from identical weights and draws; nolboSingleObject_AE; and the three entry scripts on synthetic data."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import _mm_ref as R
import _tol
import test_mm_latent_host as H

pytestmark = pytest.mark.gpu
DEV = 'cuda'
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, 'anytime-3d-reconstruction_amd')
B, LC, LI, C, I, D = 8, 4, 4, 12, 10, 16


@pytest.fixture
def dtype():
    """Sets the package's default activation dtype for one test and puts the previous one back."""
    import voxvae
    saved = voxvae.default_dtype()
    yield voxvae.set_default_dtype
    voxvae.set_default_dtype(saved)


class Encoder(torch.nn.Module):
    """images [B, 8, 8, 3] -> head outputs [B, width]: one trainable matrix."""

    def __init__(self, width, seed=5):
        super().__init__()
        w = np.random.default_rng(seed).normal(0, 0.3, (8 * 8 * 3, width)).astype(np.float32)
        self.w = torch.nn.Parameter(torch.from_numpy(w).to(DEV))
        self.eval()

    def forward(self, x):
        with torch.set_grad_enabled(self.training):                # a graph only in train(): what fit back-propagates through
            x = x if torch.is_tensor(x) else torch.from_numpy(np.asarray(x, np.float32))
            return x.to(DEV, torch.float32).reshape(len(x), -1) @ self.w


def _config():
    from voxvae import synthetic as syn
    prior = lambda name, n: {'name': name, 'input_dim': n, 'unit_num_list': [16, 8, 4], 'core_activation': 'elu', 'const_log_var': 0.0}
    return {'encoder_backbone': {'name': 'bb', 'z_category_dim': LC, 'z_inst_dim': LI}, 'encoder_head': None,
            'decoder': syn.make_config(D, LC + LI, True)['decoder'], 'prior_class': prior('priornet_class', C), 'prior_inst': prior('priornet_inst', C + I)}


def _model(**kw):
    """A nolboSingleObject with seeded weights: two calls give identical models."""
    from voxvae import synthetic as syn
    import src.module.nolbo as nolbo
    cfg = _config()
    torch.manual_seed(0)
    m = nolbo.nolboSingleObject(nolbo_structure=cfg, encoder_backbone=Encoder(2 * LC + 2 * LI), **kw)
    m._decoder.set_weights_dict(syn.make_decoder_params(cfg['decoder']))
    return m


def _data():
    from voxvae import synthetic as syn
    rng = np.random.default_rng(5)
    f = lambda *s: rng.normal(0, 1, s).astype(np.float32)
    cat, inst = rng.integers(0, C, B), rng.integers(0, I, B)
    return dict(img=f(B, 8, 8, 3), vox=syn.make_voxels(B, D, seed=2), cat_oh=np.eye(C, dtype=np.float32)[cat], inst_oh=np.eye(I, dtype=np.float32)[inst],
                eps=f(B, LC + LI), eps2=f(B, LC), eps_p=f(B, LC + LI), mask=(rng.random((B, LC)) >= 0.5).astype(np.float32),
                noise=(rng.random((B, LC + LI)) >= 0.5).astype(np.float32))


@pytest.mark.parametrize('act,training', [('f32', False), ('bf16', False), ('f32', True)])
@pytest.mark.parametrize('missing_prob', [0.0, 0.5])
def test_getEval_against_the_numpy_statement_and_the_decoder_engine(missing_prob, act, training, dtype):
    """The latents, indices and accuracies are the numpy statement's; the predictions are the decoder's on the model's own latents: the
    engine's forward (bf16: on the round-to-nearest-even twin), with training=True the trainer's batch-statistics forward."""
    from voxvae import train as T
    dtype(act)
    m, d = _model(), _data()
    mask, eps2 = (d['mask'], d['eps2']) if missing_prob > 0 else (None, None)
    torch.manual_seed(3)                                           # training=True: the prior networks' dropout draws
    out = m.getEval((d['img'], d['vox'], d['cat_oh'], d['inst_oh']), category_indices=np.identity(C), inst_indices=np.identity(I), training=training,
                    missing_prob=missing_prob, _eps=d['eps'], _mask=mask, _eps2=eps2)
    assert len(out) == (11 if missing_prob > 0 else 6) and np.array(out[0]).shape == (B, D, D, D, 1)
    torch.manual_seed(3)
    prior_cat, prior_inst = m._prior_means(d['cat_oh'], np.identity(C), np.identity(I), training)
    enc = m._encoder_backbone(d['img']).detach().cpu().numpy()
    r = R.eval_ref(enc, d['eps'], mask, eps2, prior_cat.cpu().numpy(), prior_inst.cpu().numpy(), d['cat_oh'], d['inst_oh'])
    np.testing.assert_array_equal(np.array(m._nearest), r['idx'])
    assert float(out[4]) == r['acc'][0] and float(out[5]) == r['acc'][1]
    assert H._rel(np.array(m._z), r['z']) <= H.Z_GATE
    y = m._dev(d['vox'])

    def decoded(z):
        z = torch.from_numpy(np.array(z)).to(m._device)
        if training:
            return T.Trainer.forward_only(dec=m._dec_eng).decoder_training_mode(z, y)[::2]
        pred, _, _, met = m._dec_eng.forward(z if act == 'f32' else z.to(torch.bfloat16), y, want_metrics=True)
        return pred, met

    for z, first in ((m._z, 0),) + (((m._z_corrected, 6),) if missing_prob > 0 else ()):
        pred, met = decoded(z)
        assert np.array_equal(np.array(out[first]), pred.float().cpu().numpy().reshape(B, D, D, D, 1))
        assert [float(out[first + k]) for k in (1, 2, 3)] == [float(met[k]) for k in (0, 1, 2)]
    if missing_prob > 0:
        assert float(out[10]) == r['acc'][2] and H._rel(np.array(m._z_corrected), r['z_corr']) <= H.Z_GATE


def test_sampled_methods_on_the_concatenated_latent(dtype):
    """getSampledShape / getSampledPoints / getSampledObjects take the concatenated (mean, logVar) [B, Lc+Li]: the same bits as the
    image -> 3D VAE class of latent Lc+Li with the same decoder gives."""
    import test_gpu_pose as P
    from voxvae import synthetic as syn
    import src.module.nolbo as nolbo
    dtype('f32')
    m, d = _model(), _data()
    cfg = _config()
    v = nolbo.nolboSingleObject_VAE(nolbo_structure={'encoder_backbone': {'name': 'bb', 'z_dim': LC + LI}, 'decoder': cfg['decoder']})
    v._decoder.set_weights_dict(syn.make_decoder_params(cfg['decoder']))
    enc = m._encoder_backbone(d['img']).detach()[:3]
    mean = torch.cat([enc[:, :LC], enc[:, 2 * LC:2 * LC + LI]], dim=1).contiguous()
    logvar = torch.cat([enc[:, LC:2 * LC], enc[:, 2 * LC + LI:]], dim=1).clamp(-10, 10).contiguous()
    K = 4
    eps = syn.make_eps(3 * K, LC + LI, seed=11).reshape(3, K, LC + LI)
    grid = m.getSampledShape(mean, logvar, K, _eps=eps)
    assert np.array(grid).shape == (3, D, D, D, 1) and np.array(grid).tobytes() == np.array(v.getSampledShape(mean, logvar, K, _eps=eps)).tobytes()
    prob = float(np.median(np.array(grid)))
    dims = np.ones((3, 3), dtype=np.float32)
    a, b = (x.getSampledPoints(mean, logvar, dims, sampling_num=K, prob=prob, _eps=eps) for x in (m, v))
    assert a.total() == b.total() > 0 and a.points.cpu().numpy().tobytes() == b.points.cpu().numpy().tobytes()
    g = P.golden()
    rows = np.array([g['kept'][5], g['kept'][6], g['kept'][5]])
    det = (g['bbox2d'][rows], g['bbox3d'][rows], g['sin'][rows], g['cos'][rows], tuple(g['image_size']))
    (pa, ca), (pb, cb) = (x.getSampledObjects(mean, logvar, *det, sampling_num=K, prob=prob, _eps=eps) for x in (m, v))
    assert pa.count() == pb.count() == 3 and ca.total() == cb.total() > 0
    assert ca.points.cpu().numpy().tobytes() == cb.points.cpu().numpy().tobytes()


def _e32(cap, d, noise):
    """Per gradient tensor: what float32 torch autograd of the restated closure (tests/_mm_ref.total_torch) loses against float64 on
    the step's own inputs, and the tensor's scale -- the two arguments of the backward gate of tests/test_mm_latent_host.py."""
    c = dict(enc=cap['enc_out'], eps=d['eps'], mean_cp=cap['pri'][0], lv_cp=cap['pri'][1], mean_ip=cap['pri'][2], lv_ip=cap['pri'][3], eps_p=d['eps_p'],
             noise=noise, cat_oh=d['cat_oh'], dz_in=cap['dz_in'])
    c = {k: (None if v is None else (v.detach().cpu().numpy() if torch.is_tensor(v) else v).astype(np.float32)) for k, v in c.items()}
    g64, g32 = H._autograd(c, torch.float64), H._autograd(c, torch.float32)
    return {k: (float(np.abs(g32[k] - g64[k]).max()), float(np.abs(g64[k]).max())) for k in g64}


@pytest.mark.parametrize('mix', [True, False])
def test_fit_hip_against_torch(mix, dtype):
    """One fit step with latent='hip' against latent='torch' from identical weights and draws (the prior networks' dropout included: the
    generator is seeded alike).  Gates:
      the latent stage's gradients (d_enc_out, d_mean_cp, d_mean_ip): the backward gate of tests/test_mm_latent_host.py, 4x what float32
        autograd loses against float64 on this step's inputs, plus what the two legs' DIFFERENT dz_in contribute -- the decoder sees
        z_in one float32 rounding apart and hands back gradients that differ; the stage is linear in dz_in, d_mean takes it unchanged
        and d_logVar times 0.5 sigma eps, so max|dz_hip - dz_torch| max(1, max|0.5 sigma eps|) bounds that share;
      kl, reg: twice the forward gates of the host tests (each leg is within the gate of the exact value); loss_shape, pr, rc: the decoder's float32 term on inputs one rounding apart;
      parameter gradients of the 2D encoder and the prior networks: linear images of the gradients above through the SAME torch
        backward, so the same relative gate summed over the three heads, taken against the largest gradient entry of the parameter's
        NETWORK: a bias in front of a BatchNorm has a gradient that cancels exactly, and what float32 leaves there is the rounding of
        summands as large as the layer's other gradients, not of the (near-zero) result;
      the decoder's weights after the step: tests/_tol.py's float32 term on the weights, plus what Adam's first step makes of the two
        legs' different gradients: it moves a weight by lr f(g), f(g) = g / (|g| + e), e = ADAM_EPS / sqrt(1 - beta2), and
        |f(a) - f(b)| <= min(2, |a - b| / (min(|a|, |b|) + e)) -- a gradient that is rounding noise (dense/bias in front of its
        BatchNorm cancels exactly) is normalised to about lr in either direction.  With the mix the legs' z_in are bit-identical and
        every weight agrees exactly (measured on the MI355X); without it z_in is one rounding apart in places, dense/bias differs by
        2.1e-5 and convT2/kernel by 3.9e-5."""
    from voxvae import train as T
    dtype('f32')
    d = _data()
    rand = dict(eps=d['eps'], eps_prior=d['eps_p'], mix=mix, noise=d['noise'])
    inputs = (d['img'], d['vox'], d['cat_oh'], d['inst_oh'])
    legs = {}
    for latent in ('hip', 'torch'):
        m = _model()
        w0 = {k: v.clone() for k, v in m._dec_eng.params.items()}
        m._debug = {}
        m._encoder_backbone.train()
        torch.manual_seed(9)
        out = [float(v) for v in m.fit(inputs, latent=latent, _rand=rand)]
        grads = {n: p.grad.detach().cpu().numpy() for mod, tag in ((m._encoder_backbone, 'enc'), (m._priornet_class, 'pc'), (m._priornet_inst, 'pi'))
                 for n, p in ((tag + '/' + n, p) for n, p in mod.named_parameters())}
        g_dec = {k: m._trainer2d._g('dec/' + k).detach().cpu().numpy().copy() for k in w0 if not k.endswith(('moving_mean', 'moving_variance'))}
        legs[latent] = dict(out=out, cap=m._debug, grads=grads, g_dec=g_dec, w={k: v.detach().cpu().numpy() for k, v in m._dec_eng.params.items()},
                            w0={k: v.cpu().numpy() for k, v in w0.items()})
    h, t = legs['hip'], legs['torch']
    assert set(h['cap']) >= {'d_enc_out', 'dz_in', 'enc_out', 'pri', 'd_pri'}
    noise = d['noise'] if mix else None
    e = _e32(t['cap'], d, noise)
    ddz = float((h['cap']['dz_in'] - t['cap']['dz_in']).abs().max())
    enc = t['cap']['enc_out'].cpu().numpy()
    sig = np.sqrt(np.exp(np.clip(np.concatenate([enc[:, LC:2 * LC], enc[:, 2 * LC + LI:]], axis=1), -10, 10)))
    lin = ddz * max(1.0, float(np.abs(0.5 * sig * d['eps']).max()))
    rel = 0.0
    for k, got, want in (('enc', h['cap']['d_enc_out'], t['cap']['d_enc_out']), ('mean_cp', h['cap']['d_pri'][0], t['cap']['d_pri'][0]),
                         ('mean_ip', h['cap']['d_pri'][2], t['cap']['d_pri'][2])):
        gate = H.backward_gate(*e[k]) + (lin if k == 'enc' else 0.0)
        err = float((got - want).abs().max())
        print('%s: |hip - torch| %.3e, f32 autograd error %.3e, dz share %.3e, gate %.3e' % (k, err, e[k][0], lin if k == 'enc' else 0.0, gate))
        assert err <= gate, (k, err, gate)
        rel += gate / e[k][1]
    for k in (0, 2):                                                # kl, reg; then shape, pr, rc
        print('out[%d]: hip %.8g torch %.8g' % (k, h['out'][k], t['out'][k]))
        assert abs(h['out'][k] - t['out'][k]) <= 2 * (H.KL_GATE, None, H.REG_GATE)[k] * max(abs(t['out'][k]), 1.0)
    for k in (1, 3, 4):
        print('out[%d]: hip %.8g torch %.8g' % (k, h['out'][k], t['out'][k]))
        assert abs(h['out'][k] - t['out'][k]) <= _tol.f32_term(np.array([t['out'][k]]))
    net_scale = {tag: max(float(np.abs(g).max()) for n, g in t['grads'].items() if n.startswith(tag + '/')) for tag in ('enc', 'pc', 'pi')}
    for n in t['grads']:
        scale = net_scale[n.split('/')[0]]
        err = float(np.abs(h['grads'][n] - t['grads'][n]).max())
        print('%s: |hip - torch| %.3e of %.3e, relative gate %.3e' % (n, err, scale, rel))
        assert err <= rel * scale + 2.0 ** -24 * scale, (n, err, rel * scale)
    moved = 0.0
    for n in t['w']:
        if n.endswith(('moving_mean', 'moving_variance')):
            continue
        err = float(np.abs(h['w'][n] - t['w'][n]).max())
        moved = max(moved, float(np.abs(t['w'][n] - t['w0'][n]).max()))
        ga, gb = h['g_dec'][n].astype(np.float64), t['g_dec'][n].astype(np.float64)
        adam = 1e-4 * np.minimum(2.0, np.abs(ga - gb) / (np.minimum(np.abs(ga), np.abs(gb)) + T.ADAM_EPS / np.sqrt(1.0 - T.ADAM_B2)))   # lr = 1e-4, the default
        bound = 1.004 * _tol.f32_term(t['w'][n]) + adam.reshape(t['w'][n].shape)
        print('%s: |hip - torch| %.3e, float32 term %.3e, largest Adam share %.3e' % (n, err, 1.004 * _tol.f32_term(t['w'][n]), float(adam.max())))
        assert np.all(np.abs(h['w'][n] - t['w'][n]) <= bound), (n, err)
    assert moved >= 0.5e-4                                          # the step was taken: Adam's first step is about the learning rate
    assert float(np.abs(t['grads']['enc/w']).max()) > 0 and float(np.abs(t['grads']['pi/mean.0.weight']).max()) > 0   # autograd reached them


@pytest.mark.parametrize('act', ['f32', 'bf16'])
def test_AE_getEval_and_fit_match_the_base_semantics(act, dtype):
    """nolboSingleObject_AE: the head output IS the latent.  getEval is _ModelnetBase's non-variational 10-tuple (the prediction is the
    decoder engine's on the encoder output, the corrected half present with missing_prob > 0), the 2-input form gives 4 values, getLatent
    returns the encoder output; fit returns (loss_shape, pr, rc), moves the decoder, and with dropout the 2D encoder's gradient is the
    decoder's d z times the kept mask."""
    from voxvae import synthetic as syn
    import src.module.nolbo as nolbo
    dtype(act)
    d = _data()
    L = LC + LI
    cfg = {'encoder_backbone': {'name': 'bb', 'z_dim': L}, 'encoder_head': None, 'decoder': _config()['decoder']}
    m = nolbo.nolboSingleObject_AE(nolbo_structure=cfg, encoder_backbone=Encoder(L), dropout=True)
    m._decoder.set_weights_dict(syn.make_decoder_params(cfg['decoder']))
    cats = syn.make_category_vectors(C, L)
    enc = m._encoder_backbone(d['img']).detach()
    assert np.array_equal(m.getLatent(d['img']), enc.cpu().numpy())
    out = m.getEval((d['img'], d['vox'], d['cat_oh']), cats, missing_prob=0.0)
    assert len(out) == 10 and out[5:] == (0, 0, 0, 0, 0)
    pred, _, _, met = m._dec_eng.forward(enc if act == 'f32' else enc.to(torch.bfloat16), m._dev(d['vox']), want_metrics=True)
    assert np.array_equal(np.array(out[0]), pred.float().cpu().numpy().reshape(B, D, D, D, 1))
    assert [float(out[k]) for k in (1, 2, 3)] == [float(met[k]) for k in (0, 1, 2)]
    mask = np.concatenate([d['mask'], np.ones((B, LI), np.float32)], axis=1)
    out = m.getEval((d['img'], d['vox'], d['cat_oh']), cats, missing_prob=0.5, _mask=mask, _eps2=d['eps'])
    assert len(out) == 10 and np.array(out[5]).shape == (B, D, D, D, 1) and all(np.isfinite(float(v)) for v in out[1:5] + out[6:10])
    zc = np.array(m._z_category_corrected)
    assert np.array_equal(zc[mask == 1], enc.cpu().numpy()[mask == 1])               # kept elements pass the correction unchanged
    assert len(m.getEval((d['img'], d['vox']), missing_prob=0.5, _mask=mask)) == 4
    if act == 'bf16':
        return                                                                        # the 2D encoder trains by float32 autograd
    w0, e0 = m._dec_eng.params['convT1/kernel'].clone(), m._encoder_backbone.w.detach().clone()
    keep = (np.random.default_rng(1).random((B, L)) >= 0.25).astype(np.float32)
    m._encoder_backbone.train()
    fit = m.fit((d['img'], d['vox']), _dropout=(0.25, keep))
    assert len(fit) == 3 and all(np.isfinite(float(v)) for v in fit)
    assert not torch.equal(w0, m._dec_eng.params['convT1/kernel']) and not torch.equal(e0, m._encoder_backbone.w)
    # a column of the latent that is dropped for every sample leaves the encoder's matching column where it was
    m2 = nolbo.nolboSingleObject_AE(nolbo_structure=cfg, encoder_backbone=Encoder(L), dropout=True)
    keep[:, 0] = 0
    m2._encoder_backbone.train()
    m2.fit((d['img'], d['vox']), _dropout=(0.25, keep))
    assert torch.equal(m2._encoder_backbone.w[:, 0], e0[:, 0]) and not torch.equal(m2._encoder_backbone.w[:, 1], e0[:, 1])


@pytest.mark.parametrize('script', ['train_pascal.py', 'test_pascal.py', 'test_pascal_3D.py'])
def test_entry_scripts_on_synthetic_data(script, tmp_path):
    """The three entry scripts with --max-iter 2 on the synthetic loader; test_pascal_3D.py --out-dir writes the five dumps per object,
    [D*D, D] each, under the reference's <split>/<2 * missing_pr>/3D."""
    Dv, n = 16, 2
    cmd = [sys.executable, script, '--max-iter', '2', '--batch', str(n), '--image', '64', '--voxel', str(Dv), '--latent', '8',
           '--dataset-path', 'synthetic:4:%d' % Dv]
    if script == 'test_pascal_3D.py':
        cmd += ['--out-dir', str(tmp_path / 'data_3D')]
    r = subprocess.run(cmd, cwd=PKG, capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    if script != 'test_pascal_3D.py':
        assert 'it:0002' in r.stdout and 'NaN' not in r.stdout, r.stdout[-2000:]
        return
    for split in ('train', 'test'):
        for rate in ('0.3', '0.5'):
            files = sorted(os.listdir(tmp_path / 'data_3D' / split / rate / '3D'))
            assert files == sorted('%03d_%s.txt' % (i, t) for i in range(n) for t in ('gt', 'mVAE', 'mVAE_c', 'AE', 'VAE')), files
    a = np.loadtxt(tmp_path / 'data_3D' / 'test' / '0.3' / '3D' / '001_mVAE_c.txt')
    g = np.loadtxt(tmp_path / 'data_3D' / 'test' / '0.3' / '3D' / '001_gt.txt')
    assert a.shape == g.shape == (Dv * Dv, Dv) and set(np.unique(g)) <= {0.0, 1.0} and a.min() >= 0 and a.max() <= 1 and a.std() > 0
