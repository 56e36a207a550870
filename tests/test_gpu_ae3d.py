"""GPU tests of src/module/AE3D.py (the data-parallel 3D autoencoder) against the float64 reference of tests/_ae3d_ref.py: one step
in f32 and bf16, the rescaled input, the l2 term, predict after a reload, two ranks over gloo, one rank over RCCL, the entry script."""
import os
import re
import socket
import subprocess
import sys

import numpy as np
import pytest
import torch

import _ae3d_ref as ref
from _train_ref import ADAM_UNITS, adam_units, lr_t_of

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LR = 1e-3
_MOVING = ('moving_mean', 'moving_variance')


def _params(D, Lz):
    from voxvae import synthetic as syn
    cfg = syn.make_config(D, Lz, False)
    ep = syn.make_encoder_params(cfg['encoder'], seed=42, nontrivial_affine=True)
    dp = syn.make_decoder_params(cfg['decoder'], seed=43, nontrivial_affine=True, final_gain=2.0)   # logits away from the clip's gradient discontinuity
    return cfg, ep, dp


def _model(D, Lz, B, dtype='f32'):
    import voxvae
    voxvae.set_default_dtype(dtype)
    voxvae.set_default_device(DEV)
    import src.module.AE3D as AE3D
    cfg, ep, dp = _params(D, Lz)
    model = AE3D.AE3D(cfg['encoder'], cfg['decoder'], BATCH_SIZE_PER_REPLICA=B, learning_rate=LR)
    model._encoder.set_weights_dict(ep)
    model._decoder.set_weights_dict(dp)
    return cfg, ep, dp, model


_REF = {}


def _reference(D, Lz, B, seed=100):
    """The float64 step of one shape, computed once and shared (read-only) by the tests that need it."""
    key = (D, Lz, B, seed)
    if key not in _REF:
        from voxvae import synthetic as syn
        cfg, ep, dp = _params(D, Lz)
        x = syn.make_voxels(B, D, seed=seed)
        _REF[key] = (x, ref.fit_ref(cfg, ep, dp, x, x))
    return _REF[key]


def _rel(a, b):
    return float(np.abs(a - b).max() / (np.abs(b).max() + 1e-30))


def _bias_residue_bound(tr, B):
    """A bias in front of BatchNorm has zero true prediction gradient; what the kernels leave is the float32 cancellation residue of a
    column sum of B terms of magnitude |d pre-BN| (tests/test_gpu_train.py::test_fit_step_matches_autograd_oracle)."""
    return 64 * np.finfo(np.float32).eps * B * float(tr.debug['dcv0'].float().abs().max())


def _grad_errors(tr, r, B):
    worst = {}
    for name, g_ref in r['g_pred'].items():
        g = tr.grads.views[name].cpu().numpy()
        if name == 'dec/dense/bias':
            assert np.abs(g_ref).max() < 1e-9
            assert np.abs(g).max() <= _bias_residue_bound(tr, B), np.abs(g).max()
            continue
        worst[name] = _rel(g, g_ref)
    return worst


@pytest.mark.parametrize('D,Lz,B', [(16, 16, 3), (32, 16, 4)])
def test_fit_step_matches_the_float64_reference(D, Lz, B):
    x, r = _reference(D, Lz, B)
    cfg, ep, dp, model = _model(D, Lz, B)
    tr = model._trainer
    tr.debug = {}
    out = model.fit((x, x))
    torch.cuda.synchronize()
    reg, pred, total, TP, FP, FN = (float(v) for v in out)
    print('\n[AE3D fit D%d L%d B%d] reg %.6f (ref %.6f)  pred %.4f (ref %.4f)  counts x B %s (ref %s)'
          % (D, Lz, B, reg, r['reg'], pred, r['pred'], [TP * B, FP * B, FN * B], [r['tp'], r['fp'], r['fn']]))
    assert abs(pred - r['pred']) <= 2e-4 * abs(r['pred'])
    assert abs(reg - r['reg']) <= 1e-5 * r['reg']
    assert total == float(np.float32(reg) + np.float32(pred))
    assert [float(np.rint(c * B)) for c in (TP, FP, FN)] == [r['tp'], r['fp'], r['fn']]
    assert max(abs(c * B - w) for c, w in zip((TP, FP, FN), (r['tp'], r['fp'], r['fn']))) < 0.01
    # the buckets hold d pred / dw: the l2 term enters inside the optimiser launch
    worst = _grad_errors(tr, r, B)
    bad = {k: v for k, v in worst.items() if v > 5e-5}
    assert not bad, 'gradient mismatch (max rel err): %s' % bad
    print('[AE3D fit D%d] worst grad rel err %.2e (%s)' % (D, max(worst.values()), max(worst, key=worst.get)))
    new = {**{'enc/' + k: v for k, v in model._encoder.get_weights_dict().items()}, **{'dec/' + k: v for k, v in model._decoder.get_weights_dict().items()}}
    old = {**{'enc/' + k: v for k, v in ep.items()}, **{'dec/' + k: v for k, v in dp.items()}}
    for key, v in new.items():
        if key.endswith(_MOVING):
            base = key.rsplit('/', 1)[0]
            bm, bv = r['bn_stats'][base]
            wm, wv = ref.moved_statistics(old[base + '/moving_mean'], old[base + '/moving_variance'], bm, bv)
            np.testing.assert_allclose(v, wm if key.endswith('moving_mean') else wv, rtol=1e-4, atol=1e-6, err_msg=key)
            continue
        g = r['g_total'][key]                                 # Adam on the TOTAL gradient: d pred / dw + 2 lambda w
        step_ref = ref.adam_first_step(old[key], g, LR)[0] - old[key]
        big = np.abs(g) > 1e-3 * np.abs(g).max()
        if key == 'dec/dense/bias':
            # d pred / d bias is 0 in front of BatchNorm and the bucket holds a float32 residue (bounded above) that Adam's first step,
            # m / sqrt(v) = +-1 wherever |g| >> epsilon, amplifies: the l2 fold is checked on the gradient the optimiser was handed
            g = tr.grads.views[key].cpu().numpy().astype(np.float64) + r['g_sum_reg'][key]
            step_ref = ref.adam_first_step(old[key], g, LR)[0] - old[key]
            big = np.ones(g.shape, bool)
        assert np.abs((v - old[key]) - step_ref)[big].max() <= 0.02 * LR + 1e-9, key
    # Adam's first step is ~ lr * sign(g) and says little about the SIZE of the l2 term.  A second step, from the non-zero moments the
    # first left, does: float64 Adam on the gradient the step itself computed + (2 lambda) w, from the exported weights, m and v, in
    # the units and with the bound of tests/test_gpu_ae3d_ops.py (weights of a real layer: the uncancelled unit).
    from voxvae import synthetic as syn
    snap = lambda d: {n: d(n).cpu().numpy().copy() for n, _ in tr.order}
    w1, m1, v1 = snap(tr._p), snap(lambda n: tr.m[n]), snap(lambda n: tr.v[n])
    x2 = syn.make_voxels(B, D, seed=101)
    model.fit((x2, x2))
    torch.cuda.synchronize()
    assert tr.t == 2
    coef = float(np.float32(2 * ref.L2))
    worst, without = [0.0, 0.0, 0.0], 0.0
    for n, _ in tr.order:
        g = tr.grads.views[n].cpu().numpy().astype(np.float64)
        g_eff = g + coef * w1[n].astype(np.float64) if ref.regularised(n) else g
        got = (tr._p(n).cpu().numpy(), tr.m[n].cpu().numpy(), tr.v[n].cpu().numpy())
        worst = [max(a, b) for a, b in zip(worst, adam_units(*got, w1[n], g_eff, m1[n], v1[n], lr_t_of(2, LR), uncancelled=True))]
        if ref.regularised(n):
            without = max(without, adam_units(*got, w1[n], g, m1[n], v1[n], lr_t_of(2, LR), uncancelled=True)[0])
    print('[AE3D fit D%d] second step in bound units: m %.2f v %.2f param %.2f (bound %.0f); m without the l2 term: %.0f' % ((D,) + tuple(worst) + (ADAM_UNITS + 4, without)))
    assert max(worst) <= ADAM_UNITS + 4, worst
    assert without > 100 * (ADAM_UNITS + 4)                 # the same check with the term left out misses by orders of magnitude: it sees the coefficient


def test_the_rescale_and_the_l2_term_are_exercised():
    """Negative controls at (16, 16, 3): a step fed x instead of 2x - 1 misses the gradient bound, and a step without the l2 term ends
    with other weights than the l2 step, beyond the Adam tolerance, on the largest kernel."""
    from voxvae import train as T
    D, Lz, B = 16, 16, 3
    x, r = _reference(D, Lz, B)
    cfg, ep, dp, model = _model(D, Lz, B)
    model.fit((x, x))
    with_l2 = {k: v.clone() for k, v in model._enc_eng.params.items()}
    xd = torch.from_numpy(x).to(DEV)
    # no rescale
    model._encoder.set_weights_dict(ep)
    model._decoder.set_weights_dict(dp)
    tr = T.Trainer(model._enc_eng, model._dec_eng, False, LR, weight_l2=ref.L2)
    tr.debug = {}
    tr.step(xd, xd)
    torch.cuda.synchronize()
    worst = _grad_errors(tr, r, B)
    assert max(worst.values()) > 5e-5, 'feeding x instead of 2x - 1 went unnoticed: %s' % worst
    # no l2
    model._encoder.set_weights_dict(ep)
    model._decoder.set_weights_dict(dp)
    tr0 = T.Trainer(model._enc_eng, model._dec_eng, False, LR)
    assert tr0.weight_l2 == 0.0
    tr0.step(2.0 * xd - 1.0, xd)
    torch.cuda.synchronize()
    largest = max((k for k in with_l2 if k.endswith('/kernel')), key=lambda k: with_l2[k].numel())
    d = float((model._enc_eng.params[largest] - with_l2[largest]).abs().max())
    assert d > 0.02 * LR + 1e-9, (largest, d)
    s = tr0.step_scalars(torch.zeros(B, 4, device=DEV))      # without the term the regulariser's value is 0, not stale
    assert float(s[0]) == 0.0
    # refusals: a batch other than BATCH_SIZE_PER_REPLICA (the losses are scaled by the model's GLOBAL_BATCH), and a second l2 term
    with pytest.raises(ValueError, match='BATCH_SIZE_PER_REPLICA'):
        model.fit((x[:2], x[:2]))
    half = T.Trainer(None, model._dec_eng, False, LR, weight_l2=ref.L2)
    z = torch.zeros(B, Lz, device=DEV)
    with pytest.raises(ValueError, match='twice'):
        half.step_decoder(z, xd, l2=ref.L2)
    with pytest.raises(ValueError, match='twice'):
        half.step_from_latent(z, xd, l2=ref.L2)


def test_bf16_fit_tracks_the_reference():
    """(32, 16, 8) in mixed precision with the bounds of tests/test_gpu_train.py::test_bf16_mixed_precision_fit_tracks_the_oracle: losses
    1 %, every gradient tensor within 6 % in the Frobenius norm and cosine > 0.995.  reg_loss is a float32 sum over float32 master
    weights in both modes: its f32 bound."""
    D, Lz, B = 32, 16, 8
    x, r = _reference(D, Lz, B)
    cfg, ep, dp, model = _model(D, Lz, B, dtype='bf16')
    tr = model._trainer
    out = model.fit((x, x))
    torch.cuda.synchronize()
    reg, pred, total, TP, FP, FN = (float(v) for v in out)
    assert tr.dt == 1 and tr.grads.views['enc/conv1/kernel'].dtype == torch.float32
    assert abs(pred - r['pred']) <= 1e-2 * abs(r['pred'])
    assert abs(reg - r['reg']) <= 1e-5 * r['reg']
    p_ref, r_ref = r['tp'] / (r['tp'] + r['fp'] + 1e-10), r['tp'] / (r['tp'] + r['fn'] + 1e-10)
    assert abs(TP / (TP + FP + 1e-10) - p_ref) < 1e-2 and abs(TP / (TP + FN + 1e-10) - r_ref) < 1e-2
    worst, cos = {}, {}
    for name, g_ref in r['g_pred'].items():
        if name == 'dec/dense/bias':
            continue
        g = tr.grads.views[name].cpu().numpy().astype(np.float64)
        worst[name] = float(np.linalg.norm(g - g_ref) / (np.linalg.norm(g_ref) + 1e-30))
        cos[name] = float((g * g_ref).sum() / (np.linalg.norm(g) * np.linalg.norm(g_ref) + 1e-30))
    bad = {k: (worst[k], cos[k]) for k in worst if worst[k] > 6e-2 or cos[k] < 0.995}
    assert not bad, 'bf16 gradient drift (rel Frobenius error, cosine): %s' % bad
    print('\n[AE3D bf16 fit] worst rel err %.3f (%s), min cosine %.5f' % (max(worst.values()), max(worst, key=worst.get), min(cos.values())))


def test_predict_survives_a_reload_and_matches_the_f32_oracle(tmp_path):
    from oracle import torch_oracle as to
    from voxvae import synthetic as syn
    D, Lz, B = 16, 16, 3
    cfg, ep, dp, model = _model(D, Lz, B)
    x = syn.make_voxels(B, D, seed=100)
    before = np.array(model.predict(x))
    model.saveModel(str(tmp_path))
    assert sorted(os.listdir(tmp_path)) == ['decoder.voxvae.npz', 'encoder3D.voxvae.npz']
    import src.module.AE3D as AE3D
    fresh = AE3D.AE3D(cfg['encoder'], cfg['decoder'], BATCH_SIZE_PER_REPLICA=B)
    assert not np.array_equal(np.array(fresh.predict(x)), before)
    fresh.loadModel(str(tmp_path))
    after = np.array(fresh.predict(x))
    assert before.shape == (B, D, D, D, 1) and np.array_equal(before.view(np.int32), after.view(np.int32))
    # the oracle's inference forward is written for the variational classes (mean | logVar, z = mean + sqrt(exp logVar) eps): an encoder
    # widened by Lz zero output channels (logVar = 0) with eps = 0 is this autoencoder exactly
    vcfg = syn.make_config(D, Lz, True)
    vep = dict(ep)
    k = ep['conv4/kernel']
    vep['conv4/kernel'] = np.concatenate([k, np.zeros_like(k)], axis=-1)
    logits = to.eval_forward_f32(vcfg, vep, dp, 2.0 * x - 1.0, np.zeros((B, Lz), np.float32))[0]
    want = 1.0 / (1.0 + np.exp(-logits.astype(np.float64)))
    err = float(np.abs(before - want).max())
    print('\n[AE3D predict] max |dprob| %.3e' % err)
    assert err < 2.5e-4                                        # |dprob| <= 0.25 |dlogit|, the project's f32 logit bar 1e-3


def test_loss_and_evaluation_methods_and_bf16_predict(tmp_path):
    """_lossObject / _evaluation (AE3D.py:46-59) on a prediction against float64 from the same float32 probabilities, with the model's
    GLOBAL_BATCH; predict in bf16 mode gives the same bits after a reload."""
    from voxvae import synthetic as syn
    D, Lz, B = 16, 16, 3
    cfg, ep, dp, model = _model(D, Lz, B, dtype='bf16')
    x = syn.make_voxels(B, D, seed=100)
    pred = model.predict(x)
    p = np.array(pred).astype(np.float64)
    assert p.shape == (B, D, D, D, 1) and p.min() >= 0.0 and p.max() <= 1.0
    q, y = np.clip(p, 1e-7, 1.0 - 1e-7), x.astype(np.float64)
    bce = -(0.6 * y * np.log(q) + 0.4 * (1 - y) * np.log(1 - q)).sum()
    yh = (p >= 0.5).astype(np.float64)
    want = [(y * yh).sum() / B, ((1 - y) * yh).sum() / B, (y * (1 - yh)).sum() / B]
    loss = float(model._lossObject(y_target=x, y_pred=pred, gamma=0.6))
    assert abs(loss - bce / B) <= 1e-5 * bce / B, (loss, bce / B)
    got = [float(v) for v in model._evaluation(y_target=x, y_pred=pred)]
    assert np.abs(np.array(got) - want).max() <= 2.0 ** -23 * max(want), (got, want)
    model.saveModel(str(tmp_path))
    import src.module.AE3D as AE3D
    fresh = AE3D.AE3D(cfg['encoder'], cfg['decoder'], BATCH_SIZE_PER_REPLICA=B)
    fresh.loadModel(str(tmp_path))
    assert fresh._dec_eng.dt == 1 and np.array_equal(np.array(fresh.predict(x)).view(np.int32), np.array(pred).view(np.int32))


# ------------------------------------------------------------------------------------------------------------ two ranks (gloo)
DP_D, DP_L, DP_B = 16, 16, 2


def _dp_worker(rank, world, port, shards, out):
    import torch.distributed as dist
    os.environ['MASTER_ADDR'] = '127.0.0.1'
    os.environ['MASTER_PORT'] = str(port)
    dist.init_process_group('gloo', rank=rank, world_size=world)
    cfg, ep, dp, model = _model(DP_D, DP_L, DP_B)
    assert model._GLOBAL_BATCH_SIZE == world * DP_B and model._trainer.world == world
    res = model.distributed_fit((shards[rank], shards[rank]))
    torch.cuda.synchronize()
    tr = model._trainer
    import hashlib
    grads = {n: tr.grads.views[n].cpu().numpy().copy() for n, _ in tr.order}
    out['g%d' % rank] = {n: hashlib.sha256(g.tobytes()).hexdigest() for n, g in grads.items()}
    if rank == 0:
        out[0] = grads
    weights = [(n, tr._p(n)) for n, _ in tr.order]           # the trained variables (BatchNorm's moving statistics are per replica, as the reference's)
    out['w%d' % rank] = {k: hashlib.sha256(v.cpu().numpy().tobytes()).hexdigest() for k, v in weights}      # bit identity needs no more
    out['conv3_%d' % rank] = model._enc_eng.params['conv3/kernel'].cpu().numpy().copy()
    out['mv%d' % rank] = {n: (tr.m[n].cpu().numpy().copy(), tr.v[n].cpu().numpy().copy()) for n in ('enc/conv3/kernel',)}
    out['res%d' % rank] = [float(v) for v in res]
    out['overlap%d' % rank] = bool(tr.overlap)
    dist.destroy_process_group()


def test_distributed_fit_two_ranks():
    """Two processes share the GPU over gloo (as tests/test_gpu_train.py::test_data_parallel_step_two_ranks does), D = 16, L = 16, two
    samples per rank."""
    import torch.multiprocessing as mp
    from voxvae import synthetic as syn
    from voxvae import train as T
    world = 2
    shards = [syn.make_voxels(DP_B, DP_D, seed=900 + r) for r in range(world)]
    cfg, ep, dp, model = _model(DP_D, DP_L, DP_B)
    expect, stats = None, []
    for r in range(world):                                   # single process: each shard's gradient with the global-batch scaling
        model._encoder.set_weights_dict(ep)
        model._decoder.set_weights_dict(dp)
        tr = T.Trainer(model._enc_eng, model._dec_eng, False, LR, world_size=world)
        x = torch.from_numpy(shards[r]).to(DEV)
        _, st, _ = tr.step(2.0 * x - 1.0, x)
        stats.append(st.cpu().numpy().astype(np.float64))
        g = {n: tr.grads.views[n].cpu().numpy().astype(np.float64) for n, _ in tr.order}
        expect = g if expect is None else {n: expect[n] + g[n] for n in g}
    out = mp.Manager().dict()
    with socket.socket() as s:
        s.bind(('127.0.0.1', 0))
        port = s.getsockname()[1]
    mp.spawn(_dp_worker, args=(world, port, shards, out), nprocs=world, join=True)
    for n, e in expect.items():
        assert np.abs(out[0][n].astype(np.float64) - e).max() <= 1e-6 * np.abs(e).max() + 1e-12, n
    assert out['g0'] == out['g1'] and set(out['g0']) == set(expect)          # both ranks hold the same sums, bit for bit
    assert len(out['w0']) == len(expect) and out['w0'] == out['w1']           # ... and end with the same weights
    assert out['overlap0'] and out['overlap1']               # the l2 term did not turn the bucket overlap off
    # the largest regularised kernel: Adam on g_sum + (2 * lambda * 2) * w
    name = 'enc/conv3/kernel'
    assert ep['conv3/kernel'].size == max(v.size for v in list(ep.values()) + list(dp.values()))
    w0 = ep['conv3/kernel']
    coef = float(np.float32(2 * ref.L2 * world))
    g_eff = out[0][name].astype(np.float64) + coef * w0.astype(np.float64)
    zero = np.zeros_like(w0)
    gm, gv = out['mv0'][name]
    u = adam_units(out['conv3_0'], gm, gv, w0, g_eff, zero, zero, lr_t_of(1, LR))
    print('\n[AE3D two ranks] %s in bound units: m %.2f v %.2f param %.2f (bound %.0f)' % ((name,) + u + (ADAM_UNITS + 4,)))
    assert max(u) <= ADAM_UNITS + 4, u
    # the returned tuple against the single-process values
    P = {**{'enc/' + k: v for k, v in ep.items()}, **{'dec/' + k: v for k, v in dp.items()}}
    sumsq = sum((v.astype(np.float64) ** 2).sum() for k, v in P.items() if ref.regularised(k))
    s = stats[0].sum(axis=0) + stats[1].sum(axis=0)
    rl, pl = world * ref.L2 * sumsq, s[0] / (world * DP_B)
    tp, fp, fn = (s[k] / (world * DP_B) for k in (1, 2, 3))
    want = [rl, pl, rl + pl, tp / (tp + fp + 1e-10), tp / (tp + fn + 1e-10)]
    assert out['res0'] == out['res1']
    for got, w, what in zip(out['res0'], want, ('rl', 'pl', 'tl', 'p', 'r')):
        assert abs(got - w) <= 2e-6 * abs(w), (what, got, w)


# ------------------------------------------------------------------------------------------------------------ one rank (RCCL)
def test_distributed_fit_through_rccl_is_bit_identical_to_the_plain_path():
    import json
    with socket.socket() as s:
        s.bind(('127.0.0.1', 0))
        port = s.getsockname()[1]
    e = dict(os.environ)
    e.update({'MASTER_ADDR': '127.0.0.1', 'MASTER_PORT': str(port), 'WORLD_SIZE': '1', 'RANK': '0', 'LOCAL_RANK': '0',
              'HSA_ENABLE_IPC_MODE_LEGACY': '0'})
    p = subprocess.run([sys.executable, os.path.join(ROOT, 'tests', '_ae3d_rccl_child.py'), 'f32'], env=e, stdout=subprocess.PIPE,
                       stderr=subprocess.PIPE, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-3000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith('{')]
    assert lines, p.stdout[-2000:]
    r = json.loads(lines[-1])
    assert r['backend'] == 'nccl' and r['world'] == 1
    assert all(w != 'bool' for w in r['work_types']), r['work_types']                # real collective handles ...
    assert all(w == 'bool' for w in r['plain_work_types']), r['plain_work_types']    # ... and none in the plain step
    assert r['weights_bit_identical'] and r['values_bit_identical'] and all(np.isfinite(r['values']))


# ------------------------------------------------------------------------------------------------------------ entry script
def test_entry_script_smoke():
    script = os.path.join(ROOT, 'anytime-3d-reconstruction_amd', 'train_modelnet_AE.py')
    e = {k: v for k, v in os.environ.items() if k not in ('WORLD_SIZE', 'RANK', 'LOCAL_RANK')}
    p = subprocess.run([sys.executable, script, '--voxel', '16', '--latent', '16', '--batch', '4', '--max-iter', '3'], env=e,
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-3000:]
    rows = re.findall(r'iter:(\d+) .*?rloss:([-\d.naninf]+), ploss:([-\d.naninf]+), tloss:([-\d.naninf]+)\s+pr:([-\d.naninf]+), rc:([-\d.naninf]+)', p.stdout)
    assert [int(r[0]) for r in rows] == [1, 2, 3], p.stdout[-2000:]
    vals = np.array([[float(v) for v in r[1:]] for r in rows])
    assert np.isfinite(vals).all() and (vals[:, :3] > 0).all()
    assert vals[2, 2] < vals[0, 2], vals[:, 2]
