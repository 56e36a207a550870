"""CPU tests of the data-parallel 3D autoencoder (src/module/AE3D.py): the float64 reference's own l2 gradient, the chunk table of
vv_adam_step_multi_l2 as a pure function of names and shapes, the constructor's refusals, and the summed-count metric formulas."""
import numpy as np
import pytest
import torch

import _ae3d_ref as ref
from _train_ref import ADAM_CHUNK


def _model_shapes(D, Lz=16):
    from voxvae import synthetic as syn
    cfg = syn.make_config(D, Lz, False)
    ep, dp = syn.make_encoder_params(cfg['encoder']), syn.make_decoder_params(cfg['decoder'])
    skip = ('moving_mean', 'moving_variance')
    names = [('enc/' + k, v.shape) for k, v in ep.items() if not k.endswith(skip)] + [('dec/' + k, v.shape) for k, v in dp.items() if not k.endswith(skip)]
    return cfg, ep, dp, list(reversed(names))


def test_reference_l2_gradient_is_two_lambda_w_on_regularised_variables_only():
    """d(total - pred)/dw by the reference's autograd (float64, D = 16, B = 2): 2 * lambda * w on every kernel and on the Dense bias,
    exactly 0 on every BatchNorm variable -- what vv_adam_step_multi_l2 folds in per chunk."""
    from voxvae import synthetic as syn
    cfg, ep, dp, names = _model_shapes(16)
    x = syn.make_voxels(2, 16, seed=7)
    r = ref.fit_ref(cfg, ep, dp, x, x)
    P = {**{'enc/' + k: v for k, v in ep.items()}, **{'dec/' + k: v for k, v in dp.items()}}
    seen_reg = seen_bn = 0
    for n in r['names']:
        d = r['g_total'][n] - r['g_pred'][n]
        w = P[n].astype(np.float64)
        if ref.regularised(n):
            seen_reg += 1
            assert np.abs(d - 2 * ref.L2 * w).max() <= 1e-12 * max(1.0, np.abs(r['g_pred'][n]).max()), n
            np.testing.assert_array_equal(r['g_sum_reg'][n], 2 * ref.L2 * w)
        else:
            seen_bn += 1
            assert n.rsplit('/', 1)[1] in ('gamma', 'beta') and not d.any(), n
    assert seen_reg == 12 and seen_bn == 18          # 5 + 5 conv kernels, the Dense kernel and bias; 9 BatchNorm layers
    assert abs(r['reg'] - ref.L2 * sum((P[n].astype(np.float64) ** 2).sum() for n in r['names'] if ref.regularised(n))) <= 1e-12 * r['reg']
    assert r['total'] == r['reg'] + r['pred']


@pytest.mark.parametrize('world', [1, 2])
@pytest.mark.parametrize('D', [16, 32])
def test_l2_chunk_plan(D, world):
    from voxvae import train as T
    assert T.ADAM_CHUNK == ADAM_CHUNK
    _, _, _, names = _model_shapes(D)
    lam = 5e-4
    plan = T.adam_l2_plan(names, lam, world)
    assert plan['n'].min() >= 1 and plan['n'].max() <= ADAM_CHUNK
    covered = [np.zeros(int(np.prod(s)), dtype=np.int64) for _, s in names]
    for rec in plan:
        covered[rec['var']][rec['offset']:rec['offset'] + rec['n']] += 1
        name = names[rec['var']][0]
        want = np.float32(2 * lam * world) if (name.endswith('/kernel') or name == 'dec/dense/bias') else np.float32(0)
        assert rec['coef'] == want, name
    assert all((c == 1).all() for c in covered)                         # every element of every variable in exactly one chunk
    assert len(plan) == sum((c.size + ADAM_CHUNK - 1) // ADAM_CHUNK for c in covered)
    assert (np.diff(plan['var']) >= 0).all()                            # table order = the trainer's order
    reg = {names[v][0] for v in np.unique(plan['var'][plan['coef'] != 0])}
    assert reg == {n for n, _ in names if ref.regularised(n)} and 'dec/dense/bias' in reg and not any('/bn' in n for n in reg)
    # the device table: pointers offset by 4 bytes per element, n, the coefficient's float32 bits in the low half of the sixth word
    ptrs = [(1000000 * (k + 1), 2000000000 + 16 * k, 3000000000 + 16 * k, 4000000000 + 16 * k) for k in range(len(names))]
    table = T.adam_l2_table(plan, ptrs)
    assert table.dtype == np.int64 and table.shape == (len(plan), 6)
    raw = table.tobytes()
    for i in (0, len(plan) // 2, len(plan) - 1):
        rec = np.frombuffer(raw[48 * i:48 * i + 48], dtype=np.dtype([('p', '<u8'), ('g', '<u8'), ('m', '<u8'), ('v', '<u8'), ('n', '<i8'), ('coef', '<f4'), ('pad', '<f4')]))[0]
        q = ptrs[plan['var'][i]]
        assert (rec['p'], rec['g'], rec['m'], rec['v']) == tuple(a + 4 * int(plan['offset'][i]) for a in q)
        assert rec['n'] == plan['n'][i] and rec['coef'] == plan['coef'][i] and rec['pad'] == 0


def test_constructor_refuses_mismatched_latent_and_replica_count():
    import src.module.AE3D as AE3D
    from voxvae import synthetic as syn
    wide = syn.make_config(64, 400, False)['encoder']
    with pytest.raises(ValueError, match='400'):                        # the reference's in-file example: 400 against 200
        AE3D.AE3D(wide, syn.make_config(64, 200, False)['decoder'])
    assert AE3D.encoder_structure['filter_num_list'][-1] == AE3D.decoder_structure['input_dim'] == 200
    cfg = syn.make_config(16, 16, False)

    class TwoReplicas:
        num_replicas_in_sync = 2

        def scope(self):
            raise AssertionError('the model must not be built')

    with pytest.raises(ValueError, match='2'):                          # no process group: one rank
        AE3D.AE3D(cfg['encoder'], cfg['decoder'], strategy=TwoReplicas())


@pytest.mark.skipif(torch.cuda.is_available(), reason='checks the no-GPU failure mode')
def test_consistent_structures_fail_loudly_without_gpu():
    import src.module.AE3D as AE3D
    from voxvae import lib as L
    from voxvae import synthetic as syn
    from voxvae.train import ReplicaStrategy
    s = ReplicaStrategy()
    assert s.num_replicas_in_sync == 1
    with s.scope():
        pass
    cfg = syn.make_config(16, 16, False)
    with pytest.raises(L.VoxVaeError):
        AE3D.AE3D(cfg['encoder'], cfg['decoder'], strategy=s)


def test_precision_and_recall_come_from_the_summed_counts():
    """AE3D.py:98-103: TP / FP / FN summed over the global batch, then the ratios -- not the batch mean of per-sample ratios."""
    import src.module.AE3D as AE3D
    stats = np.array([[10.0, 90, 10, 10], [20.0, 1, 9, 0], [5.0, 0, 0, 50], [7.0, 300, 0, 100]])      # (bce, TP, FP, FN) per sample
    gb = 4.0
    TP, FP, FN = (torch.tensor(stats[:, k].sum() / gb, dtype=torch.float64) for k in (1, 2, 3))
    p, r = AE3D.AE3D._precision_recall(TP, FP, FN)
    tp, fp, fn = stats[:, 1].sum() / gb, stats[:, 2].sum() / gb, stats[:, 3].sum() / gb
    assert float(p) == tp / (tp + fp + 1e-10) and float(r) == tp / (tp + fn + 1e-10)
    assert abs(float(p) - 391.0 / 410.0) < 1e-9 and abs(float(r) - 391.0 / 551.0) < 1e-9
    mean_p = np.mean(stats[:, 1] / (stats[:, 1] + stats[:, 2] + 1e-10))
    mean_r = np.mean(stats[:, 1] / (stats[:, 1] + stats[:, 3] + 1e-10))
    assert abs(float(p) - mean_p) > 0.2 and abs(float(r) - mean_r) > 0.04
