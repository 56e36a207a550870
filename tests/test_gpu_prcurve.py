"""GPU tests of the precision / recall-vs-threshold counts (csrc/pr_curve.hip, voxvae/prcurve.py, getPRCurve, test_modelnet_PR.py).

The oracle is numpy on the same float32 arrays with float32 thresholds, written as modelnetAE3.ipynb cell 2 writes it
(`np.where(yPred > prob, 1.0, 0.0)`, `np.sum(yTarget * yPred_t)` ...).  The kernel counts integers, so EVERY comparison of counts in this
file is exact integer equality: there is no tolerance anywhere but in the one cross-check against getEval's float32 batch means, whose
bound is derived there.

The data hold what the compare turns on: uniform values, saturated sigmoids (float32 sigmoid reaches exactly 1.0), every threshold
itself with its float32 neighbour below and above, 0, 1, a denormal, and NaN planted in occupied and in empty voxels.  The shapes make
rows start unaligned (27 voxels, packed rows of 513 bytes), leave ragged slots at both ends of a row, split a sample over several
workgroups with a ragged last piece, and cover the threshold-count range 1 .. 256 (more than one 64-threshold register chunk)."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from oracle import numpy_oracle as no

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, 'anytime-3d-reconstruction_amd')
DEV = 'cuda:0'
F32 = np.float32
DENORMAL = F32(1e-41)


@pytest.fixture(scope='module')
def L():
    from voxvae import lib
    lib.load()
    assert torch.cuda.is_available()
    return lib


def _st():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


# ------------------------------------------------------------------------------------------------ oracle and data
def notebook_counts(y, p, thresholds, inclusive=None, per_sample=False):
    """modelnetAE3.ipynb cell 2, per threshold: TP = sum(y * [p > t]), FP = sum((1 - y) * [p > t]), FN = sum(y * (1 - [p > t])), in the
    notebook's float arithmetic (float64 sums of {0,1} products: exact), with np.float32 thresholds; `inclusive` entries use the
    `np.greater_equal` of its thinning rows.  -> int64 [T, 3] pooled, or [B, T, 3]."""
    y = np.asarray(y, dtype=F32).reshape(len(y), -1)
    p = np.asarray(p, dtype=F32).reshape(len(p), -1)
    inclusive = [False] * len(thresholds) if inclusive is None else list(inclusive)
    ax = 1 if per_sample else None
    out = []
    for t, inc in zip(thresholds, inclusive):
        t32 = F32(t)
        pt = np.greater_equal(p, t32) * 1.0 if inc else np.where(p > t32, 1.0, 0.0)
        out.append([np.sum(y * pt, axis=ax), np.sum((1.0 - y) * pt, axis=ax), np.sum(y * (1.0 - pt), axis=ax)])
    out = np.array(out, dtype=np.float64)                       # [T, 3] or [T, 3, B]
    assert np.array_equal(out, np.round(out))
    out = out.astype(np.int64)
    return np.moveaxis(out, 2, 0) if per_sample else out


def make_target(rng, B, V):
    return (rng.random((B, V)) < 0.3).astype(F32)


def make_probs(rng, y, thresholds):
    """float32 probabilities as tests/test_gpu_latent_ops.py makes them, for a list of thresholds, plus NaN in both classes."""
    B, V = y.shape
    p = rng.random((B, V)).astype(F32)
    sat = no.sigmoid(rng.normal(0.0, 12.0, (B, V)).astype(F32)).astype(F32)
    r = rng.random((B, V))
    p = np.where(r < 0.3, sat, p).astype(F32)
    special = [F32(0.0), F32(1.0), DENORMAL, F32(1.0) - F32(1e-7), F32(np.nan)]
    for t in thresholds:
        t32 = F32(t)
        special += [t32, np.nextafter(t32, F32(-np.inf)), np.nextafter(t32, F32(np.inf))]
    special = np.array(special, dtype=F32)
    pick = (r >= 0.3) & (r < 0.6)                               # a third of the voxels: one of the special values, evenly
    p[pick] = special[rng.integers(0, len(special), int(pick.sum()))]
    flat, yf = p.reshape(-1), y.reshape(-1)
    for k in range(min(flat.size, len(special))):               # also in the smallest cases
        flat[k] = special[(k * 7 + 1) % len(special)]
    for cls in (0.0, 1.0):                                      # NaN in an occupied and in an empty voxel, wherever there is one
        idx = np.nonzero(yf == cls)[0]
        if idx.size > 1:
            flat[idx[idx.size // 2]] = np.nan
    return p


def thresholds_for(T, rng):
    from voxvae.prcurve import notebook_thresholds
    if T == 1:
        return [0.5], [False]
    if T == 3:
        return [0.9, 0.2, 0.5], [False, True, False]
    if T == 19:
        return notebook_thresholds(20), [False] * 19
    if T == 59:
        return notebook_thresholds(20, full=True), [False] * 59
    assert T == 256
    thr = list(rng.random(200)) + notebook_thresholds(10, full=True) + [0.0, 1.0, 1.0, 0.5, 0.5, float(DENORMAL), -1.0, 2.0]
    thr += list(rng.random(256 - len(thr)))
    order = rng.permutation(256)
    return [thr[i] for i in order], list(rng.random(256) < 0.5)


def check_counts(got, y, p, thr, inc, what=''):
    want = notebook_counts(y, p, thr, inc)
    for k, name in enumerate(('TP', 'FP', 'FN')):
        assert np.array_equal(got[name][0], want[:, k]), '%s %s: first difference at threshold %d' % (
            what, name, int(np.nonzero(got[name][0] != want[:, k])[0][0]))
    assert int(got['occupied'][0]) == int(y.sum()) and int(got['voxels'][0]) == y.size


# ------------------------------------------------------------------------------------------------ shapes
SHAPES = [(1, 1, 1, False), (3, 27, 19, False), (5, 4096, 59, False), (5, 4096, 59, True), (2, 8, 3, True), (7, 4104, 19, True),
          (3, 40000, 256, False), (2, 32768, 19, True)]


@pytest.mark.parametrize('B,V,T,packed', SHAPES)
def test_counts_equal_the_notebook(L, B, V, T, packed):
    from voxvae.hostio import pack_voxels
    from voxvae.prcurve import PRCurve
    rng = np.random.default_rng(B * 1000003 + V * 17 + T)
    thr, inc = thresholds_for(T, rng)
    y = make_target(rng, B, V)
    p = make_probs(rng, y, thr)
    c = PRCurve(thr, inc, device=DEV)
    c.update(pack_voxels(y) if packed else y, p)
    check_counts(c.counts(), y, p, thr, inc)
    pr = c.precision_recall()
    w = notebook_counts(y, p, thr, inc).astype(np.float64)
    assert np.array_equal(pr[0, :, 0], w[:, 0] / (w[:, 0] + w[:, 1] + 1e-10)) and np.array_equal(pr[0, :, 1], w[:, 0] / (w[:, 0] + w[:, 2] + 1e-10))


def test_counts_at_the_workload_size(L):
    """One call at (256, 32768, 59): more work items than one wave of workgroups.  The notebook's float form is 59 float64 passes over
    8.4 M voxels; for {0,1} targets it equals the boolean form used here, which is asserted on a small batch first."""
    from voxvae.prcurve import PRCurve, notebook_thresholds
    rng = np.random.default_rng(59)
    thr = notebook_thresholds(20, full=True)
    B, V = 256, 32768
    y = make_target(rng, B, V)
    p = make_probs(rng, y, thr)
    yb = y > 0.5

    def boolean_counts(yb, p):
        out = []
        for t in thr:
            m = p > F32(t)
            tp = int(np.count_nonzero(m & yb))
            out.append([tp, int(np.count_nonzero(m)) - tp, int(yb.sum()) - tp])
        return np.array(out, dtype=np.int64)

    assert np.array_equal(boolean_counts(yb[:3], p[:3]), notebook_counts(y[:3], p[:3], thr))
    c = PRCurve(thr, device=DEV).update(torch.from_numpy(y).to(DEV), torch.from_numpy(p).to(DEV))
    got, want = c.counts(), boolean_counts(yb, p)
    assert np.array_equal(got['TP'][0], want[:, 0]) and np.array_equal(got['FP'][0], want[:, 1]) and np.array_equal(got['FN'][0], want[:, 2])
    assert int(got['occupied'][0]) == int(yb.sum()) and int(got['voxels'][0]) == B * V


@pytest.mark.parametrize('off_p,off_t', [(1, 1), (3, 3), (1, 2), (0, 3), (2, 0)])
def test_unaligned_base_pointers(L, off_p, off_t):
    """Rows need no alignment beyond a float's: the same data at base pointers 4, 8 and 12 bytes into a 16-byte line, with the target at
    the same offset as the prediction (it shares the 16-byte loads) and at another one (it does not)."""
    from voxvae.prcurve import PRCurve, notebook_thresholds
    rng = np.random.default_rng(100 + 4 * off_p + off_t)
    B, V = 3, 4099
    thr = notebook_thresholds(20)
    y = make_target(rng, B, V)
    p = make_probs(rng, y, thr)
    bp = torch.full((B * V + 8,), float('nan'), dtype=torch.float32, device=DEV)
    bt = torch.full((B * V + 8,), 1.0, dtype=torch.float32, device=DEV)
    bp[off_p:off_p + B * V] = torch.from_numpy(p.reshape(-1)).to(DEV)
    bt[off_t:off_t + B * V] = torch.from_numpy(y.reshape(-1)).to(DEV)
    pv, tv = bp[off_p:off_p + B * V].view(B, V), bt[off_t:off_t + B * V].view(B, V)
    assert pv.data_ptr() % 16 == 4 * off_p and tv.data_ptr() % 16 == 4 * off_t
    c = PRCurve(thr, device=DEV).update(tv, pv)
    check_counts(c.counts(), y, p, thr, None)


@pytest.mark.parametrize('pval,yval', [(0.0, None), (1.0, None), (None, 0.0), (None, 1.0), (0.0, 1.0), (1.0, 0.0)])
@pytest.mark.parametrize('packed', [False, True])
def test_degenerate_grids(L, pval, yval, packed):
    from voxvae.hostio import pack_voxels
    from voxvae.prcurve import notebook_curve
    rng = np.random.default_rng(5)
    B, V = 3, 4104
    c = notebook_curve(20, full=True, device=DEV)
    thr, inc = list(c.thresholds), list(c.inclusive)
    y = make_target(rng, B, V) if yval is None else np.full((B, V), yval, dtype=F32)
    p = make_probs(rng, y, thr) if pval is None else np.full((B, V), pval, dtype=F32)
    c.update(pack_voxels(y) if packed else y, p)
    check_counts(c.counts(), y, p, thr, inc)


# ------------------------------------------------------------------------------------------------ accumulation
def test_two_updates_equal_one_and_reset_zeroes(L):
    from voxvae.prcurve import PRCurve, notebook_thresholds
    rng = np.random.default_rng(77)
    thr = notebook_thresholds(20)
    y = make_target(rng, 9, 5000)
    p = make_probs(rng, y, thr)
    one = PRCurve(thr, device=DEV).update(y, p).counts()
    c = PRCurve(thr, device=DEV)
    two = c.update(y[:4], p[:4]).update(y[4:], p[4:]).counts()
    for k in one:
        assert np.array_equal(one[k], two[k]), k
    check_counts(two, y, p, thr, None)
    other = PRCurve(thr, device=DEV).update(y[:4], p[:4])
    merged = PRCurve(thr, device=DEV).update(y[4:], p[4:]).merge(other).counts()
    for k in one:
        assert np.array_equal(one[k], merged[k]), k
    c.reset()
    assert not any(v.any() for v in c.counts().values())
    check_counts(c.update(y, p).counts(), y, p, thr, None)      # and it counts again from zero


# ------------------------------------------------------------------------------------------------ groups
def test_groups_out_of_range_samples_count_nowhere_and_write_nowhere(L):
    """40 classes, labels in [-1, 40]: the samples labelled -1 and 40 appear in no count, and nothing is written outside
    [G][T][2] / [G][2] (the accumulators sit between guard regions)."""
    from voxvae.prcurve import notebook_thresholds
    rng = np.random.default_rng(40)
    B, V, G = 300, 520, 40
    thr = sorted(notebook_thresholds(20))
    T = len(thr)
    y = make_target(rng, B, V)
    p = make_probs(rng, y, thr)
    labels = rng.integers(-1, G + 1, B).astype(np.int32)
    labels[:4] = [-1, G, 0, G - 1]
    assert (labels == -1).sum() >= 1 and (labels == G).sum() >= 1
    GUARD, SENT, START = 1024, -7777, 5
    acc = torch.full((GUARD + G * T * 2 + GUARD,), SENT, dtype=torch.int64, device=DEV)
    tot = torch.full((GUARD + G * 2 + GUARD,), SENT, dtype=torch.int64, device=DEV)
    acc[GUARD:GUARD + G * T * 2] = START                        # the outputs are ADDED to
    tot[GUARD:GUARD + G * 2] = START
    pd, yd, td, gd = (torch.from_numpy(a).to(DEV) for a in (p, y, np.array(thr, dtype=F32), labels))
    need = L.load().vv_pr_curve_workspace_bytes(B, V, T)
    ws = torch.empty(need, dtype=torch.uint8, device=DEV)
    L.call('vv_pr_curve_accumulate', L.ptr(pd), L.ptr(yd), 0, L.ptr(td), T, 1, L.ptr(gd), G, L.ptr(acc[GUARD:]), L.ptr(tot[GUARD:]),
           L.ptr(ws), need, B, V, _st())
    torch.cuda.synchronize()
    acc, tot = acc.cpu().numpy(), tot.cpu().numpy()
    assert (acc[:GUARD] == SENT).all() and (acc[GUARD + G * T * 2:] == SENT).all()
    assert (tot[:GUARD] == SENT).all() and (tot[GUARD + G * 2:] == SENT).all()
    tp_fp = acc[GUARD:GUARD + G * T * 2].reshape(G, T, 2) - START
    totals = tot[GUARD:GUARD + G * 2].reshape(G, 2) - START
    for g in range(G):
        sel = labels == g
        want = notebook_counts(y[sel], p[sel], thr) if sel.any() else np.zeros((T, 3), dtype=np.int64)
        assert np.array_equal(tp_fp[g], want[:, :2]), g
        assert totals[g].tolist() == [int(y[sel].sum()), int(sel.sum()) * V], g
    inside = (labels >= 0) & (labels < G)
    assert int(totals[:, 1].sum()) == int(inside.sum()) * V < B * V


def test_group_per_sample_and_one_hot(L):
    from voxvae.prcurve import PRCurve
    from voxvae.tensor import DeviceArray
    rng = np.random.default_rng(12)
    B, V = 70, 1000
    thr, inc = [0.5, 0.1, 0.99, 0.5], [True, False, False, False]
    y = make_target(rng, B, V)
    p = make_probs(rng, y, thr)
    got = PRCurve(thr, inc, groups=B, device=DEV).update(y, p, group=np.arange(B)).counts()
    want = notebook_counts(y, p, thr, inc, per_sample=True)
    assert np.array_equal(got['TP'], want[:, :, 0]) and np.array_equal(got['FP'], want[:, :, 1]) and np.array_equal(got['FN'], want[:, :, 2])
    assert np.array_equal(got['occupied'], y.sum(axis=1).astype(np.int64)) and (got['voxels'] == V).all()
    G = 40
    labels = rng.integers(0, G, B)
    onehot = np.eye(G, dtype=F32)[labels]
    a = PRCurve(thr, inc, groups=G, device=DEV).update(y, p, group=labels).counts()
    for form in (onehot, torch.from_numpy(onehot).to(DEV), DeviceArray(torch.from_numpy(onehot).to(DEV)), torch.from_numpy(labels).to(DEV)):
        b = PRCurve(thr, inc, groups=G, device=DEV).update(y, p, group=form).counts()
        for k in a:
            assert np.array_equal(a[k], b[k]), k
    assert int(a['voxels'].sum()) == B * V
    pooled = PRCurve(thr, inc, device=DEV).update(y, p).counts()
    assert np.array_equal(a['TP'].sum(axis=0), pooled['TP'][0]) and np.array_equal(a['FP'].sum(axis=0), pooled['FP'][0])


# ------------------------------------------------------------------------------------------------ threshold order
def test_unsorted_thresholds_through_the_c_call(L):
    """sorted = 0 with the thresholds in any order gives, threshold by threshold, what sorted = 1 gives for the sorted list."""
    rng = np.random.default_rng(3)
    B, V = 4, 9000
    thr = np.array([0.9, 0.1, 0.5, 0.9, 1.0, 0.0, 0.3, 1e-41, 0.1, 0.999], dtype=F32)
    order = np.argsort(thr, kind='stable')
    T = len(thr)
    y = make_target(rng, B, V)
    p = make_probs(rng, y, list(thr))
    pd, yd = torch.from_numpy(p).to(DEV), torch.from_numpy(y).to(DEV)
    need = L.load().vv_pr_curve_workspace_bytes(B, V, T)
    ws = torch.empty(need, dtype=torch.uint8, device=DEV)

    def run(t, is_sorted):
        td = torch.from_numpy(np.ascontiguousarray(t)).to(DEV)
        acc = torch.zeros(T * 2, dtype=torch.int64, device=DEV)
        tot = torch.zeros(2, dtype=torch.int64, device=DEV)
        L.call('vv_pr_curve_accumulate', L.ptr(pd), L.ptr(yd), 0, L.ptr(td), T, is_sorted, None, 1, L.ptr(acc), L.ptr(tot), L.ptr(ws), need,
               B, V, _st())
        torch.cuda.synchronize()
        return acc.cpu().numpy().reshape(T, 2), tot.cpu().numpy()

    a, ta = run(thr, 0)
    b, tb = run(thr[order], 1)
    c, _ = run(thr[order], 0)
    assert np.array_equal(a[order], b) and np.array_equal(b, c) and np.array_equal(ta, tb)
    assert np.array_equal(a, notebook_counts(y, p, list(thr))[:, :2])


# ------------------------------------------------------------------------------------------------ input forms
def test_input_forms_give_identical_counts(L):
    from voxvae.hostio import HostPrediction, pack_voxels
    from voxvae.prcurve import PRCurve
    from voxvae.tensor import DeviceArray
    rng = np.random.default_rng(8)
    B, D = 3, 16
    thr = [0.25, 0.5, 0.75]
    y = make_target(rng, B, D ** 3)
    p = make_probs(rng, y, thr)
    y5, p5 = y.reshape(B, D, D, D, 1), p.reshape(B, D, D, D, 1)
    pt, yt = torch.from_numpy(p5).to(DEV), torch.from_numpy(y5).to(DEV)
    base = PRCurve(thr, device=DEV).update(y5, p5).counts()
    check_counts(base, y, p, thr, None)
    forms = [(yt, pt), (DeviceArray(yt), DeviceArray(pt)), (y5, HostPrediction(p5.copy(), [pt[:2], pt[2:]])), (pack_voxels(y5), pt),
             (pack_voxels(y5), p5), (yt.double(), pt)]
    for t, q in forms:
        got = PRCurve(thr, device=DEV).update(t, q).counts()
        for k in base:
            assert np.array_equal(base[k], got[k]), (type(t).__name__, type(q).__name__, k)
    with pytest.raises(ValueError):
        PRCurve(thr, device=DEV).update(y5[:2], p5)


def test_function_curve_at_one_threshold_equals_voxelPrecisionRecall(L):
    import voxvae
    voxvae.set_default_device(DEV)
    import src.module.function as fn
    rng = np.random.default_rng(21)
    B, V = 6, 32 ** 3
    for prob in (0.5, 0.3):
        y = make_target(rng, B, V)
        p = make_probs(rng, y, [prob])
        p[np.isnan(p)] = prob                                   # the float-product kernel of the sibling turns a NaN into a NaN sum
        a = fn.voxelPrecisionRecall(y, p, prob)
        b = fn.voxelPrecisionRecallCurve(y, p, [prob])
        for u, v in zip(a, b):
            u, v = np.array(u), np.array(v)
            assert v.shape == (B, 1) and v.dtype == np.float32 and np.array_equal(u, v[:, 0])
    many = fn.voxelPrecisionRecallCurve(y, p, [0.9, 0.1, 0.5], inclusive=False)
    want = notebook_counts(y, p, [0.9, 0.1, 0.5], per_sample=True)
    for k in range(3):
        assert np.array_equal(np.array(many[k]), want[:, :, k].astype(F32))


# ------------------------------------------------------------------------------------------------ end to end, trained operating point
@pytest.fixture(scope='module')
def trained():
    from voxvae import synthetic as syn
    from voxvae import trained as tr
    cfg, ep, dp, info = tr.train_operating_point(device=DEV)
    assert info['reached'], info
    B = 64
    x = np.concatenate([syn.make_voxels(256, 32, seed=4321)[:48], syn.make_voxels(16, 32, seed=777)], axis=0)
    rng = np.random.default_rng(99)
    return dict(cfg=cfg, ep=ep, dp=dp, x=x, B=B, eps=syn.make_eps(B, 64, seed=70), eps2=syn.make_eps(B, 64, seed=71),
                mask=syn.make_mask(B, 64, 0.9), onehot=syn.make_onehot(B, 40), cats=syn.make_category_vectors(40, 64),
                epsK=rng.standard_normal((B, 8, 64)).astype(F32))


def _model(t, dtype):
    import voxvae
    voxvae.set_default_dtype(dtype)
    voxvae.set_default_device(DEV)
    import src.module.nolbo as nolbo
    m = nolbo.nolboSingleObject_modelnet_category_VAE(nolbo_structure=t['cfg'])
    m._encoder.set_weights_dict(t['ep'])
    m._decoder.set_weights_dict(t['dp'])
    return m


def _same_tuple(a, b):
    assert len(a) == len(b)
    for u, v in zip(a, b):
        assert np.array_equal(np.array(u), np.array(v))


@pytest.mark.parametrize('dtype', ['f32', 'bf16'])
def test_getPRCurve_equals_the_notebook_on_the_trained_model(L, trained, dtype):
    import voxvae
    from voxvae.prcurve import notebook_curve
    t = trained
    try:
        m = _model(t, dtype)
        x, y2 = t['x'], t['x'].reshape(t['B'], -1)
        inputs = (x, x, t['onehot'])
        new = lambda: notebook_curve(20, full=True, device=DEV)
        thr, inc = list(new().thresholds), list(new().inclusive)
        # missing_prob 0
        c = new()
        out = m.getPRCurve(inputs, c, category_vectors=t['cats'], _eps=t['eps'])
        _same_tuple(out, m.getEval(inputs, category_vectors=t['cats'], _eps=t['eps']))
        pred = np.array(out[0])
        check_counts(c.counts(), y2, pred.reshape(t['B'], -1), thr, inc, dtype)
        assert c.counts()['TP'][0, -1] > 0, 'the >= 1.0 row is empty: not a trained operating point'
        # missing_prob 0.9: both curves
        c, cc = new(), new()
        kw = dict(category_vectors=t['cats'], missing_prob=0.9, _eps=t['eps'], _mask=t['mask'], _eps2=t['eps2'])
        out = m.getPRCurve(inputs, c, corrected=cc, **kw)
        _same_tuple(out, m.getEval(inputs, **kw))
        check_counts(c.counts(), y2, np.array(out[0]).reshape(t['B'], -1), thr, inc, dtype + ' missing')
        check_counts(cc.counts(), y2, np.array(out[5]).reshape(t['B'], -1), thr, inc, dtype + ' corrected')
        # the sampled-mean reconstruction
        c = new()
        out = m.getPRCurve((x, x), c, sampling_num=8, _eps=t['epsK'])
        _same_tuple(out, m.getSampledEval((x, x), 8, _eps=t['epsK']))
        check_counts(c.counts(), y2, np.array(out[0]).reshape(t['B'], -1), thr, inc, dtype + ' sampled')
    finally:
        voxvae.set_default_dtype('f32')


def test_per_sample_counts_agree_with_getEval_batch_means(L, trained):
    """Per-sample groups at the single inclusive threshold 0.5: the batch means of TP / (TP + FP + 1e-10) and TP / (TP + FN + 1e-10) in
    float64 from the new counts against getEval's pr / rc.  That side is, per sample, a float32 add and a divide of exactly
    representable counts, then a B-term float32 mean: (B + 3) 2^-24 relative."""
    from voxvae.prcurve import PRCurve
    t = trained
    m = _model(t, 'f32')
    B = t['B']
    c = PRCurve([0.5], inclusive=True, groups=B, device=DEV)
    out = m.getPRCurve((t['x'], t['x'], t['onehot']), c, category_vectors=t['cats'], _eps=t['eps'], group=np.arange(B))
    n = c.counts()
    tp, fp, fn = (n[k][:, 0].astype(np.float64) for k in ('TP', 'FP', 'FN'))
    pr, rc = float(np.mean(tp / (tp + fp + 1e-10))), float(np.mean(tp / (tp + fn + 1e-10)))
    tol = (B + 3) * 2.0 ** -24
    print('\n[pr / rc] counts %.9f %.9f  getEval %.9f %.9f  bound %.2e relative' % (pr, rc, float(out[2]), float(out[3]), tol))
    assert abs(pr - float(out[2])) <= tol * pr and abs(rc - float(out[3])) <= tol * rc


# ------------------------------------------------------------------------------------------------ the entry script
def test_entry_script_tables_equal_the_notebook_on_its_own_dumps(tmp_path):
    out_dir, dump_dir = str(tmp_path / 'out'), str(tmp_path / 'dump')
    env = dict(os.environ)
    env.pop('VV_FINAL_BCE', None)
    r = subprocess.run([sys.executable, 'test_modelnet_PR.py', '--voxel', '32', '--batch', '8', '--max-iter', '2', '--missing-pr', '0.9',
                        '--out-dir', out_dir, '--dump-dir', dump_dir], cwd=PKG, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                       text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    from voxvae.prcurve import notebook_thresholds
    div = 20
    thr = notebook_thresholds(div)
    gt = np.load(os.path.join(dump_dir, '0.9_gt.npy'))
    assert gt.shape == (16, 32, 32, 32, 1)
    for stem, dump in (('0.9_pr_preds', '0.9_pred.npy'), ('0.9_pr_preds_corrected', '0.9_pred_corrected.npy')):
        table = np.load(os.path.join(out_dir, stem + '.npy'))
        assert table.shape == (len(thr) + div, 2) and table.dtype == np.float64
        pred = np.load(os.path.join(dump_dir, dump))
        n = notebook_counts(gt, pred, thr + [1.0], [False] * len(thr) + [True]).astype(np.float64)
        want = np.stack([n[:, 0] / (n[:, 0] + n[:, 1] + 1e-10), n[:, 0] / (n[:, 0] + n[:, 2] + 1e-10)], axis=1)
        assert np.array_equal(table[:len(thr)], want[:len(thr)]), stem
        occ, tp1, fp1 = float(gt.sum()), n[-1, 0], n[-1, 1]
        for i in range(div):                                    # the thinning rows: the expectation of the notebook's random mask
            a = 0.1 ** i
            tp, fp = a * tp1, a * fp1
            assert table[len(thr) + i, 0] == tp / (tp + fp + 1e-10) and table[len(thr) + i, 1] == tp / (tp + (occ - tp) + 1e-10), (stem, i)
        assert np.array_equal(np.loadtxt(os.path.join(out_dir, stem + '.txt')), table)
