"""CPU tests of the precision / recall curve's host side (voxvae/prcurve.py) and of the argument checks of its C entry points
(include/voxvae.h: vv_pr_curve_workspace_bytes, vv_pr_curve_accumulate), which refuse before any launch and so need no GPU."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, 'anytime-3d-reconstruction_amd')
for _p in (ROOT, PKG):           # also in the processes mp.spawn starts, which import this module without the suite's conftest
    if _p not in sys.path:
        sys.path.insert(0, _p)

from voxvae import prcurve as P

F32 = np.float32
DENORMAL = 1e-41                     # the smallest entry of the notebook's commented list; a float32 denormal


# ------------------------------------------------------------------------------------------------ thresholds
def test_thresholds_are_sorted_as_float32_and_results_come_back_in_the_callers_order():
    thr = [0.9, 0.1, 0.5, 0.9, 0.3, 0.1]                         # unsorted, duplicates (the notebook's own list holds 0.9 twice)
    eff, order, inverse = P.normalise_thresholds(thr)
    assert eff.dtype == np.float32 and np.array_equal(eff, np.array(thr, dtype=F32))
    s = eff[order]
    assert np.all(s[1:] >= s[:-1])
    assert np.array_equal(s[inverse], eff)                        # position j of the caller <- sorted position inverse[j]
    assert sorted(order.tolist()) == list(range(6))
    c = P.PRCurve(thr, device='cpu')
    # injected counts in the caller's order survive the trip through the sorted storage
    tp = np.array([[5, 50, 20, 5, 30, 50]])
    fp = np.array([[1, 10, 4, 1, 6, 10]])
    c.set_counts(tp, fp, [60], [1000])
    stored = c._split(c._acc.numpy())[0][0]
    assert np.array_equal(stored[:, 0], np.array([50, 50, 30, 20, 5, 5]))          # sorted thresholds: non-increasing counts
    got = c.counts()
    assert np.array_equal(got['TP'], tp) and np.array_equal(got['FP'], fp) and np.array_equal(got['FN'], 60 - tp)
    assert got['occupied'].tolist() == [60] and got['voxels'].tolist() == [1000]
    assert all(got[k].dtype == np.int64 for k in got)


@pytest.mark.parametrize('t', [0.0, 0.5, 1.0, DENORMAL])
def test_inclusive_threshold_is_the_float32_predecessor(t):
    t32 = F32(t)
    eff, _, _ = P.normalise_thresholds([t, t], [True, False])
    assert eff[1] == t32 and eff[0] == np.nextafter(t32, F32(-np.inf)) and eff[0] < t32
    # p >= t  <=>  p > predecessor(t), on both float32 neighbours of t, t itself, and the usual suspects
    with np.errstate(invalid='ignore'):
        ps = np.array([t32, np.nextafter(t32, F32(-np.inf)), np.nextafter(t32, F32(np.inf)), 0.0, -0.0, 1.0, DENORMAL, -DENORMAL, np.nan,
                       np.inf, -np.inf], dtype=F32)
        assert np.array_equal(ps >= t32, ps > eff[0])
        assert np.array_equal(ps > t32, ps > eff[1])
    if t == 0.0:
        assert eff[0] < 0 and abs(float(eff[0])) < 2e-45          # the largest negative denormal, not -0.0
    if t == DENORMAL:
        assert 0 < eff[0] < 1.2e-38                               # stays a denormal: nothing is flushed on the host


def test_threshold_count_limits_and_per_threshold_inclusive():
    with pytest.raises(ValueError):
        P.PRCurve([], device='cpu')
    with pytest.raises(ValueError):
        P.PRCurve(np.linspace(0, 1, 257), device='cpu')
    c = P.PRCurve(np.linspace(0, 1, 256), inclusive=True, device='cpu')
    assert c.T == 256 and c.inclusive.all()
    with pytest.raises(ValueError):
        P.PRCurve([0.5], groups=0, device='cpu')


def test_notebook_thresholds_against_the_lists_the_notebook_prints():
    """modelnetAE3.ipynb cell 0 prints r1 + r2 + r3 for div = 10 (%e with 8 decimals); cell 2's active list is r2."""
    printed = [1e-41, 1e-37, 1e-33, 1e-29, 1e-25, 1e-21, 1e-17, 1e-13, 1e-09, 1e-05,
               0.1, 0.2, 0.3, 0.4, 0.5, 0.6, 0.7, 0.8, 0.9,
               0.9, 0.99, 0.999, 0.9999, 0.99999, 0.999999, 0.9999999, 0.99999999, 0.999999999, 1.0]
    full = P.notebook_thresholds(10, full=True)
    assert len(full) == 29
    assert ['%.8e' % v for v in full] == ['%.8e' % v for v in printed]
    assert P.notebook_thresholds(10) == [(i + 1) * 1.0 / 10 for i in range(9)] == full[10:19]
    assert len(P.notebook_thresholds(20)) == 19 and len(P.notebook_thresholds(20, full=True)) == 59
    c = P.notebook_curve(10, full=True, device='cpu')
    assert c.T == 30 and c.thresholds[-1] == 1.0 and c.inclusive.tolist() == [False] * 29 + [True]
    assert 0 < c._eff[c._order][0] < 1.2e-38                      # 1e-41 reaches the kernel as a denormal


# ------------------------------------------------------------------------------------------------ tables from injected counts
def _injected(div=4):
    c = P.notebook_curve(div, device='cpu')                       # thresholds 1/4, 2/4, 3/4, then the inclusive 1.0
    tp = np.array([[900, 800, 700, 500]])
    fp = np.array([[300, 200, 100, 40]])
    return c.set_counts(tp, fp, [1000], [32768]), tp[0].astype(float), fp[0].astype(float)


def test_precision_recall_and_the_expectation_rows():
    c, tp, fp = _injected()
    pr = c.precision_recall()
    assert pr.shape == (1, 4, 2) and pr.dtype == np.float64
    assert np.array_equal(pr[0, :, 0], tp / (tp + fp + 1e-10)) and np.array_equal(pr[0, :, 1], tp / (tp + (1000 - tp) + 1e-10))
    tab = P.notebook_table(c, 4)
    assert tab.shape == (3 + 4, 2)
    assert np.array_equal(tab[:3], pr[0, :3])
    for i in range(4):
        a = 0.1 ** i
        t, f = a * 500, a * 40
        assert tab[3 + i, 0] == t / (t + f + 1e-10) and tab[3 + i, 1] == t / (t + (1000 - t) + 1e-10)
    assert np.array_equal(tab[3], pr[0, 3])                       # a = 1: the plain >= 1.0 row


def test_binomial_rows_under_a_fixed_rng():
    c, _, _ = _injected()
    tab = P.notebook_table(c, 4, rng=np.random.default_rng(7))
    rng = np.random.default_rng(7)
    for i in range(4):
        t, f = float(rng.binomial(500, 0.1 ** i)), float(rng.binomial(40, 0.1 ** i))
        assert tab[3 + i, 0] == t / (t + f + 1e-10) and tab[3 + i, 1] == t / (t + (1000 - t) + 1e-10)
    assert np.array_equal(tab[3], P.notebook_table(c, 4)[3])      # Binomial(n, 1) = n
    assert np.array_equal(tab[:3], P.notebook_table(c, 4)[:3])


def test_guards_at_zero_counts():
    c = P.notebook_curve(3, device='cpu')
    assert np.array_equal(c.precision_recall(), np.zeros((1, 3, 2)))            # 0 / (0 + 0 + 1e-10), never a NaN
    assert np.array_equal(P.notebook_table(c, 3), np.zeros((2 + 3, 2)))
    assert np.array_equal(P.notebook_table(c, 3, rng=np.random.default_rng(0)), np.zeros((5, 2)))
    with pytest.raises(ValueError):
        P.notebook_table(P.PRCurve([0.5, 0.7], device='cpu'), 3)                # not a notebook curve


def test_table_of_one_group_and_pooled_over_groups():
    c = P.notebook_curve(2, groups=2, device='cpu')               # thresholds 0.5, then >= 1.0
    c.set_counts([[10, 4], [30, 6]], [[2, 0], [8, 2]], [12, 40], [100, 100])
    pooled = P.notebook_table(c, 2)
    assert pooled[0, 0] == 40 / (40 + 10 + 1e-10) and pooled[0, 1] == 40 / (40 + 12 + 1e-10)
    g1 = P.notebook_table(c, 2, group=1)
    assert g1[0, 0] == 30 / (30 + 8 + 1e-10) and g1[2, 0] == 0.1 * 6 / (0.1 * 6 + 0.1 * 2 + 1e-10)


# ------------------------------------------------------------------------------------------------ merge / reset / all_reduce
def test_merge_adds_and_reset_zeroes():
    a, _, _ = _injected()
    b, _, _ = _injected()
    a.merge(b)
    got = a.counts()
    assert got['TP'].tolist() == [[1800, 1600, 1400, 1000]] and got['FP'].tolist() == [[600, 400, 200, 80]]
    assert got['occupied'].tolist() == [2000] and got['voxels'].tolist() == [65536] and got['FN'].tolist() == [[200, 400, 600, 1000]]
    with pytest.raises(ValueError):
        a.merge(P.notebook_curve(5, device='cpu'))
    with pytest.raises(ValueError):
        a.merge(P.notebook_curve(4, groups=2, device='cpu'))
    a.reset()
    assert not any(v.any() for v in a.counts().values())


def test_update_without_a_gpu_is_an_error_not_a_fallback():
    from voxvae import lib as L
    c = P.PRCurve([0.5], device='cpu')
    with pytest.raises(L.VoxVaeError):
        c.update(np.zeros((1, 8), F32), np.zeros((1, 8), F32))


def _allreduce_worker(rank, world, port, out):
    os.environ['MASTER_ADDR'] = '127.0.0.1'
    os.environ['MASTER_PORT'] = str(port)
    dist.init_process_group('gloo', rank=rank, world_size=world)
    for p in (ROOT, PKG):
        if p not in sys.path:
            sys.path.insert(0, p)
    from voxvae import prcurve
    c = prcurve.PRCurve([0.7, 0.2, 0.7], groups=2, device='cpu')
    k = rank + 1
    c.set_counts([[1 * k, 5 * k, 1 * k], [2 * k, 6 * k, 2 * k]], [[0, 3 * k, 0], [k, k, k]], [7 * k, 9 * k], [64 * k, 64 * k])
    c.all_reduce()
    got = c.counts()
    out[rank] = (got['TP'].tolist() == [[3, 15, 3], [6, 18, 6]] and got['FP'].tolist() == [[0, 9, 0], [3, 3, 3]]
                 and got['occupied'].tolist() == [21, 27] and got['voxels'].tolist() == [192, 192])
    dist.destroy_process_group()


def test_all_reduce_sums_over_a_world_2_gloo_group():
    """Every rank evaluates a shard; all_reduce leaves the split's counts on each of them (two real processes over gloo)."""
    mgr = mp.Manager()
    out = mgr.dict()
    port = 33500 + (os.getpid() % 2000)
    mp.spawn(_allreduce_worker, args=(2, port, out), nprocs=2, join=True)
    assert dict(out) == {0: True, 1: True}
    assert P.PRCurve([0.5], device='cpu').all_reduce().counts()['TP'].tolist() == [[0]]      # no group initialised: a no-op


# ------------------------------------------------------------------------------------------------ C ABI refusals
@pytest.fixture(scope='module')
def lib():
    from voxvae import build as vb
    vb.build()
    from voxvae import lib as L
    return L.load()


def _accumulate(lib, pred=64, target=64, packed=0, thr=64, nthr=3, group=None, ngroups=1, tp_fp=64, totals=64, ws=64, ws_bytes=1 << 30,
                batch=2, voxels=64):
    """The pointers are never dereferenced by a call that is refused: small aligned integers stand in for device addresses."""
    return lib.vv_pr_curve_accumulate(pred, target, packed, thr, nthr, 1, group, ngroups, tp_fp, totals, ws, ws_bytes, batch, voxels, None)


def test_abi_refuses_null_and_bad_sizes_before_any_launch(lib):
    for name in ('pred', 'target', 'thr', 'tp_fp', 'totals', 'ws'):
        assert _accumulate(lib, **{name: None}) == -1, name
    assert _accumulate(lib, nthr=0) == -2 and _accumulate(lib, nthr=257) == -2 and _accumulate(lib, nthr=-1) == -2
    assert _accumulate(lib, packed=1, voxels=27) == -2 and _accumulate(lib, packed=1, voxels=4100) == -2
    assert _accumulate(lib, ngroups=0) == -2 and _accumulate(lib, ngroups=-3) == -2
    assert _accumulate(lib, batch=0) == -2 and _accumulate(lib, voxels=0) == -2 and _accumulate(lib, batch=-1) == -2
    need = lib.vv_pr_curve_workspace_bytes(2, 64, 3)
    assert _accumulate(lib, ws_bytes=need - 1) == -5              # a short workspace: the status the other entry points use
    assert _accumulate(lib, ws_bytes=0) == -5
    assert _accumulate(lib, pred=66) == -4                        # not even float-aligned
    assert lib.vv_status_string(-5) == b'workspace missing or too small'


def test_workspace_bytes_is_host_arithmetic(lib):
    """32-bit partials, 2 T + 1 per piece of at most 4096 voxels of one sample: a function of (batch, voxels, nthr) alone."""
    w = lib.vv_pr_curve_workspace_bytes
    assert w(1, 1, 1) == 3 * 4
    assert w(256, 32768, 59) == (2 * 59 + 1) * 256 * 8 * 4
    assert w(3, 40000, 256) == 513 * 3 * 10 * 4                   # ragged last piece
    assert w(7, 4104, 19) == 39 * 7 * 2 * 4
    assert w(2, 4096, 19) == 39 * 2 * 4
    assert w(0, 64, 3) == 0 and w(2, 0, 3) == 0 and w(2, 64, 0) == 0 and w(2, 64, 257) == 0
    assert w(4, 2 ** 33, 1) == 3 * 4 * 2 ** 21 * 4                # past 2^31 voxels per sample
    assert lib.vv_abi_version() == 1
