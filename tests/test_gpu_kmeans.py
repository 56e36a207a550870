"""GPU tests of the viewpoint k-means (csrc/kmeans_cosine.hip behind vv_kmeans_cosine / vv_kmeans_cosine_assign, voxvae/kmeans.py,
function.kmeans_cosine, getKmeansAEI).

The oracle is the host twin -- the same header compiled for the CPU, which tests/test_kmeans_host.py holds against the definition and
against the reference's own class -- and every comparison here is BIT FOR BIT: centres, labels, distances and the iteration count.
There is no tolerance in this file.  The cases are those of tests/_kmeans_ref.py (one point; one short of, exactly and one past a
chunk; six chunks with a ragged last one; one centre; more centres than points; two identical centres; a run that settles long before
max_iter = 1000).  These entries have no row in tests/test_gpu_guards.py (their stream parameter is `hip_stream`), so the memory
discipline is checked here with the same arena."""
import ctypes
import random

import numpy as np
import pytest
import torch

import _guarded as G
import _kmeans_ref as R

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
GUARDED = ['chunk + 1', 'more centres than points', 'six chunks', 'twins']


@pytest.fixture(scope='module')
def L():
    import voxvae
    from voxvae import lib
    lib.load()
    assert torch.cuda.is_available()
    voxvae.set_default_device(DEV)
    return lib


def _st():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def same_bits(a, b):
    a, b = a.detach().cpu().contiguous(), b.detach().cpu().contiguous()
    if a.dtype != b.dtype or a.shape != b.shape:
        return False
    return torch.equal(a.view(torch.int64) if a.dtype == torch.float64 else a, b.view(torch.int64) if b.dtype == torch.float64 else b)


_host = {}


def host_result(name):
    """The host twin's result for a shared case, computed once."""
    from voxvae import kmeans as K
    if name not in _host:
        X, C0, max_iter = R.case(name)
        _host[name] = K.kmeans(X, C0, max_iter, host=True)
    return _host[name]


def assert_equals_host(got, name, what=''):
    c, xtoc, dist, its = host_result(name)
    assert same_bits(got[1], xtoc), '%s %s: labels' % (name, what)
    assert same_bits(got[0], c), '%s %s: centres' % (name, what)
    assert same_bits(got[2], dist), '%s %s: distances' % (name, what)
    assert int(got[3]) == its, '%s %s: iterations %d against %d' % (name, what, int(got[3]), its)


# ------------------------------------------------------------------------------------------------------ device against host twin
@pytest.mark.parametrize('name', sorted(R.CASES))
def test_device_equals_the_host_twin_bit_for_bit(L, name):
    from voxvae import kmeans as K
    X, C0, max_iter = R.case(name)
    got = K.kmeans(X, C0, max_iter)
    assert got[0].is_cuda and got[1].is_cuda and got[1].dtype == torch.int32 and got[0].dtype == got[2].dtype == torch.float64
    assert_equals_host(got, name)
    if name == 'settles':
        assert got[3] < 30 and max_iter == 1000                                  # 970 iterations' launches returned at once
    again = K.kmeans(torch.from_numpy(X).to(DEV), torch.from_numpy(C0).to(DEV), max_iter)
    assert_equals_host(again, name, 'second run, device input')


def test_an_unsettled_run_reports_max_iter(L):
    from voxvae import kmeans as K
    X, C0, _ = R.case('six chunks')
    full = host_result('six chunks')[3]
    assert full > 4
    for it in (1, 2, 3):
        h, d = K.kmeans(X, C0, it, host=True), K.kmeans(X, C0, it)
        assert d[3] == h[3] == it and same_bits(d[0], h[0]) and same_bits(d[1], h[1]) and same_bits(d[2], h[2])


# ------------------------------------------------------------------------------------------------------------ memory discipline
def _guarded_run(L, name, fill, extra=0, announce_extra=False):
    X, C0, max_iter = R.case(name)
    n, k = X.shape[0], C0.shape[0]
    need = L.load().vv_kmeans_cosine_workspace_bytes(n, k)
    assert need > 0
    a = G.Arena(DEV)
    x = a.input(torch.from_numpy(X), 'x')
    c = a.input(torch.from_numpy(C0.copy()), 'centres', inout=True)
    xtoc = a.output((n,), torch.int32, 'xtoc')
    dist = a.output((n,), torch.float64, 'distance')
    its = a.output((1,), torch.int32, 'iterations')
    ws = a.workspace(need, fill, 'workspace', extra=extra)
    a.commit()
    L.call('vv_kmeans_cosine', x.ptr, n, c.ptr, k, max_iter, xtoc.ptr, dist.ptr, its.ptr, ws.ptr, need + (extra if announce_extra else 0), _st())
    torch.cuda.synchronize()
    a.check()                                                                   # guards of every buffer intact, x unchanged
    if extra:
        assert bool((ws.payload[need:] == G.POISON).all()), 'bytes past the stated workspace size were written'
    return c.tensor.clone(), xtoc.tensor.clone(), dist.tensor.clone(), int(its.tensor.item())


@pytest.mark.parametrize('name', GUARDED)
def test_guards_inputs_and_workspace_independence(L, name):
    assert_equals_host(_guarded_run(L, name, 0x00), name, 'workspace 0x00')
    assert_equals_host(_guarded_run(L, name, 0xFF), name, 'workspace 0xFF')
    assert_equals_host(_guarded_run(L, name, 0xFF, extra=4096, announce_extra=True), name, 'workspace over-announced')
    assert_equals_host(_guarded_run(L, name, 0xA5, extra=512), name, 'second run, other fill')


@pytest.mark.parametrize('name', GUARDED)
@pytest.mark.parametrize('with_distance', [True, False])
def test_assign_guards_and_twin(L, name, with_distance):
    from voxvae import kmeans as K
    X, _, _ = R.case(name)
    centres = host_result(name)[0]
    want, wantd = K.assign(X, centres, host=True, return_distance=True)
    n, k = X.shape[0], centres.shape[0]
    a = G.Arena(DEV)
    x = a.input(torch.from_numpy(X), 'x')
    c = a.input(centres.clone(), 'centres')
    xtoc = a.output((n,), torch.int32, 'xtoc')
    dist = a.output((n,), torch.float64, 'distance')
    a.commit()
    L.call('vv_kmeans_cosine_assign', x.ptr, n, c.ptr, k, xtoc.ptr, dist.ptr if with_distance else None, _st())
    torch.cuda.synchronize()
    a.check()
    assert same_bits(xtoc.tensor, want)
    if with_distance:
        assert same_bits(dist.tensor, wantd)
    else:
        assert bool((G.as_bytes(dist.tensor) == G.POISON).all())                # NULL distance: nothing written
    got = K.assign(X, centres, return_distance=with_distance)
    labels = got[0] if with_distance else got
    assert labels.is_cuda and labels.dtype == torch.int32 and same_bits(labels, want)
    if with_distance:
        assert same_bits(got[1], wantd)


# ---------------------------------------------------------------------------------------------------------- streams and wrappers
def test_a_run_on_another_stream(L):
    from voxvae import kmeans as K
    X, C0, max_iter = R.case('six chunks')
    s = torch.cuda.Stream(device=DEV)
    with torch.cuda.stream(s):
        assert torch.cuda.current_stream().cuda_stream == s.cuda_stream != torch.cuda.default_stream().cuda_stream
        got = K.kmeans(X, C0, max_iter)
        labels = K.assign(X, got[0])
    s.synchronize()
    assert_equals_host(got, 'six chunks', 'side stream')
    assert same_bits(labels, K.assign(X, host_result('six chunks')[0], host=True))


def test_the_class_on_the_device_equals_the_class_on_the_host(L):
    from src.module.function import kmeans_cosine
    X = R.viewpoints(700, 12)
    res = []
    for kw in (dict(host=True), dict(), dict(device=DEV)):
        random.seed(3)
        km = kmeans_cosine(X, 23, 100, **kw)
        res.append(km.kmeansSample() + (km.iterations,))
    for r in res[1:]:
        assert all(np.array_equal(u, v) for u, v in zip(res[0][:3], r[:3])) and r[3] == res[0][3]
    assert res[0][1].dtype == np.int64 and res[0][0].shape == (23, 6)


def test_getKmeansAEI_on_both_loaders(L):
    import src.dataset_loader.pascal3D as P
    from src.module.function import kmeans_cosine
    for make in (lambda: P.dataLoaderSingleObject('val', 'synthetic:130:8'), lambda: P.deviceDataLoaderSingleObject('val', 'synthetic:130:8', device=DEV)):
        loader = make()
        e = np.asarray(loader._euler, dtype=np.float64)
        rows = np.concatenate([np.sin(e), np.cos(e)], axis=1)
        assert rows.shape == (130, 6)
        random.seed(9)
        c, xtoc, dist = loader.getKmeansAEI(k=6, max_iter=50)
        random.seed(9)
        c2, x2, d2 = kmeans_cosine(rows, 6, 50, host=True).kmeansSample()
        assert c.shape == (6, 6) and c.dtype == np.float64 and xtoc.shape == (130,)
        assert np.array_equal(c, c2) and np.array_equal(xtoc, x2) and np.array_equal(dist, d2)


# -------------------------------------------------------------------------------------------------------- per-cluster PR curves
def test_precision_recall_curves_per_viewpoint_cluster(L):
    """PRCurve(groups=k).update(target, pred, group=assign(...)) -- the labels as they come, int32 on the device -- equals the sum of
    one update per cluster over that cluster's samples, picked with host-side labels."""
    from voxvae import kmeans as K
    from voxvae.prcurve import PRCurve
    rng = np.random.default_rng(31)
    B, V, k = 200, 520, 7
    X = R.viewpoints(B, 31)
    centres = K.kmeans(X, X[:k], 20, host=True)[0]
    y = (rng.random((B, V)) < 0.3).astype(np.float32)
    p = rng.random((B, V)).astype(np.float32)
    thr = [0.25, 0.5, 0.75]
    labels = K.assign(X, centres)
    got = PRCurve(thr, groups=k, device=DEV).update(y, p, group=labels).counts()
    host_labels = K.assign(X, centres, host=True).numpy()
    assert len(np.unique(host_labels)) > 1
    for g in range(k):
        sel = host_labels == g
        want = PRCurve(thr, device=DEV).update(y[sel], p[sel]).counts() if sel.any() else None
        for key in got:
            assert np.array_equal(got[key][g], want[key][0] if want is not None else np.zeros_like(got[key][g])), (g, key)
    assert int(got['voxels'].sum()) == B * V
