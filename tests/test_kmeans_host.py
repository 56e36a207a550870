"""CPU tests of the viewpoint k-means (csrc/kmeans_cosine.h behind vv_kmeans_cosine_host, voxvae/kmeans.py, function.kmeans_cosine,
getKmeansAEI, pascal_kmeans_AEI.py).

The oracle is tests/_kmeans_ref.py, the definition in numpy float64 with NO early exit, and for the golden fixture the reference's own
class (tests/golden/make_kmeans_golden.py).  Tolerances are derived, not measured: every case asserts that no point sits closer than
1e-9 to a decision boundary in any iteration, so labels must match EXACTLY; with equal labels a centre is a mean of at most N values of
magnitude <= 1 taken straight from X, error <= N 2^-53 ~ 1e-13 whatever the summation order and with nothing carried between
iterations: centres and distances within 1e-12."""
import ctypes
import os
import random
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import _kmeans_ref as R
from _common import build_and_run_sanitized

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, 'anytime-3d-reconstruction_amd')
HEADER = os.path.join(ROOT, 'include', 'voxvae.h')
GOLDEN = os.path.join(ROOT, 'tests', 'golden', 'kmeans_cosine.npz')
OK, ERR_NULL, ERR_SHAPE, ERR_WORKSPACE = 0, -1, -2, -5
ENTRIES = {'vv_kmeans_cosine_workspace_bytes': 2, 'vv_kmeans_cosine': 11, 'vv_kmeans_cosine_host': 8, 'vv_kmeans_cosine_assign': 7,
           'vv_kmeans_cosine_assign_host': 6}


@pytest.fixture(scope='module')
def lib():
    from voxvae import build as vb
    vb.build()
    from voxvae import lib as L
    return L.load()


def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p)


# ------------------------------------------------------------------------------------------------------------------ the ABI
def test_the_class_is_importable():
    from src.module.function import kmeans_cosine
    assert callable(kmeans_cosine._kmeans) and callable(kmeans_cosine.kmeansSample)


def test_header_declares_the_entries(lib):
    from voxvae import lib as L
    src = re.sub(r'/\*.*?\*/', '', open(HEADER).read(), flags=re.S)
    for name, nargs in ENTRIES.items():
        m = re.search(r'\b(int|size_t)\s+%s\s*\(([^;]*?)\)\s*;' % name, src, flags=re.S)
        assert m, name
        args = [a.strip() for a in m.group(2).split(',')]
        assert len(args) == nargs == len(L.SIGNATURES[name][1]), name
        assert not any(re.search(r'\bdtype\b', a) for a in args), name
        assert not any(re.search(r'\bstream$', a) and not a.endswith('hip_stream') for a in args), name
        assert hasattr(lib, name)
    launch = re.search(r'vv_kmeans_cosine\s*\(([^;]*?)\)', src, flags=re.S).group(1)
    assert launch.strip().endswith('void *hip_stream')


def test_workspace_size(lib):
    ws = lib.vv_kmeans_cosine_workspace_bytes
    for n, k in [(0, 5), (-1, 5), (5, 0), (5, 1025), ((1 << 20) + 1, 5), (5, -3)]:
        assert ws(n, k) == 0, (n, k)
    assert ws(1, 1) > 0 and ws(1 << 20, 1024) > 0
    sizes = [ws(n, 30) for n in (1, 255, 256, 257, 512, 513, 1500, 40000, 1 << 20)]
    assert all(a <= b for a, b in zip(sizes, sizes[1:])) and sizes[0] < sizes[-1]
    assert ws(1500, 30) >= (6 * 30 * 6 * 8) + (6 * 30 * 4)              # six chunks of partial sums and counts at the least


def test_refusals_happen_before_any_launch(lib):
    """No GPU here: a refused call returns its status without touching a pointer or the stream."""
    x, c = np.zeros((8, 6)), np.zeros((1025, 6))
    xtoc, dist, its, ws = np.zeros(8, dtype=np.int32), np.zeros(8), np.zeros(1, dtype=np.int32), np.zeros(4, dtype=np.float64)
    dev = lambda **kw: lib.vv_kmeans_cosine(*[kw.get(a, d) for a, d in (
        ('x', _p(x)), ('n', 8), ('centres', _p(c)), ('k', 3), ('max_iter', 5), ('xtoc', _p(xtoc)), ('distance', _p(dist)),
        ('iterations', _p(its)), ('workspace', _p(ws)), ('workspace_bytes', 1 << 30), ('hip_stream', None))])
    host = lambda **kw: lib.vv_kmeans_cosine_host(*[kw.get(a, d) for a, d in (
        ('x', _p(x)), ('n', 8), ('centres', _p(c)), ('k', 3), ('max_iter', 5), ('xtoc', _p(xtoc)), ('distance', _p(dist)),
        ('iterations', _p(its)))])
    for name in ('x', 'centres', 'xtoc', 'distance', 'iterations'):
        assert dev(**{name: None}) == ERR_NULL and host(**{name: None}) == ERR_NULL, name
    assert dev(workspace=None) == ERR_NULL
    for bad in (dict(n=0), dict(n=-4), dict(n=(1 << 20) + 1), dict(k=0), dict(k=1025), dict(max_iter=0), dict(max_iter=-1)):
        assert dev(**bad) == ERR_SHAPE and host(**bad) == ERR_SHAPE, bad
    assert dev(workspace_bytes=lib.vv_kmeans_cosine_workspace_bytes(8, 3) - 1) == ERR_WORKSPACE
    assert dev(workspace_bytes=0) == ERR_WORKSPACE
    assert host(k=1024, max_iter=1) == OK and host(k=1025, max_iter=1) == ERR_SHAPE
    assert lib.vv_kmeans_cosine_workspace_bytes(8, 1024) > 0 == lib.vv_kmeans_cosine_workspace_bytes(8, 1025)
    # the assign entries
    assert lib.vv_kmeans_cosine_assign(None, 8, _p(c), 3, _p(xtoc), None, None) == ERR_NULL
    assert lib.vv_kmeans_cosine_assign(_p(x), 8, None, 3, _p(xtoc), None, None) == ERR_NULL
    assert lib.vv_kmeans_cosine_assign(_p(x), 8, _p(c), 3, None, None, None) == ERR_NULL
    assert lib.vv_kmeans_cosine_assign(_p(x), 0, _p(c), 3, _p(xtoc), None, None) == ERR_SHAPE
    assert lib.vv_kmeans_cosine_assign(_p(x), 8, _p(c), 1025, _p(xtoc), None, None) == ERR_SHAPE
    assert lib.vv_kmeans_cosine_assign_host(_p(x), 8, _p(c), 1025, _p(xtoc), None) == ERR_SHAPE
    assert lib.vv_kmeans_cosine_assign_host(_p(x), 8, _p(c), 1024, _p(xtoc), None) == OK           # distance may be NULL
    assert lib.vv_kmeans_cosine_assign_host(_p(x), 8, None, 3, _p(xtoc), _p(dist)) == ERR_NULL


def test_wrapper_refuses_bad_input_before_any_upload(lib):
    from voxvae import kmeans as K
    good, c = R.viewpoints(20, 1), R.viewpoints(3, 2)
    for bad in (np.zeros((4, 5)), np.zeros(6), np.zeros((0, 6)), np.zeros((2, 3, 6))):
        with pytest.raises(ValueError):
            K.kmeans(bad, c, 3)                                                 # (host=False: the shape is judged before a device is looked for)
    for v in (np.nan, np.inf, -np.inf):
        x = good.copy()
        x[7, 2] = v
        with pytest.raises(ValueError):
            K.kmeans(x, c, 3)
        with pytest.raises(ValueError):
            K.assign(torch.from_numpy(x), c, host=True)
    with pytest.raises(ValueError):
        K.kmeans(good, c, 0, host=True)
    with pytest.raises(ValueError):
        K.kmeans(good, np.zeros((1025, 6)), 1, host=True)


# ------------------------------------------------------------------------------------------------ host twin against the definition
@pytest.mark.parametrize('name', sorted(R.CASES))
def test_host_twin_equals_the_definition(lib, name):
    from voxvae import kmeans as K
    X, C0, max_iter = R.case(name)
    ref = R.reference(name)
    assert ref['gap'] >= R.MIN_GAP, 'the case sits on a decision boundary: gap %.3e' % ref['gap']
    before = C0.copy()
    c, xtoc, dist, its = K.kmeans(X, C0, max_iter, host=True)
    c, xtoc, dist = c.numpy(), xtoc.numpy(), dist.numpy()
    assert np.array_equal(C0, before) and xtoc.dtype == np.int32 and c.dtype == dist.dtype == np.float64
    assert np.array_equal(xtoc, ref['xtoc'])
    print('\n[%s] max |dcentre| %.3e  max |ddistance| %.3e  iterations %d of %d  gap %.3e' % (
        name, np.abs(c - ref['centres']).max(), np.abs(dist - ref['distance']).max(), its, max_iter, ref['gap']))
    assert np.abs(c - ref['centres']).max() <= R.TOL and np.abs(dist - ref['distance']).max() <= R.TOL
    assert 1 <= its <= max_iter
    assert its == (max_iter if ref['settled'] is None else ref['settled'])
    empty = ~ref['populated']
    assert np.array_equal(c[empty], C0[empty])                                  # never populated: the row is kept bit for bit
    l2, d2 = K.assign(X, c, host=True, return_distance=True)
    want, wantd, _ = R.assign(X, c)
    assert np.array_equal(l2.numpy(), want) and np.array_equal(d2.numpy(), wantd) and torch.equal(K.assign(X, c, host=True), l2)


def test_more_centres_than_points_keeps_the_unused_rows(lib):
    ref = R.reference('more centres than points')
    assert (~ref['populated']).sum() >= 4                                       # 9 centres, 5 points: the case is not vacuous


def test_the_first_of_two_identical_centres_takes_every_tie(lib):
    from voxvae import kmeans as K
    X, C0, max_iter = R.case('twins')
    assert np.array_equal(C0[1], C0[3])
    ref = R.reference('twins')
    assert ref['populated'].tolist() == [True, True, True, False]
    for it in (1, max_iter):
        c, xtoc, _, _ = K.kmeans(X, C0, it, host=True)
        assert (xtoc == 1).any() and not (xtoc == 3).any() and np.array_equal(c.numpy()[3], C0[3])
        assert not np.array_equal(c.numpy()[1], C0[1])


def test_a_settled_run_stops_early_and_equals_the_full_thousand(lib):
    from voxvae import kmeans as K
    X, C0, max_iter = R.case('settles')
    ref = R.reference('settles')                                                # all 1000 iterations, computed
    assert max_iter == 1000 and ref['settled'] is not None and ref['settled'] < 30
    c, xtoc, dist, its = K.kmeans(X, C0, 1000, host=True)
    assert its == ref['settled'] < 1000
    assert np.array_equal(xtoc.numpy(), ref['xtoc']) and np.abs(c.numpy() - ref['centres']).max() <= R.TOL
    # and the exit is exact on the twin's own bits: stopping anywhere past `settled` gives the same arrays
    for more in (its, its + 1, its + 7):
        c2, x2, d2, i2 = K.kmeans(X, C0, more, host=True)
        assert torch.equal(c, c2) and torch.equal(xtoc, x2) and torch.equal(dist, d2) and i2 == its
    # iteration `its` only confirmed the labels of `its` - 1; the one before still differed
    c3, x3, _, i3 = K.kmeans(X, C0, its - 2, host=True)
    assert i3 == its - 2 and not torch.equal(xtoc, x3) and not torch.equal(c, c3)


# ------------------------------------------------------------------------------------------------------------- the golden fixture
@pytest.fixture(scope='module')
def golden():
    g = np.load(GOLDEN)
    assert float(g['min_gap']) >= R.MIN_GAP
    return g


def test_host_twin_equals_the_reference_class(lib, golden):
    from voxvae import kmeans as K
    g = golden
    for name in g['sample_cases']:
        p = str(name) + '_'
        X = g[p + 'X']
        first = K.kmeans(X[g[p + 'sample_idx']], X[g[p + 'centre_idx']], 10, host=True)[0]
        c, xtoc, dist, _ = K.kmeans(X, first, int(g[p + 'max_iter']), host=True)
        assert np.array_equal(xtoc.numpy(), g[p + 'xtoc']), name
        assert np.abs(c.numpy() - g[p + 'centres']).max() <= R.TOL and np.abs(dist.numpy() - g[p + 'distance']).max() <= R.TOL, name
    X, C0 = g['twins_X'], g['twins_centres0']
    assert np.array_equal(C0[1], C0[3])
    c, xtoc, dist, _ = K.kmeans(X, C0, int(g['twins_max_iter']), host=True)
    assert np.array_equal(xtoc.numpy(), g['twins_xtoc']) and np.abs(c.numpy() - g['twins_centres']).max() <= R.TOL
    assert np.abs(dist.numpy() - g['twins_distance']).max() <= R.TOL and np.array_equal(c.numpy()[3], C0[3])


def test_the_class_under_random_seed_equals_the_reference_class(lib, golden):
    from src.module.function import kmeans_cosine
    g = golden
    for name in g['sample_cases']:
        p = str(name) + '_'
        X, k, max_iter = g[p + 'X'], int(g[p + 'k']), int(g[p + 'max_iter'])
        random.seed(int(g[p + 'seed']))
        km = kmeans_cosine(X, k, max_iter, host=True)
        c, xtoc, dist = km.kmeansSample()
        assert isinstance(c, np.ndarray) and c.shape == (k, 6) and xtoc.dtype == np.int64 and dist.dtype == np.float64
        assert np.array_equal(xtoc, g[p + 'xtoc']), name
        assert np.abs(c - g[p + 'centres']).max() <= R.TOL and np.abs(dist - g[p + 'distance']).max() <= R.TOL, name
        assert 1 <= km.iterations <= max_iter
        # the injected picks give the same result without touching `random`
        state = random.getstate()
        c2, x2, d2 = kmeans_cosine(X, k, max_iter, host=True).kmeansSample(_sample_idx=g[p + 'sample_idx'], _centre_idx=g[p + 'centre_idx'])
        assert random.getstate() == state and np.array_equal(c, c2) and np.array_equal(xtoc, x2) and np.array_equal(dist, d2)


def test_class_details(lib):
    from src.module.function import kmeans_cosine
    X = R.viewpoints(120, 3)
    km = kmeans_cosine(X, 5, host=True)
    C0 = X[:5].copy()
    out = km._kmeans(X, C0, max_iter=0)
    assert out[0] is C0 and out[1] is None and out[2] is None
    c, xtoc, dist = km._kmeans(X, C0, max_iter=4)
    assert c is C0                                                              # updated in place, as the reference does
    ref = R.kmeans(X, X[:5], 4)
    assert np.array_equal(xtoc, ref['xtoc']) and np.abs(c - ref['centres']).max() <= R.TOL
    with pytest.raises(ValueError):
        kmeans_cosine(X, 13, host=True).kmeansSample()                          # 10 k = 130 rows out of 120: random.sample's own error


def test_getKmeansAEI_on_the_host_loader(lib):
    import src.dataset_loader.pascal3D as pascal3D
    from src.module.function import kmeans_cosine
    loader = pascal3D.dataLoaderSingleObject('val', 'synthetic:130:8')
    random.seed(5)
    c, xtoc, dist = loader.getKmeansAEI(k=6, max_iter=50, host=True)
    e = loader._euler.astype(np.float64)
    rows = np.concatenate([np.sin(e), np.cos(e)], axis=1)
    random.seed(5)
    c2, x2, d2 = kmeans_cosine(rows, 6, 50, host=True).kmeansSample()
    assert c.shape == (6, 6) and xtoc.shape == dist.shape == (130,)
    assert np.array_equal(c, c2) and np.array_equal(xtoc, x2) and np.array_equal(dist, d2)
    with pytest.raises(ValueError):
        loader.getKmeansAEI()


def test_entry_script_writes_the_same_bytes_twice(lib, tmp_path):
    outs = []
    for i in range(2):
        out = str(tmp_path / ('c%d.npy' % i))
        r = subprocess.run([sys.executable, 'pascal_kmeans_AEI.py', '--k', '30', '--max-iter', '1000', '--seed', '0', '--out', out, '--leg', 'host',
                            '--dataset-path', 'synthetic:400:8'], cwd=PKG, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=300)
        assert r.returncode == 0, r.stderr[-2000:]
        outs.append(open(out, 'rb').read())
    table = np.load(str(tmp_path / 'c0.npy'))
    assert table.shape == (30, 6) and table.dtype == np.float64 and np.isfinite(table).all()
    assert outs[0] == outs[1]


# ------------------------------------------------------------------------------------------------------------------ sanitizers
@pytest.mark.skipif(torch.cuda.is_available(), reason='sanitizer programs run on CPU-only machines')
def test_standalone_sanitizer_build(tmp_path):
    """The header and tests/kmeans_main.cpp as ONE program of its own under the address and undefined-behaviour sanitizers, run on the CPU."""
    build_and_run_sanitized('kmeans_main.cpp', tmp_path, 'kmeans_asan')
