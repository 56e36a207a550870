"""GPU tests of the two entries of csrc/ae3d.hip through the C ABI: vv_adam_step_multi_l2 (Adam with the l2 gradient folded in and
sum w^2 left by the same pass) and vv_ae3d_step_scalars, against float64 restatements, with every buffer between canaries."""
import ctypes

import numpy as np
import pytest
import torch

from _train_ref import ADAM_B1, ADAM_B2, ADAM_CHUNK, ADAM_EPS, ADAM_UNITS, adam_units, lr_t_of
from test_gpu_train_ops import DEV, _canaries_intact, _chunk_table, _guarded, _guarded_empty, adam_inputs

pytestmark = pytest.mark.gpu

SIZES = [1, 255, ADAM_CHUNK, ADAM_CHUNK + 1, 40000]   # a one-element variable, a sub-workgroup chunk, an exact chunk, a one-element tail chunk, three chunks
COEF = np.float32(2 * 5e-4)                           # 2 * lambda * world at one replica
T_STEP = 3                                            # the state has run two steps
# The project's bound for its Adam kernels plus the ONE extra float32 rounding of g_eff = fma(coef, w, g), half an ulp of g_eff = one unit of
# (1-b1) g_eff: at most 1 unit in m (|(1-b1) g_eff| <= m's unit base), 2 in v (g_eff enters squared: relative error doubles, and (1-b2) g_eff^2 <= v),
# and through m / sqrt(v) at most 1 + 2/2 = 2 in the step.  4 covers the largest of them with the same margin for every output.
L2_UNITS = ADAM_UNITS + 4
SUMSQ_REL = 72 * 2.0 ** -24                           # <= 64 sequential fused adds per thread + 8 tree levels (256 threads), non-negative terms


@pytest.fixture(scope='module')
def L():
    from voxvae import lib
    lib.load()
    assert torch.cuda.is_available()
    return lib


def _st():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _l2_table(ptrs_and_sizes, coefs):
    """vv_adam_step_multi's table plus the sixth word: the chunk's float32 coefficient in its low half (include/voxvae.h)."""
    base = _chunk_table(ptrs_and_sizes).cpu().numpy()
    per_chunk = np.concatenate([np.full((n + ADAM_CHUNK - 1) // ADAM_CHUNK, c, dtype=np.float32) for (_, _, _, _, n), c in zip(ptrs_and_sizes, coefs)])
    t = np.concatenate([base, per_chunk.view(np.uint32).astype(np.int64)[:, None]], axis=1)
    return np.ascontiguousarray(t), per_chunk


def _state(seed):
    data = [adam_inputs(n, seed=31 * k + seed) for k, n in enumerate(SIZES)]
    for d in data:
        d[0][-1] = 0.375          # adam_inputs may leave the last weight 0: the one-element tail chunk's sum w^2 has something to sum
    leads = [1 + (k % 3) for k in range(len(data))]                     # 4, 8 or 12 bytes past a 16-byte boundary
    return data, leads


def _upload(data, leads):
    return [[_guarded(a, lead) for a in d[:4]] for d, lead in zip(data, leads)]


def _launch(L, var_bufs, coefs, lr_t):
    args = [tuple(view.data_ptr() for _, view in var) + (n,) for var, n in zip(var_bufs, SIZES)]
    table_np, per_chunk = _l2_table(args, coefs)
    tb, table = _guarded(np.zeros(table_np.size * 2, np.float32), lead=4)       # the table itself between canaries (16-byte aligned payload)
    table.view(torch.int64).copy_(torch.from_numpy(table_np.ravel()))
    nch = table_np.shape[0]
    sb, sumsq = _guarded_empty(nch, lead=3)
    L.call('vv_adam_step_multi_l2', L.ptr(table), nch, lr_t, ADAM_B1, ADAM_B2, ADAM_EPS, L.ptr(sumsq), _st())
    torch.cuda.synchronize()
    assert _canaries_intact(tb, 4, table_np.size * 2) and _canaries_intact(sb, 3, nch)
    assert np.array_equal(table.view(torch.int64).cpu().numpy(), table_np.ravel())
    return sumsq.cpu().numpy().copy(), per_chunk


def test_zero_coefficients_give_adam_step_multi_bit_for_bit(L):
    data, leads = _state(5)
    lr_t = lr_t_of(T_STEP)
    ours, theirs = _upload(data, leads), _upload(data, leads)
    sumsq, _ = _launch(L, ours, [0.0] * len(SIZES), lr_t)
    table = _chunk_table([tuple(view.data_ptr() for _, view in var) + (n,) for var, n in zip(theirs, SIZES)])
    L.call('vv_adam_step_multi', L.ptr(table), table.shape[0], lr_t, ADAM_B1, ADAM_B2, ADAM_EPS, _st())
    torch.cuda.synchronize()
    assert not sumsq.any() and not np.signbit(sumsq).any()
    for k, (a, b, lead, n) in enumerate(zip(ours, theirs, leads, SIZES)):
        for (ba, va), (bb, vb) in zip(a, b):
            assert _canaries_intact(ba, lead, n), k
            assert torch.equal(va.view(torch.int32), vb.view(torch.int32)), 'variable %d differs from vv_adam_step_multi' % k
    moved = sum(int((var[0][1].cpu().numpy() != d[0]).sum()) for var, d in zip(ours, data))
    assert moved > 0.8 * sum(SIZES)


@pytest.mark.parametrize('first', [0, 1])
def test_l2_step_against_float64(L, first):
    """Alternate variables regularised (first = 0: 1, 16384, 40000 elements; first = 1: 255 and 16385, the one-element tail chunk).  m, v
    and the weights in adam_units against adam_ref fed g + coef * w formed in float64, weights away from 0 measured as
    tests/test_gpu_train_ops.py measures vv_adam_step_multi (plain units); the bound is L2_UNITS (derivation at its definition).
    Partials: per regularised chunk within 72 * 2^-24 of the float64 sum w^2 of the PRE-update weights, 0 elsewhere.  A second run from the
    same state gives the same bits everywhere.  Canaries intact, gradients untouched."""
    data, leads = _state(11 + first)
    lr_t = lr_t_of(T_STEP)
    coefs = [COEF if k % 2 == first else np.float32(0) for k in range(len(SIZES))]
    runs = []
    for _ in range(2):
        bufs = _upload(data, leads)
        sumsq, per_chunk = _launch(L, bufs, coefs, lr_t)
        runs.append((bufs, sumsq))
    bufs, sumsq = runs[0]
    worst, chunk0, worst_ss = [0.0, 0.0, 0.0], 0, 0.0
    for k, (d, lead, var, n, c) in enumerate(zip(data, leads, bufs, SIZES, coefs)):
        p, g, m, v, _ = d
        for buf, _ in var:
            assert _canaries_intact(buf, lead, n), k
        gp, gg, gm, gv = (view.cpu().numpy() for _, view in var)
        assert np.array_equal(gg, g)
        assert np.isfinite(gp).all() and np.isfinite(gm).all() and np.isfinite(gv).all()
        g_eff = g.astype(np.float64) + float(c) * p.astype(np.float64)
        u = adam_units(gp, gm, gv, p, g_eff, m, v, lr_t)
        worst = [max(a, b) for a, b in zip(worst, u)]
        for off in range(0, n, ADAM_CHUNK):
            want = float((p[off:off + ADAM_CHUNK].astype(np.float64) ** 2).sum()) if c != 0 else 0.0
            got = float(sumsq[chunk0])
            if c == 0:
                assert got == 0.0, (k, off)
            else:
                assert per_chunk[chunk0] == c
                worst_ss = max(worst_ss, abs(got - want) / max(want, 1e-300))
                assert abs(got - want) <= SUMSQ_REL * want, (k, off, got, want)
            chunk0 += 1
        for (_, a), (_, b) in zip(var, runs[1][0][k]):
            assert torch.equal(a.view(torch.int32), b.view(torch.int32)), k
    assert chunk0 == sumsq.size and np.array_equal(sumsq.view(np.int32), runs[1][1].view(np.int32))
    print('\n[adam l2 first=%d] worst error in bound units: m %.2f  v %.2f  param %.2f  (bound %.0f); sum w^2 worst rel %.2e (bound %.2e)'
          % ((first,) + tuple(worst) + (L2_UNITS, worst_ss, SUMSQ_REL)))
    assert max(worst) <= L2_UNITS, worst


def test_l2_entry_validates_before_launching(L):
    lib = L.load()
    x = torch.zeros(64, dtype=torch.float32, device=DEV)
    xp, st = ctypes.c_void_p(x.data_ptr()), _st()
    assert lib.vv_adam_step_multi_l2(None, 3, 1e-3, 0.9, 0.999, 1e-7, xp, st) == -1
    assert lib.vv_adam_step_multi_l2(xp, 3, 1e-3, 0.9, 0.999, 1e-7, None, st) == -1
    assert lib.vv_adam_step_multi_l2(xp, 0, 1e-3, 0.9, 0.999, 1e-7, xp, st) == -2
    assert lib.vv_ae3d_step_scalars(None, 1, xp, 1, 5e-4, 1.0, xp, st) == -1
    assert lib.vv_ae3d_step_scalars(xp, 1, None, 1, 5e-4, 1.0, xp, st) == -1
    assert lib.vv_ae3d_step_scalars(xp, 0, xp, 1, 5e-4, 1.0, xp, st) == -2
    assert lib.vv_ae3d_step_scalars(xp, 1, xp, -1, 5e-4, 1.0, xp, st) == -2


@pytest.mark.parametrize('B,nchunks,world', [(1, 1, 1), (5, 0, 2), (257, 1623, 1), (257, 64, 8)])
def test_step_scalars_against_float64(L, B, nchunks, world):
    """stats = per-sample (bce, TP, FP, FN) with integer counts up to 32^3; every output within 2 float32 ulps of the float64 value, the
    total the float32 sum of the two outputs it is made of; stats and the partials untouched, canaries intact."""
    rng = np.random.default_rng(100 * B + nchunks)
    stats = np.empty((B, 4), np.float32)
    stats[:, 0] = rng.uniform(50.0, 9000.0, B)
    tp = rng.integers(0, 32 ** 3 + 1, B)
    fp = rng.integers(0, 32 ** 3 + 1 - tp)
    stats[:, 1], stats[:, 2], stats[:, 3] = tp, fp, rng.integers(0, 32 ** 3 + 1, B)
    stats[0, 1:] = (32 ** 3, 0, 32 ** 3)
    part = (rng.uniform(0.0, 40.0, max(nchunks, 1)) * (rng.random(max(nchunks, 1)) > 0.3)).astype(np.float32)
    l2, inv_gb = np.float32(5e-4), np.float32(1.0 / (B * world))
    sb, sd = _guarded(stats, lead=0)
    pb, pd = _guarded(part, lead=1)
    ob, od = _guarded_empty(6, lead=2)
    L.call('vv_ae3d_step_scalars', L.ptr(sd), B, L.ptr(pd) if nchunks else None, nchunks, float(l2), float(inv_gb), L.ptr(od), _st())
    torch.cuda.synchronize()
    assert _canaries_intact(sb, 0, stats.size) and _canaries_intact(pb, 1, part.size) and _canaries_intact(ob, 2, 6)
    assert np.array_equal(sd.cpu().numpy(), stats.ravel()) and np.array_equal(pd.cpu().numpy(), part)
    got = od.cpu().numpy()
    s64 = stats.astype(np.float64).sum(axis=0)
    reg = float(l2) * float(part[:nchunks].astype(np.float64).sum())
    want = np.array([reg, s64[0] * float(inv_gb), reg + s64[0] * float(inv_gb), s64[1] * float(inv_gb), s64[2] * float(inv_gb), s64[3] * float(inv_gb)])
    ulps = np.abs(got.astype(np.float64) - want) / np.spacing(np.abs(want).astype(np.float32)).astype(np.float64)
    print('\n[step scalars B=%d chunks=%d world=%d] ulps off:' % (B, nchunks, world), np.round(ulps, 3))
    assert (ulps <= 2.0).all(), (got, want)
    assert got[2] == np.float32(got[0]) + np.float32(got[1])
    if world == 1:                                                      # the counts come back exactly when multiplied by the batch
        back = got[3:].astype(np.float64) * B
        assert np.abs(back - s64[1:]).max() <= 2.0 ** -23 * s64[1:].max()
