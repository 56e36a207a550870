"""CPU tests of the one-group, one-prior latent stage: the host entries vv_prior_latent_train_fwd_host / _bwd_host and
vv_inst_latent_eval_host -- the code the kernels run, compiled for the CPU -- against the float64 numpy definition recorded in
tests/golden/prior_latent.npz (tests/golden/make_prior_golden.py), on exact cases, the backward against float64 torch autograd, the
validation order, and the header as a stand-alone sanitizer program.

Gates.  Nothing here is tuned to the host entries' own output.  Forward: the error of PLAIN float32 numpy (tests/_prior_ref.py with
dtype=float32: numpy's exp, numpy's summation order) against the float64 definition, largest over the fixture's cases, relative to
max(|definition|, 1); the host entries are held to 4x that, and never to less than 4 float32 units (2^-24) -- a float32 result cannot
be asked to sit closer than half a spacing to the float64 value.  Measured on the fixture: plain float32 numpy z_in 1.01e-7, kl 1.11e-7,
reg 1.17e-7, evaluation z 1.45e-7 (gates 4.0e-7, 4.4e-7, 4.7e-7, 5.8e-7).  The host entries: z_in 1.02e-7, kl 1.32e-7, reg 1.09e-7,
z 9.3e-8.
Backward: the gate of tests/test_mm_latent_host.py -- 4x what float32 torch autograd of the same closure loses against float64, or
4 units of the tensor's largest magnitude where that is more; the host entry's error is printed beside it."""
import os

import numpy as np
import pytest
import torch

from _common import build_and_run_sanitized
import _prior_ref as R
from voxvae import lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, 'tests', 'golden', 'prior_latent.npz')
UNIT = 2.0 ** -24


def load_golden():
    """{'t': training cases, 'e': evaluation cases}, each a dict of arrays (absent optional inputs None): the flat arrays of the file cut
    up by its layout (tests/golden/make_prior_golden.py)."""
    import json
    z = np.load(GOLDEN)
    g, at = {}, dict(f32=0, f64=0, i32=0)
    for name, t, shape in json.loads(str(z['layout'])):
        n = int(np.prod(shape, dtype=np.int64))
        g[name] = z[t][at[t]:at[t] + n].reshape(shape).copy()
        at[t] += n
    out = {}
    for tag, count, optional in (('t', 'train_cases', ('keep',)), ('e', 'eval_cases', ('mask', 'fill'))):
        cases = []
        for i in range(int(z[count])):
            pre = '%s%d_' % (tag, i)
            c = {k[len(pre):]: g[k] for k in g if k.startswith(pre)}
            for k in optional:
                c.setdefault(k, None)
            cases.append(c)
        out[tag] = cases
    return out


@pytest.fixture(scope='module')
def golden():
    from voxvae import build as vb
    vb.build()
    return load_golden()


def _rel(a, b):
    return float((np.abs(a.astype(np.float64) - b) / np.maximum(np.abs(b), 1.0)).max())


def forward_gates(golden):
    """{quantity: 4 x plain float32 numpy's largest relative error against the float64 definition over the fixture, at least 4 units}."""
    e = dict(z_in=0.0, kl=0.0, reg=0.0, z=0.0)
    for c in golden['t']:
        o = R.train_fwd(*R.train_args(c), dtype=np.float32)
        for k in ('z_in', 'kl', 'reg'):
            e[k] = max(e[k], _rel(o[k], c[k]))
    for c in golden['e']:
        e['z'] = max(e['z'], _rel(R.inst_eval(*R.eval_args(c), dtype=np.float32)['z'], c['z']))
    print('plain float32 numpy against float64: ' + ', '.join('%s %.3e' % kv for kv in sorted(e.items())))
    return {k: 4.0 * max(v, UNIT) for k, v in e.items()}


@pytest.fixture(scope='module')
def gates(golden):
    return forward_gates(golden)


# ------------------------------------------------------------------------------------------------------------------ a. the fixture
def test_fixture_covers_the_cases_the_issue_names(golden):
    shapes = {(c['mean_p'].shape, c['keep'] is not None) for c in golden['t']}
    assert shapes == {((B, Lz), k) for B in (1, 2, 5) for Lz in (1, 16) for k in (False, True)}
    shapes = {(c['enc'].shape[0], c['prior'].shape[1], c['prior'].shape[0], c['mask'] is not None) for c in golden['e']}
    assert shapes == {(B, Lz, I, m) for B in (1, 2, 5) for Lz in (1, 16) for I in (1, 10) for m in (False, True)}
    assert {(float(c['dist']) / c['mean_p'].shape[1], float(c['reg_weight'])) for c in golden['t']} == {(10.0, 1.0), (3.0, 0.01)}
    assert os.path.getsize(GOLDEN) < 64 * 1024


def test_host_forward_against_the_float64_definition(golden, gates):
    worst = dict(z_in=0.0, kl=0.0, reg=0.0)
    for c in golden['t']:
        o = R.call_train(L, 'cpu', c)
        for k in worst:
            worst[k] = max(worst[k], _rel(o[k], c[k]))
    print('host entries against float64: ' + ', '.join('%s %.3e (gate %.3e)' % (k, v, gates[k]) for k, v in sorted(worst.items())))
    for k in worst:
        assert worst[k] <= gates[k], (k, worst[k], gates[k])


def test_host_eval_against_the_float64_definition(golden, gates):
    gate = gates['z']
    worst = 0.0
    for c in golden['e']:
        o = R.call_eval(L, 'cpu', c)
        np.testing.assert_array_equal(o['idx'], c['idx'])
        np.testing.assert_array_equal(o['z_corr'], c['prior'][c['idx']])             # a copied row: exact
        worst = max(worst, _rel(o['z'], c['z']))
    print('host z against float64: %.3e (gate %.3e)' % (worst, gate))
    assert worst <= gate


# ------------------------------------------------------------------------------------------------------------------ b. exact cases
def exact_train_case(kind):
    """B = 3 (or as stated), L = 4 training cases with one planted property each; dist = 3 L = 12, reg_weight = 0.01."""
    c = R.train_case(31, 3, 4)
    if kind == 'duplicates':                                  # rows 0 and 2 coincide: d_02 = d_20 = -dist exactly
        c['mean_p'][2] = c['mean_p'][0]
    elif kind in ('on_hinge', 'above_hinge', 'below_hinge'):  # L = 1, scale exp(0) = 1: d_01 = |0 - m| - dist
        c = R.train_case(32, 2, 1)
        m = {'on_hinge': np.float32(3.0), 'above_hinge': np.nextafter(np.float32(3.0), np.float32(4.0)),
             'below_hinge': np.nextafter(np.float32(3.0), np.float32(0.0))}[kind]
        c['mean_p'][:, 0], c['lv_p'][:] = [0.0, m], 0.0
    elif kind == 'clip':
        c['enc'][0, 4:8] = [10.0, -10.0, np.nextafter(np.float32(10.0), np.float32(11.0)), np.nextafter(np.float32(-10.0), np.float32(-11.0))]
    elif kind == 'keep_zeros':
        c['keep'][:] = 0.0
    elif kind == 'keep_ones':
        c['keep'][:] = 1.0
    elif kind == 'no_keep':
        c['keep'] = None
    return c


TRAIN_KINDS = ['duplicates', 'on_hinge', 'above_hinge', 'below_hinge', 'clip', 'keep_zeros', 'keep_ones', 'no_keep', 'random']


@pytest.mark.parametrize('kind', TRAIN_KINDS)
def test_host_train_forward_exact_cases(kind, gates):
    c = exact_train_case(kind)
    o, r = R.call_train(L, 'cpu', c), R.train_fwd(*R.train_args(c))
    for k in ('z_in', 'kl', 'reg'):
        assert _rel(o[k], r[k]) <= gates[k], (k, _rel(o[k], r[k]), gates[k])
    dist = np.float32(c['dist'])
    if kind == 'duplicates':                                  # the diagonal and the duplicate both give exactly dist^2; the third pair adds >= 0
        assert o['reg'][0] >= 2 * dist * dist and o['reg'][2] >= 2 * dist * dist and o['reg'][1] >= dist * dist
    same = lambda a, b: np.array_equal(a.view(np.uint32), b.view(np.uint32))
    if kind in ('on_hinge', 'above_hinge', 'below_hinge'):
        # d_01 == 0 keeps d^2 = 0, d_01 > 0 gives 0, and one spacing inside d^2 = 2^-44 vanishes beside the diagonal's 9: reg is exactly dist^2.
        # The regulariser's gradient tells them apart: 2 d is 0 on and above the hinge (reg_weight 0 and 2^20 give the same bits) and
        # -2^-21 one spacing inside (2^20 times it is of the KL gradient's size).
        assert o['reg'][0] == dist * dist and o['reg'][1] == dist * dist
        heavy, none = (R.call_train(L, 'cpu', dict(c, reg_weight=w))['d_mean_p'] for w in (2.0 ** 20, 0.0))
        assert same(heavy, none) == (kind != 'below_hinge')
    if kind == 'keep_ones':                                   # the posterior's sample everywhere: the bits of the call without keep
        assert same(o['z_in'], R.call_train(L, 'cpu', dict(c, keep=None))['z_in'])
    if kind == 'keep_zeros':                                  # the prior's sample everywhere: z_prior, and dz_in reaches the prior only
        zp = R.train_fwd(*R.train_args(dict(c, enc=np.concatenate([c['mean_p'], c['lv_p']], axis=1), eps=c['eps_p'], keep=None)))['z_in']
        assert _rel(o['z_in'], zp) <= gates['z_in']
        n = R.call_train(L, 'cpu', dict(c, dz_in=np.zeros_like(c['dz_in'])))
        assert same(o['d_enc_out'], n['d_enc_out']) and not same(o['d_mean_p'], n['d_mean_p'])
    if kind == 'clip':
        assert same(o['z_in'], R.call_train(L, 'cpu', dict(c, enc=_clipped(c)))['z_in'])       # outside the clip: the value at the clip
        # raw exactly +-10 passes the clip's gradient, one spacing outside does not
        assert o['d_enc_out'][0, 4] != 0 and o['d_enc_out'][0, 5] != 0 and np.all(o['d_enc_out'][0, 6:8] == 0)


def _clipped(c):
    """The case with its log-variances already clipped: the same z."""
    e = c['enc'].copy()
    e[:, e.shape[1] // 2:] = np.clip(e[:, e.shape[1] // 2:], -10.0, 10.0)
    return e


def exact_eval_case(kind):
    c = R.eval_case(41, 6, 5, 4, 0.4)
    if kind == 'duplicates':                                  # rows 0 and 2 of the table coincide and every sample sits on them: a tie
        c['prior'][2] = c['prior'][0]
        c['enc'][:, :5], c['eps'][:] = c['prior'][2], 0.0
        c['mask'][:] = 1.0
        c['mask'][:, 0] = 0.0                                 # one masked column keeps the tie (its term is 0 for every row)
    elif kind == 'zeros':                                     # unmasked elements that are exactly +0 and -0 after sampling
        c['mask'][:] = 1.0
        c['enc'][0, 0], c['eps'][0, 0] = 0.0, 0.0
        c['enc'][1, 1], c['eps'][1, 1] = -0.0, 0.0
    elif kind == 'all_masked':
        c['mask'][::2] = 0.0
    elif kind == 'nonfinite':
        c['enc'][0, 0], c['enc'][1, 1] = np.nan, np.inf
        c['enc'][2, :5] = -np.inf
        c['mask'][:3] = 1.0
    elif kind == 'clip':
        c['enc'][0, 5:10] = [10.0, -10.0, 10.000001, -37.5, 88.0]
    return c


EVAL_KINDS = ['duplicates', 'zeros', 'all_masked', 'nonfinite', 'clip']


@pytest.mark.parametrize('kind', EVAL_KINDS)
def test_host_eval_exact_cases(kind, gates):
    gate = gates['z']
    c = exact_eval_case(kind)
    for case in (c, dict(c, mask=None, fill=None)):
        o, r = R.call_eval(L, 'cpu', case), R.inst_eval(*R.eval_args(case))
        assert np.array_equal(np.isnan(o['z']), np.isnan(r['z'])) and np.array_equal(np.isfinite(o['z']), np.isfinite(r['z']))
        fin = np.isfinite(r['z'])
        assert _rel(o['z'][fin], r['z'][fin]) <= gate
        np.testing.assert_array_equal(o['z_corr'], case['prior'][o['idx']])
        if kind not in ('duplicates',):                       # float64 may break a float32 tie the other way: the tie has its own rule below
            np.testing.assert_array_equal(o['idx'], r['idx'])
    o = R.call_eval(L, 'cpu', c)
    if kind == 'duplicates':
        assert np.all(o['idx'] == 0)                          # the lowest index of the tie, never 2
    if kind == 'zeros':                                       # an unmasked +-0 takes the fill, bit for bit
        assert o['z'][0, 0] == c['fill'][0, 0] and o['z'][1, 1] == c['fill'][1, 1]
    if kind == 'all_masked':                                  # every distance is 0: index 0; z is the fill
        assert np.all(o['idx'][::2] == 0) and np.array_equal(o['z'][::2], c['fill'][::2])
    if kind == 'nonfinite':                                   # no distance below +inf: index 0
        assert np.all(o['idx'][:3] == 0)


# ------------------------------------------------------------------------------------------------------------------ c. backward
def backward_gate(e32, scale):
    """4x the error float32 autograd makes against float64, where that error is at least one float32 unit (2^-24) of the tensor's largest
    magnitude; below that the unit stands in for it (the rule and the reason of tests/test_mm_latent_host.py)."""
    return 4.0 * max(e32, UNIT * scale)


@pytest.mark.parametrize('kind', TRAIN_KINDS)
def test_host_backward_against_float64_autograd(kind):
    c = exact_train_case(kind)
    o = R.call_train(L, 'cpu', c)
    g64, g32 = R.autograd(c, torch.float64), R.autograd(c, torch.float32)
    ours = dict(enc=o['d_enc_out'], mean_p=o['d_mean_p'], lv_p=o['d_lv_p'])
    for k in g64:
        assert np.all(np.isfinite(ours[k])), k
        scale = max(float(np.abs(g64[k]).max()), 1e-30)
        e32 = float(np.abs(g32[k] - g64[k]).max())
        gate = backward_gate(e32, scale)
        err = float(np.abs(ours[k] - g64[k]).max())
        print('%s %s: |host - f64| %.3e, |f32 autograd - f64| %.3e, gate %.3e' % (kind, k, err, e32, gate))
        assert err <= gate, (k, err, gate)


@pytest.mark.parametrize('B,Lz', [(1, 1), (2, 16), (5, 16)])
def test_host_backward_on_fixture_shapes(B, Lz, golden):
    for c in golden['t']:
        if c['mean_p'].shape != (B, Lz):
            continue
        c = dict(c, dist=float(c['dist']), reg_weight=float(c['reg_weight']))
        o = R.call_train(L, 'cpu', c)
        g64, g32 = R.autograd(c, torch.float64), R.autograd(c, torch.float32)
        for k, got in (('enc', o['d_enc_out']), ('mean_p', o['d_mean_p']), ('lv_p', o['d_lv_p'])):
            gate = backward_gate(float(np.abs(g32[k] - g64[k]).max()), max(float(np.abs(g64[k]).max()), 1e-30))
            assert float(np.abs(got - g64[k]).max()) <= gate, (k, gate)


def test_null_prior_outputs():
    """A constant-log-variance prior network has no d_lv_p; either prior output may be NULL and the others do not change."""
    c = exact_train_case('random')
    o = R.call_train(L, 'cpu', c)
    n = R.call_train(L, 'cpu', c, null_lv=True)
    assert np.all(np.isnan(n['d_lv_p']))
    for k in ('d_enc_out', 'd_mean_p'):
        np.testing.assert_array_equal(o[k], n[k])
    n = R.call_train(L, 'cpu', c, null_mean=True, null_lv=True)
    assert np.all(np.isnan(n['d_mean_p'])) and np.all(np.isnan(n['d_lv_p']))
    np.testing.assert_array_equal(o['d_enc_out'], n['d_enc_out'])


def test_validation_comes_before_any_access():
    """Every pointer below is either NULL or one 16 KB block: a status comes back without a launch or a touch of memory."""
    lib = L.load()
    x = torch.zeros(4096)
    p = R._p(x)
    for fn, extra in (('vv_prior_latent_train_fwd_host', []), ('vv_prior_latent_train_fwd', [None])):
        f = getattr(lib, fn)
        ok = [p, p, p, p, p, None, 12.0, p, None, p, p]
        for k in (0, 1, 2, 3, 4, 7, 9, 10):
            a = list(ok)
            a[k] = None
            assert f(*a, 2, 4, *extra) == -1, (fn, k)
        for B, Lz in ((0, 4), (2, 0), (2, 65), (-1, 4)):
            assert f(*ok, B, Lz, *extra) == -2, (fn, B, Lz)
    for fn, extra in (('vv_prior_latent_train_bwd_host', []), ('vv_prior_latent_train_bwd', [None])):
        f = getattr(lib, fn)
        ok = [p, p, p, p, p, None, 12.0, p, 0.5, 0.01, p, None, None]
        for k in (0, 1, 2, 3, 4, 7, 10):
            a = list(ok)
            a[k] = None
            assert f(*a, 2, 4, *extra) == -1, (fn, k)
        for B, Lz in ((0, 4), (2, 0), (2, 65)):
            assert f(*ok, B, Lz, *extra) == -2, (fn, B, Lz)
    for fn, extra in (('vv_inst_latent_eval_host', []), ('vv_inst_latent_eval', [None])):
        f = getattr(lib, fn)
        ok = [p, p, None, None, p, p, p, None, None, p]
        for k in (0, 1, 4, 5, 6, 9):
            a = list(ok)
            a[k] = None
            assert f(*a, 2, 4, 3, *extra) == -1, (fn, k)
        for B, Lz, I in ((0, 4, 3), (2, 0, 3), (2, 65, 3), (2, 4, 0), (2, 4, 257)):
            assert f(*ok, B, Lz, I, *extra) == -2, (fn, B, Lz, I)
        mask_only, fill_only = list(ok), list(ok)
        mask_only[2], fill_only[3] = p, p
        assert f(*mask_only, 2, 4, 3, *extra) == -1 and f(*fill_only, 2, 4, 3, *extra) == -1
    assert float(x.abs().sum()) == 0.0


# ------------------------------------------------------------------------------------------------------------------ d. sanitizers
@pytest.mark.skipif(torch.cuda.is_available(), reason='sanitizer programs run on CPU-only machines')
def test_standalone_sanitizer_build(tmp_path):
    """The header and tests/prior_latent_main.cpp as ONE program of its own under the address and undefined-behaviour sanitizers, run on the CPU."""
    build_and_run_sanitized('prior_latent_main.cpp', tmp_path, 'prior_latent_asan')
