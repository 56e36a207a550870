"""CPU tests of the multi-modal latent stage: the host entries vv_mm_latent_*_host -- the code the kernels run, compiled for
the CPU -- against what the reference's own nolboSingleObject.getEval, kl_loss and regulizer_loss computed (tests/golden/mm_latent.npz,
recorded by tests/golden/make_mm_golden.py), against the numpy statement tests/_mm_ref.py on exact cases, and the backward against
float64 torch autograd.

Measured on the fixture (largest |host - fixture| over all cases, relative to max(|fixture|, 1)): z and z_corrected 2.4e-7, kl 3.4e-7,
reg 4.3e-7; the gates below are 4x these.  Backward: the host entry's error against float64 autograd is at most 2.04x the error float32
autograd of the same closure makes (gate 4x, computed in the test)."""
import os

import numpy as np
import pytest
import torch

from _common import build_and_run_sanitized
import _mm_ref as R
from voxvae import lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, 'tests', 'golden', 'mm_latent.npz')
Z_GATE, KL_GATE, REG_GATE = 4 * 2.4e-7, 4 * 3.4e-7, 4 * 4.3e-7


@pytest.fixture(scope='module')
def golden():
    from voxvae import build as vb
    vb.build()
    g = np.load(GOLDEN)
    cases = []
    for i in range(int(g['cases'])):
        c = {k[len('c%d_' % i):]: g[k] for k in g.files if k.startswith('c%d_' % i)}
        c.setdefault('mask', None), c.setdefault('eps2', None)
        cases.append(c)
    return cases


def _rel(a, b):
    return float((np.abs(a.astype(np.float64) - b) / np.maximum(np.abs(b), 1.0)).max())


def _eval_args(c):
    return [c[k] for k in ('enc_out', 'eps', 'mask', 'eps2', 'prior_cat', 'prior_inst', 'cat_onehot', 'inst_onehot')]


# ------------------------------------------------------------------------------------------------------------------ a. the fixture
def test_fixture_covers_the_cases_the_issue_names(golden):
    dims = [tuple(int(v) for v in c['dims']) for c in golden]
    assert {d[0] for d in dims} == {1, 2, 5, 72}
    assert any(d[1] != d[2] and (d[1] % 2 or d[2] % 2) for d in dims) and any(d[3] == 1 for d in dims) and any(d[4] == 1 for d in dims)
    assert {float(c['missing_prob']) for c in golden} == {0.0, 0.3, 0.9}


def test_host_eval_reproduces_the_reference(golden):
    worst = 0.0
    for c in golden:
        for name, fn in (('host', lambda: R.call_eval(L, 'cpu', *_eval_args(c))), ('numpy', lambda: R.eval_ref(*_eval_args(c)))):
            o = fn()
            n = c['idx'].shape[1]
            np.testing.assert_array_equal(o['idx'][:, :n], c['idx'], err_msg=name)
            np.testing.assert_array_equal(o['acc'][:len(c['acc'])], c['acc'], err_msg=name)
            d = _rel(o['z'], c['z'])
            if c['mask'] is not None:
                d = max(d, _rel(o['z_corr'], c['z_corrected']))
            else:
                assert np.array_equal(o['idx'][:, 2], o['idx'][:, 0]) and np.array_equal(o['idx'][:, 3], o['idx'][:, 0]) and o['acc'][2] == o['acc'][0]
            worst = max(worst, d)
    print('largest |z - fixture| (relative above 1): %.3e' % worst)
    assert worst <= Z_GATE


def test_host_losses_reproduce_the_reference(golden):
    wk = wr = 0.0
    for c in golden:
        B, Lc, Li = [int(v) for v in c['dims'][:3]]
        zeros = np.zeros((B, Lc + Li), np.float32)
        args = (c['enc_out'], zeros, c['mean_cp'], c['lv_cp'], c['mean_ip'], c['lv_ip'], zeros, None, c['cat_onehot'])
        for o in (R.call_train(L, 'cpu', *args, zeros), R.train_fwd_ref(*args)):
            wk, wr = max(wk, _rel(o['kl'], c['kl'])), max(wr, _rel(o['reg'], c['reg']))
    print('largest relative |kl - fixture| %.3e, |reg - fixture| %.3e' % (wk, wr))
    assert wk <= KL_GATE and wr <= REG_GATE


# ------------------------------------------------------------------------------------------------------------------ b. exact cases
def _agree(o, r, mask):
    np.testing.assert_array_equal(o['idx'], r['idx'])
    np.testing.assert_array_equal(o['acc'], r['acc'])
    keys = ('z', 'z_corr') if mask is not None else ('z',)
    for k in keys:
        assert np.array_equal(np.isnan(o[k]), np.isnan(r[k])), k
        fin = np.isfinite(r[k])
        assert np.array_equal(np.isfinite(o[k]), fin), k
        assert _rel(o[k][fin], r[k][fin]) <= Z_GATE if fin.any() else True, k


def _exact_case(kind):
    c = R.random_eval_case(7, 6, 5, 3, 4, 3, 0.4)
    if kind == 'duplicates':
        c['prior_cat'][2] = c['prior_cat'][0]
        c['prior_inst'][:, 1] = c['prior_inst'][:, 0]
        c['enc'][:, :5] = c['prior_cat'][2]
        c['enc'][:, 10:13] = c['prior_inst'][:, 1]
    elif kind == 'zeros':                        # unmasked elements that are exactly +0 and -0 after sampling
        c['mask'][:] = 1.0
        c['enc'][0, 0], c['eps'][0, 0] = 0.0, 0.0
        c['enc'][1, 1], c['eps'][1, 1] = -0.0, 0.0
    elif kind == 'all_masked':
        c['mask'][::2] = 0.0
    elif kind == 'nonfinite':
        c['enc'][0, 0], c['enc'][1, 1], c['enc'][2, 10] = np.nan, np.inf, np.nan
        c['enc'][3, :5] = -np.inf
    elif kind == 'clip':
        c['enc'][0, 5:10] = [10.0, -10.0, 10.000001, -37.5, 88.0]
        c['enc'][1, 13:16] = [-10.0, 1e30, -1e30]
    return c


@pytest.mark.parametrize('kind', ['duplicates', 'zeros', 'all_masked', 'nonfinite', 'clip'])
def test_host_eval_exact_cases(kind):
    c = _exact_case(kind)
    args = [c[k] for k in ('enc', 'eps', 'mask', 'eps2', 'prior_cat', 'prior_inst', 'cat_oh', 'inst_oh')]
    o, r = R.call_eval(L, 'cpu', *args), R.eval_ref(*args)
    _agree(o, r, c['mask'])
    if kind == 'duplicates':
        assert np.all(o['idx'][:, 1] == 0) and not np.any(o['idx'][:, 0] == 2)
    if kind == 'zeros':
        colmean = c['prior_cat'].mean(axis=0)
        assert abs(o['z'][0, 0] - colmean[0]) < 1e-6 and abs(o['z'][1, 1] - colmean[1]) < 1e-6
    if kind == 'nonfinite':
        assert o['idx'][0, 0] == 0 and o['idx'][1, 0] == 0 and o['idx'][2, 1] == 0 and o['idx'][3, 0] == 0
    if kind == 'all_masked':
        assert np.all(o['idx'][::2, 2] == 0)
    # without a mask
    args[2] = args[3] = None
    _agree(R.call_eval(L, 'cpu', *args), R.eval_ref(*args), None)


def _train_case(kind):
    if kind == 'B1':
        return R.random_train_case(3, 1, 5, 3, 4)
    c = R.random_train_case(4, 6, 5, 3, 2)
    if kind == 'identical_means':
        c['mean_cp'][3], c['mean_ip'][3], c['cat_oh'][3] = c['mean_cp'][0], c['mean_ip'][0], c['cat_oh'][0]
    elif kind == 'clip':
        c['enc'][0, 5:10] = [10.0, -10.0, 10.000001, -37.5, 12.0]
    elif kind == 'classes':
        c['cat_oh'][:] = np.eye(2, dtype=np.float32)[[0, 0, 1, 1, 0, 1]]
    elif kind == 'no_noise':
        c['noise'] = None
    return c


def _train_args(c):
    return [c[k] for k in ('enc', 'eps', 'mean_cp', 'lv_cp', 'mean_ip', 'lv_ip', 'eps_p', 'noise', 'cat_oh', 'dz_in')]


TRAIN_KINDS = ['B1', 'identical_means', 'clip', 'classes', 'no_noise', 'random']


@pytest.mark.parametrize('kind', TRAIN_KINDS)
def test_host_train_forward_exact_cases(kind):
    c = _train_case(kind)
    o, r = R.call_train(L, 'cpu', *_train_args(c)), R.train_fwd_ref(*_train_args(c)[:-1])
    assert _rel(o['z_in'], r['z_in']) <= Z_GATE and _rel(o['kl'], r['kl']) <= KL_GATE and _rel(o['reg'], r['reg']) <= REG_GATE
    if kind == 'B1':                                      # the only pair is the diagonal: distance 0, hinge (3 L)^2 per group
        assert o['reg'][0] == np.float32(15.0 ** 2 + 9.0 ** 2)
    if c['noise'] is not None:                            # the sense of the mix: noise == 0 keeps the posterior's sample
        keep = R.train_fwd_ref(*_train_args(c)[:7], None, c['cat_oh'])['z_in']
        assert _rel(o['z_in'][c['noise'] == 0], keep[c['noise'] == 0]) <= Z_GATE


# ------------------------------------------------------------------------------------------------------------------ c. backward
def _autograd(c, dtype):
    names = ('enc', 'eps', 'mean_cp', 'lv_cp', 'mean_ip', 'lv_ip', 'eps_p', 'noise', 'cat_oh', 'dz_in')
    t = {k: (None if c[k] is None else torch.from_numpy(c[k]).to(dtype)) for k in names}
    leaves = ['enc', 'mean_cp', 'lv_cp', 'mean_ip', 'lv_ip']
    for k in leaves:
        t[k].requires_grad_(True)
    # dz_in enters as d shape / d z_in: the closure adds <dz_in, z_in>; the entry takes total = mean kl + mean reg + shape
    R.total_torch(*[t[k] for k in names]).backward()
    return {k: t[k].grad.numpy().astype(np.float64) for k in leaves}


def backward_gate(e32, scale):
    """4x the error float32 autograd makes against float64, where that error is at least one float32 unit (2^-24) of the tensor's
    largest magnitude; below that the unit stands in for it: no float32 result can be asked to sit closer than half a spacing to the
    float64 value, and float32 autograd gets there only by the luck of its roundings.  Measured over the thirty (case, tensor) pairs
    below: the unit decides exactly ONE, d_enc_out of 'clip' (log-variance +10: largest element 2158, spacing 2.44e-4; the host is off
    by 2.37e-4 = 1.85 units, float32 autograd by 6.7e-6 = 0.05 units); every other pair is within 2.04x float32 autograd's own error."""
    return 4.0 * max(e32, 2.0 ** -24 * scale)


@pytest.mark.parametrize('kind', TRAIN_KINDS)
def test_host_backward_against_float64_autograd(kind):
    c = _train_case(kind)
    o = R.call_train(L, 'cpu', *_train_args(c))
    g64, g32 = _autograd(c, torch.float64), _autograd(c, torch.float32)
    ours = dict(enc=o['d_enc_out'], mean_cp=o['d_mean_cp'], lv_cp=o['d_lv_cp'], mean_ip=o['d_mean_ip'], lv_ip=o['d_lv_ip'])
    for k in g64:
        assert np.all(np.isfinite(ours[k])), k
        scale = max(float(np.abs(g64[k]).max()), 1e-30)
        e32 = float(np.abs(g32[k] - g64[k]).max())
        gate = backward_gate(e32, scale)
        err = float(np.abs(ours[k] - g64[k]).max())
        print('%s %s: |host - f64| %.3e, |f32 autograd - f64| %.3e, ratio %.2f' % (kind, k, err, e32, 4.0 * err / gate))
        assert err <= gate, (k, err, gate)
    if kind == 'identical_means':
        assert np.all(np.isfinite(o['d_mean_cp'][[0, 3]]))
    if kind == 'clip':                                    # raw exactly +-10 passes, beyond does not
        assert o['d_enc_out'][0, 5] != 0 and o['d_enc_out'][0, 6] != 0 and np.all(o['d_enc_out'][0, 7:10] == 0)


def test_null_prior_outputs_and_validation():
    c = _train_case('random')
    o, n = R.call_train(L, 'cpu', *_train_args(c)), R.call_train(L, 'cpu', *_train_args(c), null_lv=True)
    assert np.all(np.isnan(n['d_lv_cp'])) and np.all(np.isnan(n['d_lv_ip']))
    for k in ('d_enc_out', 'd_mean_cp', 'd_mean_ip'):
        np.testing.assert_array_equal(o[k], n[k])
    lib = L.load()
    x = torch.zeros(4096)
    p = R._p(x)
    for fn, extra in (('vv_mm_latent_eval_host', []), ('vv_mm_latent_eval', [None])):          # validation comes before any launch
        f = getattr(lib, fn)
        base = lambda mask, eps2, zc, B=2, Lc=4, Li=4, C=3, I=3, dt=0, za=None: f(p, p, mask, eps2, p, p, p, p, p, zc, za, None, dt, p, p, B, Lc,
                                                                                  Li, C, I, *extra)
        assert base(None, None, None, B=0) == -2 and base(None, None, None, Lc=65) == -2 and base(None, None, None, Li=0) == -2
        assert base(None, None, None, C=257) == -2 and base(None, None, None, I=0) == -2
        assert base(p, None, p) == -1 and base(None, p, p) == -1 and base(p, p, None) == -1
        assert base(None, None, None, dt=2, za=p) == -3                                            # the rule of vv_latent_mask_fill
        assert f(None, p, None, None, p, p, p, p, p, None, None, None, 0, p, p, 2, 4, 4, 3, 3, *extra) == -1
    for fn, extra in (('vv_mm_latent_train_fwd_host', []), ('vv_mm_latent_train_fwd', [None])):
        f = getattr(lib, fn)
        assert f(p, p, p, p, p, p, p, None, p, p, None, 0, p, p, 2, 4, 65, 3, *extra) == -2
        assert f(p, p, p, None, p, p, p, None, p, p, None, 0, p, p, 2, 4, 4, 3, *extra) == -1
    for fn, extra in (('vv_mm_latent_train_bwd_host', []), ('vv_mm_latent_train_bwd', [None])):
        f = getattr(lib, fn)
        assert f(p, p, p, p, p, p, p, None, p, p, 0.5, p, None, None, None, None, 0, 4, 4, 3, *extra) == -2
        assert f(p, p, p, p, p, p, p, None, p, None, 0.5, p, None, None, None, None, 2, 4, 4, 3, *extra) == -1


# ------------------------------------------------------------------------------------------------------------------ d. sanitizers
@pytest.mark.skipif(torch.cuda.is_available(), reason='sanitizer programs run on CPU-only machines')
def test_standalone_sanitizer_build(tmp_path):
    """The header and tests/mm_latent_main.cpp as ONE program of its own under the address and undefined-behaviour sanitizers, run on the CPU."""
    build_and_run_sanitized('mm_latent_main.cpp', tmp_path, 'mm_latent_asan')
