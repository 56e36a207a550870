"""GPU tests of the one-group, one-prior latent stage: the device entries vv_prior_latent_train_fwd / _bwd and vv_inst_latent_eval equal
their host twins BIT FOR BIT (what the host twins compute is pinned on the CPU, tests/test_prior_latent_host.py) on the fixture cases,
the exact cases and the limits; a NaN meets a NaN; the bfloat16 twins are the round-to-nearest-even of the float32 outputs;
guard-banded buffers stay intact for all three entries, NULL optional outputs included, and a second run gives the same bits."""
import ctypes

import numpy as np
import pytest
import torch

import _guarded as G
import _prior_ref as R
import test_prior_latent_host as H
from voxvae import lib as L

pytestmark = pytest.mark.gpu
DEV = 'cuda'


def _same_bits(a, b, what):
    assert set(a) == set(b), what
    for k in a:
        assert a[k].dtype == b[k].dtype and a[k].shape == b[k].shape, (what, k)
        x, y = np.ascontiguousarray(a[k]), np.ascontiguousarray(b[k])
        if x.dtype == np.float32:                              # a NaN must meet a NaN (its payload is the platform's); all else bit for bit
            nan = np.isnan(y)
            assert np.array_equal(np.isnan(x), nan), '%s: %s: NaNs differ between device and host' % (what, k)
            x, y = np.where(nan, np.float32(0), x).view(np.uint32), np.where(nan, np.float32(0), y).view(np.uint32)
        assert np.array_equal(x, y), '%s: %s differs between device and host' % (what, k)


def _bf16_is_rne(o, pairs):
    for f32, twin in pairs:
        want = torch.from_numpy(o[f32]).to(torch.bfloat16).float().numpy()
        fin = np.isfinite(o[f32])
        assert np.array_equal(R.bf16_to_f32(o[twin])[fin], want[fin]), twin
        assert np.array_equal(np.isnan(R.bf16_to_f32(o[twin])), np.isnan(o[f32])), twin


@pytest.fixture(scope='module')
def golden():
    return H.load_golden()


def test_train_fixture_cases_bit_for_bit(golden):
    for i, c in enumerate(golden['t']):
        c = dict(c, dist=float(c['dist']), reg_weight=float(c['reg_weight']))
        d, h = R.call_train(L, DEV, c, bf16=True), R.call_train(L, 'cpu', c, bf16=True)
        _same_bits(d, h, 'training fixture case %d' % i)
        _bf16_is_rne(d, [('z_in', 'z_in_bf16')])


def test_eval_fixture_cases_bit_for_bit(golden):
    for i, c in enumerate(golden['e']):
        d, h = R.call_eval(L, DEV, c, bf16=True), R.call_eval(L, 'cpu', c, bf16=True)
        _same_bits(d, h, 'evaluation fixture case %d' % i)
        _bf16_is_rne(d, [('z', 'z_bf16'), ('z_corr', 'z_corr_bf16')])
        np.testing.assert_array_equal(d['idx'], c['idx'])


@pytest.mark.parametrize('kind', H.TRAIN_KINDS)
def test_train_exact_cases_bit_for_bit(kind):
    c = H.exact_train_case(kind)
    _same_bits(R.call_train(L, DEV, c), R.call_train(L, 'cpu', c), kind)
    _same_bits(R.call_train(L, DEV, c, null_lv=True), R.call_train(L, 'cpu', c, null_lv=True), kind + ' NULL d_lv_p')
    _same_bits(R.call_train(L, DEV, c, null_mean=True, null_lv=True), R.call_train(L, 'cpu', c, null_mean=True, null_lv=True), kind + ' NULL prior outputs')


@pytest.mark.parametrize('kind', H.EVAL_KINDS)
def test_eval_exact_cases_bit_for_bit(kind):
    c = H.exact_eval_case(kind)
    _same_bits(R.call_eval(L, DEV, c, bf16=True), R.call_eval(L, 'cpu', c, bf16=True), kind)
    c = dict(c, mask=None, fill=None)
    _same_bits(R.call_eval(L, DEV, c), R.call_eval(L, 'cpu', c), kind + ' without a mask')


def test_train_nonfinite_inputs_bit_for_bit():
    """NaN and infinities in the head output and in the prior outputs: the same NaNs in the same places on both sides."""
    c = R.train_case(51, 6, 5)
    c['enc'][0, 0], c['enc'][1, 6], c['enc'][2, 1] = np.nan, np.inf, -np.inf
    c['mean_p'][3, 2], c['lv_p'][4, 0] = np.nan, 1e30
    _same_bits(R.call_train(L, DEV, c), R.call_train(L, 'cpu', c), 'non-finite inputs')


@pytest.mark.parametrize('B,Lz', [(257, 64), (65, 1)])
def test_train_limits_bit_for_bit(B, Lz):
    """(257, 64): past four whole pieces of the pair sums, the widest latent, a last workgroup with one live row; (65, 1): a second
    piece of one row, the narrowest latent."""
    c = R.train_case(60 + Lz, B, Lz)
    c['mean_p'] *= 0.25                                        # keep a good share of the pairs inside the hinge at L = 64
    d, h = R.call_train(L, DEV, c, bf16=True), R.call_train(L, 'cpu', c, bf16=True)
    assert float(np.count_nonzero(h['reg'] > np.float32(c['dist']) ** 2)) > 0     # pairs beside the diagonal count
    _same_bits(d, h, 'training at (%d, %d)' % (B, Lz))


def test_eval_limits_bit_for_bit():
    """I = 256: every thread of the workgroup holds a prior row; L = 64."""
    c = R.eval_case(70, 9, 64, 256, 0.3)
    _same_bits(R.call_eval(L, DEV, c, bf16=True), R.call_eval(L, 'cpu', c, bf16=True), 'evaluation at I = 256')
    c = R.eval_case(71, 3, 1, 256, 0.0)
    _same_bits(R.call_eval(L, DEV, c), R.call_eval(L, 'cpu', c), 'evaluation at I = 256, L = 1')


@pytest.mark.parametrize('optional', [True, False])
def test_guard_bands_and_repeat_runs(optional):
    """Every buffer of the three device entries between guard bands (tests/_guarded.Arena): inputs and guards unchanged, every element
    of every output written, the same bits on a second run.  optional=False: keep / mask / fill and every optional output NULL."""
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    for B, Lz, I in ((1, 7, 10), (5, 3, 1), (70, 16, 33)):
        t, e = R.train_case(B, B, Lz, keep=optional), R.eval_case(B + 1, B, Lz, I, 0.3 if optional else 0.0)
        runs = []
        for _ in range(2):
            a = G.Arena('cuda:0')
            tin = lambda x, n: None if x is None else a.input(torch.from_numpy(x), n)
            ptr = lambda b: None if b is None else b.ptr
            tr = [tin(t[k], 't_' + k) for k in R.TRAIN_KEYS[:-1]]
            dz = tin(t['dz_in'], 'dz_in')
            zin, kl, reg = a.output((B, Lz), torch.float32, 'z_in'), a.output((B,), torch.float32, 'kl'), a.output((B,), torch.float32, 'reg')
            de = a.output((B, 2 * Lz), torch.float32, 'd_enc_out')
            ev = [tin(e[k], 'e_' + k) for k in R.EVAL_KEYS]
            z, zc, idx = a.output((B, Lz), torch.float32, 'z'), a.output((B, Lz), torch.float32, 'z_corr'), a.output((B,), torch.int32, 'idx')
            opt = []
            if optional:
                opt = [a.output((B, Lz), torch.bfloat16, 'z_in_bf16'), a.output((B, Lz), torch.float32, 'd_mean_p'), a.output((B, Lz), torch.float32, 'd_lv_p'),
                       a.output((B, Lz), torch.bfloat16, 'z_bf16'), a.output((B, Lz), torch.bfloat16, 'z_corr_bf16')]
            zinb, dm, dlv, zb, zcb = opt if optional else [None] * 5
            a.commit()
            L.call('vv_prior_latent_train_fwd', *[ptr(b) for b in tr], t['dist'], zin.ptr, ptr(zinb), kl.ptr, reg.ptr, B, Lz, st)
            L.call('vv_prior_latent_train_bwd', *[ptr(b) for b in tr], t['dist'], dz.ptr, 1.0 / B, t['reg_weight'], de.ptr, ptr(dm), ptr(dlv), B, Lz, st)
            L.call('vv_inst_latent_eval', *[ptr(b) for b in ev], z.ptr, zc.ptr, ptr(zb), ptr(zcb), idx.ptr, B, Lz, I, st)
            torch.cuda.synchronize()
            a.check()
            written = [zin, kl, reg, de, z, zc, idx] + opt
            runs.append([b.payload.clone() for b in written])
            for b in written:                                  # every element of every output was written: no element still holds the pre-fill
                assert not bool((b.payload.view(torch.uint8).reshape(-1, b.tensor.element_size()) == G.POISON).all(dim=1).any()), b.name
        for x, y in zip(*runs):
            assert torch.equal(x, y)
