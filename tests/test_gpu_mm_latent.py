"""GPU tests of the multi-modal latent stage: the device entries vv_mm_latent_eval / _train_fwd / _train_bwd equal their host
twins BIT FOR BIT (what the host twins compute is pinned on the CPU, tests/test_mm_latent_host.py) on the fixture cases, the exact cases
and the limits; the bf16 twins are the round-to-nearest-even of the float32 outputs; guard-banded buffers stay intact and a second run
gives the same bits."""
import ctypes
import os

import numpy as np
import pytest
import torch

import _guarded as G
import _mm_ref as R
import test_mm_latent_host as H
from voxvae import lib as L

pytestmark = pytest.mark.gpu
DEV = 'cuda'


def _same_bits(a, b, what):
    for k in a:
        assert a[k].dtype == b[k].dtype and a[k].shape == b[k].shape, (what, k)
        x, y = np.ascontiguousarray(a[k]), np.ascontiguousarray(b[k])
        if x.dtype == np.float32:                              # a NaN must meet a NaN (its payload is the platform's); all else bit for bit
            nan = np.isnan(y)
            assert np.array_equal(np.isnan(x), nan), '%s: %s: NaNs differ between device and host' % (what, k)
            x, y = np.where(nan, np.float32(0), x), np.where(nan, np.float32(0), y)
        assert np.array_equal(x.view(np.uint32), y.view(np.uint32)), '%s: %s differs between device and host' % (what, k)


def _bf16_is_rne(o, pairs):
    for f32, act in pairs:
        want = torch.from_numpy(o[f32]).to(torch.bfloat16).float().numpy()
        fin = np.isfinite(o[f32])
        assert np.array_equal(o[act][fin], want[fin]), act


@pytest.fixture(scope='module')
def golden():
    g = np.load(H.GOLDEN)
    cases = []
    for i in range(int(g['cases'])):
        c = {k[len('c%d_' % i):]: g[k] for k in g.files if k.startswith('c%d_' % i)}
        c.setdefault('mask', None), c.setdefault('eps2', None)
        cases.append(c)
    return cases


def test_eval_fixture_cases_bit_for_bit(golden):
    for i, c in enumerate(golden):
        for act in (None, 'bf16'):
            d, h = R.call_eval(L, DEV, *H._eval_args(c), act=act), R.call_eval(L, 'cpu', *H._eval_args(c), act=act)
            _same_bits(d, h, 'fixture case %d act %s' % (i, act))
        _bf16_is_rne(d, [('z', 'z_act')] + ([('z_corr', 'z_corr_act')] if c['mask'] is not None else []))
        np.testing.assert_array_equal(d['idx'][:, :c['idx'].shape[1]], c['idx'])
        np.testing.assert_array_equal(d['acc'][:len(c['acc'])], c['acc'])


def test_train_fixture_cases_bit_for_bit(golden):
    for i, c in enumerate(golden):
        B, Lc, Li = [int(v) for v in c['dims'][:3]]
        rng = np.random.default_rng(i)
        f = lambda *s: rng.normal(0, 1, s).astype(np.float32)
        noise = rng.integers(0, 2, (B, Lc + Li)).astype(np.float32) if i % 2 else None
        args = (c['enc_out'], f(B, Lc + Li), c['mean_cp'], c['lv_cp'], c['mean_ip'], c['lv_ip'], f(B, Lc + Li), noise, c['cat_onehot'], f(B, Lc + Li))
        d, h = R.call_train(L, DEV, *args, act='bf16'), R.call_train(L, 'cpu', *args, act='bf16')
        _same_bits(d, h, 'fixture case %d' % i)
        _bf16_is_rne(d, [('z_in', 'z_in_act')])


@pytest.mark.parametrize('kind', ['duplicates', 'zeros', 'all_masked', 'nonfinite', 'clip'])
def test_eval_exact_cases_bit_for_bit(kind):
    c = H._exact_case(kind)
    args = [c[k] for k in ('enc', 'eps', 'mask', 'eps2', 'prior_cat', 'prior_inst', 'cat_oh', 'inst_oh')]
    _same_bits(R.call_eval(L, DEV, *args, act='f32'), R.call_eval(L, 'cpu', *args, act='f32'), kind)
    args[2] = args[3] = None
    _same_bits(R.call_eval(L, DEV, *args), R.call_eval(L, 'cpu', *args), kind + ' without a mask')


@pytest.mark.parametrize('kind', H.TRAIN_KINDS)
def test_train_exact_cases_bit_for_bit(kind):
    c = H._train_case(kind)
    _same_bits(R.call_train(L, DEV, *H._train_args(c)), R.call_train(L, 'cpu', *H._train_args(c)), kind)
    _same_bits(R.call_train(L, DEV, *H._train_args(c), null_lv=True), R.call_train(L, 'cpu', *H._train_args(c), null_lv=True), kind + ' NULL outputs')


def test_limits_bit_for_bit():
    """B = 257 (a second piece of the pair sums and of the strided partials), C = I = 256, Lc = Li = 64."""
    c = R.random_eval_case(11, 257, 64, 64, 256, 256, 0.3)
    args = [c[k] for k in ('enc', 'eps', 'mask', 'eps2', 'prior_cat', 'prior_inst', 'cat_oh', 'inst_oh')]
    _same_bits(R.call_eval(L, DEV, *args, act='bf16'), R.call_eval(L, 'cpu', *args, act='bf16'), 'eval at the limits')
    t = R.random_train_case(12, 257, 64, 64, 256)
    _same_bits(R.call_train(L, DEV, *H._train_args(t)), R.call_train(L, 'cpu', *H._train_args(t)), 'training at the limits')


def test_guard_bands_and_repeat_runs():
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    for B, Lc, Li, C, I in ((1, 7, 12, 12, 10), (5, 3, 9, 12, 1), (72, 8, 8, 12, 10)):
        c = R.random_eval_case(B, B, Lc, Li, C, I, 0.3)
        t = R.random_train_case(B + 1, B, Lc, Li, C)
        runs = []
        for _ in range(2):
            a = G.Arena('cuda:0')
            tin = lambda x, n: a.input(torch.from_numpy(x), n)
            ev = [tin(c[k], k) for k in ('enc', 'eps', 'mask', 'eps2', 'prior_cat', 'prior_inst', 'cat_oh', 'inst_oh')]
            z, zc = a.output((B, Lc + Li), torch.float32, 'z'), a.output((B, Lc + Li), torch.float32, 'z_corr')
            za, zca = a.output((B, Lc + Li), torch.bfloat16, 'z_act'), a.output((B, Lc + Li), torch.bfloat16, 'z_corr_act')
            idx, acc = a.output((B, 4), torch.int32, 'idx'), a.output((3,), torch.float32, 'acc')
            tr = [tin(t[k], 't_' + k) for k in ('enc', 'eps', 'mean_cp', 'lv_cp', 'mean_ip', 'lv_ip', 'eps_p', 'noise', 'cat_oh')]
            dz = tin(t['dz_in'], 'dz_in')
            zin, zina = a.output((B, Lc + Li), torch.float32, 'z_in'), a.output((B, Lc + Li), torch.bfloat16, 'z_in_act')
            kl, reg = a.output((B,), torch.float32, 'kl'), a.output((B,), torch.float32, 'reg')
            outs = [a.output(s, torch.float32, n) for n, s in (('d_enc_out', (B, 2 * Lc + 2 * Li)), ('d_mean_cp', (B, Lc)), ('d_lv_cp', (B, Lc)),
                                                               ('d_mean_ip', (B, Li)), ('d_lv_ip', (B, Li)))]
            a.commit()
            L.call('vv_mm_latent_eval', *[b.ptr for b in ev], z.ptr, zc.ptr, za.ptr, zca.ptr, L.VV_BF16, idx.ptr, acc.ptr, B, Lc, Li, C, I, st)
            L.call('vv_mm_latent_train_fwd', *[b.ptr for b in tr], zin.ptr, zina.ptr, L.VV_BF16, kl.ptr, reg.ptr, B, Lc, Li, C, st)
            L.call('vv_mm_latent_train_bwd', *[b.ptr for b in tr], dz.ptr, 1.0 / B, *[b.ptr for b in outs], B, Lc, Li, C, st)
            torch.cuda.synchronize()
            a.check()
            written = [z, zc, za, zca, idx, acc, zin, zina, kl, reg] + outs
            runs.append([b.payload.clone() for b in written])
            for b in written:                                  # every element of every output was written: no element still holds the pre-fill
                assert not bool((b.payload.view(torch.uint8).reshape(-1, b.tensor.element_size()) == G.POISON).all(dim=1).any()), b.name
        for x, y in zip(*runs):
            assert torch.equal(x, y)
