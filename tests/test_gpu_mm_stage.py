"""GPU tests of voxvae/mm_latent.py, the callers of the two-prior latent stage: latent_stage (the autograd node of nolboSingleObject.fit)
against direct train_fwd + train_bwd calls and against the entries called with their raw argument lists (tests/_mm_ref.call_train), and
eval against the entry called the way nolboSingleObject.getEval called it inline -- all BIT FOR BIT on seeded inputs.  The shape
B = 5, Lc = 3, Li = 2, C = 3 (I = 2) is the smallest with several pairs per row, both latent groups, and samples that share and do not
share a class; what the entries compute is pinned by tests/test_gpu_mm_latent.py."""
import numpy as np
import pytest
import torch

import _mm_ref as R
from voxvae import lib as L
from voxvae import mm_latent as ML

pytestmark = pytest.mark.gpu
DEV = 'cuda'
B, LC, LI, C, I = 5, 3, 2, 3, 2
PRI = ('mean_cp', 'lv_cp', 'mean_ip', 'lv_ip')


def _bits(t):
    return None if t is None else t.detach().cpu().contiguous().view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32).numpy()


def _same(got, want, what):
    assert (got is None) == (want is None), what
    if got is not None:
        g, w = (_bits(x) if torch.is_tensor(x) else np.ascontiguousarray(x).view(np.int32) for x in (got, want))
        assert g.shape == w.shape and np.array_equal(g, w), what


@pytest.mark.parametrize('const_lv,noise,bf16', [(False, True, False), (True, True, False), (False, False, False), (False, True, True)])
def test_latent_stage_is_train_fwd_and_train_bwd(const_lv, noise, bf16, monkeypatch):
    c = R.random_train_case(3, B, LC, LI, C, noise=noise)
    classes = c['cat_oh'].argmax(1)
    assert 1 < len(set(classes)) < B                                   # samples that share a class and samples that do not
    t = {k: (None if v is None else torch.from_numpy(v).to(DEV)) for k, v in c.items()}
    pri = [t[k].clone().requires_grad_(not (const_lv and k.startswith('lv'))) for k in PRI]
    e = t['enc'].clone().requires_grad_(True)
    calls = []
    real = L.call
    monkeypatch.setattr(L, 'call', lambda name, *a: (calls.append((name, a)), real(name, *a))[1])
    z_in, extra, kl, reg, twin = ML.latent_stage(e, *pri, t['eps'], t['eps_p'], t['noise'], t['cat_oh'], bf16=bf16)
    z_in.backward(t['dz_in'])
    torch.cuda.synchronize()
    monkeypatch.undo()
    assert [n for n, _ in calls] == ['vv_mm_latent_train_fwd', 'vv_mm_latent_train_bwd']
    # ..., dz_in, inv_batch, d_enc_out, d_mean_cp, d_lv_cp, d_mean_ip, d_lv_ip, B, Lc, Li, C, stream: a constant log-variance gets NULL
    bwd = calls[1][1]
    assert bwd[10] == 1.0 / B and [bwd[k] is None for k in (11, 12, 13, 14, 15)] == [False, False, const_lv, False, const_lv]
    assert not (kl.requires_grad or reg.requires_grad) and z_in.requires_grad and extra.requires_grad
    # the module's own two calls on the same tensors
    pri4 = [t[k] for k in PRI]
    want = tuple(not (const_lv and k.startswith('lv')) for k in PRI)
    fz, ftwin, fkl, freg = ML.train_fwd(t['enc'], t['eps'], pri4, t['eps_p'], t['noise'], t['cat_oh'], bf16=bf16)
    grads = ML.train_bwd(t['enc'], t['eps'], pri4, t['eps_p'], t['noise'], t['cat_oh'], t['dz_in'], 1.0 / B, want=want)
    for got, ref, what in ((z_in, fz, 'z_in'), (kl, fkl, 'kl'), (reg, freg, 'reg'), (twin, ftwin, 'twin'), (extra, fkl.mean() + freg.mean(), 'extra'),
                           (e.grad, grads[0], 'd_enc_out')) + tuple((p.grad, g, 'd_' + k) for p, g, k in zip(pri, grads[1:], PRI)):
        _same(got, ref, what)
    assert [g is None for g in grads[1:]] == [not w for w in want] == [p.grad is None for p in pri]
    # the entries with their raw argument lists
    raw = R.call_train(L, DEV, *[c[k] for k in ('enc', 'eps') + PRI + ('eps_p', 'noise', 'cat_oh', 'dz_in')], act='bf16' if bf16 else None, null_lv=const_lv)
    for k, got in (('z_in', z_in), ('kl', kl), ('reg', reg), ('d_enc_out', e.grad), ('d_mean_cp', pri[0].grad), ('d_mean_ip', pri[2].grad)) + (
            () if const_lv else (('d_lv_cp', pri[1].grad), ('d_lv_ip', pri[3].grad))):
        _same(got, raw[k], 'raw ' + k)
    if bf16:                                                            # the twin is vv_le_bf16 of z_in: round to nearest even on finite values
        assert twin.dtype == torch.bfloat16 and bool(torch.isfinite(z_in).all()) and torch.equal(twin, z_in.detach().to(torch.bfloat16))
    else:
        assert twin is None


@pytest.mark.parametrize('act', ['f32', 'bf16'])
@pytest.mark.parametrize('masked', [False, True])
def test_eval_is_the_inline_call(masked, act):
    c = R.random_eval_case(4, B, LC, LI, C, I, 0.4 if masked else 0.0)
    names = ('enc', 'eps', 'mask', 'eps2', 'prior_cat', 'prior_inst', 'cat_oh', 'inst_oh')
    t = [None if c[k] is None else torch.from_numpy(c[k]).to(DEV) for k in names]
    z, zc, z_act, zc_act, idx, acc = ML.eval(*t, L.VV_BF16 if act == 'bf16' else L.VV_F32)
    torch.cuda.synchronize()
    # what getEval allocated inline: no corrected latent without a mask, twins only in bf16
    assert (zc is not None) == masked and (z_act is not None) == (act == 'bf16') and (zc_act is not None) == (masked and act == 'bf16')
    assert tuple(idx.shape) == (B, 4) and idx.dtype == torch.int32 and tuple(acc.shape) == (3,)
    raw = R.call_eval(L, DEV, *[c[k] for k in names], act='bf16' if act == 'bf16' else None)
    _same(z, raw['z'], 'z'), _same(idx, raw['idx'], 'idx')
    np.testing.assert_array_equal(acc.cpu().numpy()[:3 if masked else 2], raw['acc'][:3 if masked else 2])
    if masked:
        _same(zc, raw['z_corr'], 'z_corr')
    if act == 'bf16':
        assert torch.equal(z_act.float().cpu(), torch.from_numpy(raw['z_act']))
        if masked:
            assert torch.equal(zc_act.float().cpu(), torch.from_numpy(raw['z_corr_act']))
