"""The latent stage of nolboSingleObject (reference nolbo.py:93-147, :183-252; function.py:35-98) restated in numpy float32, with every sum in
index order (the order csrc/mm_latent.h uses), and the callers of the vv_mm_latent_* entries the tests share.  Held to the fixture
tests/golden/mm_latent.npz by tests/test_mm_latent_host.py, like the host entries."""
import numpy as np
import torch

from _common import _np, _p, _stream, _t, first_argmin as _first_argmin

F = np.float32


def _seq_sum(x):
    """Sum over the last axis in index order, float32."""
    s = np.zeros(x.shape[:-1], F)
    for j in range(x.shape[-1]):
        s = (s + x[..., j]).astype(F)
    return s


def split(enc, Lc, Li):
    lv = lambda x: np.minimum(np.maximum(x, F(-10)), F(10))
    return enc[:, :Lc], lv(enc[:, Lc:2 * Lc]), enc[:, 2 * Lc:2 * Lc + Li], lv(enc[:, 2 * Lc + Li:])


def sample(mean, lv, eps):
    with np.errstate(all='ignore'):
        return (mean + (np.sqrt(np.exp(lv.astype(F))) * eps).astype(F)).astype(F)


def eval_ref(enc, eps, mask, eps2, prior_cat, prior_inst, cat_oh, inst_oh):
    B, (C, Lc), Li = enc.shape[0], prior_cat.shape, prior_inst.shape[2]
    with np.errstate(all='ignore'):
        mc, lc, mi, li = split(enc, Lc, Li)
        zc, zi = sample(mc, lc, eps[:, :Lc]), sample(mi, li, eps[:, Lc:])
        if mask is not None:
            colmean = (_seq_sum(np.ascontiguousarray(prior_cat.T)) / F(C)).astype(F)
            zc = (zc * mask).astype(F)
            zc = np.where(zc == 0, colmean[None, :] * np.ones_like(zc), zc).astype(F)
        sq = lambda z, p: np.square((z[:, None, :] - p).astype(F)).astype(F)
        idx = np.zeros((B, 4), np.int32)
        idx[:, 0] = _first_argmin(_seq_sum(sq(zc, prior_cat[None])))
        idx[:, 1] = _first_argmin(_seq_sum(sq(zi, prior_inst)))
        idx[:, 2] = idx[:, 3] = idx[:, 0]
        out = dict(z=np.concatenate([zc, zi], axis=1))
        if mask is not None:
            idx[:, 2] = _first_argmin(_seq_sum((mask[:, None, :] * sq(zc, prior_cat[None])).astype(F)))
            zcc = np.where(mask == 0, (prior_cat[idx[:, 2]] + eps2).astype(F), zc).astype(F)
            idx[:, 3] = _first_argmin(_seq_sum(sq(zcc, prior_cat[None])))
            out['z_corr'] = np.concatenate([zcc, zi], axis=1)
    tc, ti = np.argmax(cat_oh, axis=1), np.argmax(inst_oh, axis=1)
    out['idx'] = idx
    out['acc'] = np.asarray([F((idx[:, 0] == tc).sum()) / F(B), F((idx[:, 1] == ti).sum()) / F(B), F((idx[:, 3] == tc).sum()) / F(B)], F)
    return out


def _reg(mean, lv, dist, cls=None):
    with np.errstate(all='ignore'):
        d = _seq_sum((np.abs((mean[:, None, :] - mean[None, :, :]).astype(F)) / np.exp((F(0.5) * lv).astype(F))[:, None, :]).astype(F))
        x = (d - F(dist)).astype(F)
        v = np.where(x > 0, F(0), np.square(x)).astype(F)
        if cls is not None:
            cd = _seq_sum(np.abs(cls[:, None, :] - cls[None, :, :]).astype(F))
            v = (v * np.where(cd > 0, F(0), F(1))).astype(F)
        return _seq_sum(v)                       # B <= 256: the strided partials are the terms themselves


def _kl(m, lv, mt, lvt):
    with np.errstate(all='ignore'):
        a = (F(0.5) * (lvt - lv)).astype(F)
        q = ((np.exp(lv) + np.square((m - mt).astype(F))).astype(F) / (F(2) * np.exp(lvt)).astype(F)).astype(F)
        return _seq_sum(((a + q).astype(F) - F(0.5)).astype(F))


def train_fwd_ref(enc, eps, mean_cp, lv_cp, mean_ip, lv_ip, eps_p, noise, cat_oh):
    Lc, Li = mean_cp.shape[1], mean_ip.shape[1]
    mc, lc, mi, li = split(enc, Lc, Li)
    z = np.concatenate([sample(mc, lc, eps[:, :Lc]), sample(mi, li, eps[:, Lc:])], axis=1)
    zp = np.concatenate([sample(mean_cp, lv_cp, eps_p[:, :Lc]), sample(mean_ip, lv_ip, eps_p[:, Lc:])], axis=1)
    z_in = z if noise is None else np.where(noise == 0, z, zp).astype(F)
    kl = (_kl(mc, lc, mean_cp, lv_cp) + _kl(mi, li, mean_ip, lv_ip)).astype(F)
    reg = (_reg(mean_cp, lv_cp, 3.0 * Lc) + _reg(mean_ip, lv_ip, 3.0 * Li, cat_oh)).astype(F)
    return dict(z_in=z_in, kl=kl, reg=reg)


def total_torch(enc, eps, mean_cp, lv_cp, mean_ip, lv_ip, eps_p, noise, cat_oh, dz_in):
    """total = mean_b kl + mean_b reg + <dz_in, z_in> as a torch closure in the dtype of its arguments (the restated fit algebra)."""
    Lc, Li = mean_cp.shape[1], mean_ip.shape[1]
    mc, lc, mi, li = enc[:, :Lc], enc[:, Lc:2 * Lc].clamp(-10, 10), enc[:, 2 * Lc:2 * Lc + Li], enc[:, 2 * Lc + Li:].clamp(-10, 10)
    smp = lambda m, lv, e: m + torch.sqrt(torch.exp(lv)) * e
    z = torch.cat([smp(mc, lc, eps[:, :Lc]), smp(mi, li, eps[:, Lc:])], dim=1)
    zp = torch.cat([smp(mean_cp, lv_cp, eps_p[:, :Lc]), smp(mean_ip, lv_ip, eps_p[:, Lc:])], dim=1)
    z_in = z if noise is None else torch.where(noise == 0, z, zp)
    kl = lambda m, lv, mt, lvt: (0.5 * (lvt - lv) + (torch.exp(lv) + (m - mt) ** 2) / (2.0 * torch.exp(lvt)) - 0.5).sum(-1)

    def reg(mean, lv, dist, cls=None):
        d = ((mean[:, None, :] - mean[None, :, :]).abs() / torch.exp(0.5 * lv)[:, None, :]).sum(-1) - dist
        v = torch.where(d > 0, torch.zeros_like(d), d ** 2)
        if cls is not None:
            v = v * ((cls[:, None, :] - cls[None, :, :]).abs().sum(-1) <= 0).to(v.dtype)
        return v.sum(-1)

    k = kl(mc, lc, mean_cp, lv_cp) + kl(mi, li, mean_ip, lv_ip)
    r = reg(mean_cp, lv_cp, 3.0 * Lc) + reg(mean_ip, lv_ip, 3.0 * Li, cat_oh)
    return k.mean() + r.mean() + (dz_in * z_in).sum()


# ---------------------------------------------------------------------------------------------------- callers of the entries
def call_eval(L, device, enc, eps, mask, eps2, prior_cat, prior_inst, cat_oh, inst_oh, act=None, lib_call=None):
    """vv_mm_latent_eval (device 'cuda') or vv_mm_latent_eval_host ('cpu') -> dict of numpy outputs; untouched outputs stay NaN / -1."""
    B, (C, Lc), (I, Li) = enc.shape[0], prior_cat.shape, prior_inst.shape[1:]
    ins = [_t(x, device) for x in (enc, eps, mask, eps2, prior_cat, prior_inst, cat_oh, inst_oh)]
    nan = lambda *s, dt=torch.float32: torch.full(s, float('nan'), dtype=dt, device=device)
    z, zc, acc = nan(B, Lc + Li), nan(B, Lc + Li), nan(3)
    adt = {None: None, 'f32': torch.float32, 'bf16': torch.bfloat16}[act]
    za, zca = (nan(B, Lc + Li, dt=adt), nan(B, Lc + Li, dt=adt)) if adt else (None, None)
    idx = torch.full((B, 4), -1, dtype=torch.int32, device=device)
    name = 'vv_mm_latent_eval_host' if device == 'cpu' else 'vv_mm_latent_eval'
    (lib_call or L.call)(name, *[_p(x) for x in ins], _p(z), _p(zc if mask is not None else None), _p(za), _p(zca if mask is not None else None),
                         L.VV_BF16 if act == 'bf16' else L.VV_F32, _p(idx), _p(acc), B, Lc, Li, C, I, *_stream(device))
    if device != 'cpu':
        torch.cuda.synchronize()
    out = dict(z=_np(z), z_corr=_np(zc), idx=_np(idx), acc=_np(acc))
    if adt:
        out.update(z_act=_np(za), z_corr_act=_np(zca))
    return out


def call_train(L, device, enc, eps, mean_cp, lv_cp, mean_ip, lv_ip, eps_p, noise, cat_oh, dz_in, act=None, null_lv=False):
    """The forward and the backward entry on the same arrays -> dict of numpy outputs."""
    B, Lc, Li, C = enc.shape[0], mean_cp.shape[1], mean_ip.shape[1], cat_oh.shape[1]
    ins = [_t(x, device) for x in (enc, eps, mean_cp, lv_cp, mean_ip, lv_ip, eps_p, noise, cat_oh)]
    nan = lambda *s, dt=torch.float32: torch.full(s, float('nan'), dtype=dt, device=device)
    adt = {None: None, 'f32': torch.float32, 'bf16': torch.bfloat16}[act]
    z_in, za, kl, reg = nan(B, Lc + Li), (nan(B, Lc + Li, dt=adt) if adt else None), nan(B), nan(B)
    host = device == 'cpu'
    L.call('vv_mm_latent_train_fwd' + ('_host' if host else ''), *[_p(x) for x in ins], _p(z_in), _p(za),
           L.VV_BF16 if act == 'bf16' else L.VV_F32, _p(kl), _p(reg), B, Lc, Li, C, *_stream(device))
    de, dmc, dlc, dmi, dli = nan(B, 2 * Lc + 2 * Li), nan(B, Lc), nan(B, Lc), nan(B, Li), nan(B, Li)
    L.call('vv_mm_latent_train_bwd' + ('_host' if host else ''), *[_p(x) for x in ins], _p(_t(dz_in, device)), 1.0 / B, _p(de), _p(dmc),
           _p(None if null_lv else dlc), _p(dmi), _p(None if null_lv else dli), B, Lc, Li, C, *_stream(device))
    if not host:
        torch.cuda.synchronize()
    out = dict(z_in=_np(z_in), kl=_np(kl), reg=_np(reg), d_enc_out=_np(de), d_mean_cp=_np(dmc), d_lv_cp=_np(dlc), d_mean_ip=_np(dmi), d_lv_ip=_np(dli))
    if adt:
        out['z_in_act'] = _np(za)
    return out


def random_train_case(seed, B, Lc, Li, C, noise=True):
    rng = np.random.default_rng(seed)
    f = lambda x: np.ascontiguousarray(x, dtype=np.float32)
    cat = rng.integers(0, C, B)
    enc = f(rng.normal(0, 1, (B, 2 * Lc + 2 * Li)))
    enc[:, Lc:2 * Lc] = rng.normal(-2, 1, (B, Lc))
    enc[:, 2 * Lc + Li:] = rng.normal(-2, 1, (B, Li))
    return dict(enc=enc, eps=f(rng.normal(0, 1, (B, Lc + Li))), mean_cp=f(rng.normal(0, 1.5, (C, Lc))[cat] + rng.normal(0, 0.3, (B, Lc))),
                lv_cp=f(rng.normal(0, 0.3, (B, Lc))), mean_ip=f(rng.normal(0, 1.0, (B, Li))), lv_ip=f(rng.normal(0, 0.3, (B, Li))),
                eps_p=f(rng.normal(0, 1, (B, Lc + Li))), noise=f(rng.integers(0, 2, (B, Lc + Li))) if noise else None, cat_oh=f(np.eye(C)[cat]),
                dz_in=f(rng.normal(0, 0.1, (B, Lc + Li))))


def random_eval_case(seed, B, Lc, Li, C, I, missing_prob):
    rng = np.random.default_rng(seed)
    f = lambda x: np.ascontiguousarray(x, dtype=np.float32)
    cat, inst = rng.integers(0, C, B), rng.integers(0, I, B)
    prior_cat, prior_inst = f(rng.normal(0, 1.5, (C, Lc))), f(rng.normal(0, 1.5, (B, I, Li)))
    enc = f(np.concatenate([prior_cat[cat] + rng.normal(0, 0.7, (B, Lc)), rng.normal(-2, 1, (B, Lc)),
                            prior_inst[np.arange(B), inst] + rng.normal(0, 0.7, (B, Li)), rng.normal(-2, 1, (B, Li))], axis=1))
    mask = f(rng.random((B, Lc)) >= missing_prob) if missing_prob > 0 else None
    return dict(enc=enc, eps=f(rng.normal(0, 1, (B, Lc + Li))), mask=mask, eps2=f(rng.normal(0, 1, (B, Lc))) if mask is not None else None,
                prior_cat=prior_cat, prior_inst=prior_inst, cat_oh=f(np.eye(C)[cat]), inst_oh=f(np.eye(I)[inst]))
