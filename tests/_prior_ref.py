"""The one-group, one-prior latent stage (include/voxvae.h: vv_prior_latent_train_fwd / _bwd, vv_inst_latent_eval) stated in numpy from
the formulas of the header -- once in float64 (the definition the fixture tests/golden/prior_latent.npz records and the tests hold the
host entries to) and once in plain float32 numpy (whose distance from the float64 statement sets the tests' gates) -- the same total as
a torch closure for autograd, and the callers of the entries that the CPU and the GPU tests share."""
import numpy as np
import torch

from _common import _np, _p, _stream, _t, first_argmin  # noqa: F401  (first_argmin: also for the tests that import this module)

F = np.float32


# ---------------------------------------------------------------------------------------------------- the definition
def _sample(mean, lv, eps):
    with np.errstate(all='ignore'):
        return mean + np.sqrt(np.exp(lv)) * eps


def train_fwd(enc, eps, mean_p, lv_p, eps_p, keep, dist, dtype=np.float64):
    """z_in, kl, reg in `dtype` arithmetic (float64: the definition; float32: plain numpy, its sums in numpy's own order)."""
    c = lambda x: None if x is None else np.asarray(x).astype(dtype)
    enc, eps, mean_p, lv_p, eps_p, keep = (c(x) for x in (enc, eps, mean_p, lv_p, eps_p, keep))
    L = mean_p.shape[1]
    with np.errstate(all='ignore'):
        mean, lv = enc[:, :L], np.clip(enc[:, L:], dtype(-10), dtype(10))
        z, zp = _sample(mean, lv, eps), _sample(mean_p, lv_p, eps_p)
        z_in = z if keep is None else np.where(keep == 1, z, zp)
        kl = (dtype(0.5) * (lv_p - lv) + (np.exp(lv) + (mean - mean_p) ** 2) / (dtype(2) * np.exp(lv_p)) - dtype(0.5)).sum(-1)
        d = (np.abs(mean_p[:, None, :] - mean_p[None, :, :]) / np.exp(dtype(0.5) * lv_p)[:, None, :]).sum(-1) - dtype(dist)
        reg = np.where(d > 0, dtype(0), d * d).sum(-1)                # d <= 0 keeps d^2
    return dict(z_in=z_in.astype(dtype), kl=kl.astype(dtype), reg=reg.astype(dtype))


def inst_eval(enc, eps, mask, fill, prior, dtype=np.float64):
    c = lambda x: None if x is None else np.asarray(x).astype(dtype)
    enc, eps, mask, fill, prior = (c(x) for x in (enc, eps, mask, fill, prior))
    L = prior.shape[1]
    with np.errstate(all='ignore'):
        z = _sample(enc[:, :L], np.clip(enc[:, L:], dtype(-10), dtype(10)), eps)
        if mask is not None:
            z = z * mask
            z = np.where(z == 0, fill, z)
        sq = (z[:, None, :] - prior[None, :, :]) ** 2
        idx = first_argmin((sq if mask is None else mask[:, None, :] * sq).sum(-1))
    return dict(z=z.astype(dtype), idx=idx, z_corr=prior[idx].astype(dtype))


def total_torch(enc, eps, mean_p, lv_p, eps_p, keep, dz_in, dist, reg_weight):
    """total = mean_b kl + reg_weight mean_b reg + <dz_in, z_in> as a torch closure in the dtype of its arguments."""
    L = mean_p.shape[1]
    mean, lv = enc[:, :L], enc[:, L:].clamp(-10, 10)
    z, zp = mean + torch.sqrt(torch.exp(lv)) * eps, mean_p + torch.sqrt(torch.exp(lv_p)) * eps_p
    z_in = z if keep is None else torch.where(keep == 1, z, zp)
    kl = (0.5 * (lv_p - lv) + (torch.exp(lv) + (mean - mean_p) ** 2) / (2.0 * torch.exp(lv_p)) - 0.5).sum(-1)
    d = ((mean_p[:, None, :] - mean_p[None, :, :]).abs() / torch.exp(0.5 * lv_p)[:, None, :]).sum(-1) - dist
    reg = torch.where(d > 0, torch.zeros_like(d), d ** 2).sum(-1)
    return kl.mean() + reg_weight * reg.mean() + (dz_in * z_in).sum()


def autograd(c, dtype):
    """d total / d (enc, mean_p, lv_p) of a training case by torch autograd in `dtype` -> dict of float64 numpy arrays."""
    names = ('enc', 'eps', 'mean_p', 'lv_p', 'eps_p', 'keep', 'dz_in')
    t = {k: (None if c[k] is None else torch.from_numpy(c[k]).to(dtype)) for k in names}
    leaves = ['enc', 'mean_p', 'lv_p']
    for k in leaves:
        t[k].requires_grad_(True)
    total_torch(*[t[k] for k in names], float(c['dist']), float(c['reg_weight'])).backward()
    return {k: t[k].grad.numpy().astype(np.float64) for k in leaves}


# ---------------------------------------------------------------------------------------------------- cases
def _f(x):
    return np.ascontiguousarray(x, dtype=np.float32)


def train_case(seed, B, L, keep=True, dist_per_dim=3.0, reg_weight=0.01):
    """Prior means a few scales apart, so that some pairs sit inside the hinge and some outside."""
    rng = np.random.default_rng(seed)
    enc = _f(rng.normal(0, 1, (B, 2 * L)))
    enc[:, L:] = rng.normal(-2, 1, (B, L))
    return dict(enc=enc, eps=_f(rng.normal(0, 1, (B, L))), mean_p=_f(rng.normal(0, 2.0, (B, L))), lv_p=_f(rng.normal(0, 0.3, (B, L))),
                eps_p=_f(rng.normal(0, 1, (B, L))), keep=_f(rng.random((B, L)) < 0.7) if keep else None, dz_in=_f(rng.normal(0, 0.1, (B, L))),
                dist=float(dist_per_dim * L), reg_weight=float(reg_weight))


def eval_case(seed, B, L, I, missing_prob):
    rng = np.random.default_rng(seed)
    prior = _f(rng.normal(0, 1.5, (I, L)))
    enc = _f(np.concatenate([prior[rng.integers(0, I, B)] + rng.normal(0, 0.7, (B, L)), rng.normal(-2, 1, (B, L))], axis=1))
    mask = _f(rng.random((B, L)) >= missing_prob) if missing_prob > 0 else None
    return dict(enc=enc, eps=_f(rng.normal(0, 1, (B, L))), mask=mask, fill=_f(rng.normal(0, 1, (B, L))) if mask is not None else None, prior=prior)


TRAIN_KEYS = ('enc', 'eps', 'mean_p', 'lv_p', 'eps_p', 'keep', 'dist')
EVAL_KEYS = ('enc', 'eps', 'mask', 'fill', 'prior')


def train_args(c):
    return [c[k] for k in TRAIN_KEYS]


def eval_args(c):
    return [c[k] for k in EVAL_KEYS]


# ---------------------------------------------------------------------------------------------------- callers of the entries
def bf16_to_f32(u16):
    return (u16.astype(np.uint32) << 16).view(np.float32)


def call_train(L, device, c, bf16=False, null_mean=False, null_lv=False):
    """The forward and the backward entry on one case -> dict of numpy outputs; untouched outputs stay NaN.  z_in_bf16: raw uint16."""
    B, Lz = c['mean_p'].shape
    ins = [_t(c[k], device) for k in TRAIN_KEYS[:-1]]
    nan = lambda *s, dt=torch.float32: torch.full(s, float('nan'), dtype=dt, device=device)
    z_in, zb, kl, reg = nan(B, Lz), (nan(B, Lz, dt=torch.bfloat16) if bf16 else None), nan(B), nan(B)
    host = device == 'cpu'
    L.call('vv_prior_latent_train_fwd' + ('_host' if host else ''), *[_p(x) for x in ins], float(c['dist']), _p(z_in), _p(zb), _p(kl), _p(reg), B, Lz,
           *_stream(device))
    de, dm, dlv = nan(B, 2 * Lz), nan(B, Lz), nan(B, Lz)
    L.call('vv_prior_latent_train_bwd' + ('_host' if host else ''), *[_p(x) for x in ins], float(c['dist']), _p(_t(c['dz_in'], device)), 1.0 / B,
           float(c['reg_weight']), _p(de), _p(None if null_mean else dm), _p(None if null_lv else dlv), B, Lz, *_stream(device))
    if not host:
        torch.cuda.synchronize()
    out = dict(z_in=_np(z_in), kl=_np(kl), reg=_np(reg), d_enc_out=_np(de), d_mean_p=_np(dm), d_lv_p=_np(dlv))
    if bf16:
        out['z_in_bf16'] = _np(zb, bf16_bits=True)
    return out


def call_eval(L, device, c, bf16=False):
    """vv_inst_latent_eval (device 'cuda') or its host twin ('cpu') -> dict of numpy outputs; the bf16 twins as raw uint16."""
    B, Lz, I = c['enc'].shape[0], c['prior'].shape[1], c['prior'].shape[0]
    ins = [_t(c[k], device) for k in EVAL_KEYS]
    nan = lambda *s, dt=torch.float32: torch.full(s, float('nan'), dtype=dt, device=device)
    z, zc = nan(B, Lz), nan(B, Lz)
    zb, zcb = (nan(B, Lz, dt=torch.bfloat16), nan(B, Lz, dt=torch.bfloat16)) if bf16 else (None, None)
    idx = torch.full((B,), -1, dtype=torch.int32, device=device)
    L.call('vv_inst_latent_eval' + ('_host' if device == 'cpu' else ''), *[_p(x) for x in ins], _p(z), _p(zc), _p(zb), _p(zcb), _p(idx), B, Lz, I,
           *_stream(device))
    if device != 'cpu':
        torch.cuda.synchronize()
    out = dict(z=_np(z), z_corr=_np(zc), idx=_np(idx))
    if bf16:
        out.update(z_bf16=_np(zb, bf16_bits=True), z_corr_bf16=_np(zcb, bf16_bits=True))
    return out
