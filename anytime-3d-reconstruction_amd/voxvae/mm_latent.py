"""Callers of the two-group, two-prior ("multi-modal") latent stage (csrc/mm_latent.hip; include/voxvae.h has the contract): the latent
algebra of nolboSingleObject between the head output [mean_c | logVar_c | mean_i | logVar_i] and the decoder's input.  The twin of
voxvae/prior_latent.py: every function takes contiguous float32 tensors on one device and returns tensors.

    train_fwd / train_bwd     one launch each: sampling | prior / posterior choice | KL | the two pairwise regularisers, and its backward
    eval                      one launch: getEval's sampling | mask fill | nearest priors | correction | accuracies
    latent_stage              the two training launches as ONE autograd node, beside Trainer.step_decoder in nolboSingleObject.fit
"""
import torch

from . import lib as _L
from . import train as _T
from .prior_latent import _check, stage_node


def _st():
    """The stream of the decoder step the stage sits beside: the trainer's, looked up at each call."""
    return _T._st()


def _train_inputs(enc_out, eps, pri4, eps_p, noise, cat_onehot):
    mean_cp, lv_cp, mean_ip, lv_ip = pri4
    if mean_cp.dim() != 2 or mean_ip.dim() != 2 or cat_onehot.dim() != 2:
        raise ValueError('the prior means and cat_onehot must be 2-D, got %s' % ([tuple(t.shape) for t in (mean_cp, mean_ip, cat_onehot)],))
    B, Lc, Li, C = enc_out.shape[0], mean_cp.shape[1], mean_ip.shape[1], cat_onehot.shape[1]
    for name, t, width in (('enc_out', enc_out, 2 * Lc + 2 * Li), ('eps', eps, Lc + Li), ('eps_p', eps_p, Lc + Li), ('noise', noise, Lc + Li),
                           ('mean_cp', mean_cp, Lc), ('lv_cp', lv_cp, Lc), ('mean_ip', mean_ip, Li), ('lv_ip', lv_ip, Li), ('cat_onehot', cat_onehot, C)):
        _check(name, t, (B, width))
    ptrs = [_L.ptr(t) for t in (enc_out, eps, mean_cp, lv_cp, mean_ip, lv_ip, eps_p, noise, cat_onehot)]
    return ptrs, (B, Lc, Li, C)


def train_fwd(enc_out, eps, pri4, eps_p, noise, cat_onehot, bf16=False):
    """vv_mm_latent_train_fwd -> (z_in [B, Lc+Li], its bfloat16 twin or None, kl [B], reg [B]); pri4 = (mean_cp, lv_cp, mean_ip, lv_ip)."""
    ptrs, (B, Lc, Li, C) = _train_inputs(enc_out, eps, pri4, eps_p, noise, cat_onehot)
    new = lambda *shape, dt=torch.float32: torch.empty(shape, dtype=dt, device=enc_out.device)
    z_in, kl, reg = new(B, Lc + Li), new(B), new(B)
    twin = new(B, Lc + Li, dt=torch.bfloat16) if bf16 else None
    _L.call('vv_mm_latent_train_fwd', *ptrs, _L.ptr(z_in), _L.ptr(twin), _L.VV_BF16 if bf16 else _L.VV_F32, _L.ptr(kl), _L.ptr(reg), B, Lc, Li, C, _st())
    return z_in, twin, kl, reg


def train_bwd(enc_out, eps, pri4, eps_p, noise, cat_onehot, dz_in, inv_batch, want=(True, True, True, True)):
    """vv_mm_latent_train_bwd -> (d_enc_out [B, 2Lc+2Li], d_mean_cp, d_lv_cp, d_mean_ip, d_lv_ip) of
    total = inv_batch sum_b (kl + reg) + shape, dz_in = d shape / d z_in; a prior output that is not wanted is NULL to the kernel and None here."""
    ptrs, (B, Lc, Li, C) = _train_inputs(enc_out, eps, pri4, eps_p, noise, cat_onehot)
    _check('dz_in', dz_in, (B, Lc + Li))
    new = lambda *shape: torch.empty(shape, dtype=torch.float32, device=enc_out.device)
    d_e = new(B, 2 * Lc + 2 * Li)
    d_pri = [new(*t.shape) if w else None for t, w in zip(pri4, want)]
    _L.call('vv_mm_latent_train_bwd', *ptrs, _L.ptr(dz_in), float(inv_batch), _L.ptr(d_e), *[_L.ptr(g) for g in d_pri], B, Lc, Li, C, _st())
    return (d_e,) + tuple(d_pri)


def eval(enc_out, eps, mask, eps2, prior_cat, prior_inst, cat_onehot, inst_onehot, act_dtype):
    """vv_mm_latent_eval -> (z [B, Lc+Li], z_corr or None, z_act or None, z_corr_act or None, idx int32 [B,4], acc [3]): the corrected
    latent only with a mask, the bfloat16 twins only when act_dtype is not VV_F32.  prior_cat [C, Lc], prior_inst [B, I, Li]."""
    if prior_cat.dim() != 2 or prior_inst.dim() != 3 or (mask is None) != (eps2 is None):
        raise ValueError('prior_cat [C, Lc], prior_inst [B, I, Li], mask and eps2 together: got %s %s' % (tuple(prior_cat.shape), tuple(prior_inst.shape)))
    B, (C, Lc), (I, Li) = enc_out.shape[0], prior_cat.shape, prior_inst.shape[1:]
    for name, t, shape in (('enc_out', enc_out, (B, 2 * Lc + 2 * Li)), ('eps', eps, (B, Lc + Li)), ('mask', mask, (B, Lc)), ('eps2', eps2, (B, Lc)),
                           ('prior_cat', prior_cat, (C, Lc)), ('prior_inst', prior_inst, (B, I, Li)), ('cat_onehot', cat_onehot, (B, C)),
                           ('inst_onehot', inst_onehot, (B, I))):
        _check(name, t, shape)
    new =lambda dt=torch.float32: torch.empty(B, Lc + Li, dtype=dt, device=enc_out.device)
    twin, corr = act_dtype != _L.VV_F32, mask is not None
    z, zc = new(), (new() if corr else None)
    z_act, zc_act = (new(torch.bfloat16) if twin else None), (new(torch.bfloat16) if twin and corr else None)
    idx = torch.empty(B, 4, dtype=torch.int32, device=enc_out.device)
    acc = torch.empty(3, dtype=torch.float32, device=enc_out.device)
    _L.call('vv_mm_latent_eval', _L.ptr(enc_out), _L.ptr(eps), _L.ptr(mask), _L.ptr(eps2), _L.ptr(prior_cat), _L.ptr(prior_inst),
            _L.ptr(cat_onehot), _L.ptr(inst_onehot), _L.ptr(z), _L.ptr(zc), _L.ptr(z_act), _L.ptr(zc_act), act_dtype, _L.ptr(idx), _L.ptr(acc),
            B, Lc, Li, C, I, _st())
    return z, zc, z_act, zc_act, idx, acc


def latent_stage(enc_out, mean_cp, lv_cp, mean_ip, lv_ip, eps, eps_p, noise, cat_onehot, bf16=False):
    """The training stage as one autograd node -> (z_in [B, Lc+Li], extra, kl [B], reg [B], bfloat16 twin of z_in or None), with
    extra = mean_b kl + mean_b reg.  Forward is ONE vv_mm_latent_train_fwd; backward is ONE vv_mm_latent_train_bwd that takes the
    gradient arriving at z_in as d shape / d z_in and gives the gradients of enc_out and the four prior tensors (one that does not
    require a gradient -- a constant log-variance -- gets a NULL output).  The gradient arriving at `extra` is taken to be 1, as in
    voxvae.prior_latent.latent_stage; kl, reg and the twin carry none."""
    fwd = lambda e, *pri4: train_fwd(e, eps, pri4, eps_p, noise, cat_onehot, bf16)
    bwd = lambda e, mc, lc, mi, li, dz, want: train_bwd(e, eps, (mc, lc, mi, li), eps_p, noise, cat_onehot, dz, 1.0 / e.shape[0], want=want)
    return stage_node(fwd, bwd, None, bf16, enc_out, mean_cp, lv_cp, mean_ip, lv_ip)
