"""Callers of the one-group, one-prior latent stage (csrc/prior_latent.hip; include/voxvae.h has the contract): the latent algebra of
nolboSingleObject_instOnly, nolboSingleObject_category_only and nolboSingleObject_modelnet_category_only between the head output and
the decoder's input.  Every function takes contiguous float32 tensors on one device and returns tensors.

    train_fwd / train_bwd     one launch each: sampling | prior / posterior choice | KL | pairwise regulariser, and its backward
    inst_eval                 one launch: instOnly.getEval's sampling | mask | fill | nearest prior row
    latent_stage              the two training launches as ONE autograd node, so that they stand where a torch closure stands in
                              voxvae.train.Trainer.step_custom_latent and beside Trainer.step_decoder in the image models
    mask_scale                inverted dropout on the latent through vv_mask_scale, forward and on dz
"""
import ctypes

import torch

from . import lib as _L


def _st():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _check(name, t, shape):
    if t is None:
        return
    if t.dtype != torch.float32 or tuple(t.shape) != tuple(shape) or not t.is_contiguous():
        raise ValueError('%s must be a contiguous float32 tensor of shape %s, got %s %s' % (name, tuple(shape), t.dtype, tuple(t.shape)))


def _train_inputs(enc_out, eps, mean_p, lv_p, eps_p, keep):
    if enc_out.dim() != 2 or enc_out.shape[1] % 2:
        raise ValueError('enc_out must be [B, 2 L] (mean | logVar), got %s' % (tuple(enc_out.shape),))
    B, Lz = enc_out.shape[0], enc_out.shape[1] // 2
    _check('enc_out', enc_out, (B, 2 * Lz))
    for name, t in (('eps', eps), ('mean_p', mean_p), ('lv_p', lv_p), ('eps_p', eps_p), ('keep', keep)):
        _check(name, t, (B, Lz))
    return B, Lz


def train_fwd(enc_out, eps, mean_p, lv_p, eps_p, keep, dist, bf16=False):
    """vv_prior_latent_train_fwd -> (z_in [B,L], its bfloat16 twin or None, kl [B], reg [B])."""
    B, Lz = _train_inputs(enc_out, eps, mean_p, lv_p, eps_p, keep)
    new = lambda *shape, dt=torch.float32: torch.empty(shape, dtype=dt, device=enc_out.device)
    z_in, kl, reg = new(B, Lz), new(B), new(B)
    twin = new(B, Lz, dt=torch.bfloat16) if bf16 else None
    _L.call('vv_prior_latent_train_fwd', _L.ptr(enc_out), _L.ptr(eps), _L.ptr(mean_p), _L.ptr(lv_p), _L.ptr(eps_p),
            _L.ptr(keep), float(dist), _L.ptr(z_in), _L.ptr(twin), _L.ptr(kl), _L.ptr(reg), B, Lz, _st())
    return z_in, twin, kl, reg


def train_bwd(enc_out, eps, mean_p, lv_p, eps_p, keep, dist, dz_in, inv_batch, reg_weight, want_mean=True, want_lv=True):
    """vv_prior_latent_train_bwd -> (d_enc_out [B,2L], d_mean_p or None, d_lv_p or None) of
    total = mean_b kl + reg_weight mean_b reg + shape, dz_in = d shape / d z_in."""
    B, Lz = _train_inputs(enc_out, eps, mean_p, lv_p, eps_p, keep)
    _check('dz_in', dz_in, (B, Lz))
    new = lambda *shape: torch.empty(shape, dtype=torch.float32, device=enc_out.device)
    d_e, d_m, d_lv = new(B, 2 * Lz), (new(B, Lz) if want_mean else None), (new(B, Lz) if want_lv else None)
    _L.call('vv_prior_latent_train_bwd', _L.ptr(enc_out), _L.ptr(eps), _L.ptr(mean_p), _L.ptr(lv_p), _L.ptr(eps_p),
            _L.ptr(keep), float(dist), _L.ptr(dz_in), float(inv_batch), float(reg_weight), _L.ptr(d_e), _L.ptr(d_m), _L.ptr(d_lv), B, Lz,
            _st())
    return d_e, d_m, d_lv


def inst_eval(enc_out, eps, mask, fill, prior, bf16=False):
    """vv_inst_latent_eval -> (z [B,L], z_corr [B,L], their bfloat16 twins or None, idx int32 [B])."""
    B, Lz = _train_inputs(enc_out, eps, None, None, None, None)
    _check('mask', mask, (B, Lz)), _check('fill', fill, (B, Lz))
    if prior.dim() != 2:
        raise ValueError('prior must be [I, L], got %s' % (tuple(prior.shape),))
    _check('prior', prior, (prior.shape[0], Lz))
    new = lambda *shape, dt=torch.float32: torch.empty(shape, dtype=dt, device=enc_out.device)
    z, zc, idx = new(B, Lz), new(B, Lz), new(B, dt=torch.int32)
    zb, zcb = (new(B, Lz, dt=torch.bfloat16), new(B, Lz, dt=torch.bfloat16)) if bf16 else (None, None)
    _L.call('vv_inst_latent_eval', _L.ptr(enc_out), _L.ptr(eps), _L.ptr(mask), _L.ptr(fill), _L.ptr(prior), _L.ptr(z),
            _L.ptr(zc), _L.ptr(zb), _L.ptr(zcb), _L.ptr(idx), B, Lz, prior.shape[0], _st())
    return z, zc, zb, zcb, idx


class _LatentStage(torch.autograd.Function):
    """The node of both learned-prior stages (voxvae.mm_latent.latent_stage is the other caller).  leaves: enc_out, then the prior
    tensors.  fwd(*leaves) -> (z_in, twin or None, kl, reg) and bwd(*leaves, dz, want) -> (d_enc_out, the prior gradients or None) are a
    stage's train_fwd / train_bwd with everything else bound; want[k]: prior tensor k needs its gradient.  reg_weight None: 1."""
    @staticmethod
    def forward(ctx, fwd, bwd, reg_weight, *leaves):
        ctx.bwd, ctx.leaves = bwd, [t.detach().float().contiguous() for t in leaves]
        z_in, twin, kl, reg = fwd(*ctx.leaves)
        ctx.z_shape = z_in.shape
        extra = kl.mean() + (reg.mean() if reg_weight is None else float(reg_weight) * reg.mean())
        if twin is None:
            twin = z_in.new_empty(0)
        ctx.mark_non_differentiable(kl, reg, twin)            # one call: a second one would replace the first one's set
        return z_in, extra, kl, reg, twin

    @staticmethod
    def backward(ctx, dz, _d_extra, _d_kl, _d_reg, _d_twin):
        need = ctx.needs_input_grad[3:]
        dz = ctx.leaves[0].new_zeros(ctx.z_shape) if dz is None else dz.contiguous()
        d = ctx.bwd(*ctx.leaves, dz, need[1:])
        return (None, None, None, (d[0] if need[0] else None)) + tuple(d[1:])


def stage_node(fwd, bwd, reg_weight, bf16, *leaves):
    """_LatentStage over `leaves` -> (z_in, extra, kl, reg, bfloat16 twin of z_in or None)."""
    z_in, extra, kl, reg, twin = _LatentStage.apply(fwd, bwd, reg_weight, *leaves)
    return z_in, extra, kl, reg, (twin if bf16 else None)


def latent_stage(enc_out, mean_p, lv_p, eps, eps_p, keep, dist, reg_weight, bf16=False):
    """The training stage as one autograd node -> (z_in [B,L], extra, kl [B], reg [B], bfloat16 twin of z_in or None), with
    extra = mean_b kl + reg_weight mean_b reg.  Forward is ONE vv_prior_latent_train_fwd; backward is ONE vv_prior_latent_train_bwd that
    takes the gradient arriving at z_in as d shape / d z_in and gives the gradients of enc_out, mean_p and lv_p (an input that does not
    require a gradient gets a NULL output).  The gradient arriving at `extra` is taken to be 1 -- what Trainer.step_custom_latent and the
    image models pass; kl, reg and the twin carry none."""
    dist, reg_weight = float(dist), float(reg_weight)
    fwd = lambda e, m, lv: train_fwd(e, eps, m, lv, eps_p, keep, dist, bf16)
    bwd = lambda e, m, lv, dz, want: train_bwd(e, eps, m, lv, eps_p, keep, dist, dz, 1.0 / e.shape[0], reg_weight, *want)
    return stage_node(fwd, bwd, reg_weight, bf16, enc_out, mean_p, lv_p)


class _MaskScale(torch.autograd.Function):
    @staticmethod
    def forward(ctx, z, keep, scale):
        ctx.saved = (keep, float(scale))
        return _mask_scale(z.detach().contiguous(), keep, scale)

    @staticmethod
    def backward(ctx, dz):
        keep, scale = ctx.saved
        return _mask_scale(dz.contiguous(), keep, scale), None, None


def _mask_scale(x, keep, scale):
    y = torch.empty_like(x)
    _L.call('vv_mask_scale', _L.ptr(x), _L.ptr(keep), float(scale), _L.ptr(y), x.shape[0], x.shape[1], _st())
    return y


def mask_scale(z, keep, scale):
    """(z * keep) * scale over a float32 [B, L] latent as an autograd node: vv_mask_scale forward, and on dz backward."""
    return _MaskScale.apply(z, keep, scale)
