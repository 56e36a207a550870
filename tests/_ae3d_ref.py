"""Float64 reference of one AE3D.fit step (reference src/module/AE3D.py:67-90), shared by tests/test_ae3d_host.py and
tests/test_gpu_ae3d.py.  A helper, not a test: the committed training oracle (oracle.torch_oracle.forward_train, variational=False) fed
2x - 1 with the 0/1 target, plus lambda * sum w^2 over the regularised names, Adam from tests/_train_ref.adam_ref.  `world` and
`global_batch` are arguments, so one rank of a two-rank run is the same function."""
import numpy as np
import torch

from oracle import torch_oracle as to

from _train_ref import adam_ref, lr_t_of

L2 = 5e-4                      # autoencoder3D.py:29,44,60-61,88,131
BN_MOM = 0.99


def regularised(name):
    """Every Conv3D / Conv3DTranspose / Dense kernel and the Dense bias; no BatchNorm variable."""
    return name.endswith('/kernel') or name == 'dec/dense/bias'


def tensors(ep, dp):
    P = {}
    for pre, d in (('enc/', ep), ('dec/', dp)):
        for k, v in d.items():
            P[pre + k] = to._t(v, grad=not k.endswith(('moving_mean', 'moving_variance')))
    return P


def reg_sumsq(P):
    """sum w^2 over the regularised variables, as a torch scalar on P's graph."""
    return sum((P[n] ** 2).sum() for n in to.trainable_names(P) if regularised(n))


def fit_ref(cfg, ep, dp, x, y, lam=L2, world=1, global_batch=None, rescale=True):
    """One replica's step quantities.  x, y [B,D,D,D,1] in {0,1}.  Returns a dict:
      reg, pred, total     the replica's losses: lam * sum w^2, sum_b bce_b / global_batch, their sum (AE3D.py:74, 82-84)
      tp, fp, fn           the replica's counts summed over its samples (unscaled integers)
      g_pred, g_total      d pred / dw and d total / dw of THIS replica, by autograd
      g_sum_reg            what the regulariser contributes to the gradient SUMMED over `world` replicas: world * 2 * lam * w
      bn_stats             name -> (batch mean, biased batch variance)
    rescale=False feeds x itself to the encoder (the negative control of the rescale test)."""
    B = x.shape[0]
    gb = B * world if global_batch is None else global_batch
    P = tensors(ep, dp)
    xin = 2.0 * np.asarray(x, np.float64) - 1.0 if rescale else np.asarray(x, np.float64)
    _, shape, p, stats = to.forward_train(cfg, P, to._t(xin), to._t(y), None, variational=False)
    pred = shape * B / gb                                    # forward_train returns the mean over the B local samples
    reg = lam * reg_sumsq(P)
    total = pred + reg
    names = to.trainable_names(P)
    plist = [P[n] for n in names]
    gp = torch.autograd.grad(pred, plist, retain_graph=True, allow_unused=True)
    gt = torch.autograd.grad(total, plist, allow_unused=True)
    as_np = lambda gs: {n: (np.zeros(P[n].shape) if g is None else g.numpy()) for n, g in zip(names, gs)}
    pn, yn = p.detach().numpy(), np.asarray(y, np.float64)
    yh = (pn >= 0.5).astype(np.float64)
    cnt = lambda a: float(a.sum())
    return {'reg': float(reg.detach()), 'pred': float(pred.detach()), 'total': float(total.detach()),
            'tp': cnt(yn * yh), 'fp': cnt((1 - yn) * yh), 'fn': cnt(yn * (1 - yh)),
            'g_pred': as_np(gp), 'g_total': as_np(gt),
            'g_sum_reg': {n: (world * 2.0 * lam * P[n].detach().numpy() if regularised(n) else np.zeros(P[n].shape)) for n in names},
            'bn_stats': stats, 'probs': pn, 'names': names}


def adam_first_step(w, g, lr):
    """Keras Adam's first step from zero moments on gradient g (float64) -> (new weights, m, v, step)."""
    z = np.zeros_like(np.asarray(g, np.float64))
    return adam_ref(w, g, z, z, lr_t_of(1, lr))


def moved_statistics(old_mean, old_var, batch_mean, batch_var):
    return old_mean * BN_MOM + batch_mean * (1 - BN_MOM), old_var * BN_MOM + batch_var * (1 - BN_MOM)
