"""Drop-in for the loss/latent ops of the reference's src/module/function.py (lines 35-38, 40-71, 73-115), each a
hand-written HIP kernel behind the C ABI (include/voxvae.h).  Same names, argument order and meaning:
note that binary_loss takes (xPred, xTarget) while voxelPrecisionRecall takes (xTarget, xPred), and that
xPred is a PROBABILITY in both, exactly as in the reference.  Inputs may be numpy arrays, DeviceArrays or
torch tensors; results are DeviceArrays (np.array()-able)."""
import ctypes

import numpy as np
import torch

import voxvae
from voxvae import lib as _L
from voxvae.tensor import DeviceArray, as_device_f32


def _st():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _dev(x):
    return as_device_f32(x, voxvae.default_device())


def sampling(mu, logVar, epsilon=None):
    """reference function.py:35-38.  `epsilon` (extension) injects the N(0,1) draw; default: drawn on device."""
    mu, logVar = _dev(mu), _dev(logVar)
    eps = torch.randn_like(mu) if epsilon is None else _dev(epsilon)
    out = torch.empty_like(mu)
    _L.call('vv_sampling', _L.ptr(mu), _L.ptr(logVar), _L.ptr(eps), _L.ptr(out), mu.numel(), _st())
    return DeviceArray(out)


def binary_loss(xPred, xTarget, epsilon=1e-7, gamma=0.5, b_range=False):
    """reference function.py:73-82 -> per-sample loss [B]."""
    p, t = _dev(xPred), _dev(xTarget)
    B = p.shape[0]
    V = p.numel() // B
    if t.numel() != p.numel():
        raise ValueError('xPred %s and xTarget %s differ in size' % (tuple(p.shape), tuple(t.shape)))
    out = torch.empty(B, dtype=torch.float32, device=p.device)
    _L.call('vv_binary_loss', _L.ptr(p), _L.ptr(t), float(epsilon), float(gamma), float(b_range), _L.ptr(out), B, V, _st())
    return DeviceArray(out)


def kl_loss(mean, logVar, mean_target, logVar_target):
    """reference function.py:84-98 -> [B]."""
    m, lv, mt, lvt = _dev(mean), _dev(logVar), _dev(mean_target), _dev(logVar_target)
    B, Lz = m.shape[0], m.numel() // m.shape[0]
    out = torch.empty(B, dtype=torch.float32, device=m.device)
    _L.call('vv_kl_loss', _L.ptr(m), _L.ptr(lv), _L.ptr(mt), _L.ptr(lvt), _L.ptr(out), B, Lz, _st())
    return DeviceArray(out)


def regulizer_loss(z_mean, z_logVar, dist_in_z_space, class_input=None):
    """reference function.py:40-71 -> [B]: pairwise hinge that keeps latent means at least `dist_in_z_space` apart
    (scaled L1), optionally only between samples of the same class."""
    m, lv = _dev(z_mean), _dev(z_logVar)
    B, Lz = m.shape[0], m.numel() // m.shape[0]
    c = None if class_input is None else _dev(class_input)
    out = torch.empty(B, dtype=torch.float32, device=m.device)
    _L.call('vv_regulizer_loss', _L.ptr(m), _L.ptr(lv), _L.ptr(c), float(dist_in_z_space), _L.ptr(out), B, Lz,
            0 if c is None else c.numel() // B, _st())
    return DeviceArray(out)


def voxelPrecisionRecall(xTarget, xPred, prob=0.5):
    """reference function.py:100-115 -> (TP, FP, FN), each [B]."""
    t, p = _dev(xTarget), _dev(xPred)
    B = p.shape[0]
    V = p.numel() // B
    tp, fp, fn = (torch.empty(B, dtype=torch.float32, device=p.device) for _ in range(3))
    _L.call('vv_voxel_precision_recall', _L.ptr(t), _L.ptr(p), float(prob), _L.ptr(tp), _L.ptr(fp), _L.ptr(fn), B, V, _st())
    return DeviceArray(tp), DeviceArray(fp), DeviceArray(fn)


def voxelPrecisionRecallCurve(xTarget, xPred, probs, inclusive=True):
    """voxelPrecisionRecall at every threshold of `probs` in one pass over the data (vv_pr_curve_accumulate; the sweep the reference's
    notebooks run on the host, modelnetAE3.ipynb cell 2) -> (TP, FP, FN), each [B, T] float32 like its single-threshold sibling.
    inclusive=True counts p >= prob as function.py:110 does; False counts p > prob (the notebook's compare); one bool or one per
    threshold."""
    from voxvae.prcurve import PRCurve
    p = _dev(xPred)
    B = p.shape[0]
    curve = PRCurve(np.atleast_1d(np.asarray(probs, dtype=np.float64)), inclusive, groups=B, device=p.device)
    curve.update(xTarget, p, group=torch.arange(B, dtype=torch.int32, device=p.device))
    tp, fp, fn, _, _ = curve.counts_device()
    return DeviceArray(tp.float()), DeviceArray(fp.float()), DeviceArray(fn.float())


class kmeans_cosine(object):
    """reference function.py:156-200: k-means over rows (sin a, sin e, sin i, cos a, cos e, cos i) with its "cosine" distance, on
    vv_kmeans_cosine (voxvae/kmeans.py; csrc/kmeans_cosine.h states the arithmetic).  Same constructor, `_kmeans` and `kmeansSample`,
    same numpy results; the picks of kmeansSample come from Python's `random` in the reference's order, so `random.seed(s)` reproduces
    them.  `host=True` runs the same code compiled for the CPU, `device=` names the GPU; by default the device when there is one.
    `iterations` holds how many iterations of the last `_kmeans` did work (the rest would have repeated the last one bit for bit)."""

    def __init__(self, X, k, max_iter=100, device=None, host=None):
        self._X = np.array(X, dtype=np.float64)
        self._k = k
        self._max_iter = max_iter
        self._host = (not torch.cuda.is_available()) if host is None and device is None else bool(host)
        self._device = device
        self.iterations = 0

    def _kmeans(self, X, centres, max_iter=100):
        """-> (centres [k,6] float64, xtoc [N] int64, distance [N] float64); a float64 numpy `centres` is updated in place, as the
        reference updates it.  max_iter=0 -> (centres, None, None)."""
        from voxvae import kmeans as _K
        if max_iter < 1:
            return centres, None, None
        x, c = np.asarray(X, dtype=np.float64), np.asarray(centres, dtype=np.float64)
        if not self._host and self._device is not None:
            x, c = torch.from_numpy(np.ascontiguousarray(x)).to(self._device), torch.from_numpy(np.ascontiguousarray(c)).to(self._device)
        out, xtoc, dist, self.iterations = _K.kmeans(x, c, max_iter, host=self._host)
        out = out.cpu().numpy()
        if isinstance(centres, np.ndarray) and centres.dtype == np.float64 and centres.shape == out.shape:
            centres[...] = out
            out = centres
        return out, xtoc.cpu().numpy().astype(np.int64), dist.cpu().numpy()

    def kmeansSample(self, nsample=0, *, _sample_idx=None, _centre_idx=None):
        """reference :193-200: 10 iterations on a random sample of rows from k random rows of X, then max_iter iterations on all of X.
        `_sample_idx` / `_centre_idx` (extensions) inject the two picks."""
        import random
        N = self._X.shape[0]
        if nsample == 0:
            nsample = max(2 * np.sqrt(N), 10 * self._k)
        sample = random.sample(range(N), int(nsample)) if _sample_idx is None else list(_sample_idx)
        first = random.sample(range(N), int(self._k)) if _centre_idx is None else list(_centre_idx)
        centres = self._kmeans(self._X[sample], self._X[first], max_iter=10)[0]
        return self._kmeans(self._X, centres, max_iter=self._max_iter)
