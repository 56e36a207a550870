"""Viewpoint clustering on the device (csrc/kmeans_cosine.hip and csrc/kmeans_cosine.h behind vv_kmeans_cosine / vv_kmeans_cosine_host).

The reference clusters the (sin, cos) rows of every object's Euler angles with a Python loop over the centres, a fixed number of times
(src/module/function.py:156-200, kmeans_cosine; pascal3D.py:156-181, getKmeansAEI).  Here an iteration is two launches, all of them
enqueued by one call, and the iterations after the labels have settled cost a launch that returns at once:

    centres, xtoc, distance, iterations = kmeans(X, centres0, max_iter)        # X [N,6], centres0 [k,6]
    labels = assign(X_new, centres)                                            # int32 on the device
    PRCurve(thresholds, groups=k).update(target, pred, group=labels)           # precision / recall per viewpoint cluster

All arithmetic is float64; the distance, the lowest-index tie rule and the summation order of the update are stated in
csrc/kmeans_cosine.h.  The host entries run the same code compiled for the CPU and give the same bits.
"""
import ctypes

import numpy as np
import torch

MAX_POINTS = 1 << 20
MAX_CENTRES = 1024
MAX_ITER = 1 << 16


def _rows(a, what, check_finite):
    """-> (a contiguous float64 [n, 6] tensor where it already lives, its device or None).  Raises ValueError before any upload."""
    from .tensor import DeviceArray
    if isinstance(a, DeviceArray):
        a = a.t
    if isinstance(a, torch.Tensor):
        t = a.detach()
    else:
        t = torch.from_numpy(np.ascontiguousarray(np.asarray(a, dtype=np.float64)))
    if t.dim() != 2 or t.shape[1] != 6 or t.shape[0] < 1:
        raise ValueError('%s must be [N, 6] = (sin a, sin e, sin i, cos a, cos e, cos i) with N >= 1, got %s' % (what, tuple(t.shape)))
    t = t.to(torch.float64)
    if check_finite and not bool(torch.isfinite(t).all()):
        raise ValueError('%s holds a value that is not finite' % what)
    return t.contiguous(), (t.device if t.is_cuda else None)


def _device(host, held):
    import voxvae
    from . import lib as L
    if host:
        return torch.device('cpu')
    device = next((d for d in held if d is not None), None) or torch.device(voxvae.default_device())
    if device.type != 'cuda' or not torch.cuda.is_available():
        raise L.VoxVaeError('kmeans runs on the GPU (default device %s, CUDA available: %s); there is no silent CPU fallback: '
                            'pass host=True for the host entry' % (device, torch.cuda.is_available()))
    return device


def _stream(device):
    return ctypes.c_void_p(torch.cuda.current_stream(device).cuda_stream)


def kmeans(X, centres, max_iter, host=False):
    """max_iter iterations of the reference's _kmeans from the given centres -> (centres [k,6] float64, xtoc [N] int32, distance [N]
    float64, iterations int): tensors on the device (on the CPU for host=True); `centres` itself is not written.  xtoc / distance are
    the last iteration's assignment, taken before its update; iterations counts the iterations that did work (reading it is THE
    synchronisation).  X and centres: numpy arrays, torch tensors or DeviceArrays."""
    from . import lib as L
    x, dx = _rows(X, 'X', True)
    c, dc = _rows(centres, 'centres', True)
    n, k, max_iter = int(x.shape[0]), int(c.shape[0]), int(max_iter)
    if n > MAX_POINTS or k > MAX_CENTRES:
        raise ValueError('at most %d points and %d centres per call, got %d and %d' % (MAX_POINTS, MAX_CENTRES, n, k))
    if not 1 <= max_iter <= MAX_ITER:
        raise ValueError('max_iter must be in 1 .. %d, got %d' % (MAX_ITER, max_iter))
    device = _device(host, (dx, dc))
    x = x.to(device)
    c = c.to(device).clone()
    xtoc = torch.empty(n, dtype=torch.int32, device=device)
    dist = torch.empty(n, dtype=torch.float64, device=device)
    its = torch.empty(1, dtype=torch.int32, device=device)
    if host:
        L.call('vv_kmeans_cosine_host', L.ptr(x), n, L.ptr(c), k, max_iter, L.ptr(xtoc), L.ptr(dist), L.ptr(its))
        return c, xtoc, dist, int(its.item())
    need = L.load().vv_kmeans_cosine_workspace_bytes(n, k)
    ws = torch.empty(need, dtype=torch.uint8, device=device)
    L.call('vv_kmeans_cosine', L.ptr(x), n, L.ptr(c), k, max_iter, L.ptr(xtoc), L.ptr(dist), L.ptr(its), L.ptr(ws), need, _stream(device))
    return c, xtoc, dist, int(its.item())


def assign(X, centres, host=False, return_distance=False):
    """The nearest centre of every row of X -> int32 [N] on the device (on the CPU for host=True), what PRCurve.update(group=...) takes
    as it is; with return_distance=True -> (labels, distance float64 [N]).  One launch on the current stream, no synchronisation."""
    from . import lib as L
    x, dx = _rows(X, 'X', True)
    c, dc = _rows(centres, 'centres', True)
    n, k = int(x.shape[0]), int(c.shape[0])
    if n > MAX_POINTS or k > MAX_CENTRES:
        raise ValueError('at most %d points and %d centres per call, got %d and %d' % (MAX_POINTS, MAX_CENTRES, n, k))
    device = _device(host, (dx, dc))
    x, c = x.to(device), c.to(device)
    xtoc = torch.empty(n, dtype=torch.int32, device=device)
    dist = torch.empty(n, dtype=torch.float64, device=device) if return_distance else None
    if host:
        L.call('vv_kmeans_cosine_assign_host', L.ptr(x), n, L.ptr(c), k, L.ptr(xtoc), L.ptr(dist))
    else:
        L.call('vv_kmeans_cosine_assign', L.ptr(x), n, L.ptr(c), k, L.ptr(xtoc), L.ptr(dist), _stream(device))
    return (xtoc, dist) if return_distance else xtoc
