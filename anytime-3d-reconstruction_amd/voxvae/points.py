"""Predicted occupancy grids -> posed point clouds on the device (csrc/voxel_points.hip behind vv_voxel_points_count / _emit).

The reference turns every averaged prediction into the object's points in the world on the host (src/visualizer/visualizer.py:171-188,
objRescaleTransform: threshold at 0.5, the occupied cells in row-major order, shifted to their bounding box, scaled so that the largest
extent is max(h, w, l), centred per axis, then the 4x4 pose).  Here the probabilities are already in device memory when getEval /
getSampledShape return, and what a viewer or a pose step needs is a few thousand points per object, not the 4 D^3 bytes of the grid:

    cloud = voxel_points(pred, dims, pose)            # pred [B,D,D,D,1] on the device, dims [B,3] = (h, w, l), pose [B,4,4]
    objsPoints = cloud.split()                        # the reference's list of [n_b,3] arrays

Per object: cells = the occupied (i, j, k) in increasing flat index, lo / hi their per-axis extremes, ext = hi - lo, E = max(ext),
scale = max(h, w, l) / E, q = (cell - lo) scale - (ext scale) / 2, point = P[:3,:3] q + P[:3,3] in float32.  Two cases the reference
leaves undefined are defined here: an object without an occupied cell has no points and the box (D, D, D, -1, -1, -1) (the reference
raises inside np.min); E == 0 (a single cell) takes scale = 0, so its point is the translation (the reference computes 0 * inf = NaN).
"""
import ctypes

import numpy as np
import torch


class PointCloud(object):
    """The packed result of voxel_points for B objects: object b owns rows offsets[b] .. offsets[b + 1] - 1 of `points`.

    points   float32 [N,3] on the device (N = the total, or the caller's capacity)
    offsets  int64 [B+1] on the device, offsets[B] = the true total even when `points` is shorter
    counts   int32 [B] on the device;  bbox int32 [B,6] = (lo_i, lo_j, lo_k, hi_i, hi_j, hi_k) of ALL occupied cells"""
    __slots__ = ('points', 'offsets', 'counts', 'bbox')

    def __init__(self, points, offsets, counts, bbox):
        self.points, self.offsets, self.counts, self.bbox = points, offsets, counts, bbox

    def __len__(self):
        return int(self.counts.shape[0])

    def total(self):
        """Points of all objects (reads 8 bytes: synchronises)."""
        return int(self.offsets[-1].item())

    def truncated(self):
        """True when `points` was too short for the total (a caller-given capacity); synchronises."""
        return self.total() > int(self.points.shape[0])

    def split(self):
        """-> list of B numpy [n_b,3] float32 arrays, the reference's `objsPoints`; rows cut off by a capacity are missing."""
        off = self.offsets.cpu().numpy()
        pts = self.points.cpu().numpy()
        return [pts[min(int(off[b]), len(pts)):min(int(off[b + 1]), len(pts))] for b in range(len(off) - 1)]


def _device_rows(x, device, shape, what):
    from .tensor import DeviceArray
    if isinstance(x, DeviceArray):
        x = x.t
    t = x if isinstance(x, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32))
    t = t.to(device=device, dtype=torch.float32).reshape(-1, *shape[1:]).contiguous()
    if tuple(t.shape) != shape:
        raise ValueError('%s must be %s, got %s' % (what, list(shape), list(t.shape)))
    return t


def _pose_rows(pose, B, device):
    """None, [4,4] / [3,4] (one pose for every object) or a batch of them -> float32 [B,16] on the device (or None)."""
    from .tensor import DeviceArray
    if pose is None:
        return None
    if isinstance(pose, DeviceArray):
        pose = pose.t
    t = pose if isinstance(pose, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(pose, dtype=np.float32))
    t = t.to(device=device, dtype=torch.float32)
    if t.dim() == 2:
        t = t.unsqueeze(0).expand(B, -1, -1)
    if t.dim() != 3 or t.shape[0] != B or tuple(t.shape[1:]) not in ((4, 4), (3, 4)):
        raise ValueError('pose must be [4,4] or [3,4], or a batch [%d,...] of them, got %s' % (B, list(t.shape)))
    full = torch.eye(4, dtype=torch.float32, device=device).repeat(B, 1, 1)
    full[:, :t.shape[1]] = t
    return full.reshape(B, 16).contiguous()


def voxel_points(occ, dims, pose=None, prob=0.5, surface_only=False, packed=False, side=None, capacity=None):
    """Occupancy grids -> PointCloud.

    occ           [B,D,D,D,1] (any shape [B, D^3 values]) probabilities: torch CUDA tensor, DeviceArray, HostPrediction or numpy; a cell is
                  occupied iff p > prob (a NaN cell is not).  Or bits: a PackedVoxels, or with packed=True a uint8 array / tensor
                  [B, D^3 / 8] in the layout of vv_pack_bits (then `side` is needed); `prob` plays no part.
    dims          [B,3] = (h, w, l) per object;  pose: None (identity), one [4,4] / [3,4] or [B, ...] of them.
    surface_only  only occupied cells on the grid boundary or with an unoccupied face neighbour (an extension; the reference emits solid
                  objects).  The box and the scale stay those of all occupied cells: the result is the ordered subset of the full one.
    capacity      None: the count runs, its 8-byte total is read (THE one synchronisation of this call), exactly that many rows are
                  allocated and filled.  A number: `points` gets that many rows and nothing synchronises; rows past it are not written
                  and PointCloud.truncated() tells.
    Runs on the current stream of the device `occ` lives on (voxvae's default device for host input).  There is no CPU fallback."""
    import voxvae
    from . import lib as L
    from .hostio import PackedVoxels
    from .tensor import DeviceArray, as_device_f32
    held = occ.t if isinstance(occ, DeviceArray) else occ
    device = held.device if isinstance(held, torch.Tensor) and held.is_cuda else torch.device(voxvae.default_device())
    if device.type != 'cuda':
        raise L.VoxVaeError('voxel_points runs on the GPU only (default device %s); there is no CPU fallback' % device)
    if isinstance(occ, PackedVoxels):
        packed, side = True, (int(occ.shape[1]) if side is None else side)
        occ = occ.bits
    if packed:
        if side is None:
            raise ValueError('packed bits carry no shape: pass side')
        t = occ if isinstance(occ, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(occ, dtype=np.uint8))
        if t.dtype != torch.uint8:
            raise ValueError('packed occupancy must be uint8, got %s' % t.dtype)
        t = t.to(device).contiguous()
        B = int(t.shape[0]) if t.dim() else 0
        per = t.numel() * 8 // B if B else 0
    else:
        t = as_device_f32(occ, device)
        B = int(t.shape[0]) if t.dim() else 0
        per = t.numel() // B if B else 0
        if side is None:
            side = int(t.shape[1]) if t.dim() >= 4 else int(round(per ** (1.0 / 3.0)))
    side = int(side)
    if B == 0 or side ** 3 != per:
        raise ValueError('occupancy %s is not a batch of %d^3 grids' % (list(t.shape), side))
    dims_d = _device_rows(dims, device, (B, 3), 'dims')
    pose_d = _pose_rows(pose, B, device)
    lib = L.load()
    need = lib.vv_voxel_points_workspace_bytes(B, side)
    if need == 0:
        raise ValueError('unsupported shape: batch %d, side %d (1 .. 128)' % (B, side))
    ws = torch.empty(need, dtype=torch.uint8, device=device)
    counts = torch.empty(B, dtype=torch.int32, device=device)
    bbox = torch.empty(B, 6, dtype=torch.int32, device=device)
    offsets = torch.empty(B + 1, dtype=torch.int64, device=device)
    st = ctypes.c_void_p(torch.cuda.current_stream(device).cuda_stream)
    head = (L.ptr(t), int(bool(packed)), float(prob), int(bool(surface_only)))
    L.call('vv_voxel_points_count', *head, B, side, L.ptr(counts), L.ptr(bbox), L.ptr(offsets), L.ptr(ws), need, st)
    cap = int(offsets[-1].item()) if capacity is None else int(capacity)
    if cap < 0:
        raise ValueError('capacity must be >= 0, got %r' % (capacity,))
    points = torch.empty(cap, 3, dtype=torch.float32, device=device)
    L.call('vv_voxel_points_emit', *head, L.ptr(dims_d), L.ptr(pose_d), L.ptr(offsets), L.ptr(bbox), L.ptr(points) if cap else None, cap,
           L.ptr(ws), need, B, side, st)
    return PointCloud(points, offsets, counts, bbox)
