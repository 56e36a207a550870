"""Occupancy grid -> posed point cloud A/B: (a) vv_voxel_points_count + vv_voxel_points_emit into a preallocated buffer (no
synchronisation) against what is available without them --
  (b1) torch on the device: `torch.nonzero` of the thresholded grids (it synchronises: the result's size is data), per-object
       amin / amax through scatter_reduce, then elementwise ops and a batched matmul;
  (b2) the host path: the float32 probabilities copied device -> host, then the definition in float64 numpy per object (what the
       reference's src/visualizer/visualizer.py:171-188 does with a downloaded grid).
HIP events for (a) and (b1), wall clock around copy + numpy for (b2); the sides alternate back to back; medians and spreads (max - min) over
the alternations go to profiles/points_ab.json, with input bytes / time for (a) beside the 6.29 TB/s copy rate DESIGN uses.

The object is a solid ellipsoid with per-object radii, about 10 % of the grid (ModelNet's fill at these sides), predicted with the
confidence of a trained model: sigmoid of N(+-14, 12) logits.

    python profiles/microbench/mb_points.py [--out PATH] [--alternations 7]
"""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np
import torch

_R = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, _R)
sys.path.insert(0, os.path.join(_R, 'anytime-3d-reconstruction_amd'))
from voxvae import lib as L

DEV = 'cuda:0'
COPY_TB_S = 6.29
SHAPES = ((256, 32, 20), (64, 64, 10))            # batch, side, launches per timing


def _st():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _timed(fn, n):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    e1.synchronize()
    return 1e3 * e0.elapsed_time(e1) / n          # us per call


def _wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return 1e6 * (time.perf_counter() - t0)


def _median(v):
    s = sorted(v)
    return s[len(s) // 2] if len(s) % 2 else 0.5 * (s[len(s) // 2 - 1] + s[len(s) // 2])


def _stat(v):
    return {'median': round(_median(v), 2), 'spread': round(max(v) - min(v), 2), 'all': [round(x, 2) for x in v]}


def make_objects(B, D):
    g = torch.Generator(device=DEV).manual_seed(B + D)
    ax = (torch.arange(D, device=DEV, dtype=torch.float32) + 0.5) / D - 0.5
    zi, yi, xi = torch.meshgrid(ax, ax, ax, indexing='ij')
    r = 0.18 + 0.22 * torch.rand(B, 3, device=DEV, generator=g)                  # semi-axes: fill 4/3 pi r0 r1 r2 ~ 10 %
    inside = ((zi[None] / r[:, 0, None, None, None]) ** 2 + (yi[None] / r[:, 1, None, None, None]) ** 2
              + (xi[None] / r[:, 2, None, None, None]) ** 2) < 1.0
    logits = 12.0 * torch.randn(B, D, D, D, device=DEV, generator=g) + torch.where(inside, 14.0, -14.0)
    return torch.sigmoid(logits).contiguous()


def numpy_definition(p, dims, pose):
    """The step's definition in float64 numpy, object by object: what a host caller runs on the downloaded grids."""
    out = []
    for b in range(len(p)):
        cells = np.argwhere(p[b] > 0.5).astype(np.float64)                      # row-major order
        if not len(cells):
            out.append(np.zeros((0, 3)))
            continue
        lo = cells.min(axis=0)
        ext = cells.max(axis=0) - lo
        E = ext.max()
        scale = float(dims[b].max()) / E if E > 0 else 0.0
        q = (cells - lo) * scale - ext * scale / 2.0
        out.append(q @ pose[b, :3, :3].astype(np.float64).T + pose[b, :3, 3])
    return out


def run_case(lib, B, D, n, alternations, surface):
    V = D ** 3
    p = make_objects(B, D)
    rng = np.random.default_rng(B)
    dims_h = rng.uniform(0.3, 5.0, (B, 3)).astype(np.float32)
    pose_h = np.tile(np.eye(4, dtype=np.float32), (B, 1, 1))
    for b in range(B):
        q, _ = np.linalg.qr(rng.standard_normal((3, 3)))
        pose_h[b, :3, :3], pose_h[b, :3, 3] = q, rng.uniform(-20, 20, 3)
    dims, pose = torch.from_numpy(dims_h).to(DEV), torch.from_numpy(pose_h).to(DEV)
    need = lib.vv_voxel_points_workspace_bytes(B, D)
    ws = torch.empty(need, dtype=torch.uint8, device=DEV)
    counts, bbox = torch.empty(B, dtype=torch.int32, device=DEV), torch.empty(B, 6, dtype=torch.int32, device=DEV)
    offsets = torch.empty(B + 1, dtype=torch.int64, device=DEV)
    cap = B * V
    points = torch.empty(cap, 3, dtype=torch.float32, device=DEV)

    def a():
        L.call('vv_voxel_points_count', L.ptr(p), 0, 0.5, surface, B, D, L.ptr(counts), L.ptr(bbox), L.ptr(offsets), L.ptr(ws), need, _st())
        L.call('vv_voxel_points_emit', L.ptr(p), 0, 0.5, surface, L.ptr(dims), L.ptr(pose), L.ptr(offsets), L.ptr(bbox), L.ptr(points), cap,
               L.ptr(ws), need, B, D, _st())

    held = {}

    def b1():
        idx = torch.nonzero(p > 0.5)                                            # [N,4] = (b, i, j, k), row-major: synchronises
        ob, cell = idx[:, 0], idx[:, 1:].float()
        lo = torch.full((B, 3), float(D), device=DEV).scatter_reduce(0, ob[:, None].expand(-1, 3), cell, 'amin')
        hi = torch.full((B, 3), -1.0, device=DEV).scatter_reduce(0, ob[:, None].expand(-1, 3), cell, 'amax')
        ext = hi - lo
        scale = dims.max(dim=1).values / ext.max(dim=1).values
        q = (cell - lo[ob]) * scale[ob, None] - (ext * scale[:, None])[ob] / 2.0
        held['b1'] = torch.einsum('nij,nj->ni', pose[ob, :3, :3], q) + pose[ob, :3, 3]

    def b2():
        held['b2'] = numpy_definition(p.cpu().numpy(), dims_h, pose_h)

    a(); torch.cuda.synchronize()
    total = int(offsets[-1].item())
    res = {'batch': B, 'side': D, 'surface_only': bool(surface), 'points': total, 'fill': round(float((p > 0.5).float().mean().item()), 4),
           'launches_per_timing': n, 'alternations': alternations}
    if not surface:
        b1(); b2(); torch.cuda.synchronize()
        ref = np.concatenate(held['b2'], axis=0)
        got = points[:total].cpu().numpy().astype(np.float64)
        res['a_vs_numpy_max_abs'] = float(np.abs(got - ref).max())
        res['b1_vs_numpy_max_abs'] = float(np.abs(held['b1'].cpu().numpy().astype(np.float64) - ref).max())
    for _ in range(2):
        _timed(a, n)
        if not surface:
            _timed(b1, max(1, n // 5))
    ta, tb1, tb2 = [], [], []
    for _ in range(alternations):
        ta.append(_timed(a, n))
        if not surface:
            tb1.append(_timed(b1, max(1, n // 5)))
            tb2.append(_wall(b2))
    ma = _median(ta)
    in_bytes = 2 * B * V * 4                                                    # the grid is read by the count and by the emit
    res.update({'a_count_emit_us': _stat(ta), 'a_input_bytes': in_bytes, 'a_input_TB_per_s': round(in_bytes / (ma * 1e-6) / 1e12, 3),
                'a_share_of_copy_rate': round(in_bytes / (ma * 1e-6) / 1e12 / COPY_TB_S, 3)})
    if not surface:
        res.update({'b1_torch_nonzero_us': _stat(tb1), 'b2_d2h_numpy_us': _stat(tb2), 'b1_over_a': round(_median(tb1) / ma, 2),
                    'b2_over_a': round(_median(tb2) / ma, 2)})
    return res


if __name__ == '__main__':
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument('--out', default=os.path.join(_R, 'profiles', 'points_ab.json'))
    ap.add_argument('--alternations', type=int, default=7)
    args = ap.parse_args()
    lib = L.load()
    res = {'library': os.path.relpath(lib._name, _R), 'device': torch.cuda.get_device_name(0), 'copy_rate_TB_per_s': COPY_TB_S,
           'counters': 'not measured', 'cases': []}
    for B, D, n in SHAPES:
        for surface in (0, 1):
            r = run_case(lib, B, D, n, args.alternations, surface)
            print(json.dumps(r), flush=True)
            res['cases'].append(r)
    with open(args.out, 'w') as f:
        json.dump(res, f, indent=1)
        f.write('\n')
