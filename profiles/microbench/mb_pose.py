"""Detections -> posed objects: device time per call of vv_object_pose (two launches, HIP events) beside the host entry
vv_object_pose_host on the same inputs (wall clock, one thread), for n in {1, 16, 256, 4096} detections tiled from the recorded fixtures
(tests/golden/pose_kitti.npz: 88 % kept, the rest pre-filtered or without an accepted candidate).  Medians and spreads (max - min) over
the alternations go to profiles/pose_ab.json.  No gate is attached to these numbers: they are a record, not a promise.

The file also carries the one figure known for the reference's own code: its getTranslation alone takes 21 ms per object (numpy 2.2 on a
CPU-only box, 200 synthetic KITTI-like detections) -- measured on another machine and another CPU, so it is context, not one side of an A/B.

    python profiles/microbench/mb_pose.py [--out PATH] [--alternations 7]
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
SIZES = ((1, 50), (16, 50), (256, 20), (4096, 5))          # n, launches per timing


def _median(v):
    s = sorted(v)
    return s[len(s) // 2] if len(s) % 2 else 0.5 * (s[len(s) // 2 - 1] + s[len(s) // 2])


def _stat(v):
    return {'median': round(_median(v), 2), 'spread': round(max(v) - min(v), 2), 'all': [round(x, 2) for x in v]}


def _timed(fn, n):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    e1.synchronize()
    return 1e3 * e0.elapsed_time(e1) / n          # us per call


def run_case(lib, g, n, launches, alternations):
    rows = np.arange(n) % len(g['bbox2d'])
    host_in = [np.ascontiguousarray(g[k][rows]) for k in ('bbox2d', 'bbox3d', 'sin', 'cos')]
    dev_in = [torch.from_numpy(a).to(DEV) for a in host_in]
    P = np.ascontiguousarray(g['proj_mat'])
    Pinv = np.ascontiguousarray(np.linalg.inv(P))
    col, row = float(g['image_size'][0]), float(g['image_size'][1])
    pp = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    shapes = (('keep', (n,), 'i'), ('candidate', (n,), 'i'), ('iou', (n,), 'f'), ('count', (1,), 'i'), ('index', (n,), 'i'), ('pose', (n, 16), 'f'),
              ('size', (n, 3), 'f'), ('box2d', (n, 4), 'i'), ('proj', (n, 16), 'f'))
    dev_out = [torch.empty(s, dtype=torch.int32 if t == 'i' else torch.float32, device=DEV) for _, s, t in shapes]
    host_out = [np.zeros(s, dtype=np.int32 if t == 'i' else np.float32) for _, s, t in shapes]
    need = lib.vv_object_pose_workspace_bytes(n)
    ws = torch.empty(need, dtype=torch.uint8, device=DEV)
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

    def a():
        L.call('vv_object_pose', *[L.ptr(t) for t in dev_in], n, col, row, pp(P), pp(Pinv), *[L.ptr(t) for t in dev_out], L.ptr(ws), need, st)

    def b():
        t0 = time.perf_counter()
        L.call('vv_object_pose_host', *[pp(x) for x in host_in], n, col, row, pp(P), pp(Pinv), *[pp(x) for x in host_out], None, 0)
        return 1e6 * (time.perf_counter() - t0)

    a(); torch.cuda.synchronize(); b()
    M = int(host_out[3][0])                       # per-detection outputs and the count whole, compacted outputs up to the count
    same = all(np.array_equal(d.cpu().numpy()[:len(h) if k < 4 else M], h[:len(h) if k < 4 else M]) for k, (d, h) in enumerate(zip(dev_out, host_out)))
    for _ in range(2):
        _timed(a, launches)
    ta, tb = [], []
    for _ in range(alternations):
        ta.append(_timed(a, launches))
        tb.append(b())
    return {'n': n, 'kept': int(host_out[3][0]), 'launches_per_timing': launches, 'alternations': alternations,
            'device_equals_host_bit_for_bit': bool(same), 'device_us_per_call': _stat(ta), 'host_entry_us_per_call': _stat(tb),
            'device_us_per_detection': round(_median(ta) / n, 3), 'host_entry_us_per_detection': round(_median(tb) / n, 3),
            'host_over_device': round(_median(tb) / _median(ta), 2)}


if __name__ == '__main__':
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument('--out', default=os.path.join(_R, 'profiles', 'pose_ab.json'))
    ap.add_argument('--alternations', type=int, default=7)
    args = ap.parse_args()
    lib = L.load()
    g = dict(np.load(os.path.join(_R, 'tests', 'golden', 'pose_kitti.npz')))
    res = {'library': os.path.relpath(lib._name, _R), 'device': torch.cuda.get_device_name(0), 'counters': 'not measured',
           'solver_term_host_vs_reference': 2.58e-13,
           'reference_getTranslation_ms_per_object': {'value': 21, 'note': 'measured on a CPU-only box with numpy 2.2, 200 synthetic KITTI-like '
                                                      'detections; another machine: context, not a side of this A/B'},
           'cases': []}
    for n, launches in SIZES:
        r = run_case(lib, g, n, launches, args.alternations)
        print(json.dumps(r), flush=True)
        res['cases'].append(r)
    with open(args.out, 'w') as f:
        json.dump(res, f, indent=1)
        f.write('\n')
