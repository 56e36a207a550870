"""Detector head -> selected detections: device time per call of vv_detect_decode (ONE launch, a workgroup per frame, HIP events) beside
the host entry vv_detect_decode_host on the same frame (wall clock, one thread).  Frames: the reference's 13x13 grid and KITTI's 11x38
(5 predictors, 16 latents: 245 channels) with about 15 % of the predictors lit, top_1 on and off, in both layouts; and the scan's worst
case, 32x32 cells x 4 predictors with every predictor a candidate and disjoint boxes: 4096 picks.  Medians and spreads (max - min) over
the alternations go to profiles/detect_ab.json.  No gate is attached to these numbers: they are a record, not a promise.

    python profiles/microbench/mb_detect.py [--out PATH] [--alternations 7]
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
sys.path.insert(0, os.path.join(_R, 'tests'))
import _detect_ref as R
from voxvae import lib as L

DEV = 'cuda:0'
FIELDS = (('count', None), ('index', 1), ('bbox2d', 5), ('bbox3d', 3), ('inst_mean', 'Z'), ('inst_log_var', 'Z'), ('sin', 3), ('cos', 3), ('rad', 3))


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


def worst_case_head():
    rng = np.random.default_rng(32)
    W = R.width(16)
    f = np.zeros((1, 32, 32, 4, W), np.float32)
    f[..., 0] = rng.uniform(1.0, 4.0, (1, 32, 32, 4))
    f[..., 1:3] = -8.0
    f[..., 3] = np.float32([-2.0, -0.7, 0.7, 2.0])
    f[..., 5:] = rng.normal(0, 1, (1, 32, 32, 4, W - 5))
    return f.reshape(1, 32, 32, 4 * W)


def run_case(name, head, P, Z, top_1, layout, launches, alternations):
    B, Rr, C, CH = head.shape
    N = Rr * C * (1 if top_1 else P)
    stored = np.ascontiguousarray(head.transpose(0, 3, 1, 2)) if layout else head
    dev_in = torch.from_numpy(stored).to(DEV)
    shapes = [(B,) if w is None else (B, N, Z if w == 'Z' else w) for _, w in FIELDS]
    dts = [np.int32 if k in ('count', 'index') else np.float32 for k, _ in FIELDS]
    dev_out = [torch.zeros(s, dtype=torch.int32 if d is np.int32 else torch.float32, device=DEV) for s, d in zip(shapes, dts)]
    host_out = [np.zeros(s, dtype=d) for s, d in zip(shapes, dts)]
    pp = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    scal = (layout, B, Rr, C, P, Z, CH, 0.5, 0.5, 1 if top_1 else 0)

    def a():
        L.call('vv_detect_decode', L.ptr(dev_in), *scal, *[L.ptr(t) for t in dev_out], st)

    def b():
        t0 = time.perf_counter()
        L.call('vv_detect_decode_host', pp(stored), *scal, *[pp(x) for x in host_out])
        return 1e6 * (time.perf_counter() - t0)

    a(); torch.cuda.synchronize(); b()
    M = int(host_out[0][0])
    same = all(np.array_equal(d.cpu().numpy()[:, :M] if k else d.cpu().numpy(), h[:, :M] if k else h, equal_nan=bool(k > 1))
               for k, (d, h) in enumerate(zip(dev_out, host_out)))
    for _ in range(2):
        _timed(a, launches)
    ta, tb = [], []
    for _ in range(alternations):
        ta.append(_timed(a, launches))
        tb.append(b())
    lit = int((head.reshape(-1, R.width(Z))[:, 0] > 0).sum())
    return {'case': name, 'grid': [Rr, C], 'predictors': P, 'top_1': bool(top_1), 'layout': 'planes' if layout else 'channels innermost',
            'slots': N, 'predictors_above_threshold': lit, 'picks': M, 'head_bytes': int(head.nbytes), 'launches_per_timing': launches,
            'alternations': alternations, 'device_equals_host_bit_for_bit': bool(same), 'device_us_per_call': _stat(ta),
            'host_entry_us_per_call': _stat(tb), 'host_over_device': round(_median(tb) / _median(ta), 2)}


if __name__ == '__main__':
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument('--out', default=os.path.join(_R, 'profiles', 'detect_ab.json'))
    ap.add_argument('--alternations', type=int, default=7)
    args = ap.parse_args()
    lib = L.load()
    res = {'library': os.path.relpath(lib._name, _R), 'device': torch.cuda.get_device_name(0), 'counters': 'not measured',
           'host_entry_vs_reference_max_float_difference': R.FIXTURE_MAX_DIFF, 'activation_max_error_float32_units': R.ACT_MAX_ULP, 'cases': []}
    cases = []
    for name, (Rr, C) in (('13x13', (13, 13)), ('11x38', (11, 38))):
        head = R.seeded_head(Rr * C, 1, Rr, C, 5, 16)
        for top_1 in (True, False):
            for layout in (0, 1):
                cases.append((name, head, 5, 16, top_1, layout, 50))
    cases.append(('32x32x4 all candidates, disjoint', worst_case_head(), 4, 16, False, 0, 3))
    for c in cases:
        r = run_case(*c, args.alternations)
        print(json.dumps(r), flush=True)
        res['cases'].append(r)
    with open(args.out, 'w') as f:
        json.dump(res, f, indent=1)
        f.write('\n')
