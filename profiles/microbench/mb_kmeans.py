"""Viewpoint k-means: device time of vv_kmeans_cosine (HIP events around the one call that enqueues every launch) beside the host entry
vv_kmeans_cosine_host (wall clock, one thread) and the numpy definition of tests/_kmeans_ref.py (wall clock; the stand-in for the
reference's loop over the centres, which builds the same [N, k] temporaries), at (N, k) = (40000, 360) -- a Pascal3D+ split with the
reference's k = 30 * 12 -- and (1500, 30).  Per shape:

    full call      max_iter = 1000 with the early exit: the iterations that do work plus the launches that return at once
    per iteration  the exit defeated by measuring only iterations that do work: (time at max_iter = 8 - time at max_iter = 4) / 4, with
                   `iterations` checked to be 8 (the labels have not settled by then)

Medians and spreads (max - min) over the repeats go to profiles/kmeans_ab.json.  No gate is attached to these numbers: they are a
record, not a promise.

    python profiles/microbench/mb_kmeans.py [--out PATH] [--repeats 5]
"""
import argparse
import json
import os
import random
import sys
import time

import numpy as np
import torch

_R = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, _R)
sys.path.insert(0, os.path.join(_R, 'anytime-3d-reconstruction_amd'))
sys.path.insert(0, os.path.join(_R, 'tests'))
import _kmeans_ref as R
from voxvae import kmeans as K
from voxvae import lib as L

DEV = 'cuda:0'
SHAPES = ((40000, 360), (1500, 30))


def _median(v):
    s = sorted(v)
    return s[len(s) // 2] if len(s) % 2 else 0.5 * (s[len(s) // 2 - 1] + s[len(s) // 2])


def _stat(v):
    return {'median': round(_median(v), 3), 'spread': round(max(v) - min(v), 3), 'all': [round(x, 3) for x in v]}


def device_ms(x, c0, max_iter):
    """-> (ms between events around the call, iterations, result)."""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    out = K.kmeans(x, c0, max_iter)                 # (allocates its outputs and reads `iterations` back: both inside the window)
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1), out[3], out


def host_ms(X, C0, max_iter):
    t0 = time.perf_counter()
    out = K.kmeans(X, C0, max_iter, host=True)
    return 1e3 * (time.perf_counter() - t0), out[3], out


def run_case(n, k, repeats):
    X = R.viewpoints(n, 1000 + n)
    random.seed(n)
    C0 = X[random.sample(range(n), k)].copy()
    x, c0 = torch.from_numpy(X).to(DEV), torch.from_numpy(C0).to(DEV)
    device_ms(x, c0, 2)                             # warm up: module load, allocator
    full_d, t4_d, t8_d = [], [], []
    for _ in range(repeats):
        ms, its, out_d = device_ms(x, c0, 1000)
        full_d.append(ms)
        t4_d.append(device_ms(x, c0, 4)[0])
        ms8, its8, _ = device_ms(x, c0, 8)
        t8_d.append(ms8)
    ms_h, its_h, out_h = host_ms(X, C0, 1000)
    h4 = [host_ms(X, C0, 4)[0] for _ in range(2)]
    h8 = [host_ms(X, C0, 8)[0] for _ in range(2)]
    same = all(torch.equal(a.cpu(), b) for a, b in zip(out_d[:3], out_h[:3])) and its == its_h
    ref = []
    for _ in range(2):                              # one iteration of the definition: assignment and update
        t0 = time.perf_counter()
        xtoc, _, _ = R.assign(X, C0)
        R.update(X, C0, xtoc)
        ref.append(1e3 * (time.perf_counter() - t0))
    per_d = (_median(t8_d) - _median(t4_d)) / 4
    per_h = (_median(h8) - _median(h4)) / 4
    return {'n': n, 'k': k, 'repeats': repeats, 'iterations_that_did_work': int(its), 'iterations_at_max_iter_8': int(its8),
            'device_equals_host_bit_for_bit': bool(same),
            'device_full_call_ms': _stat(full_d), 'device_max_iter_4_ms': _stat(t4_d), 'device_max_iter_8_ms': _stat(t8_d),
            'device_ms_per_working_iteration': round(per_d, 4),
            'host_entry_full_call_ms': round(ms_h, 2), 'host_entry_max_iter_4_ms': _stat(h4), 'host_entry_max_iter_8_ms': _stat(h8),
            'host_entry_ms_per_working_iteration': round(per_h, 3),
            'numpy_definition_ms_per_iteration': _stat(ref),
            'host_entry_over_device_per_iteration': round(per_h / per_d, 1) if per_d > 0 else None,
            'numpy_definition_over_device_per_iteration': round(_median(ref) / per_d, 1) if per_d > 0 else None,
            'host_entry_over_device_full_call': round(ms_h / _median(full_d), 1)}


if __name__ == '__main__':
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument('--out', default=os.path.join(_R, 'profiles', 'kmeans_ab.json'))
    ap.add_argument('--repeats', type=int, default=5)
    args = ap.parse_args()
    lib = L.load()
    res = {'library': os.path.relpath(lib._name, _R), 'device': torch.cuda.get_device_name(0), 'counters': 'not measured',
           'note': 'the numpy definition stands in for the reference class, which was not timed; device windows include the output '
                   'allocations and the 4-byte read-back of `iterations`', 'cases': []}
    for n, k in SHAPES:
        r = run_case(n, k, args.repeats)
        print(json.dumps(r), flush=True)
        res['cases'].append(r)
    with open(args.out, 'w') as f:
        json.dump(res, f, indent=1)
        f.write('\n')
