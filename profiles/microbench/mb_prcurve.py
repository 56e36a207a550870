"""Precision / recall curve A/B: (a) one vv_pr_curve_accumulate call (sorted thresholds, one group) against (b) the composition available
without it -- torch `((p > t) & y).sum()` and `((p > t) & ~y).sum()` per threshold on the same device tensors (the target as a bool tensor
prepared outside the timing).  HIP events, the two sides alternating back to back; medians and spreads (max - min) over the alternations go
to profiles/pr_curve_ab.json, with input bytes / time for (a) beside the 6.29 TB/s copy rate DESIGN uses.

Probabilities: 'uniform' (every wave scans most of the thresholds) and 'saturated' (sigmoid of N(0, 12) logits at 3 % occupancy-like
skew: what a trained model emits; a wave stops at the first threshold none of its voxels exceeds).

    python profiles/microbench/mb_prcurve.py [--out PATH] [--alternations 7]
"""
import argparse
import ctypes
import json
import os
import sys

os.environ.setdefault('VOXVAE_TEST_HOOKS', '1')   # as the other microbenchmarks; no kernel-form override is set here
import numpy as np
import torch

_R = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, _R)
sys.path.insert(0, os.path.join(_R, 'anytime-3d-reconstruction_amd'))
from voxvae import lib as L
from voxvae.prcurve import notebook_thresholds

DEV = 'cuda:0'
COPY_TB_S = 6.29
SHAPES = ((256, 32 ** 3, 19, 20), (256, 32 ** 3, 59, 10), (64, 64 ** 3, 19, 10))     # batch, voxels, thresholds, launches per timing


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


def _median(v):
    s = sorted(v)
    return s[len(s) // 2] if len(s) % 2 else 0.5 * (s[len(s) // 2 - 1] + s[len(s) // 2])


def _stat(v):
    return {'median': round(_median(v), 2), 'spread': round(max(v) - min(v), 2), 'all': [round(x, 2) for x in v]}


def run_case(lib, B, V, T, n, alternations, kind, packed):
    torch.manual_seed(B + T)
    thr = np.sort(np.array(notebook_thresholds(20, full=(T == 59)), dtype=np.float32))
    assert len(thr) == T
    y = (torch.rand(B, V, device=DEV) < 0.1)
    if kind == 'uniform':
        p = torch.rand(B, V, device=DEV)
    else:                                          # confident and mostly right, as at a trained model
        p = torch.sigmoid(12.0 * torch.randn(B, V, device=DEV) + torch.where(y, 14.0, -14.0))
    yf = y.float().contiguous()
    bits = torch.empty(B * V // 8, dtype=torch.uint8, device=DEV)
    L.call('vv_pack_bits', L.ptr(yf), L.ptr(bits), 0.5, B * V, _st())
    tgt = bits if packed else yf
    td = torch.from_numpy(thr).to(DEV)
    ws = torch.empty(lib.vv_pr_curve_workspace_bytes(B, V, T), dtype=torch.uint8, device=DEV)
    acc, tot = torch.zeros(T * 2, dtype=torch.int64, device=DEV), torch.zeros(2, dtype=torch.int64, device=DEV)
    out_b = torch.zeros(T, 2, dtype=torch.int64, device=DEV)
    ny = ~y
    tl = [float(t) for t in thr]

    def a():
        L.call('vv_pr_curve_accumulate', L.ptr(p), L.ptr(tgt), int(packed), L.ptr(td), T, 1, None, 1, L.ptr(acc), L.ptr(tot), L.ptr(ws),
               ws.numel(), B, V, _st())

    def b():
        for i, t in enumerate(tl):
            m = p > t
            out_b[i, 0] = (m & y).sum()
            out_b[i, 1] = (m & ny).sum()

    a(); b(); torch.cuda.synchronize()
    same = bool(torch.equal(acc.view(T, 2), out_b))
    for _ in range(2):
        _timed(a, n); _timed(b, max(1, n // 5))
    ta, tb = [], []
    for _ in range(alternations):
        ta.append(_timed(a, n))
        tb.append(_timed(b, max(1, n // 5)))
    in_bytes = B * V * 4 + (B * V // 8 if packed else B * V * 4)
    ma = _median(ta)
    return {'batch': B, 'voxels': V, 'thresholds': T, 'probabilities': kind, 'target': 'packed' if packed else 'float32',
            'launches_per_timing': n, 'alternations': alternations, 'a_pr_curve_us': _stat(ta), 'b_torch_per_threshold_us': _stat(tb),
            'b_over_a': round(_median(tb) / ma, 2), 'a_input_bytes': in_bytes, 'a_input_TB_per_s': round(in_bytes / (ma * 1e-6) / 1e12, 3),
            'a_share_of_copy_rate': round(in_bytes / (ma * 1e-6) / 1e12 / COPY_TB_S, 3), 'counts_identical_a_vs_b': same}


if __name__ == '__main__':
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument('--out', default=os.path.join(_R, 'profiles', 'pr_curve_ab.json'))
    ap.add_argument('--alternations', type=int, default=7)
    args = ap.parse_args()
    lib = L.load()
    res = {'library': os.path.relpath(lib._name, _R), 'device': torch.cuda.get_device_name(0), 'copy_rate_TB_per_s': COPY_TB_S,
           'counters': 'not measured', 'cases': []}
    for B, V, T, n in SHAPES:
        for kind in ('uniform', 'saturated'):
            for packed in (False, True):
                r = run_case(lib, B, V, T, n, args.alternations, kind, packed)
                print(json.dumps(r), flush=True)
                res['cases'].append(r)
    with open(args.out, 'w') as f:
        json.dump(res, f, indent=1)
        f.write('\n')
