"""Sampled-mean last layer A/B (bf16): (a) vv_convT3d_final_mean_fwd against (b) the composition available without it --
vv_convT3d_final_bce_fwd with `probs` over the same B*K samples (target tiled K times), the torch mean over K and the torch recomputation of
(bce, TP, FP, FN) on the averaged grid.  HIP events, the two sides alternating back to back; medians and spreads (max - min) over the
alternations go to profiles/sampled_mean_ab.json.

    python profiles/microbench/mb_sampled.py [--out PATH] [--alternations 7]
"""
import argparse
import ctypes
import json
import os
import sys

os.environ.setdefault('VOXVAE_TEST_HOOKS', '1')   # the kernel-form overrides live in lib/libvoxvae_hooks.so (voxvae/lib.py); none is set here
import torch

_R = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, _R)
sys.path.insert(0, os.path.join(_R, 'anytime-3d-reconstruction_amd'))
from voxvae import lib as L

DEV = 'cuda:0'
GAMMA, EPS = 0.6, 1e-7
SHAPES = (('32^3', 16, 8, 32, 20), ('32^3', 16, 1, 32, 40), ('64^3', 32, 8, 32, 5))     # model, side of the last hidden layer, B, K, launches per timing


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


def run_shape(lib, model, side, B, K, n, alternations):
    D = 2 * side
    torch.manual_seed(side * 100 + B)
    x = torch.randn(B * K, side, side, side, 64, device=DEV).to(torch.bfloat16)
    w = (torch.randn(4, 4, 4, 1, 64, device=DEV) / 16).float().contiguous()
    y = (torch.rand(B, D, D, D, 1, device=DEV) < 0.1).float().contiguous()
    y_tiled = y[:, None].expand(B, K, D, D, D, 1).reshape(B * K, D, D, D, 1).contiguous()
    ws_a = torch.empty(max(lib.vv_convT3d_final_mean_workspace_bytes(B, K, side), 16), dtype=torch.uint8, device=DEV)
    ws_b = torch.empty(max(lib.vv_convT3d_final_bce_workspace_bytes(B * K, side), 16), dtype=torch.uint8, device=DEV)
    mean_a, stats_a = torch.empty(B, D, D, D, 1, device=DEV), torch.empty(B, 4, device=DEV)
    probs, stats_k = torch.empty(B * K, D, D, D, 1, device=DEV), torch.empty(B * K, 4, device=DEV)
    out_b = {}

    def a():
        L.call('vv_convT3d_final_mean_fwd', L.ptr(x), L.ptr(w), L.ptr(y), L.ptr(mean_a), L.ptr(stats_a), B, K, side, 64, GAMMA, EPS, L.VV_BF16,
               L.ptr(ws_a), ws_a.numel(), _st())

    def b():
        L.call('vv_convT3d_final_bce_fwd', L.ptr(x), L.ptr(w), L.ptr(y_tiled), L.ptr(probs), None, L.ptr(stats_k), B * K, side, 64, GAMMA, EPS,
               L.VV_BF16, L.ptr(ws_b), ws_b.numel(), _st())
        p = probs.view(B, K, -1).mean(dim=1)
        t = y.view(B, -1)
        q = p.clamp(EPS, 1.0 - EPS)
        bce = -(GAMMA * t * torch.log(q) + (1.0 - GAMMA) * (1.0 - t) * torch.log(1.0 - q)).sum(-1)
        yh = (p >= 0.5).float()
        out_b['mean'], out_b['stats'] = p, torch.stack([bce, (t * yh).sum(-1), ((1.0 - t) * yh).sum(-1), (t * (1.0 - yh)).sum(-1)], dim=1)

    a(); b(); torch.cuda.synchronize()
    dmean = (mean_a.view(B, -1) - out_b['mean']).abs().max().item()
    dcount = (stats_a[:, 1:] - out_b['stats'][:, 1:]).abs().max().item()
    for _ in range(2):
        _timed(a, n); _timed(b, n)
    ta, tb = [], []
    for _ in range(alternations):
        ta.append(_timed(a, n))
        tb.append(_timed(b, n))
    x_bytes = x.numel() * 2
    ma, mb = _median(ta), _median(tb)
    return {'model': model, 'side': side, 'objects': B, 'samples': K, 'launches_per_timing': n, 'alternations': alternations,
            'a_final_mean_us': {'median': round(ma, 2), 'spread': round(max(ta) - min(ta), 2), 'all': [round(v, 2) for v in ta]},
            'b_composition_us': {'median': round(mb, 2), 'spread': round(max(tb) - min(tb), 2), 'all': [round(v, 2) for v in tb]},
            'a_within_b_plus_spread': bool(ma <= mb + (max(tb) - min(tb))),
            'x_bytes': x_bytes, 'a_input_TB_per_s': round(x_bytes / (ma * 1e-6) / 1e12, 3),
            'max_abs_mean_diff_a_vs_b': dmean, 'max_count_diff_a_vs_b': dcount}


if __name__ == '__main__':
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument('--out', default=os.path.join(_R, 'profiles', 'sampled_mean_ab.json'))
    ap.add_argument('--alternations', type=int, default=7)
    args = ap.parse_args()
    lib = L.load()
    res = {'library': os.path.relpath(lib._name, _R), 'device': torch.cuda.get_device_name(0), 'dtype': 'bf16', 'shapes': []}
    for model, side, B, K, n in SHAPES:
        r = run_shape(lib, model, side, B, K, n, args.alternations)
        print(json.dumps(r), flush=True)
        res['shapes'].append(r)
    with open(args.out, 'w') as f:
        json.dump(res, f, indent=1)
        f.write('\n')
