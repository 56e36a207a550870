"""The image encoder (Darknet19 + head2D) on csrc/conv2d.hip beside the stock PyTorch path, per layer and whole, for the two workloads the
project ships: one 416x416 frame with nolbo_test's head (3 x 1024 k3 + 245), and 72 frames of 256x256 with nolboSingleObject_VAE's head
(one 1x1 to 32, BASELINE config 3).  engine='hip' in 'f32' and 'bf16'; baseline engine='torch' (float32, what users have today) in the
same process; torch in channels_last bf16 as an honesty row (whole encoder only).  HIP events around n calls, medians over alternating
runs.  Records time, valid-MAC rate and the fraction of the MFMA peak of the dtype (dense bf16 2516.6 TFLOP/s, f32 157.3 TFLOP/s).
No gate is attached to these numbers: they are a record, not a promise.

    python profiles/microbench/mb_conv2d.py [--out PATH] [--alternations 5]
"""
import argparse
import ctypes
import json
import os
import sys

import numpy as np
import torch

_R = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, _R)
sys.path.insert(0, os.path.join(_R, 'anytime-3d-reconstruction_amd'))
import voxvae
from voxvae import lib as L
from voxvae import workload as W

DEV = 'cuda:0'
PEAK_TMACS = {'f32': 157.3 / 2, 'bf16': 2516.6 / 2}


def _median(v):
    s = sorted(v)
    return s[len(s) // 2] if len(s) % 2 else 0.5 * (s[len(s) // 2 - 1] + s[len(s) // 2])


def _timed(fn, n):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    e1.synchronize()
    return 1e3 * e0.elapsed_time(e1) / n          # us per call


def alternate(fns, n, alternations):
    """{name: median us} of several callables timed in turn, `alternations` rounds after one warm-up round."""
    for f in fns.values():
        _timed(f, max(1, n // 2))
    t = {k: [] for k in fns}
    for _ in range(alternations):
        for k, f in fns.items():
            t[k].append(_timed(f, n))
    return {k: round(_median(v), 2) for k, v in t.items()}, {k: round(max(v) - min(v), 2) for k, v in t.items()}


def build(engine, head, activation='lrelu'):
    import src.net_core.darknet as darknet
    torch.manual_seed(0)
    b = darknet.Darknet19(name='b', activation=activation, device=DEV, engine=engine)
    h = darknet.head2D('h', (None, None, 1024), head[2], head[0], head[1], last_pooling=None, activation=activation, device=DEV, engine=engine)
    return b, h


def layer_fns(chain, x):
    """One callable per conv step of a chain, on the chain's own cached buffers (after a full call has filled them)."""
    chain(x)
    first = next(l for l in chain.layers if l is not None)
    h = x.contiguous().float() if first.cin == 3 else x.contiguous().to(chain.tdt)
    steps, acts, ws, need = chain._buffers(tuple(h.shape))
    st = ctypes.c_void_p(torch.cuda.current_stream(DEV).cuda_stream)
    B, fns = int(h.shape[0]), []
    for (kind, r, c, cin, cout, k), l, y in zip(steps, chain.layers, acts):
        if kind == 'conv':
            odt = L.VV_F32 if y.dtype == torch.float32 else L.VV_BF16
            args = (L.ptr(h), L.ptr(l.packed), L.ptr(l.scale), L.ptr(l.shift), L.ptr(y), B, r, c, cin, cout, k, l.act, float(l.alpha), chain.dt, odt,
                    L.ptr(ws) if need else None, need, st)
            fns.append((lambda a=args: L.call('vv_conv2d_fwd', *a), (r, c, cin, cout, k), L.load().vv_conv2d_splits(B, r, c, k, cin, cout)))
        h = y
    return fns


def torch_layer_fns(module, x_nchw):
    fns, h = [], x_nchw
    with torch.no_grad():
        for m in list(module.layers) + ([module.last] if hasattr(module, 'last') else []):
            if not isinstance(m, torch.nn.MaxPool2d):
                fns.append(lambda m=m, h=h: m(h))
            h = m(h)
    return fns


def run_workload(name, B, side, head, alternations, n_small, n_big):
    res = {'workload': name, 'batch': B, 'image': [side, side], 'head': {'filter_num_list': head[0], 'filter_size_list': head[1], 'output_dim': head[2]}}
    macs = W.image_encoder_macs(side, side, head=head)
    x = torch.from_numpy(np.random.default_rng(0).uniform(0, 1, (B, side, side, 3)).astype(np.float32)).to(DEV)
    tb, th = build('torch', head)
    models = {}
    for dt in ('f32', 'bf16'):
        voxvae.set_default_dtype(dt)
        models[dt] = build('hip', head)
        for i in (0, 1):
            models[dt][i].load_state_dict((tb, th)[i].state_dict())
    voxvae.set_default_dtype('f32')
    # bf16 channels_last twin of the torch modules (honesty row)
    import copy
    cl = [copy.deepcopy(m).to(torch.bfloat16).to(memory_format=torch.channels_last).eval() for m in (tb, th)]
    xcl = x.permute(0, 3, 1, 2).to(torch.bfloat16).contiguous(memory_format=torch.channels_last)

    def torch_cl():
        with torch.no_grad():
            return cl[1].last(cl[1].layers(cl[0].layers(xcl)))

    whole = {'torch_f32': lambda: th(tb(x)), 'torch_bf16_channels_last': torch_cl,
             'hip_f32': lambda: models['f32'][1](models['f32'][0](x)), 'hip_bf16': lambda: models['bf16'][1](models['bf16'][0](x))}
    n = n_big
    med, spread = alternate(whole, n, alternations)
    valid = B * sum(v for _, v, _ in macs)
    res['whole_encoder'] = {k: {'us': med[k], 'spread_us': spread[k], 'valid_tmacs': round(valid / med[k] / 1e6, 2)} for k in med}
    for dt in ('f32', 'bf16'):
        res['whole_encoder']['hip_' + dt]['fraction_of_mfma_peak'] = round(valid / med['hip_' + dt] / 1e6 / PEAK_TMACS[dt], 4)
        res['whole_encoder']['hip_' + dt]['torch_f32_over_hip'] = round(med['torch_f32'] / med['hip_' + dt], 3)
    # per layer
    feats = tb(x)
    tf = torch_layer_fns(tb, x.permute(0, 3, 1, 2).contiguous()) + torch_layer_fns(th, feats.permute(0, 3, 1, 2).contiguous())
    hf = {dt: layer_fns(models[dt][0]._chain, x) + layer_fns(models[dt][1]._chain, models[dt][0](x)) for dt in ('f32', 'bf16')}
    assert len(tf) == len(macs) == len(hf['f32'])
    res['layers'] = []
    for i, (lname, v, d) in enumerate(macs):
        r, c, cin, cout, k = hf['f32'][i][1]
        nl = n_small if B * v < 2e9 else n_big
        med, spread = alternate({'torch_f32': tf[i], 'hip_f32': hf['f32'][i][0], 'hip_bf16': hf['bf16'][i][0]}, nl, alternations)
        row = {'layer': lname, 'grid': [r, c], 'cin': cin, 'cout': cout, 'k': k, 'rows_M': B * r * c, 'splits': hf['f32'][i][2], 'valid_macs': B * v,
               'dense_macs': B * d, 'us': med, 'spread_us': spread}
        for dt in ('f32', 'bf16'):
            rate = B * v / med['hip_' + dt] / 1e6
            row['hip_%s_valid_tmacs' % dt] = round(rate, 2)
            row['hip_%s_fraction_of_mfma_peak' % dt] = round(rate / PEAK_TMACS[dt], 4)
            row['torch_f32_over_hip_%s' % dt] = round(med['torch_f32'] / med['hip_' + dt], 3)
        print(json.dumps(row), flush=True)
        res['layers'].append(row)
    return res


if __name__ == '__main__':
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument('--out', default=os.path.join(_R, 'profiles', 'conv2d_ab.json'))
    ap.add_argument('--alternations', type=int, default=5)
    ap.add_argument('--only', default=None, choices=['frame', 'batch'])
    args = ap.parse_args()
    lib = L.load()
    voxvae.set_default_device(DEV)
    res = {'library': os.path.relpath(lib._name, _R), 'device': torch.cuda.get_device_name(0), 'counters': 'not measured',
           'peak_tmacs': PEAK_TMACS, 'torch_per_layer': 'Conv2d + BatchNorm2d + activation, eager, float32 NCHW (the parent path)', 'workloads': []}
    if args.only in (None, 'frame'):
        res['workloads'].append(run_workload('one 416x416 frame, nolbo_test head', 1, 416, W.NOLBO_HEAD, args.alternations, 20, 5))
    if args.only in (None, 'batch'):
        res['workloads'].append(run_workload('72 x 256x256, nolboSingleObject_VAE head (config 3)', 72, 256, ([], [], 32), args.alternations, 5, 2))
    for w in res['workloads']:
        print(json.dumps(w['whole_encoder']), flush=True)
    with open(args.out, 'w') as f:
        json.dump(res, f, indent=1)
        f.write('\n')
