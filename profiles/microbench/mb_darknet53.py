"""Darknet53 and Darknet53Tiny on csrc/conv2d.hip beside the stock PyTorch path, in the method of mb_conv2d.py (HIP events around n calls,
medians over alternating runs): the whole backbone per engine and dtype -- torch float32 (the default path, the baseline), hip f32, hip
bf16 -- on one 416x416 frame and on 72 frames of 256x256; for the frame a per-layer table of Darknet53, and for its 23 residual blocks
the fused epilogue (vv_conv2d_ex_fwd with `residual`) beside "the same entry without it + a separate add launch".
No gate is attached to these numbers: they are a record, not a promise.

    python profiles/microbench/mb_darknet53.py [--out PATH] [--alternations 5]
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
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import voxvae
from voxvae import conv2d as C
from voxvae import lib as L
from mb_conv2d import DEV, PEAK_TMACS, alternate


def build(builder, engine, activation='lrelu'):
    import src.net_core.darknet as darknet
    torch.manual_seed(0)
    return getattr(darknet, builder)(name='b', activation=activation, device=DEV, engine=engine)


def conv_steps(chain, x):
    """(step index, args of vv_conv2d_ex_fwd without / with the residual, geometry) per conv step, on the chain's cached buffers."""
    chain(x)
    h = x.contiguous().float()
    steps, acts, ws, need = chain._buffers(tuple(h.shape))
    st = ctypes.c_void_p(torch.cuda.current_stream(DEV).cuda_stream)
    B, out = int(h.shape[0]), []
    for i, ((kind, r, c, cin, cout, k), l, y) in enumerate(zip(steps, chain.layers, acts)):
        if kind == 'conv':
            odt = L.VV_F32 if y.dtype == torch.float32 else L.VV_BF16
            res = None if l.res is None else acts[l.res]

            def args(residual, h=h, l=l, y=y, r=r, c=c, cin=cin, cout=cout, k=k, odt=odt):
                return (L.ptr(h), L.ptr(l.packed), L.ptr(l.scale), L.ptr(l.shift), L.ptr(residual), L.ptr(y), B, r, c, cin, cout, k, l.stride, l.act,
                        float(l.alpha), chain.dt, odt, L.ptr(ws) if need else None, need, st)
            ro, co = C.out_grid('conv', r, c, l.stride)
            out.append(dict(step=i, plain=args(None), fused=args(res) if res is not None else None, res=res, y=y, grid=[r, c], out_grid=[ro, co], cin=cin,
                            cout=cout, k=k, stride=l.stride, rows_M=B * ro * co, macs=B * ro * co * k * k * cin * cout,
                            splits=L.load().vv_conv2d_ex_splits(B, r, c, k, l.stride, cin, cout)))
        h = y
    return out


def torch_conv_fns(module, x_nchw):
    """One callable per conv step of the torch module: Conv2d + BatchNorm2d + activation (+ the residual add), eager float32 NCHW."""
    fns, held, h = [], {}, x_nchw
    keep = set(module._res.values())
    with torch.no_grad():
        for i, m in enumerate(module.layers):
            src = held.get(module._res.get(i))
            if hasattr(m, 'conv'):
                fns.append((lambda m=m, h=h, src=src: m(h) if src is None else src + m(h)))
            h = m(h) if src is None else src + m(h)
            if i in keep:
                held[i] = h
    return fns


def run_workload(name, builder, B, side, alternations, n, per_layer, n_layer=20):
    res = {'workload': name, 'backbone': builder, 'batch': B, 'image': [side, side]}
    x = torch.from_numpy(np.random.default_rng(0).uniform(0, 1, (B, side, side, 3)).astype(np.float32)).to(DEV)
    tor, models = build(builder, 'torch'), {}
    for dt in ('f32', 'bf16'):
        voxvae.set_default_dtype(dt)
        models[dt] = build(builder, 'hip')
        models[dt].load_state_dict(tor.state_dict())
    voxvae.set_default_dtype('f32')
    steps = {dt: conv_steps(models[dt]._chain, x) for dt in ('f32', 'bf16')}
    macs = sum(s['macs'] for s in steps['f32'])
    med, spread = alternate({'torch_f32': lambda: tor(x), 'hip_f32': lambda: models['f32'](x), 'hip_bf16': lambda: models['bf16'](x)}, n, alternations)
    res['dense_macs'] = macs
    res['launches'] = {'conv': len(steps['f32']), 'pool': len(models['f32']._chain.plan) - len(steps['f32'])}
    res['whole_backbone'] = {k: {'us': med[k], 'spread_us': spread[k], 'dense_tmacs': round(macs / med[k] / 1e6, 2)} for k in med}
    for dt in ('f32', 'bf16'):
        w = res['whole_backbone']['hip_' + dt]
        w['fraction_of_mfma_peak'] = round(macs / med['hip_' + dt] / 1e6 / PEAK_TMACS[dt], 4)
        w['torch_f32_over_hip'] = round(med['torch_f32'] / med['hip_' + dt], 3)
    print(json.dumps({k: res[k] for k in ('workload', 'backbone', 'whole_backbone')}), flush=True)
    if not per_layer:
        return res
    tf = torch_conv_fns(tor, x.permute(0, 3, 1, 2).contiguous())
    assert len(tf) == len(steps['f32'])
    res['layers'], fused_sum, apart_sum = [], {'f32': 0.0, 'bf16': 0.0}, {'f32': 0.0, 'bf16': 0.0}
    for i, s in enumerate(steps['f32']):
        fns = {'torch_f32': tf[i]}
        for dt in ('f32', 'bf16'):
            sd = steps[dt][i]
            fns['hip_' + dt] = (lambda a=(sd['fused'] or sd['plain']): L.call('vv_conv2d_ex_fwd', *a))
            if sd['fused'] is not None:
                tmp = torch.empty_like(sd['y'])
                fns['hip_%s_conv_then_add' % dt] = (lambda a=sd['plain'], y=sd['y'], r=sd['res'], t=tmp: (L.call('vv_conv2d_ex_fwd', *a), torch.add(y, r, out=t)))
        med, spread = alternate(fns, n_layer, alternations)
        row = {'layer': 'C%d' % (i + 1), 'step': s['step'], 'grid': s['grid'], 'out_grid': s['out_grid'], 'cin': s['cin'], 'cout': s['cout'], 'k': s['k'],
               'stride': s['stride'], 'residual': s['fused'] is not None, 'rows_M': s['rows_M'], 'splits': s['splits'], 'dense_macs': s['macs'], 'us': med,
               'spread_us': spread}
        for dt in ('f32', 'bf16'):
            row['hip_%s_dense_tmacs' % dt] = round(s['macs'] / med['hip_' + dt] / 1e6, 2)
            row['torch_f32_over_hip_%s' % dt] = round(med['torch_f32'] / med['hip_' + dt], 3)
            if s['fused'] is not None:
                fused_sum[dt] += med['hip_' + dt]
                apart_sum[dt] += med['hip_%s_conv_then_add' % dt]
        print(json.dumps(row), flush=True)
        res['layers'].append(row)
    res['residual_blocks'] = {dt: {'blocks': sum(1 for s in steps[dt] if s['fused'] is not None), 'fused_epilogue_us': round(fused_sum[dt], 2),
                                   'conv_then_separate_add_us': round(apart_sum[dt], 2)} for dt in ('f32', 'bf16')}
    print(json.dumps(res['residual_blocks']), flush=True)
    return res


if __name__ == '__main__':
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument('--out', default=os.path.join(_R, 'profiles', 'darknet53_ab.json'))
    ap.add_argument('--alternations', type=int, default=5)
    args = ap.parse_args()
    lib = L.load()
    voxvae.set_default_device(DEV)
    res = {'library': os.path.relpath(lib._name, _R), 'device': torch.cuda.get_device_name(0), 'counters': 'not measured', 'peak_tmacs': PEAK_TMACS,
           'torch': 'the modules of src/net_core/darknet.py, eager, float32 NCHW (the default engine)', 'workloads': []}
    res['workloads'].append(run_workload('one 416x416 frame', 'Darknet53', 1, 416, args.alternations, 5, True))
    res['workloads'].append(run_workload('one 416x416 frame', 'Darknet53Tiny', 1, 416, args.alternations, 10, False))
    res['workloads'].append(run_workload('72 x 256x256', 'Darknet53', 72, 256, args.alternations, 2, False))
    res['workloads'].append(run_workload('72 x 256x256', 'Darknet53Tiny', 72, 256, args.alternations, 2, False))
    with open(args.out, 'w') as f:
        json.dump(res, f, indent=1)
        f.write('\n')
