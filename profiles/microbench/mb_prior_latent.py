"""The one-group, one-prior latent stage where its users meet it: time per optimisation step with the latent algebra as torch autograd
code (latent='torch') against the two HIP launches (latent='hip'), for

    modelnet   nolboSingleObject_modelnet_category_only.fit at 32^3, B = 256, latent 64 (voxel encoder + decoder on the HIP trainer)
    image      nolboSingleObject_category_only.fit on supplied head outputs [256, 128], 32^3 decoder, latent 64

and the stage alone at [256, 64]: vv_prior_latent_train_fwd + _bwd against the torch closure (tests/_prior_ref.total_torch).

A step is timed by the host clock around fit() followed by a device synchronise; the two legs run on two models built alike and
ALTERNATE step by step inside one process (ROUNDS x STEPS timed steps per leg after WARM warm-up steps each), so that drift of the
host hits both; median and the 10 % / 90 % points per leg.  The stage alone is timed by device events.  What a step issues is counted
in one untimed step per leg: calls into the library, and aten operators dispatched by torch (each is at least one launch or a view).

    python profiles/microbench/mb_prior_latent.py [out.json]
"""
import ctypes
import json
import os
import sys
import time

import numpy as np
import torch
from torch.utils._python_dispatch import TorchDispatchMode

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [os.path.join(ROOT, 'anytime-3d-reconstruction_amd'), os.path.join(ROOT, 'tests')]
import _prior_ref as R  # noqa: E402
from voxvae import lib as L  # noqa: E402

WARM, ROUNDS, STEPS = 10, 5, 20
B, LZ, D = 256, 64, 32


class _Count(TorchDispatchMode):
    def __init__(self):
        super().__init__()
        self.n = 0

    def __torch_dispatch__(self, func, types, args=(), kwargs=None):
        self.n += 1
        return func(*args, **(kwargs or {}))


def issued(step):
    """(library calls, aten operators) of one step."""
    calls, real = [0], L.call

    def counting(name, *a):
        calls[0] += 1
        return real(name, *a)

    L.call = counting
    try:
        with _Count() as c:
            step()
        torch.cuda.synchronize()
    finally:
        L.call = real
    return calls[0], c.n


def quantiles(ms):
    ms = np.sort(np.asarray(ms))
    return dict(median_ms=float(np.median(ms)), p10_ms=float(ms[len(ms) // 10]), p90_ms=float(ms[len(ms) * 9 // 10]), steps=len(ms))


def alternate(steps):
    """{leg: [ms per step]} with the legs taking turns."""
    for _ in range(WARM):
        for s in steps.values():
            s()
    torch.cuda.synchronize()
    ms = {k: [] for k in steps}
    for _ in range(ROUNDS * STEPS):
        for k, s in steps.items():
            t0 = time.perf_counter()
            s()
            torch.cuda.synchronize()
            ms[k].append((time.perf_counter() - t0) * 1e3)
    return ms


def compare(steps):
    ms = alternate(steps)
    out = {k: quantiles(v) for k, v in ms.items()}
    for k, s in steps.items():
        out[k]['library_calls_per_step'], out[k]['aten_ops_per_step'] = issued(s)
    out['hip_over_torch_median'] = out['hip']['median_ms'] / out['torch']['median_ms']
    return out


def modelnet_steps():
    from voxvae import synthetic as syn
    import src.module.nolbo as nolbo
    import src.net_core.priornet as priornet
    cfg = syn.make_config(D, LZ, True)
    cfg['prior_class'] = dict(priornet.priornet_structure, unit_num_list=[64, 32, LZ])
    x = torch.from_numpy(syn.make_voxels(B, D, seed=1)).cuda()
    oh = syn.make_onehot(B, 40)
    steps = {}
    for latent in ('torch', 'hip'):
        torch.manual_seed(0)
        m = nolbo.nolboSingleObject_modelnet_category_only(nolbo_structure=cfg)
        m._encoder.set_weights_dict(syn.make_encoder_params(cfg['encoder'], seed=42))
        m._decoder.set_weights_dict(syn.make_decoder_params(cfg['decoder'], seed=43))
        steps[latent] = (lambda m=m, latent=latent: m.fit((x, x, oh), latent=latent))
    return steps


def image_steps():
    from voxvae import synthetic as syn
    import src.module.nolbo as nolbo
    cfg = {'encoder_backbone': {'name': 'bb', 'z_category_dim': LZ}, 'encoder_head': None, 'decoder': syn.make_config(D, LZ, True)['decoder'],
           'prior_class': {'name': 'priornet_class', 'input_dim': 12, 'unit_num_list': [32, LZ], 'core_activation': 'elu', 'const_log_var': 0.0}}
    rng = np.random.default_rng(3)
    head = torch.from_numpy(rng.normal(0, 1, (B, 2 * LZ)).astype(np.float32)).cuda()
    y = torch.from_numpy(syn.make_voxels(B, D, seed=2)).cuda()
    oh = np.eye(12, dtype=np.float32)[rng.integers(0, 12, B)]
    steps = {}
    for latent in ('torch', 'hip'):
        torch.manual_seed(0)
        m = nolbo.nolboSingleObject_category_only(nolbo_structure=cfg)
        m._decoder.set_weights_dict(syn.make_decoder_params(cfg['decoder'], seed=43))
        steps[latent] = (lambda m=m, latent=latent: m.fit((head, y, oh), latent=latent))
    return steps


def stage_alone():
    reps, warm = 500, 50
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    c = R.train_case(1, B, LZ)
    c['mean_p'] *= 0.25
    t = lambda x: None if x is None else torch.from_numpy(x).cuda()
    p = lambda x: None if x is None else ctypes.c_void_p(x.data_ptr())
    ins, dz = [t(c[k]) for k in R.TRAIN_KEYS[:-1]], t(c['dz_in'])
    new = lambda *s: torch.empty(s, device='cuda')
    zin, kl, reg, de, dm, dlv = new(B, LZ), new(B), new(B), new(B, 2 * LZ), new(B, LZ), new(B, LZ)
    lib = L.load()

    def hip():
        lib.vv_prior_latent_train_fwd(*[p(x) for x in ins], c['dist'], p(zin), None, p(kl), p(reg), B, LZ, st)
        lib.vv_prior_latent_train_bwd(*[p(x) for x in ins], c['dist'], p(dz), 1.0 / B, c['reg_weight'], p(de), p(dm), p(dlv), B, LZ, st)

    leaves = [ins[i].clone().requires_grad_(True) if i in (0, 2, 3) else ins[i] for i in range(6)]

    def closure():
        for x in leaves:
            if x is not None and x.requires_grad:
                x.grad = None
        R.total_torch(*leaves, dz, c['dist'], c['reg_weight']).backward()

    out = {}
    for name, fn in (('hip_fwd_bwd', hip), ('torch_closure', closure)):
        for _ in range(warm):
            fn()
        torch.cuda.synchronize()
        ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)]
        for a, b in ev:
            a.record()
            fn()
            b.record()
        torch.cuda.synchronize()
        us = np.sort([a.elapsed_time(b) * 1e3 for a, b in ev])
        out[name] = dict(median_us=float(np.median(us)), p10_us=float(us[reps // 10]), p90_us=float(us[reps * 9 // 10]), reps=reps, warmup=warm)
    return out


def main():
    import voxvae
    voxvae.set_default_dtype('f32')
    out = {'shape': dict(B=B, L=LZ, voxel=D), 'device': torch.cuda.get_device_name(0), 'warmup_steps': WARM, 'rounds': ROUNDS, 'steps_per_round': STEPS}
    out['stage_alone'] = stage_alone()
    out['modelnet_category_only_fit'] = compare(modelnet_steps())
    out['category_only_fit_on_head_outputs'] = compare(image_steps())
    text = json.dumps(out, indent=1)
    print(text)
    if len(sys.argv) > 1:
        with open(sys.argv[1], 'w') as f:
            f.write(text + '\n')


if __name__ == '__main__':
    main()
