"""AE3D.fit, ms per step: the committed form (leg A: l2 folded into the optimiser launch, step scalars in one launch) beside the form the
code before it could compose (leg B: the same Trainer with weight_l2 = 0, the per-tensor `add_` of Trainer._add_l2 with the bucket overlap
off, sum w^2 as the torch ops of Model.losses, the scalars as torch ops on the step's stats).  Leg B exists in this script only.

Shapes: the reference's own size (64^3, latent 16, 110 per replica, train_modelnet_AE.py:112) and 32^3 batch 64, bf16.  The legs alternate
in one process after WARM warm-up steps each; every step sits between two device events; median and the 10 % / 90 % points over REPS
steps per leg, and leg A's own spread between the two halves of its samples.  Launches per step: kernel records of torch.profiler over one
step where the profiler is available, and the count of library calls (voxvae.lib.call) always.

    python profiles/microbench/mb_ae3d.py [out.json]
"""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [os.path.join(ROOT, 'anytime-3d-reconstruction_amd')]
import voxvae  # noqa: E402
from voxvae import lib as L  # noqa: E402
from voxvae import synthetic as syn  # noqa: E402
from voxvae import train as T  # noqa: E402

WARM, REPS = 5, 30
SHAPES = [(64, 16, 110), (32, 16, 64)]
LR = 1e-4


class ComposedTrainer(T.Trainer):
    """Leg B: the l2 gradient added per tensor before the optimiser (Trainer._add_l2's loop, which needs the overlap off)."""
    l2 = 0.0

    def _apply(self):
        self._add_l2(self.l2 * self.world)          # _add_l2 divides by world (the decoder-only steps' rule); AE3D's term is unscaled
        super()._apply()


def leg_b_step(model, tr, x):
    xs = model._rescaled(x)
    _, stats, _ = tr.step(xs, x)
    reg = torch.stack(model._encoder.losses + model._decoder.losses).sum()       # Model.losses: L2_REG * (w ** 2).sum() per variable
    s = stats.sum(dim=0) * (1.0 / (x.shape[0] * tr.world))
    return torch.stack([reg, s[0], reg + s[0], s[1], s[2], s[3]])


def kernel_count(fn):
    try:
        from torch.profiler import ProfilerActivity, profile
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        return sum(1 for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA and 'emcpy' not in e.name and 'emset' not in e.name)
    except Exception as e:              # noqa: BLE001 -- the count is a figure, not a result
        return 'unavailable: %s' % type(e).__name__


def call_count(fn):
    n, real = [0], L.call

    def counting(name, *a):
        n[0] += 1
        return real(name, *a)

    L.call = counting
    try:
        fn()
    finally:
        L.call = real
    return n[0]


def bench(D, Lz, B):
    import src.module.AE3D as AE3D
    cfg = syn.make_config(D, Lz, False)
    x = torch.from_numpy(syn.make_voxels(B, D, seed=5)).to('cuda')
    a = AE3D.AE3D(cfg['encoder'], cfg['decoder'], BATCH_SIZE_PER_REPLICA=B, learning_rate=LR)
    b = AE3D.AE3D(cfg['encoder'], cfg['decoder'], BATCH_SIZE_PER_REPLICA=B, learning_rate=LR)
    trb = ComposedTrainer(b._enc_eng, b._dec_eng, variational=False, learning_rate=LR)
    trb.l2, trb.overlap = a._trainer.weight_l2, False
    legs = {'A': lambda: a._fit_scalars((x, x)), 'B': lambda: leg_b_step(b, trb, x)}
    for _ in range(WARM):
        for f in legs.values():
            f()
    torch.cuda.synchronize()
    ev = {k: [] for k in legs}
    for _ in range(REPS):
        for k, f in legs.items():          # A, B, A, B, ...
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            f()
            e1.record()
            ev[k].append((e0, e1))
    torch.cuda.synchronize()
    out = {'shape': dict(D=D, latent=Lz, batch=B, dtype='bf16'), 'reps': REPS, 'warmup': WARM}
    for k in legs:
        ms = np.array([p.elapsed_time(q) for p, q in ev[k]])
        out[k] = dict(median_ms=float(np.median(ms)), p10_ms=float(np.sort(ms)[REPS // 10]), p90_ms=float(np.sort(ms)[REPS * 9 // 10]),
                      first_half_median_ms=float(np.median(ms[:REPS // 2])), second_half_median_ms=float(np.median(ms[REPS // 2:])),
                      kernels_per_step=kernel_count(legs[k]), library_calls_per_step=call_count(legs[k]))
    va, vb = legs['A'](), legs['B']()
    torch.cuda.synchronize()
    out['A']['scalars'], out['B']['scalars'] = [float(v) for v in va], [float(v) for v in vb]
    out['A_minus_B_ms'] = out['A']['median_ms'] - out['B']['median_ms']
    out['A_spread_ms'] = abs(out['A']['first_half_median_ms'] - out['A']['second_half_median_ms'])
    return out


def main():
    voxvae.set_default_device('cuda:0')
    voxvae.set_default_dtype('bf16')
    res = {'device': torch.cuda.get_device_name(0), 'legs': {'A': 'AE3D.fit as committed', 'B': 'weight_l2 = 0 + per-tensor add_ (overlap off) + torch sum w^2 and scalars'},
           'cases': [bench(*s) for s in SHAPES]}
    text = json.dumps(res, indent=1)
    print(text)
    if len(sys.argv) > 1:
        with open(sys.argv[1], 'w') as f:
            f.write(text + '\n')


if __name__ == '__main__':
    main()
