"""The multi-modal latent stage at the reference's shape (B = 72, Lc = Li = 8, C = 12, I = 10): device time per call of
vv_mm_latent_eval beside the same stage as torch ops, and of vv_mm_latent_train_fwd + _bwd beside the torch autograd closure
(tests/_mm_ref.py: total_torch).  HIP events around each call, WARM warm-up calls, REPS timed calls, median and the 10 % / 90 % points.

    python profiles/microbench/mb_mm_latent.py [out.json]
"""
import ctypes
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [os.path.join(ROOT, 'anytime-3d-reconstruction_amd'), os.path.join(ROOT, 'tests')]
import _mm_ref as R  # noqa: E402
from voxvae import lib as L  # noqa: E402

WARM, REPS = 50, 500
B, Lc, Li, C, I = 72, 8, 8, 12, 10


def timed(fn):
    for _ in range(WARM):
        fn()
    torch.cuda.synchronize()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(REPS)]
    for a, b in ev:
        a.record()
        fn()
        b.record()
    torch.cuda.synchronize()
    us = np.sort([a.elapsed_time(b) * 1e3 for a, b in ev])
    return dict(median_us=float(np.median(us)), p10_us=float(us[REPS // 10]), p90_us=float(us[REPS * 9 // 10]), reps=REPS, warmup=WARM)


def torch_eval(enc, eps, mask, eps2, pc, pi, coh, ioh):
    mc, lc, mi, li = enc[:, :Lc], enc[:, Lc:2 * Lc].clamp(-10, 10), enc[:, 2 * Lc:2 * Lc + Li], enc[:, 2 * Lc + Li:].clamp(-10, 10)
    zc, zi = mc + torch.sqrt(torch.exp(lc)) * eps[:, :Lc], mi + torch.sqrt(torch.exp(li)) * eps[:, Lc:]
    zc = zc * mask
    zc = torch.where(zc == 0, pc.mean(0) * torch.ones_like(zc), zc)
    sq = (zc[:, None, :] - pc[None]) ** 2
    a0 = (sq.sum(-1).argmin(-1) == coh.argmax(-1)).float().mean()
    a1 = (((zi[:, None, :] - pi) ** 2).sum(-1).argmin(-1) == ioh.argmax(-1)).float().mean()
    idx = (mask[:, None, :] * sq).sum(-1).argmin(-1)
    zcc = torch.where(mask == 0, pc[idx] + eps2, zc)
    a2 = (((zcc[:, None, :] - pc[None]) ** 2).sum(-1).argmin(-1) == coh.argmax(-1)).float().mean()
    return torch.cat([zc, zi], 1), torch.cat([zcc, zi], 1), a0, a1, a2


def main():
    dev = 'cuda'
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    t = lambda x: None if x is None else torch.from_numpy(x).to(dev)
    p = lambda x: None if x is None else ctypes.c_void_p(x.data_ptr())
    c = R.random_eval_case(1, B, Lc, Li, C, I, 0.3)
    ev = [t(c[k]) for k in ('enc', 'eps', 'mask', 'eps2', 'prior_cat', 'prior_inst', 'cat_oh', 'inst_oh')]
    z, zc = torch.empty(B, Lc + Li, device=dev), torch.empty(B, Lc + Li, device=dev)
    idx, acc = torch.empty(B, 4, dtype=torch.int32, device=dev), torch.empty(3, device=dev)
    lib = L.load()
    out = {'shape': dict(B=B, Lc=Lc, Li=Li, C=C, I=I), 'device': torch.cuda.get_device_name(0)}
    out['eval_hip'] = timed(lambda: lib.vv_mm_latent_eval(*[p(x) for x in ev], p(z), p(zc), None, None, 0, p(idx), p(acc), B, Lc, Li, C, I, st))
    out['eval_torch_ops'] = timed(lambda: torch_eval(*ev))
    k = R.random_train_case(2, B, Lc, Li, C)
    names = ('enc', 'eps', 'mean_cp', 'lv_cp', 'mean_ip', 'lv_ip', 'eps_p', 'noise', 'cat_oh')
    tr, dz = [t(k[n]) for n in names], t(k['dz_in'])
    zin, kl, reg = torch.empty(B, Lc + Li, device=dev), torch.empty(B, device=dev), torch.empty(B, device=dev)
    outs = [torch.empty(B, n, device=dev) for n in (2 * Lc + 2 * Li, Lc, Lc, Li, Li)]

    def hip_train():
        lib.vv_mm_latent_train_fwd(*[p(x) for x in tr], p(zin), None, 0, p(kl), p(reg), B, Lc, Li, C, st)
        lib.vv_mm_latent_train_bwd(*[p(x) for x in tr], p(dz), 1.0 / B, *[p(x) for x in outs], B, Lc, Li, C, st)

    leaves = [tr[i].clone().requires_grad_(True) if i in (0, 2, 3, 4, 5) else tr[i] for i in range(9)]

    def torch_train():
        for x in leaves:
            if x is not None and x.requires_grad:
                x.grad = None
        R.total_torch(*leaves, dz).backward()

    out['train_hip_fwd_bwd'] = timed(hip_train)
    out['train_torch_closure'] = timed(torch_train)
    text = json.dumps(out, indent=1)
    print(text)
    if len(sys.argv) > 1:
        with open(sys.argv[1], 'w') as f:
            f.write(text + '\n')


if __name__ == '__main__':
    main()
