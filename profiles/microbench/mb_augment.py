"""Building one Pascal3D image batch, ms: the device pair of launches (leg A: vv_augment_draw + vv_augment_images out of photos that are
already in device memory) beside the host twin plus the upload (leg B: vv_augment_draw_host + vv_augment_images_host on one core, then
the float32 batch copied to the device), and leg A as a share of one train_pascal.py step with the host loader (the step as the parent
commit runs it: two getNextBatch, fit, two getEval).

Sizes: batch 72, 256 x 256 output, 72 seeded photos around 500 x 400 with a box over 50 .. 90 % of each extent, augmentation on.  Leg A
sits between two device events, REPS_A times after WARM warm-ups; leg B and the step are a host clock around work that ends in a device
synchronise (REPS_B times, and REPS_STEP times after WARM_STEP warm-up steps: they take seconds).  A and B alternate (one B after
every REPS_A / REPS_B A's).  Both legs' outputs are compared bit for bit on the first batch.  Bytes: what leg A must read and write at least (the crops once, the output once)
over its median, against the HBM peak -- a bound on what the kernel could reach, not a kernel time (that is rocprofv3's, in a run of its
own).

    python profiles/microbench/mb_augment.py [out.json] [--no-step]
"""
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
PKG = os.path.join(ROOT, 'anytime-3d-reconstruction_amd')
sys.path[:0] = [PKG]
import voxvae  # noqa: E402
from voxvae import augment as A  # noqa: E402

B, OUT = 72, (256, 256)
WARM, REPS_A, REPS_B, WARM_STEP, REPS_STEP = 5, 60, 3, 4, 6
HBM_PEAK = 8.0e12            # bytes / s, MI355X


def photos(seed=7):
    rng = np.random.default_rng(seed)
    images, boxes = [], np.empty((B, 4), dtype=np.float32)
    for i in range(B):
        rows, cols = int(rng.integers(350, 451)), int(rng.integers(450, 551))
        images.append(rng.integers(0, 256, (rows, cols, 3), dtype=np.uint8))
        bh, bw = rng.uniform(0.5, 0.9) * rows, rng.uniform(0.5, 0.9) * cols
        r0, c0 = rng.uniform(0, rows - bh), rng.uniform(0, cols - bw)
        boxes[i] = (c0, r0, c0 + bw, r0 + bh)
    return images, boxes


def stats(ms):
    ms = np.sort(np.asarray(ms, dtype=np.float64))
    return dict(median_ms=float(np.median(ms)), min_ms=float(ms[0]), max_ms=float(ms[-1]), p10_ms=float(ms[len(ms) // 10]),
                p90_ms=float(ms[(len(ms) * 9) // 10]), n=int(len(ms)))


def train_step_ms():
    """One loop body of train_pascal.py at its defaults (batch 72, 256 x 256, 64^3), host loader."""
    import train_pascal as TP
    import src.dataset_loader.pascal3D as pascal3D
    import src.module.nolbo as nolbo
    import src.net_core.darknet as Darknet
    voxvae.set_default_dtype('f32')
    config = TP.make_config(16, 64)
    model = nolbo.nolboSingleObject(nolbo_structure=config, backbone_style=Darknet.Darknet19, learning_rate=1e-4)
    idx = TP.indices_of(config)
    instances = idx['inst_indices'].shape[0]
    loader = pascal3D.dataLoaderSingleObject('train', None, voxel=64, instances=instances)
    loader_test = pascal3D.dataLoaderSingleObject('val', None, voxel=64, instances=instances)

    def body():
        inputs = TP.inputs_of(loader.getNextBatch(batchSizeof3DShape=B, imageSize=OUT))
        inputs_test = TP.inputs_of(loader_test.getNextBatch(batchSizeof3DShape=B, imageSize=OUT, augmentation=False))
        r = (model.fit(inputs=inputs), model.getEval(inputs=inputs, **idx)[1:], model.getEval(inputs=inputs_test, **idx)[1:])
        torch.cuda.synchronize()
        return r

    for _ in range(WARM_STEP):            # the first steps load code objects and let the 2D convolutions pick their algorithms
        body()
    ms = []
    for _ in range(REPS_STEP):
        t0 = time.perf_counter()
        body()
        ms.append((time.perf_counter() - t0) * 1e3)
    return stats(ms)


def main():
    args = [a for a in sys.argv[1:] if not a.startswith('--')]
    voxvae.set_default_device('cuda:0')
    voxvae.manual_seed(1357)
    images, boxes = photos()
    arena = A.ImageArena.from_arrays(images, device='cuda:0')
    idx = np.arange(B, dtype=np.int32)
    idx_d, box_d = torch.from_numpy(idx).cuda(), torch.from_numpy(boxes).cuda()
    out = torch.empty(B, OUT[0], OUT[1], 3, dtype=torch.float32, device='cuda:0')

    def leg_a(step):
        return A.augment_images(arena, A.draw_params(arena, idx_d, box_d, True, step), OUT, out=out)

    def leg_b(step):
        p = A.draw_params(arena, idx, boxes, True, step, host=True)
        r = A.augment_images(arena, p, OUT, host=True).to('cuda:0')
        torch.cuda.synchronize()
        return r

    same = bool(torch.equal(leg_a(0), leg_b(0)))
    params = A.draw_params(arena, idx, boxes, True, 0, host=True).numpy()
    for s in range(WARM):
        leg_a(s)
    torch.cuda.synchronize()
    ev, b_ms, per = [], [], REPS_A // REPS_B
    for r in range(REPS_A):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        leg_a(10 + r)
        e1.record()
        ev.append((e0, e1))
        if r % per == per - 1:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            leg_b(10 + r)
            b_ms.append((time.perf_counter() - t0) * 1e3)
    torch.cuda.synchronize()
    a = stats([p.elapsed_time(q) for p, q in ev])
    b = stats(b_ms)
    crop_bytes = int((params[:, 3].astype(np.int64) * params[:, 4]).sum()) * 3
    least_bytes = crop_bytes + out.numel() * 4
    res = {'device': torch.cuda.get_device_name(0),
           'setting': dict(batch=B, out=list(OUT), photos='350..450 x 450..550 uint8', box='50..90 % of each extent', augmentation=True,
                           mean_crop=[float(params[:, 3].mean()), float(params[:, 4].mean())]),
           'legs': {'A': 'vv_augment_draw + vv_augment_images, device events', 'B': 'host twins on one core + upload of the float32 batch, host clock to a synchronise'},
           'outputs_bit_identical': same, 'A': a, 'B': b, 'B_over_A': b['median_ms'] / a['median_ms'],
           'A_least_bytes': least_bytes, 'A_least_bytes_over_median_TBps': least_bytes / (a['median_ms'] * 1e-3) / 1e12,
           'A_share_of_hbm_peak_by_least_bytes': least_bytes / (a['median_ms'] * 1e-3) / HBM_PEAK}
    if '--no-step' in sys.argv:
        res['train_pascal_step'] = 'not measured'
    else:
        res['train_pascal_step'] = train_step_ms()
        res['A_share_of_train_pascal_step'] = a['median_ms'] / res['train_pascal_step']['median_ms']
    text = json.dumps(res, indent=1)
    print(text)
    if args:
        with open(args[0], 'w') as f:
            f.write(text + '\n')


if __name__ == '__main__':
    main()
