"""Building one Pascal3D image batch through the device loader with colour_ops='invert_add' (leg A: vv_augment_draw +
vv_augment_images, what the loader always did) against colour_ops='all' (leg C: vv_augment_draw_ex + the colour pre-pass + the warp
reading flagged samples' slabs), ms, and the host twin beside both (legs HA, HC: the same rows through the _host entries on one core).

Sizes: batch 72 to 64 x 64 through pascal3D.deviceDataLoaderSingleObject.from_arrays, 72 seeded photos around 500 x 400 with a box over
50 .. 90 % of each extent, augmentation on; under colour_ops='all' about 3 samples in 8 carry a flag (the gate at 0.5, then blur or
hue/saturation at 0.5 each), sigma uniform in [0, 3).  The two device legs alternate call by call, each getNextBatch between two device
events, REPS times after WARM warm-ups (the loader also gathers the CAD grids in both legs: the difference of the medians is the colour
path's).  The host legs are a host clock around the two _host calls on the rows of one step, REPS_H times.  The images of the first
'all' batch are compared with the host twin bit for bit.  The flagged share and the blurred pixels of the timed steps are recorded,
because leg C's time depends on them.

    python profiles/microbench/mb_augment_colour.py [out.json]
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

B, OUT = 72, (64, 64)
WARM, REPS, REPS_H = 5, 60, 3


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


def main():
    import src.dataset_loader.pascal3D as P
    args = [a for a in sys.argv[1:] if not a.startswith('--')]
    voxvae.set_default_device('cuda:0')
    voxvae.manual_seed(1357)
    images, boxes = photos()
    grids = (np.random.default_rng(3).random((4, 8, 8, 8)) > 0.7).astype(np.float32)

    def loader(colour_ops):
        return P.deviceDataLoaderSingleObject.from_arrays(images=images, boxes=boxes, classes=np.arange(B) % 12, cad_index=np.arange(B) % 4,
                                                          euler=np.zeros((B, 3)), cad_grids=grids, device='cuda:0', seed=1, shuffle=False,
                                                          colour_ops=colour_ops)

    legs = {'A': loader('invert_add'), 'C': loader('all')}
    size = (OUT[1], OUT[0])
    first = legs['C'].getNextBatch(B, size)[4]
    p0, c0 = legs['C'].last_params.cpu(), legs['C'].last_colour.cpu()
    same = bool(torch.equal(first.cpu(), A.augment_images(legs['C']._arena, p0, OUT, colour=c0, host=True)))
    legs['A'].getNextBatch(B, size)
    for _ in range(WARM):
        for ld in legs.values():
            ld.getNextBatch(B, size)
    torch.cuda.synchronize()
    ev, flagged, blurred_px, rows_kept = {'A': [], 'C': []}, [], [], None
    for r in range(REPS):
        for name, ld in legs.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            ld.getNextBatch(B, size)
            e1.record()
            ev[name].append((e0, e1))
        p, c = legs['C'].last_params.cpu().numpy(), legs['C'].last_colour.cpu().numpy()
        flagged.append(float((c[:, 0] != 0).mean()))
        blur = ((c[:, 0] & 1) != 0) & (c[:, 1:2].copy().view(np.float32)[:, 0] >= 0.125)
        blurred_px.append(int((p[blur, 3].astype(np.int64) * p[blur, 4]).sum()))
        rows_kept = (p, c)
    torch.cuda.synchronize()
    a, cst = stats([x.elapsed_time(y) for x, y in ev['A']]), stats([x.elapsed_time(y) for x, y in ev['C']])

    arena = legs['C']._arena
    p, c = rows_kept
    ha, hc = [], []
    for _ in range(REPS_H):
        t0 = time.perf_counter()
        A.augment_images(arena, p, OUT, host=True)
        ha.append((time.perf_counter() - t0) * 1e3)
        t0 = time.perf_counter()
        A.augment_images(arena, p, OUT, colour=c, host=True)
        hc.append((time.perf_counter() - t0) * 1e3)
    res = {'device': torch.cuda.get_device_name(0),
           'setting': dict(batch=B, out=list(OUT), photos='350..450 x 450..550 uint8', box='50..90 % of each extent', augmentation=True,
                           mean_crop=[float(p[:, 3].mean()), float(p[:, 4].mean())]),
           'legs': {'A': "getNextBatch, colour_ops='invert_add', device events", 'C': "getNextBatch, colour_ops='all', device events",
                    'HA': 'vv_augment_images_host on the last timed step\'s rows, one core, host clock',
                    'HC': 'vv_augment_images_ex_host on the same rows with their colour table, one core, host clock'},
           'first_all_batch_bit_identical_to_host_twin': same,
           'A': a, 'C': cst, 'C_over_A': cst['median_ms'] / a['median_ms'], 'C_minus_A_ms': cst['median_ms'] - a['median_ms'],
           'flagged_share_mean': float(np.mean(flagged)), 'blurred_pixels_per_step_mean': float(np.mean(blurred_px)),
           'HA': stats(ha), 'HC': stats(hc), 'HC_over_C': float(np.median(hc)) / cst['median_ms'], 'HA_over_A': float(np.median(ha)) / a['median_ms']}
    text = json.dumps(res, indent=1)
    print(text)
    if args:
        with open(args[0], 'w') as f:
            f.write(text + '\n')


if __name__ == '__main__':
    main()
