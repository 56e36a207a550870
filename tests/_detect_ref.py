"""Our numpy statement of the detection decode, for shapes tests/golden/detect_frames.npz does not cover.  It is held to that
fixture exactly as the host entry is (tests/test_detect_host.py).

Decisions and box arithmetic are float32 in the reference's operation order.  The activations are float64 numpy rounded to float32
(`act='numpy'`), or the entry's own through vv_detect_activation_host (`act='entry'`): with the latter every decision falls exactly as
the entry's, which is what the tests on ties and on-the-dot thresholds compare against.
"""
import os

import numpy as np

# The largest difference between the host entry's float fields and the REFERENCE's recorded outputs over the fixture frames, measured by
# tests/test_detect_host.py::test_host_entry_against_the_fixture (it prints the figure): 1.19e-7 absolute on fields of magnitude <= 1
# (one float32 unit at 1).  The gate is that figure times 4.
FIXTURE_MAX_DIFF = 1.1920929e-07
FIXTURE_TOL = 4 * FIXTURE_MAX_DIFF
# The activations' largest error in float32 units against float64 numpy over 2^20 random bit patterns per function plus the ends and
# clamp points, measured by tests/test_detect_host.py::test_activations_against_float64 (it prints the figures).  The gate is twice these.
ACT_MAX_ULP = {'exp': 0.987, 'sigmoid': 2.223, 'tanh': 1.254}

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'detect_frames.npz')
f32 = np.float32


def width(Z):
    return 17 + 2 * Z


def _act(x, which, act):
    x = np.asarray(x, dtype=np.float32)
    if act == 'entry':
        from voxvae.detect import activation_host
        return activation_host(x, which).reshape(x.shape)
    with np.errstate(all='ignore'):
        x64 = x.astype(np.float64)
        y = {'exp': np.exp, 'tanh': np.tanh, 'sigmoid': lambda v: 1.0 / (1.0 + np.exp(-v))}[which](x64)
        return y.astype(np.float32)


def _max(a, b):         # numpy's maximum: NaN if either is
    return np.maximum(f32(a), f32(b))


def suppresses(a, b, thr):
    """Picked box a against box b, (col_min, row_min, col_max, row_max) float32."""
    with np.errstate(all='ignore'):
        area_a = f32(f32(a[3] - a[1]) * f32(a[2] - a[0]))
        area_b = f32(f32(b[3] - b[1]) * f32(b[2] - b[0]))
        w = _max(f32(0), f32(np.minimum(a[2], b[2]) - np.maximum(a[0], b[0])))
        h = _max(f32(0), f32(np.minimum(a[3], b[3]) - np.maximum(a[1], b[1])))
        inter = f32(w * h)
        iou = f32(inter / f32(f32(area_a + area_b) - inter))
    return bool(iou > f32(thr))


def decode_frame(frame, P, Z, obj_thresh=0.5, iou_thresh=0.5, top_1=True, act='numpy'):
    """frame float32 [R,C,P*W] -> dict(count, index, bbox2d, bbox3d, inst_mean, inst_log_var, sin, cos, rad_log_var) in pick order."""
    R, C, _ = frame.shape
    W = width(Z)
    v = np.asarray(frame, dtype=np.float32).reshape(R * C, P, W)
    obj = _act(v[..., 0], 'sigmoid', act)
    hw, xy = _act(v[..., 1:3], 'exp', act), _act(v[..., 3:5], 'sigmoid', act)
    othr = f32(obj_thresh)
    score, cand, box = [], [], []
    with np.errstate(all='ignore'):
        for cell in range(R * C):
            gr, gc = divmod(cell, C)
            # descending objectness, ties to the lower predictor, NaN last
            order = sorted(range(P), key=lambda p: (not obj[cell, p] == obj[cell, p], -obj[cell, p] if obj[cell, p] == obj[cell, p] else 0.0, p))
            for p in order:
                if obj[cell, p] > othr:
                    h, w = hw[cell, p]
                    x, y = xy[cell, p]
                    qr = f32(f32(f32(gr) + y) / f32(R))
                    qc = f32(f32(f32(gc) + x) / f32(C))
                    hh, hwid = f32(h / f32(2)), f32(w / f32(2))
                    box.append([f32(qc - hwid), f32(qr - hh), f32(qc + hwid), f32(qr + hh)])
                    score.append(obj[cell, p]), cand.append(cell * P + p)
                if top_1:
                    break
    n = len(score)
    # descending objectness, ties to the HIGHER candidate index
    ranked = sorted(range(n), key=lambda j: (-score[j], -j))
    live, picks = [True] * n, []
    for i, a in enumerate(ranked):
        if not live[i]:
            continue
        picks.append(a)
        for k in range(i + 1, n):
            if live[k] and suppresses(box[a], box[ranked[k]], iou_thresh):
                live[k] = False
    M = len(picks)
    out = dict(count=M, index=np.asarray([cand[a] for a in picks], dtype=np.int32).reshape(M))
    out['bbox2d'] = np.asarray([box[a] + [score[a]] for a in picks], dtype=np.float32).reshape(M, 5)
    rows = v[[cand[a] // P for a in picks], [cand[a] % P for a in picks]].reshape(M, W)
    with np.errstate(all='ignore'):
        out['bbox3d'] = np.maximum(rows[:, [6, 5, 7]], f32(0))
    out['inst_mean'], out['inst_log_var'] = rows[:, 8:8 + Z], rows[:, 8 + Z:8 + 2 * Z]
    out['sin'], out['cos'] = _act(rows[:, 8 + 2 * Z:11 + 2 * Z], 'tanh', act), _act(rows[:, 11 + 2 * Z:14 + 2 * Z], 'tanh', act)
    out['rad_log_var'] = rows[:, 14 + 2 * Z:17 + 2 * Z]
    return out


def decode(head, P, Z, obj_thresh=0.5, iou_thresh=0.5, top_1=True, act='numpy'):
    """head [B,R,C,P*W] -> a list of decode_frame results."""
    return [decode_frame(f, P, Z, obj_thresh, iou_thresh, top_1, act) for f in np.asarray(head, dtype=np.float32)]


def golden_frames():
    """-> a list of dicts: head, obj_thresh, iou_thresh, top_1 and the reference's outputs (index, bbox2D, bbox3D, sin, cos, rad)."""
    with np.load(GOLDEN) as z:
        out = []
        for i in range(int(z['frames'])):
            a = z['f%d_args' % i]
            d = dict(head=z['f%d_head' % i], obj_thresh=float(a[0]), iou_thresh=float(a[1]), top_1=bool(a[2]))
            for k in ('index', 'bbox2D', 'bbox3D', 'sin', 'cos', 'rad'):
                d[k] = z['f%d_out_%s' % (i, k)]
            for k in ('objness', 'bbox2D', 'bbox3D', 'sin', 'cos'):
                d['held_' + k] = z['f%d_%s' % (i, k)]
            out.append(d)
        return out


FIELDS = ('index', 'bbox2d', 'bbox3d', 'inst_mean', 'inst_log_var', 'sin', 'cos', 'rad_log_var')


def detections_as_dicts(det):
    """voxvae.detect.Detections -> a list of dicts like decode()'s, rows below count only."""
    counts = det.counts()
    whole = {k: getattr(det, k).cpu().numpy() for k in FIELDS}              # one copy per output
    return [dict(count=M, **{k: whole[k][b, :M] for k in FIELDS}) for b, M in enumerate(counts)]


def seeded_head(seed, B, R, C, P, Z, lit=0.15):
    """A head output with about `lit` of the predictors above an objectness of 0.5 and boxes a few cells wide: NMS has work to do."""
    rng = np.random.default_rng(seed)
    W = width(Z)
    f = rng.normal(0.0, 1.0, size=(B, R, C, P, W)).astype(np.float32)
    f[..., 0] = np.where(rng.random((B, R, C, P)) < lit, rng.uniform(0.2, 4.0, (B, R, C, P)), rng.normal(-4.0, 0.7, (B, R, C, P)))
    f[..., 1] = np.log(rng.uniform(1.0, 3.0, (B, R, C, P)) / R)
    f[..., 2] = np.log(rng.uniform(1.0, 3.0, (B, R, C, P)) / C)
    return np.ascontiguousarray(f.reshape(B, R, C, P * W))
