"""Records tests/golden/detect_frames.npz: what the REFERENCE's own nolbo_test.getPred(get_3D_shape=False) selects on seeded head outputs.

    python tests/golden/make_detect_golden.py --reference /path/to/the/reference/checkout

No test imports this file.  The reference module is imported by path; `tensorflow` and `cv2` are replaced in sys.modules by stand-ins:
numpy float32 statements of the seven functions _encOutPartitioning uses (sigmoid, exp, tanh, nn.relu, transpose, stack, concat) and a
no-op `rectangle`.  The backbone and the head are callables that return the frame.  Everything else -- the per-cell loops, the box
arithmetic, nonMaximumSuppresion -- is the reference's code running under this interpreter's numpy (2.x: NEP 50 promotion).

The stand-ins' transcendentals are numpy's, not the kernel's, so the fixture pins decisions only on frames with margins; a frame is
redrawn when
    an objectness lies within 1e-5 of the threshold, or
    two candidates' objectness values lie within 1e-5 of each other, or
    an IoU the reference's NMS actually evaluates lies within 1e-4 of its threshold.
(The fields are in [0, 1]; a few float32 units of activation difference is ~1e-7; the IoU of 0.05-wide boxes amplifies that to ~1e-5;
the margins are 10-100 times that.)  More than 10 % redraws: the generator is wrong, and the recorder stops.  It prints the largest
difference between the stand-ins' activated fields and the host entry's (vv_detect_activation_host), which must stay below a tenth of
the margins.

Stored per frame i: f{i}_head (the raw frame, float32 [1,R,C,245]), f{i}_args (obj_thresh, IOU_thresh, top_1_pred), the activated fields
the reference held (f{i}_objness / _bbox2D / _bbox3D / _sin / _cos) and its outputs (f{i}_out_bbox2D / _bbox3D / _sin / _cos / _rad),
plus f{i}_out_index: the flat cell * 5 + predictor of every selected row, found by matching the row's rad_log_var (raw values, copied
by the reference without arithmetic) against the frame.
"""
import argparse
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
P, Z, W = 5, 16, 49
OBJ_MARGIN, IOU_MARGIN = 1e-5, 1e-4
SETTINGS = [(0.5, 0.5, True), (0.5, 0.5, False), (0.3, 0.4, False), (0.7, 0.2, True)]
# (grid_row, grid_col, settings, seeds per setting): the 13x13 frames are 166 kB each, hence two of them
PLAN = [(1, 1, SETTINGS, 2), (3, 5, SETTINGS, 2), (6, 9, SETTINGS, 1), (13, 13, [SETTINGS[0], SETTINGS[2]], 1)]


def _stand_ins():
    f32 = lambda x: np.asarray(x, dtype=np.float32)
    tf = types.ModuleType('tensorflow')
    tf.sigmoid = lambda x: (np.float32(1) / (np.float32(1) + np.exp(-f32(x)))).astype(np.float32)
    tf.exp = lambda x: np.exp(f32(x))
    tf.tanh = lambda x: np.tanh(f32(x))
    tf.transpose = lambda x, perm: np.transpose(f32(x), perm)
    tf.stack = lambda xs, axis=0: np.stack([f32(x) for x in xs], axis=axis)
    tf.concat = lambda xs, axis=0: np.concatenate([f32(x) for x in xs], axis=axis)
    tf.nn = types.SimpleNamespace(relu=lambda x: np.maximum(f32(x), np.float32(0)))
    cv2 = types.ModuleType('cv2')
    cv2.rectangle = lambda *a, **k: None
    return tf, cv2


class _Threshold(object):
    """IOU_thresh as the reference's NMS sees it, recording every IoU array it is compared with: `IOU > thresh` reaches __lt__ here
    because numpy defers to an operand with __array_ufunc__ = None; the comparison itself is numpy's float32 one."""
    __array_ufunc__ = None

    def __init__(self, v):
        self.v, self.seen = v, []

    def __lt__(self, iou):
        self.seen.append(np.array(iou))
        return iou > self.v


def draw_frame(rng, R, C, hostile=False):
    """A head output [1,R,C,245] (values on a 2^-10 grid, so that the file compresses): a quiet background and 1-4 objects that light
    1-4 neighbouring cells and 1-3 predictors each with near-equal boxes."""
    f = rng.normal(0.0, 1.0, size=(R, C, P, W)).astype(np.float32)
    f[..., 0] = rng.normal(-4.0, 0.7, size=(R, C, P))                    # objectness: off
    f[..., 1:3] = rng.normal(-2.5, 0.3, size=(R, C, P, 2))               # h, w logits
    for _ in range(int(rng.integers(1, 5))):
        cy, cx = rng.uniform(0.15, 0.85), rng.uniform(0.15, 0.85)        # the object's centre and size, image-normalised
        h, w = rng.uniform(0.15, 0.4), rng.uniform(0.15, 0.4)
        gr0, gc0 = min(R - 1, int(cy * R)), min(C - 1, int(cx * C))
        cells = [(gr0, gc0)] + [(gr0 + dr, gc0 + dc) for dr, dc in ((0, 1), (1, 0), (1, 1)) if gr0 + dr < R and gc0 + dc < C]
        for gr, gc in cells[:int(rng.integers(1, 5))]:
            for p in rng.permutation(P)[:int(rng.integers(1, 4))]:
                y = np.clip(cy * R - gr + rng.normal(0, 0.05), 0.04, 0.96)          # the centre as seen from this cell
                x = np.clip(cx * C - gc + rng.normal(0, 0.05), 0.04, 0.96)
                f[gr, gc, p, 0] = rng.uniform(0.2, 4.0)
                f[gr, gc, p, 1] = np.log(h * rng.uniform(0.9, 1.1))
                f[gr, gc, p, 2] = np.log(w * rng.uniform(0.9, 1.1))
                f[gr, gc, p, 3] = np.log(x / (1 - x))
                f[gr, gc, p, 4] = np.log(y / (1 - y))
    f = (np.round(f * 1024.0) / 1024.0).astype(np.float32)
    if hostile:
        f[0, 0, 1, 0] = f[0, 0, 3, 0] = 2.5                              # one cell, two equal best logits (run with top_1)
        f[0, 0, [0, 2, 4], 0] = -3.0
        # inf and NaN box fields sit in predictors that are NOT candidates: the reference's own drawing loop (int(box * imcol)) raises
        # on a selected box that is not finite, so such candidates are covered by the edge-case tests against tests/_detect_ref.py
        f[1, 2, 0, 0], f[1, 2, 0, 1] = -3.0, 100.0                       # a size logit of 100: exp = inf
        f[2, 1, :2, 0] = np.nan                                          # NaN objectness entries
        f[2, 3, 2, 0], f[2, 3, 2, 3] = -3.0, np.nan                      # a NaN box coordinate
    return np.ascontiguousarray(f.reshape(1, R, C, P * W))


def run_reference(ref_mod, frame, obj_thresh, iou_thresh, top_1):
    inst = object.__new__(ref_mod.nolbo_test)
    inst._enc_backbone_str = ref_mod.config['encoder_backbone']
    inst._encoder_backbone = lambda x, training=False: x
    inst._encoder_head = lambda x, training=False: frame
    _, R, C, _ = frame.shape
    thr = _Threshold(iou_thresh)
    with np.errstate(all='ignore'):
        out = inst.getPred(np.zeros((1, R * 32, C * 32, 3), np.float32), obj_thresh=obj_thresh, IOU_thresh=thr, top_1_pred=top_1,
                           get_3D_shape=False, image_reduced=32)
    held = dict(objness=inst._objness, bbox2D=inst._bbox2D, bbox3D=inst._bbox3D, sin=inst._ori_sin_mean, cos=inst._ori_cos_mean)
    return out[1:], held, thr.seen


def has_margins(held, seen, obj_thresh, iou_thresh, top_1):
    s = np.asarray(held['objness'], dtype=np.float64)[0, ..., 0]            # [R,C,P]
    ok = ~np.isnan(s)
    if np.any(np.abs(s[ok] - obj_thresh) < OBJ_MARGIN):
        return False
    filled = np.where(ok, s, -1.0)
    if top_1:                                                              # which predictor is a cell's best must be clear too
        top2 = np.sort(filled, axis=-1)[..., -2:]
        near = (top2[..., 1] - top2[..., 0] < OBJ_MARGIN) & (top2[..., 1] > obj_thresh) & (top2[..., 1] != top2[..., 0])
        if np.any(near):
            return False
        cand = filled.max(axis=-1).ravel()
    else:
        cand = filled.ravel()
    cand = np.sort(cand[cand > obj_thresh])
    if np.any(np.diff(cand) < OBJ_MARGIN):
        return False
    for iou in seen:
        v = np.asarray(iou, dtype=np.float64)
        v = v[np.isfinite(v)]
        if np.any(np.abs(v - iou_thresh) < IOU_MARGIN):
            return False
    return True


def find_index(frame, rad_rows):
    cells = frame.reshape(-1, P, W)[..., W - 3:].reshape(-1, 3)
    idx = []
    for row in rad_rows:
        hit = np.nonzero(np.all(cells == row, axis=1))[0]
        assert len(hit) == 1, 'a selected row must name one (cell, predictor)'
        idx.append(int(hit[0]))
    return np.asarray(idx, dtype=np.int32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reference', required=True, help='the reference checkout (holds src/module/nolbo_test.py)')
    ap.add_argument('--out', default=os.path.join(HERE, 'detect_frames.npz'))
    a = ap.parse_args()
    tf, cv2 = _stand_ins()
    sys.modules['tensorflow'], sys.modules['cv2'] = tf, cv2
    sys.path.insert(0, os.path.abspath(a.reference))                       # `src` is the reference's from here on
    import importlib.util
    spec = importlib.util.spec_from_file_location('reference_nolbo_test', os.path.join(a.reference, 'src', 'module', 'nolbo_test.py'))
    ref_mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ref_mod)
    sys.path.insert(1, os.path.join(ROOT, 'anytime-3d-reconstruction_amd'))
    from voxvae import detect as D                                         # for the activation comparison only

    store, drawn, redrawn, worst = {}, 0, 0, 0.0
    jobs = [(R, C, s, seed, False) for R, C, settings, seeds in PLAN for s in settings for seed in range(seeds)]
    jobs.append((3, 5, SETTINGS[0], 0, True))
    for i, (R, C, (ot, it, top_1), seed, hostile) in enumerate(jobs):
        rng = np.random.default_rng([R, C, int(ot * 10), int(it * 10), int(top_1), seed, int(hostile)])
        while True:
            frame = draw_frame(rng, R, C, hostile)
            drawn += 1
            outs, held, seen = run_reference(ref_mod, frame, ot, it, top_1)
            if has_margins(held, seen, ot, it, top_1):
                break
            redrawn += 1
        raw = frame.reshape(1, R, C, P, W)
        with np.errstate(all='ignore'):
            for name, which, sl in (('objness', 'sigmoid', slice(0, 1)), ('bbox2D', 'exp', slice(1, 3)), ('bbox2D', 'sigmoid', slice(3, 5)),
                                    ('sin', 'tanh', slice(W - 9, W - 6)), ('cos', 'tanh', slice(W - 6, W - 3))):
                ours = D.activation_host(raw[..., sl], which)
                theirs = np.asarray(held[name], dtype=np.float32)
                theirs = theirs[..., 2:] if (name, which) == ('bbox2D', 'sigmoid') else (theirs[..., :2] if name == 'bbox2D' else theirs)
                fin = np.isfinite(ours) & np.isfinite(theirs)
                assert np.array_equal(np.isnan(ours), np.isnan(theirs)) and np.array_equal(np.isinf(ours), np.isinf(theirs))
                d = np.abs(ours[fin].astype(np.float64) - theirs[fin]) / (np.maximum(np.abs(theirs[fin]), 1.0) if which == 'exp' else 1.0)
                worst = max(worst, float(d.max()) if d.size else 0.0)
        b2, b3, sn, cs, rad = [np.asarray(o, dtype=np.float32) for o in outs]
        store['f%d_head' % i] = frame
        store['f%d_args' % i] = np.asarray([ot, it, float(top_1)], dtype=np.float64)
        for k, v in held.items():
            store['f%d_%s' % (i, k)] = np.asarray(v, dtype=np.float32)
        n = len(b2)
        store['f%d_out_bbox2D' % i], store['f%d_out_bbox3D' % i] = b2.reshape(n, 5), b3.reshape(n, 3)
        store['f%d_out_sin' % i], store['f%d_out_cos' % i], store['f%d_out_rad' % i] = sn.reshape(n, 3), cs.reshape(n, 3), rad.reshape(n, 3)
        store['f%d_out_index' % i] = find_index(frame, rad.reshape(n, 3))
        print('frame %2d  %2dx%-2d  obj %.1f iou %.1f top_1 %d%s: %d selected, %d IoU arrays seen' % (
            i, R, C, ot, it, top_1, ' hostile' if hostile else '', n, len(seen)))
    store['frames'] = np.asarray(len(jobs), dtype=np.int64)
    print('drawn %d, redrawn %d (%.1f %%)' % (drawn, redrawn, 100.0 * redrawn / drawn))
    assert redrawn <= 0.1 * drawn, 'more than 10 % of the frames were redrawn: the generator is wrong'
    print('largest |stand-in activation - host entry| (relative for exp above 1): %.3e' % worst)
    assert worst < 0.1 * OBJ_MARGIN, 'the activations differ by more than a tenth of the margins'
    np.savez_compressed(a.out, **store)
    print('wrote %s: %d bytes' % (a.out, os.path.getsize(a.out)))
    assert os.path.getsize(a.out) < 1000000


if __name__ == '__main__':
    main()
