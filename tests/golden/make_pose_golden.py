"""Records tests/golden/pose_kitti.npz by running the reference's own getObjectInRealWorld and getTranslation
(src/visualizer/visualizer.py of the reference tree) on seeded, KITTI-like detections.  No test imports this file.

    python tests/golden/make_pose_golden.py /path/to/reference [out.npz]

The reference module imports cv2 for its drawing functions only; an empty stand-in module is put into sys.modules when cv2 is missing.
Inputs are stored as float32 and handed to the reference as float64 arrays, so the reference computes in float64 throughout.

Rows (in a seeded shuffle, so that kept and dropped rows interleave):
    yaw        objects of size w, h, l in [1.4,2.0] x [1.3,1.9] x [3,5] at x in [-8,8], y in [0.8,1.8], z in [6,40] with a random
               azimuth; the detected box = the projected box + N(0, 2 px) per edge; re-drawn until the clean box lies inside the
               pre-filter's margins
    general    the same with elevation and in-plane angles too
    border     the same without the re-draw: boxes that touch or leave the margins (pre-filtered) beside boxes that do not
    odd        far-off boxes (30 image heights above the image) and boxes with their sides swapped; the latter are the rows for which
               every candidate is rejected, X = 0
    nan        one row with a NaN size: stored, the reference is not run on it, expected "not kept"
Per row the reference's result, and from tests/_pose_ref.py (cross-checked against the reference's translation) the winning k, its
IoU and the IoU gap to the best candidate with a DIFFERENT translation.  Rows with a gap below 1e-9 are dropped and reported (none is
expected; more than 1 % dropped means the generator is wrong).
"""
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import _pose_ref as PR  # noqa: E402

IMAGE = (1242, 375)
GAP_MIN = 1e-9


def load_reference(path):
    try:
        import cv2  # noqa: F401
    except Exception:
        sys.modules['cv2'] = types.ModuleType('cv2')
    sys.path.insert(0, path)
    import src.visualizer.visualizer as V
    return V


def draw(rng, P, Pinv, general, inside):
    """One detection: (bbox2d [5], bbox3d [3], sin [3], cos [3]) as float64."""
    while True:
        w, h, l = rng.uniform([1.4, 1.3, 3.0], [2.0, 1.9, 5.0])
        X = np.array([rng.uniform(-8, 8), rng.uniform(0.8, 1.8), rng.uniform(6, 40 if inside else 14)])
        ang = np.array([rng.uniform(-np.pi, np.pi), 0.0, 0.0])
        if general:
            ang[1:] = rng.uniform(-0.3, 0.3), rng.uniform(-0.2, 0.2)
        sn, cs = np.sin(ang), np.cos(ang)
        c = P @ np.concatenate([X, [1.0]])
        R = PR.ray_rotation(Pinv, c[0] / c[2], c[1] / c[2]) @ PR.object_rotation(sn.astype(np.float32), cs.astype(np.float32))
        uv = PR.corners_projection(P, R, X, w, h, l).reshape(-1, 2)
        box = np.array([uv[:, 0].min(), uv[:, 1].min(), uv[:, 0].max(), uv[:, 1].max()])
        norm = box / np.array([IMAGE[0], IMAGE[1], IMAGE[0], IMAGE[1]])
        if inside and not (norm[0] > 0.12 and norm[2] < 0.88 and norm[3] < 0.88 and norm[1] > 0.0):
            continue
        box = box + rng.normal(0, 2, 4)
        norm = box / np.array([IMAGE[0], IMAGE[1], IMAGE[0], IMAGE[1]])
        return np.concatenate([norm, [rng.uniform(0.5, 1.0)]]), np.array([w, h, l]), sn, cs


def odd(rng, kind):
    """Boxes that no detector emits for such an object.  kind 0: far off above the image (they pass the pre-filter, which has no upper
    margin; every one we tried still finds a candidate, hundreds of metres away).  kind 1: the sides swapped (x_min > x_max, with or
    without y_min > y_max): the rows for which every candidate is rejected."""
    cx, cy = rng.uniform(0.3, 0.7), rng.uniform(0.3, 0.6)
    hw, hh = rng.uniform(0.02, 0.1), rng.uniform(0.05, 0.2)
    box = [cx - hw, cy - hh - 30.0, cx + hw, cy + hh - 30.0] if kind == 0 else [cx + hw, cy + (hh if rng.random() < 0.5 else -hh), cx - hw, cy]
    ang = np.array([rng.uniform(-np.pi, np.pi), rng.uniform(-0.3, 0.3), rng.uniform(-0.2, 0.2)])
    return (np.array(box + [0.9]), rng.uniform([1.4, 1.3, 3.0], [2.0, 1.9, 5.0]), np.sin(ang), np.cos(ang))


def main():
    V = load_reference(sys.argv[1])
    out = sys.argv[2] if len(sys.argv) > 2 else os.path.join(HERE, 'pose_kitti.npz')
    P = np.array(V.kitti_proj_mat, dtype=np.float64)
    Pinv = np.linalg.inv(P)
    rng = np.random.default_rng(20260)
    rows = [draw(rng, P, Pinv, False, True) for _ in range(230)] + [draw(rng, P, Pinv, True, True) for _ in range(90)]
    rows += [draw(rng, P, Pinv, bool(i & 1), False) for i in range(50)] + [odd(rng, i % 2) for i in range(30)]
    rows = [rows[i] for i in rng.permutation(len(rows))]
    nan_row = draw(rng, P, Pinv, False, True)
    nan_row[1][1] = np.nan
    rows.insert(len(rows) // 2, nan_row)
    b2, b3, sn, cs = [np.array([r[j] for r in rows]).astype(np.float32) for j in range(4)]
    grid = np.zeros((64, 64, 64), dtype=np.float64)                # the reference poses a 64^3 grid alongside; two cells do
    grid[10, 10, 10] = grid[20, 30, 40] = 1.0
    N = len(rows)
    rec = dict(ran=np.ones(N, bool), keep=np.zeros(N, bool), candidate=np.full(N, -2), iou=np.full(N, -1.0), translation=np.zeros((N, 3)),
               gap=np.full(N, np.inf), pose=np.full((N, 4, 4), np.nan), size=np.full((N, 3), np.nan), box2d=np.zeros((N, 4), np.int64),
               proj=np.full((N, 2, 2, 2, 2), np.nan))
    dropped, worst = [], 0.0
    for i in range(N):
        a2, a3, asn, acs = [v[i].astype(np.float64) for v in (b2, b3, sn, cs)]
        if np.isnan(np.concatenate([a2, a3, asn, acs])).any():
            rec['ran'][i] = False
            continue
        with np.errstate(all='ignore'):
            pose, size, _, box, proj = V.getObjectInRealWorld([a2], [a3], [asn], [acs], [grid], IMAGE, proj_mat=P, proj_mat_inv=Pinv)
        mine = PR.object_pose(b2[i], b3[i], sn[i], cs[i], IMAGE, P, Pinv)
        rec['keep'][i] = len(pose) == 1
        assert mine['keep'] == rec['keep'][i], i
        rec['candidate'][i] = mine['candidate']
        if mine['fit'] is None:                                   # pre-filtered: the reference never fits
            continue
        px = a2[:4] * np.array([IMAGE[0], IMAGE[1], IMAGE[0], IMAGE[1]])
        R = pose[0][:3, :3] if rec['keep'][i] else mine['R']      # the reference's own rotation where it returns one
        assert np.abs(R - mine['R']).max() <= 1e-14, i
        with np.errstate(all='ignore'):
            Xref = V.getTranslation(P, R, tuple(px), tuple(a3)).reshape(3)
        scale = max(np.abs(Xref).max(), 1e-300)
        worst = max(worst, np.abs(mine['X'] - Xref).max() / scale)
        assert np.abs(mine['X'] - Xref).max() <= 1e-9 * scale, (i, mine['X'], Xref)
        rec['iou'][i], rec['translation'][i], rec['gap'][i] = mine['iou'], Xref, PR.distinct_gap(mine['fit'])
        if rec['gap'][i] < GAP_MIN:
            dropped.append(i)
        if rec['keep'][i]:
            assert np.array_equal(pose[0][:3, 3], Xref), i
            rec['pose'][i], rec['size'][i], rec['box2d'][i], rec['proj'][i] = pose[0], size[0], box[0], proj[0]
    print('rows %d: kept %d, pre-filtered %d, fitted without a winner %d, not run %d' % (
        N, rec['keep'].sum(), (rec['candidate'] == -2).sum() - (~rec['ran']).sum(), (rec['candidate'] == -1).sum(), (~rec['ran']).sum()))
    print('our float64 statement vs the reference translation: max relative difference %.2e' % worst)
    print('smallest IoU gap to a distinct translation %.3e; dropped (gap < %.0e): %s' % (rec['gap'].min(), GAP_MIN, dropped))
    assert len(dropped) <= 0.01 * N, 'the generator is wrong: %d rows dropped' % len(dropped)
    assert (rec['candidate'] == -1).sum() >= 1 and (rec['candidate'] == -2).sum() >= 5 and rec['keep'].sum() >= 300
    sel = np.array([i for i in range(N) if i not in dropped])
    np.savez_compressed(out, bbox2d=b2[sel], bbox3d=b3[sel], sin=sn[sel], cos=cs[sel], image_size=np.array(IMAGE, dtype=np.int64), proj_mat=P,
                        **{k: v[sel] for k, v in rec.items()})
    print('wrote %s (%d rows, %d bytes)' % (out, len(sel), os.path.getsize(out)))


if __name__ == '__main__':
    main()
