"""The float64 definition of the detection -> world-pose step, written from its description for the tests of voxvae/pose.py,
csrc/pose_solve.h and csrc/object_pose.hip.  numpy only (the smallest singular vector comes from np.linalg.svd); nothing here touches
the product.  It serves the shapes the recorded fixtures (tests/golden/pose_kitti.npz) do not cover, and is itself checked against them.

Per detection: normalised box (x1, y1, x2, y2, objectness), size (w, h, l), sines and cosines of (A, E, I), one camera (P, P^-1, image size):
    inputs     a NaN among the 14 numbers: not kept, candidate -2
    pre-filter x1 > 0.1 and x2 < 0.9 and y2 < 0.9, else not kept, candidate -2
    pixels     x * image_col, y * image_row
    elevation  E - (-5 degrees): sinE' = sinE cos b - cosE sin b, cosE' = cosE cos b + sinE sin b, b = -5 / 180 pi
    rotation   r = RA RE RI;  R_obj = rows (r1, -r3, r2)
    ray        through the box centre: P^-1 (px, py, 1, 1), normalised;  R_ray from it;  R = R_ray R_obj
    fit        candidates k = 0 .. 127 (see `candidate_corners`): rows B_x[0] - x_min B_x[2], B_y[1] - y_min B_y[2], ... with
               B = P [I | R d; 0 0 0 1]; t = right singular vector of the smallest singular value; accepted when t3 t2 > 0, the
               reprojected box is proper, and its IoU with the detected box (intersection NOT clamped) is < 1.  Winner: the largest IoU
               above -1, ties to the lowest k;  none: X = 0, candidate -1
    pose       [R X; 0 0 0 1];  corners: P (R (+-h/2, +-l/2, +-w/2) + X) as [2,2,2,2], index 0 = +;  size row (h, l, w)
    post       kept when X[2] > 0.1;  pixel box truncated toward zero
"""
import numpy as np

BETA = -5.0 / 180.0 * np.pi
# corner signs in units of (dx, dy, dz) = (w / 2, l / 2, h / 2): [list][element]
XMIN = [[(-1, -1, -1), (-1, -1, 1)], [(-1, 1, -1), (-1, 1, 1)]]
XMAX = [[(1, 1, -1), (1, 1, 1)], [(1, -1, 1), (1, -1, -1)]]
YMIN = [[(-1, -1, 1), (1, -1, 1)], [(-1, 1, 1), (1, 1, 1)]]
YMAX = [[(-1, 1, -1), (1, 1, -1)], [(-1, -1, -1), (1, -1, -1)]]


def candidate_corners(k):
    """k -> the sign triples of the corners tied to (x_min, y_min, x_max, y_max).  k counts the loop nest in execution order: 4 x-side
    pairings (XMIN[0]/XMAX[0], XMIN[1]/XMAX[1], then the two with the sides swapped), 2 y-side pairings, then one bit each for the
    element of the xmin, ymin, xmax and ymax set."""
    px, py, a, b, c, d = (k >> 5) & 3, (k >> 4) & 1, (k >> 3) & 1, (k >> 2) & 1, (k >> 1) & 1, k & 1
    xmin_set, xmax_set = (XMIN[px], XMAX[px]) if px < 2 else (XMAX[px - 2], XMIN[px - 2])
    return xmin_set[a], YMIN[py][b], xmax_set[c], YMAX[py][d]


def object_rotation(sn, cs):
    sinA, sinE, sinI = [float(v) for v in sn]
    cosA, cosE, cosI = [float(v) for v in cs]
    sinE, cosE = sinE * np.cos(BETA) - cosE * np.sin(BETA), cosE * np.cos(BETA) + sinE * np.sin(BETA)
    r11, r12, r13 = -sinA * sinE * sinI + cosA * cosI, -sinA * cosE, sinA * sinE * cosI + sinI * cosA
    r21, r22, r23 = sinA * cosI + sinE * sinI * cosA, cosA * cosE, sinA * sinI - sinE * cosA * cosI
    r31, r32, r33 = -sinI * cosE, sinE, cosE * cosI
    return np.array([[r11, r12, r13], [-r31, -r32, -r33], [r21, r22, r23]])


def ray_rotation(Pinv, px, py):
    ray = (Pinv @ np.array([px, py, 1.0, 1.0]))[:3]
    ray = ray / np.sqrt((ray * ray).sum())
    rx, ry, rz = ray / np.sqrt((ray * ray).sum())
    n = np.sqrt(ry * ry + rz * rz)
    cy, cx, sx, sy = n, rz / n, -ry / n, rx
    return np.array([[cy, 0.0, sy], [sx * sy, cx, -sx * cy], [-cx * sy, sx, cx * cy]])


def _rows(P, R, sign, half):
    M = np.eye(4)
    M[:3, 3] = R @ (np.array(sign, dtype=np.float64) * half)
    return P @ M


def candidate(k, P, R, box, w, h, l):
    """-> (iou, t[3]) or None when rejected."""
    x_min, y_min, x_max, y_max = box
    half = np.array([w / 2.0, l / 2.0, h / 2.0])
    B0, B1, B2, B3 = [_rows(P, R, s, half) for s in candidate_corners(k)]
    A = np.stack([B0[0] - x_min * B0[2], B1[1] - y_min * B1[2], B2[0] - x_max * B2[2], B3[1] - y_max * B3[2]])
    if not np.isfinite(A).all():
        return None
    t = np.linalg.svd(A)[2][-1]
    if not t[3] * t[2] > 0:
        return None
    t = t / t[3]
    xa, ya, xb, yb = (B0 @ t), (B1 @ t), (B2 @ t), (B3 @ t)
    xa, ya, xb, yb = xa[0] / xa[2], ya[1] / ya[2], xb[0] / xb[2], yb[1] / yb[2]
    if not (xa < xb and ya < yb):
        return None
    pred, gt = (xb - xa) * (yb - ya), (x_max - x_min) * (y_max - y_min)
    inter = (min(xb, x_max) - max(xa, x_min)) * (min(yb, y_max) - max(ya, y_min))
    iou = inter / (pred + gt - inter)
    if not iou < 1.0:
        return None
    return float(iou), t[:3].copy()


def fit(P, R, box, w, h, l):
    """-> dict(candidate, iou, X, ious [128] (NaN = rejected), ts [128,3]): the winner by (largest IoU above -1, lowest k)."""
    ious, ts = np.full(128, np.nan), np.zeros((128, 3))
    best_k, best_iou, X = -1, -1.0, np.zeros(3)
    for k in range(128):
        c = candidate(k, P, R, box, w, h, l)
        if c is None:
            continue
        ious[k], ts[k] = c
        if c[0] > best_iou:
            best_k, best_iou, X = k, c[0], c[1]
    return dict(candidate=best_k, iou=best_iou, X=X, ious=ious, ts=ts)


def distinct_gap(f, rel=1e-9):
    """IoU gap between the winner and the best candidate with a DIFFERENT translation (inf when there is none or no winner)."""
    if f['candidate'] < 0:
        return np.inf
    X = f['X']
    ok = ~np.isnan(f['ious'])
    other = ok & (np.abs(f['ts'] - X).max(axis=1) > rel * np.abs(X).max())
    return float(f['iou'] - f['ious'][other].max()) if other.any() else np.inf


def corners_projection(P, R, X, w, h, l):
    """The [2,2,2,2] array of projected corners for half extents (w / 2, l / 2, h / 2) along the object's axes; index 0 = +."""
    out = np.zeros((2, 2, 2, 2))
    for i in range(2):
        for j in range(2):
            for k in range(2):
                d = np.array([(1 - 2 * i) * w / 2.0, (1 - 2 * j) * l / 2.0, (1 - 2 * k) * h / 2.0])
                x = P @ np.concatenate([R @ d + X, [1.0]])
                out[i, j, k] = x[:2] / x[2]
    return out


def object_pose(b2, b3, sn, cs, image_size, P, Pinv):
    """One detection (float32 values, computed in float64) -> dict(keep, candidate, iou, X, R, pose, size, box2d, proj, fit)."""
    b2, b3, sn, cs = [np.asarray(v, dtype=np.float32).astype(np.float64) for v in (b2, b3, sn, cs)]
    out = dict(keep=False, candidate=-2, iou=-1.0, X=np.zeros(3), fit=None)
    if np.isnan(np.concatenate([b2, b3, sn, cs])).any():
        return out
    x1, y1, x2, y2 = b2[:4]
    if not (x1 > 1e-1 and x2 < 1.0 - 1e-1 and y2 < 1.0 - 1e-1):
        return out
    col, row = float(image_size[0]), float(image_size[1])
    x1, y1, x2, y2 = x1 * col, y1 * row, x2 * col, y2 * row
    w, h, l = b3
    R = ray_rotation(Pinv, (x2 + x1) / 2.0, (y2 + y1) / 2.0) @ object_rotation(sn, cs)
    f = fit(P, R, (x1, y1, x2, y2), w, h, l)
    X = f['X']
    pose = np.eye(4)
    pose[:3, :3], pose[:3, 3] = R, X
    out.update(keep=bool(X[2] > 1e-1), candidate=f['candidate'], iou=f['iou'], X=X, R=R, pose=pose, size=np.array([h, l, w]),
               box2d=np.array([int(x1), int(y1), int(x2), int(y2)]), proj=corners_projection(P, R, X, h, w, l), fit=f)
    return out


def batch(bbox2d, bbox3d, sn, cs, image_size, P, Pinv=None):
    """-> dict(keep, candidate, iou, X per detection; count, index, pose, size, box2d, proj compacted in input order)."""
    P = np.asarray(P, dtype=np.float64)
    Pinv = np.linalg.inv(P) if Pinv is None else np.asarray(Pinv, dtype=np.float64)
    rows = [object_pose(bbox2d[i], bbox3d[i], sn[i], cs[i], image_size, P, Pinv) for i in range(len(bbox2d))]
    kept = [i for i, r in enumerate(rows) if r['keep']]
    pick = lambda key, shape: np.array([rows[i][key] for i in kept]).reshape((len(kept),) + shape)
    return dict(keep=np.array([r['keep'] for r in rows]), candidate=np.array([r['candidate'] for r in rows]),
                iou=np.array([r['iou'] for r in rows]), X=np.array([r['X'] for r in rows]), count=len(kept), index=np.array(kept, dtype=np.int64),
                pose=pick('pose', (4, 4)), size=pick('size', (3,)), box2d=pick('box2d', (4,)).astype(np.int64), proj=pick('proj', (2, 2, 2, 2)),
                rows=rows)
