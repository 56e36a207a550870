"""The float64 definition of the occupancy-grid -> posed-point-cloud step, written from its formulas for the tests of
voxvae/points.py and csrc/voxel_points.hip.  numpy only; nothing here touches the product.

Per object with grid p of side D, threshold prob, size (h, w, l), pose P (4x4, rows 0 .. 2 used; None = identity):
    occupied   p > prob, strictly (a NaN cell is not occupied); for bits: the bit
    cells      the occupied (i, j, k) in increasing flat index v = (i D + j) D + k
    lo, hi     per-axis minimum / maximum of the cells;  ext = hi - lo;  E = max(ext)
    scale      max(h, w, l) / E;  0 when E == 0
    q          (cell - lo) scale - (ext scale) / 2, per axis
    point      P[:3,:3] q + P[:3,3]
    surface    an occupied cell on the grid boundary in some axis, or with an unoccupied face neighbour; lo, hi, scale stay those of ALL
               occupied cells
    empty      no cell: no points, lo = (D, D, D), hi = (-1, -1, -1)
"""
import numpy as np


def occupancy(p, prob=0.5):
    """[..., D, D, D(, 1)] probabilities -> bool, NaN not occupied."""
    with np.errstate(invalid='ignore'):
        return np.asarray(p) > np.float32(prob)


def surface_mask(m):
    """bool [D,D,D] -> the occupied cells on the grid boundary or with an unoccupied face neighbour."""
    inner = np.zeros_like(m)
    if min(m.shape) >= 3:
        inner[1:-1, 1:-1, 1:-1] = (m[1:-1, 1:-1, 1:-1] & m[:-2, 1:-1, 1:-1] & m[2:, 1:-1, 1:-1] & m[1:-1, :-2, 1:-1] & m[1:-1, 2:, 1:-1]
                                   & m[1:-1, 1:-1, :-2] & m[1:-1, 1:-1, 2:])
    return m & ~inner


def object_points(mask, h, w, l, pose=None, surface_only=False):
    """bool [D,D,D] -> (points float64 [n,3], bbox int64 [6] = (lo, hi))."""
    mask = np.asarray(mask, dtype=bool)
    D = mask.shape[0]
    assert mask.shape == (D, D, D)
    P = np.eye(4) if pose is None else np.asarray(pose, dtype=np.float64)
    cells = np.argwhere(mask)                                      # row-major: increasing flat index
    if len(cells) == 0:
        return np.zeros((0, 3)), np.array([D, D, D, -1, -1, -1], dtype=np.int64)
    lo, hi = cells.min(axis=0), cells.max(axis=0)
    ext = hi - lo
    E = int(ext.max())
    scale = float(max(h, w, l)) / E if E > 0 else 0.0
    if surface_only:
        cells = np.argwhere(surface_mask(mask))
    q = (cells - lo).astype(np.float64) * scale - (ext.astype(np.float64) * scale) / 2.0
    return q @ P[:3, :3].T + P[:3, 3], np.concatenate([lo, hi]).astype(np.int64)


def batch_points(masks, dims, poses=None, surface_only=False):
    """bool [B,D,D,D], dims [B,3], poses None / [B,4,4] -> dict(points float64 [N,3], counts int64 [B], bbox int64 [B,6],
    offsets int64 [B+1], parts = the per-object point arrays)."""
    parts, boxes = [], []
    for b in range(len(masks)):
        pts, box = object_points(masks[b], dims[b][0], dims[b][1], dims[b][2], None if poses is None else poses[b], surface_only)
        parts.append(pts)
        boxes.append(box)
    counts = np.array([len(p) for p in parts], dtype=np.int64)
    return dict(points=np.concatenate(parts, axis=0), counts=counts, bbox=np.stack(boxes),
                offsets=np.concatenate([[0], np.cumsum(counts)]).astype(np.int64), parts=parts)


def extent(mask):
    """E = the largest bounding-box extent of a bool grid (0 for an empty or single-cell one)."""
    cells = np.argwhere(mask)
    return int((cells.max(axis=0) - cells.min(axis=0)).max()) if len(cells) else 0


def affine_bound(dims, poses, units=16):
    """[B,3] per-coordinate bound of the float32 path against this definition: units 2^-24 (sum_j |P_ij| max(h, w, l) + |P_i3|).  The path
    has at most ten float32 roundings (the scale, one product, the half extent, one subtraction, three multiply-adds per output, rounded
    up), each at most one unit of that bracket; ten rounded up to a power of two."""
    dims, poses = np.asarray(dims, dtype=np.float64), np.asarray(poses, dtype=np.float64)
    m = dims.max(axis=1)
    return units * 2.0 ** -24 * (np.abs(poses[:, :3, :3]).sum(axis=2) * m[:, None] + np.abs(poses[:, :3, 3]))


def random_poses(rng, B, tmax=20.0):
    """Rotations from the QR of a seeded Gaussian, translations uniform in [-tmax, tmax] -> float32 [B,4,4]."""
    out = np.zeros((B, 4, 4), dtype=np.float64)
    for b in range(B):
        q, r = np.linalg.qr(rng.standard_normal((3, 3)))
        out[b, :3, :3] = q * np.sign(np.diag(r))
        out[b, :3, 3] = rng.uniform(-tmax, tmax, 3)
        out[b, 3, 3] = 1.0
    return out.astype(np.float32)
