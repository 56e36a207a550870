"""numpy float64 statement of the viewpoint k-means (csrc/kmeans_cosine.h; the reference's kmeans_cosine._kmeans), with NO early exit:
every one of the max_iter iterations is computed.  Shared by tests/test_kmeans_host.py, tests/test_gpu_kmeans.py and
profiles/microbench/mb_kmeans.py.

    distance   per j = 0, 1, 2:  p = x[j] c[j];  q = x[j+3] c[j+3];  s = p + q;  t = 1 - s;  u_j = t t;      d = (u_0 + u_1) + u_2
    label      np.argmin: the lowest index among equal minima
    update     a populated cluster becomes sum / count, the sum taken chunk by chunk of CHUNK consecutive rows (members in index order
               inside a chunk, chunks in order); an empty cluster keeps its row

Besides the result it reports the smallest NON-ZERO gap between a point's best and second-best distance over all iterations: while
that gap exceeds the centres' rounding differences by orders of magnitude, two summation orders give the same labels, and with the same
labels a centre is a mean of at most N values of magnitude <= 1 taken straight from X -- error <= N 2^-53 whatever the order, nothing
carried from iteration to iteration.  That is where the tests' 1e-12 comes from."""
import numpy as np

CHUNK = 256          # VV_KM_CHUNK


def distances(X, centres):
    """-> D [N, k], every operation rounded once, in the order stated above."""
    X, C = np.asarray(X, dtype=np.float64), np.asarray(centres, dtype=np.float64)
    u = []
    for j in range(3):
        p = X[:, j, None] * C[None, :, j]
        q = X[:, j + 3, None] * C[None, :, j + 3]
        s = p + q
        t = 1.0 - s
        u.append(t * t)
    return (u[0] + u[1]) + u[2]


def min_gap(D):
    """Smallest non-zero (second best - best) over the rows of D; inf for one centre or when every gap is zero."""
    if D.shape[1] < 2:
        return np.inf
    two = np.partition(D, 1, axis=1)[:, :2]
    g = two[:, 1] - two[:, 0]
    g = g[g > 0]
    return float(g.min()) if g.size else np.inf


def assign(X, centres):
    D = distances(X, centres)
    xtoc = np.argmin(D, axis=1)
    return xtoc, D[np.arange(len(D)), xtoc], D


def update(X, centres, xtoc, chunk=CHUNK):
    """The centres after one update (a new array)."""
    out = centres.copy()
    for c in np.unique(xtoc):
        idx = np.flatnonzero(xtoc == c)
        total = np.zeros(6)
        for ch in np.unique(idx // chunk):
            part = np.zeros(6)
            for i in idx[idx // chunk == ch]:
                part = part + X[i]
            total = total + part
        out[c] = total / float(idx.size)
    return out


def kmeans(X, centres, max_iter, chunk=CHUNK):
    """-> dict(centres, xtoc, distance, gap, populated, settled): all max_iter iterations; xtoc / distance are the last iteration's,
    taken before its update.  `populated` [k]: the cluster had a member in some iteration; `settled`: the first iteration (1-based)
    whose labels equal the previous iteration's, or None."""
    X = np.ascontiguousarray(X, dtype=np.float64)
    C = np.array(centres, dtype=np.float64)
    gap, settled, prev = np.inf, None, None
    populated = np.zeros(C.shape[0], dtype=bool)
    xtoc = dist = None
    for it in range(1, int(max_iter) + 1):
        xtoc, dist, D = assign(X, C)
        gap = min(gap, min_gap(D))
        populated[np.unique(xtoc)] = True
        if settled is None and prev is not None and np.array_equal(prev, xtoc):
            settled = it
        C = update(X, C, xtoc, chunk)                                         # (also after `settled`: no early exit)
        prev = xtoc
    return dict(centres=C, xtoc=xtoc, distance=dist, gap=gap, populated=populated, settled=settled)


# ---------------------------------------------------------------------------------------------------------------- the shared cases
# name: (points, centres, max_iter, seed).  C = CHUNK: one short of, exactly and one past a chunk; several chunks with a ragged last
# one; a single centre; more centres than points; two identical initial centres; a run far longer than it takes to settle.
MIN_GAP = 1e-9
TOL = 1e-12
CASES = {'one point': (1, 3, 5, 1), 'chunk - 1': (CHUNK - 1, 7, 25, 2), 'chunk': (CHUNK, 7, 25, 3), 'chunk + 1': (CHUNK + 1, 7, 25, 4),
         'one centre': (2 * CHUNK + 3, 1, 4, 5), 'more centres than points': (5, 9, 12, 6), 'twins': (300, 4, 25, 7),
         'settles': (300, 5, 1000, 8), 'six chunks': (1500, 30, 40, 9)}
_cache = {}


def case(name):
    """-> (X, centres0, max_iter) of a shared case; the initial centres are rows of X where there are enough."""
    n, k, max_iter, seed = CASES[name]
    if name == 'twins':
        X, C = twin_case(n, seed)
    else:
        X = viewpoints(n, seed)
        C = X[np.random.default_rng(seed + 100).choice(n, k, replace=False)].copy() if k <= n else viewpoints(k, seed + 100, duplicates=0)
    return X, C, max_iter


def reference(name):
    """The definition's result for a shared case, computed once per process and never modified (arrays are read-only)."""
    if name not in _cache:
        X, C, max_iter = case(name)
        r = kmeans(X, C, max_iter)
        for v in r.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        _cache[name] = r
    return _cache[name]


def twin_case(n, seed):
    """-> (X [n, 6], centres0 [4, 6]) with rows 1 and 3 of centres0 IDENTICAL.  The first twin must take every tie, the second must stay
    empty and keep its row -- in every iteration, not only the first, so the stale twin has to lose against the moved one for good:
    the azimuths lie in [-1, 1], the twins sit outside at 1.6 (the other two centres at -0.8 and -0.2, none a row of X).  Iteration 1
    gives the first twin the points above ~0.7; it moves to their mean near 0.85, and from then on every point is nearer to a moved
    centre than to the stale twin at 1.6."""
    rng = np.random.default_rng(seed)
    e = np.stack([rng.uniform(-1.0, 1.0, n), rng.normal(0.15, 0.2, n), rng.normal(0.0, 0.1, n)], axis=1)
    c = np.array([[-0.8, 0.15, 0.0], [1.6, 0.15, 0.0], [-0.2, 0.15, 0.0], [1.6, 0.15, 0.0]])
    return np.concatenate([np.sin(e), np.cos(e)], axis=1), np.concatenate([np.sin(c), np.cos(c)], axis=1)


def viewpoints(n, seed, duplicates=0.25):
    """[n, 6] rows as a Pascal3D+ split has them: azimuth uniform, elevation and in-plane rotation narrow normals, and `duplicates` of
    the rows copies of other rows (the same annotation on several objects)."""
    rng = np.random.default_rng(seed)
    e = np.stack([rng.uniform(-np.pi, np.pi, n), rng.normal(0.15, 0.2, n), rng.normal(0.0, 0.1, n)], axis=1)
    m = int(n * duplicates)
    if m and n > 1:
        dst = rng.choice(n, m, replace=False)
        e[dst] = e[rng.integers(0, n, m)]
    return np.concatenate([np.sin(e), np.cos(e)], axis=1)
