"""Maker of tests/golden/kmeans_cosine.npz: runs the REFERENCE's own kmeans_cosine class on a CPU and records what it computed.

    python tests/golden/make_kmeans_golden.py --reference /path/to/reference/src/module/function.py

The class is loaded from that file at generation time (the module imports TensorFlow, which this needs not: only the text from the
class statement on is compiled, against numpy and a recording stand-in for `random`); none of it is kept here.  Recorded per case:

    kmeansSample cases  X, k, max_iter, seed, the two replayed random.sample picks, and the reference's centres, xtoc, distance
    the _kmeans case    X, initial centres with rows 1 and 3 IDENTICAL, max_iter, and the reference's centres, xtoc, distance

The reference sums a cluster's members in plain index order, the project in chunks of 256; the two agree on the labels as long as no
point sits closer to a decision boundary than the centres' rounding differences.  So the maker measures, in every iteration of every
case, the smallest non-zero gap between a point's best and second-best distance and REFUSES to write unless it is at least 1e-9
(rounding differences are below N 2^-53 ~ 1e-13).  With equal labels the centres agree within 1e-12, the tests' tolerance."""
import argparse
import contextlib
import io
import os
import random
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import _kmeans_ref as R  # noqa: E402

MIN_GAP = 1e-9
SAMPLE_CASES = [dict(name='s300', n=300, k=5, max_iter=100, seed=11), dict(name='s700', n=700, k=23, max_iter=100, seed=12),
                dict(name='s1000', n=1000, k=40, max_iter=60, seed=13)]
PLAIN_CASE = dict(name='twins', n=513, k=4, max_iter=30, seed=14)


class _Random(object):
    """random.sample, recorded."""

    def __init__(self):
        self.picks = []

    def sample(self, population, count):
        out = random.sample(population, count)
        self.picks.append(list(out))
        return out


def load_reference_class(path, rnd):
    text = open(path).read()
    start = text.index('class kmeans_cosine')
    ns = {'np': np, 'random': rnd, 'sys': sys}
    exec(compile(text[start:], path, 'exec'), ns)
    base = ns['kmeans_cosine']

    class Measured(base):
        gap = np.inf

        def _dist_cosine(self, X, centres):
            D = base._dist_cosine(self, X, centres)
            Measured.gap = min(Measured.gap, R.min_gap(D))
            return D

    return Measured


def main():
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument('--reference', required=True, help="the reference's src/module/function.py")
    ap.add_argument('--out', default=os.path.join(HERE, 'kmeans_cosine.npz'))
    a = ap.parse_args()
    rnd = _Random()
    cls = load_reference_class(a.reference, rnd)
    rec = {}
    with contextlib.redirect_stdout(io.StringIO()):                           # the class prints a progress line per iteration
        for c in SAMPLE_CASES:
            X = R.viewpoints(c['n'], c['seed'])
            random.seed(c['seed'])
            rnd.picks = []
            centres, xtoc, dist = cls(X=X, k=c['k'], max_iter=c['max_iter']).kmeansSample()
            assert len(rnd.picks) == 2
            p = c['name'] + '_'
            rec.update({p + 'X': X, p + 'k': c['k'], p + 'max_iter': c['max_iter'], p + 'seed': c['seed'],
                        p + 'sample_idx': np.array(rnd.picks[0], dtype=np.int64), p + 'centre_idx': np.array(rnd.picks[1], dtype=np.int64),
                        p + 'centres': np.array(centres), p + 'xtoc': np.array(xtoc, dtype=np.int64), p + 'distance': np.array(dist)})
        c = PLAIN_CASE
        X, first = R.twin_case(c['n'], c['seed'])
        centres, xtoc, dist = cls(X=X, k=c['k'])._kmeans(X, first.copy(), max_iter=c['max_iter'])
        assert (xtoc == 1).any() and not (xtoc == 3).any() and np.array_equal(centres[3], first[3]), \
            'np.argmin gives every tie to the first of two identical centres; the second stays empty and keeps its row'
        p = c['name'] + '_'
        rec.update({p + 'X': X, p + 'centres0': first, p + 'max_iter': c['max_iter'], p + 'centres': np.array(centres),
                    p + 'xtoc': np.array(xtoc, dtype=np.int64), p + 'distance': np.array(dist)})
    gap = float(cls.gap)
    print('smallest non-zero gap between best and second-best distance over all iterations of all cases: %.3e' % gap)
    if not gap >= MIN_GAP:
        sys.exit('refused: the gap is below %g, the labels would depend on the summation order' % MIN_GAP)
    rec['min_gap'] = np.float64(gap)
    rec['sample_cases'] = np.array([c['name'] for c in SAMPLE_CASES])
    np.savez_compressed(a.out, **rec)
    print('wrote', a.out, os.path.getsize(a.out), 'bytes')


if __name__ == '__main__':
    main()
