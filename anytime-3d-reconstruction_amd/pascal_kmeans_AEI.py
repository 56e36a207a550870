"""Entry point for the driver the reference keeps commented out at the end of src/dataset_loader/pascal3D.py (:552-558): cluster the
viewpoints of a Pascal3D+ split with getKmeansAEI, print the centres and the median distance, and save the centres -- the table the
reference pastes back into its source as AEI_kmeans.
`python pascal_kmeans_AEI.py --k 30 --max-iter 1000 --seed 0 --out centres.npy`.
The split must hold at least 10 * k objects (kmeansSample draws that many rows without replacement); the synthetic stand-in is sized
by --dataset-path synthetic:N:D, and only its Euler angles are read."""
import random
import sys

import numpy as np

import src.dataset_loader.pascal3D as pascal3D


def run(k=30 * 12, max_iter=1000, seed=None, out=None, split='val', dataset_path=None, loader='host', leg=None):
    data_loader_pascal = pascal3D.LOADERS[loader](trainOrVal=split, Pascal3DDataPath=dataset_path)
    if seed is not None:
        random.seed(seed)
    kw = {} if leg is None else {'host': leg == 'host'}
    center, xtoc, dist = data_loader_pascal.getKmeansAEI(k=k, max_iter=max_iter, **kw)
    print(center)
    print(np.median(dist))
    if out is not None:
        with open(out, 'wb') as f:                                           # (np.save appends .npy to a bare name; a file object is taken as is)
            np.save(f, center)
    return center, xtoc, dist


if __name__ == '__main__':
    import argparse
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument('--k', type=int, default=30 * 12, help='centres; the reference runs 30 * 12')
    ap.add_argument('--max-iter', type=int, default=1000)
    ap.add_argument('--seed', type=int, default=None, help="random.seed before the picks of kmeansSample")
    ap.add_argument('--out', default=None, help='centres as a float64 [k, 6] .npy')
    ap.add_argument('--split', default='val', choices=['train', 'val'])
    ap.add_argument('--dataset-path', default='synthetic:4000:8', help='None-like default: a seeded stand-in of 4000 objects')
    ap.add_argument('--loader', default='host', choices=sorted(pascal3D.LOADERS))
    ap.add_argument('--leg', default=None, choices=['device', 'host'], help='where the k-means runs; default: the device when there is one')
    a = ap.parse_args()
    c, _, _ = run(k=a.k, max_iter=a.max_iter, seed=a.seed, out=a.out, split=a.split, dataset_path=a.dataset_path, loader=a.loader, leg=a.leg)
    sys.exit(0 if c.shape == (a.k, 6) and c.dtype == np.float64 else 1)
