"""Writes tests/golden/prior_latent.npz: seeded float32 inputs of the one-group, one-prior latent stage and what the float64 numpy
definition (tests/_prior_ref.py, written from the formulas of include/voxvae.h) makes of them.

    training   t<k>: enc, eps, mean_p, lv_p, eps_p[, keep], dz_in, dist, reg_weight -> z_in, kl, reg (float64)
               B in {1, 2, 5} x L in {1, 16} x {without, with} keep; dist / reg_weight alternate between the two classes' constants
    evaluation e<k>: enc, eps[, mask, fill], prior -> z, z_corr (float64), idx (int32)
               B in {1, 2, 5} x L in {1, 16} x I in {1, 10} x {without, with} mask

The file holds one flat array per element type (f32, f64, i32) and `layout`, a JSON list of [name, type, shape] in the order the
arrays were appended (a zip member per array would cost more than the numbers); tests/test_prior_latent_host.load_golden reads it.
`python tests/golden/make_prior_golden.py` rewrites the file; it is deterministic."""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

import _prior_ref as R  # noqa: E402

TYPES = {'f32': np.float32, 'f64': np.float64, 'i32': np.int32}


def main():
    flat, layout = {k: [] for k in TYPES}, []

    def add(name, v):
        v = np.asarray(v)
        t = {np.dtype(np.float32): 'f32', np.dtype(np.float64): 'f64', np.dtype(np.int32): 'i32'}[v.dtype]
        flat[t].append(v.reshape(-1))
        layout.append([name, t, list(v.shape)])

    nt = ne = 0
    for B in (1, 2, 5):
        for L in (1, 16):
            for keep in (False, True):
                per_dim, weight = ((10.0, 1.0), (3.0, 0.01))[nt % 2]
                c = R.train_case(100 + nt, B, L, keep=keep, dist_per_dim=per_dim, reg_weight=weight)
                r = R.train_fwd(*R.train_args(c))
                for k, v in list(c.items()) + list(r.items()):
                    if v is not None:
                        add('t%d_%s' % (nt, k), v)
                nt += 1
            for I in (1, 10):
                for p in (0.0, 0.4):
                    c = R.eval_case(200 + ne, B, L, I, p)
                    r = R.inst_eval(*R.eval_args(c))
                    for k, v in list(c.items()) + list(r.items()):
                        if v is not None:
                            add('e%d_%s' % (ne, k), v)
                    ne += 1
    out = {t: np.concatenate(flat[t]).astype(TYPES[t]) for t in TYPES}
    path = os.path.join(HERE, 'prior_latent.npz')
    np.savez_compressed(path, layout=np.array(json.dumps(layout)), train_cases=np.int32(nt), eval_cases=np.int32(ne), **out)
    print('%s: %d training and %d evaluation cases, %d bytes' % (path, nt, ne, os.path.getsize(path)))


if __name__ == '__main__':
    main()
