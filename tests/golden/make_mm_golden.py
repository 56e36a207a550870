"""Records tests/golden/mm_latent.npz: what the REFERENCE's own nolboSingleObject.getEval computes between the head output and the
decoder input, and what its kl_loss / regulizer_loss give, on seeded arrays.

    python tests/golden/make_mm_golden.py --reference /path/to/the/reference/checkout

No test imports this file.  The reference's src/module/nolbo.py and src/module/function.py are imported by path; `tensorflow` and `cv2`
are replaced in sys.modules by stand-ins -- numpy float32 statements of the TensorFlow calls getEval and the two loss functions use --
and the reference's network modules by empty ones.  The sub-models are callables that return seeded arrays (the instance prior looks
its [B * I, C + I] input rows up in a seeded [C, I, Li] table).  Every `sampling` draw (tf.random.normal), the np.random.choice mask and
every tf.argmin (its distance rows and its result) are recorded.  Everything else is the reference's code under this interpreter's numpy.

numpy sums a row pairwise, the kernel in index order, so the fixture pins decisions only with margin: a case is redrawn when, in any
row an argmin compares, the two smallest distances d1 <= d2 lie within MARGIN_UNITS float32 units of d2 (100 units of 2^-23 d2; the two
summation orders differ by a few units at the widths used here).  More than 10 % redraws: the generator is wrong, and it stops.

Stored per case i: c{i}_dims (B, Lc, Li, C, I), c{i}_missing_prob, the inputs (c{i}_enc_out, _eps, _mask, _eps2, _prior_cat, _prior_inst,
_cat_onehot, _inst_onehot), the outputs (c{i}_z, _z_corrected, _idx [B, 2 or 4], _acc [2 or 3]) and, on the training arrays
(c{i}_mean_cp, _lv_cp, _mean_ip, _lv_ip, with the case's enc_out), c{i}_kl [B] and c{i}_reg [B].
"""
import argparse
import importlib.util
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
MARGIN_UNITS = 100.0
UNIT = 2.0 ** -23
# (B, Lc, Li, C, I, missing_prob)
CASES = [(1, 7, 12, 12, 10, 0.0), (1, 7, 12, 12, 10, 0.3), (2, 16, 5, 1, 1, 0.9), (2, 7, 12, 12, 10, 0.0), (5, 16, 5, 4, 3, 0.3),
         (5, 7, 12, 12, 10, 0.9), (5, 3, 9, 12, 1, 0.3), (72, 8, 8, 12, 10, 0.0), (72, 7, 12, 12, 10, 0.3), (72, 16, 5, 12, 10, 0.9),
         (72, 8, 8, 1, 10, 0.3)]


class T(np.ndarray):
    """An eager tensor's surface, as far as the reference uses it."""
    __hash__ = None

    def numpy(self):
        return np.asarray(self)

    def get_shape(self):
        return types.SimpleNamespace(as_list=lambda: list(self.shape))

    def __ne__(self, o):
        return True if o is None else np.ndarray.__ne__(self, o)

    def __eq__(self, o):
        return False if o is None else np.ndarray.__eq__(self, o)


def t(x):
    return np.asarray(x).view(T)


def _ints(s):
    return tuple(int(v) for v in np.asarray(s).ravel())


class Recorder(object):
    def __init__(self):
        self.reset(None)

    def reset(self, rng):
        self.rng, self.draws, self.argmins, self.masks = rng, [], [], []


def _stand_ins(rec):
    f32 = np.float32
    tf = types.ModuleType('tensorflow')
    tf.float32 = np.float32
    tf.convert_to_tensor = t
    tf.reshape = lambda x, shape: t(np.reshape(x, _ints(shape)))
    tf.tile = lambda x, m: t(np.tile(x, _ints(m)))
    tf.stack = lambda xs, axis=0: t(np.stack([np.asarray(x) for x in xs], axis=axis))
    tf.transpose = lambda x, perm: t(np.transpose(x, perm))
    tf.concat = lambda xs, axis=0: t(np.concatenate(xs, axis=axis))
    tf.clip_by_value = lambda x, clip_value_min, clip_value_max: t(np.minimum(np.maximum(x, f32(clip_value_min)), f32(clip_value_max)))
    tf.reduce_mean = lambda x, axis=None: t(np.mean(np.asarray(x), axis=axis, dtype=np.float32))
    tf.reduce_sum = lambda x, axis=None: t(np.sum(np.asarray(x), axis=axis, dtype=np.float32))
    tf.shape = lambda x: t(np.array(np.shape(x), dtype=np.int32))
    tf.where = lambda c, a, b: t(np.where(c, a, b))
    tf.ones_like = lambda x: t(np.ones_like(x))
    tf.zeros_like = lambda x: t(np.zeros_like(x))
    tf.square = lambda x: t(np.square(x))
    tf.abs = lambda x: t(np.abs(x))
    tf.exp = lambda x: t(np.exp(x))
    tf.sqrt = lambda x: t(np.sqrt(x))
    tf.equal = lambda a, b: t(np.equal(np.asarray(a), np.asarray(b)))
    tf.greater = lambda a, b: t(np.greater(np.asarray(a), np.asarray(b)))
    tf.greater_equal = lambda a, b: t(np.greater_equal(np.asarray(a), np.asarray(b)))
    tf.argmax = lambda x, axis=None: t(np.argmax(np.asarray(x), axis=axis))
    tf.cast = lambda x, dtype: t(np.asarray(x).astype(dtype))

    def argmin(x, axis=None):
        r = np.argmin(np.asarray(x), axis=axis)
        rec.argmins.append((np.array(x), np.array(r)))
        return t(r)

    def gather_nd(params, indices, batch_dims=0):
        assert batch_dims == 1
        p, ix = np.asarray(params), np.asarray(indices)
        return t(p[np.arange(p.shape[0]), ix[:, 0]])

    def normal(shape, mean=0.0, stddev=1.0, dtype=np.float32):
        d = (f32(mean) + f32(stddev) * rec.rng.standard_normal(_ints(shape)).astype(np.float32)).astype(np.float32)
        rec.draws.append(d.copy())
        return t(d)

    tf.argmin, tf.gather_nd = argmin, gather_nd
    tf.random = types.SimpleNamespace(normal=normal)
    tf.math = types.SimpleNamespace(log=lambda x: t(np.log(x)))
    tf.keras = types.SimpleNamespace(backend=types.SimpleNamespace(log=lambda x: t(np.log(x))))
    cv2 = types.ModuleType('cv2')
    return tf, cv2


def load_reference(path, rec):
    tf, cv2 = _stand_ins(rec)
    sys.modules['tensorflow'], sys.modules['cv2'] = tf, cv2
    for name in ('src', 'src.net_core', 'src.net_core.darknet', 'src.net_core.autoencoder3D', 'src.net_core.priornet', 'src.module'):
        sys.modules[name] = types.ModuleType(name)
    mods = {}
    for name, rel in (('src.module.function', 'function.py'), ('reference_nolbo', 'nolbo.py')):
        spec = importlib.util.spec_from_file_location(name, os.path.join(path, 'src', 'module', rel))
        mods[name] = importlib.util.module_from_spec(spec)
        sys.modules[name] = mods[name]
        spec.loader.exec_module(mods[name])
    return mods['reference_nolbo']


def draw_case(rng, B, Lc, Li, C, I):
    f = lambda x: np.ascontiguousarray(x, dtype=np.float32)
    prior_cat = f(rng.normal(0, 1.5, (C, Lc)))
    inst_table = f(rng.normal(0, 1.5, (C, I, Li)))
    cat, inst = rng.integers(0, C, B), rng.integers(0, I, B)
    lv = lambda n: np.where(rng.random((B, n)) < 0.1, rng.normal(0, 12.0, (B, n)), rng.normal(-2.0, 1.0, (B, n)))   # a tenth beyond the clip
    enc = np.concatenate([prior_cat[cat] + rng.normal(0, 0.7, (B, Lc)), lv(Lc), inst_table[cat, inst] + rng.normal(0, 0.7, (B, Li)), lv(Li)], axis=1)
    enc = f(np.round(enc * 4096.0) / 4096.0)
    tr = dict(mean_cp=f(prior_cat[cat] + rng.normal(0, 0.05, (B, Lc))), lv_cp=f(rng.normal(0, 0.3, (B, Lc))),
              mean_ip=f(inst_table[cat, inst] * 0.3), lv_ip=f(rng.normal(0, 0.3, (B, Li))))
    return dict(enc_out=enc, prior_cat=prior_cat, inst_table=inst_table, cat_onehot=f(np.eye(C)[cat]), inst_onehot=f(np.eye(I)[inst]), **tr)


def run_reference(ref, rec, d, dims, missing_prob, seed):
    B, Lc, Li, C, I = dims
    m = object.__new__(ref.nolboSingleObject)
    m._enc_backbone_str = {'z_category_dim': Lc, 'z_inst_dim': Li}
    m._encoder_backbone = lambda x, training=False: x
    m._encoder_head = lambda x, training=False: t(d['enc_out'])
    m._priornet_class = lambda x, training=False: (t(d['prior_cat']), t(np.zeros_like(d['prior_cat'])))

    def prior_inst(x, training=False):
        x = np.asarray(x)
        rows = d['inst_table'][np.argmax(x[:, :C], axis=1), np.argmax(x[:, C:], axis=1)]
        return t(rows), t(np.zeros_like(rows))

    m._priornet_inst = prior_inst
    m._decoder = lambda z, training=False: t(np.full((B, 2, 2, 2, 1), 0.25, np.float32))
    rec.reset(np.random.default_rng([seed, 1]))
    np.random.seed(seed % (2 ** 31))
    choice = np.random.choice

    def recording_choice(*a, **k):
        r = choice(*a, **k)
        rec.masks.append(np.array(r))
        return r

    np.random.choice = recording_choice
    try:
        vox = np.zeros((B, 2, 2, 2, 1), np.float32)
        out = m.getEval((np.zeros((B, 1), np.float32), vox, d['cat_onehot'], d['inst_onehot']), category_indices=np.identity(C),
                        inst_indices=np.identity(I), training=False, missing_prob=missing_prob)
    finally:
        np.random.choice = choice
    return m, out


def has_margins(rec):
    for dist, _ in rec.argmins:
        if dist.shape[-1] < 2:
            continue
        s = np.sort(dist.astype(np.float64), axis=-1)
        tied_at_zero = s[:, 1] == 0.0           # an all-masked row: every distance is exactly 0 in any summation order, index 0 wins
        if np.any((s[:, 1] - s[:, 0] <= MARGIN_UNITS * UNIT * s[:, 1]) & ~tied_at_zero):
            return False
    return True


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reference', required=True, help='the reference checkout (holds src/module/nolbo.py)')
    ap.add_argument('--out', default=os.path.join(HERE, 'mm_latent.npz'))
    a = ap.parse_args()
    rec = Recorder()
    ref = load_reference(os.path.abspath(a.reference), rec)
    store, drawn, redrawn = {}, 0, 0
    for i, (B, Lc, Li, C, I, mp) in enumerate(CASES):
        rng = np.random.default_rng([B, Lc, Li, C, I, int(mp * 10)])
        while True:
            d = draw_case(rng, B, Lc, Li, C, I)
            drawn += 1
            with np.errstate(all='ignore'):
                m, out = run_reference(ref, rec, d, (B, Lc, Li, C, I), mp, 1000 * i + drawn)
            if has_margins(rec):
                break
            redrawn += 1
            assert redrawn <= 0.1 * (len(CASES) + redrawn), 'more than 10 % of the cases were redrawn: the generator is wrong'
        k = 'c%d_' % i
        store[k + 'dims'] = np.asarray([B, Lc, Li, C, I], dtype=np.int64)
        store[k + 'missing_prob'] = np.asarray(mp, dtype=np.float64)
        for name in ('enc_out', 'prior_cat', 'cat_onehot', 'inst_onehot', 'mean_cp', 'lv_cp', 'mean_ip', 'lv_ip'):
            store[k + name] = d[name]
        store[k + 'prior_inst'] = np.ascontiguousarray(d['inst_table'][np.argmax(d['cat_onehot'], axis=1)])          # [B, I, Li]
        assert np.array_equal(store[k + 'prior_inst'], np.asarray(m._mean_inst_prior_tile))
        assert len(rec.draws) == (3 if mp > 0 else 2) and len(rec.argmins) == (4 if mp > 0 else 2) and len(rec.masks) == (1 if mp > 0 else 0)
        store[k + 'eps'] = np.concatenate(rec.draws[:2], axis=1)
        store[k + 'idx'] = np.stack([r for _, r in rec.argmins], axis=1).astype(np.int32)
        store[k + 'z'] = np.asarray(m._z, dtype=np.float32)
        if mp > 0:
            store[k + 'mask'] = rec.masks[0].reshape(B, Lc).astype(np.float32)
            store[k + 'eps2'] = rec.draws[2]
            store[k + 'z_corrected'] = np.asarray(m._z_corrected, dtype=np.float32)
            store[k + 'acc'] = np.asarray([out[4], out[5], out[10]], dtype=np.float32)
        else:
            store[k + 'acc'] = np.asarray([out[4], out[5]], dtype=np.float32)
        # the two loss functions on the same arrays, as fit calls them (:127-140)
        Tn = lambda x: t(x)
        mean_c, lv_c = d['enc_out'][:, :Lc], np.clip(d['enc_out'][:, Lc:2 * Lc], -10, 10).astype(np.float32)
        mean_i, lv_i = d['enc_out'][:, 2 * Lc:2 * Lc + Li], np.clip(d['enc_out'][:, 2 * Lc + Li:], -10, 10).astype(np.float32)
        kl = ref.kl_loss(mean=Tn(mean_c), logVar=Tn(lv_c), mean_target=Tn(d['mean_cp']), logVar_target=Tn(d['lv_cp'])) + \
            ref.kl_loss(mean=Tn(mean_i), logVar=Tn(lv_i), mean_target=Tn(d['mean_ip']), logVar_target=Tn(d['lv_ip']))
        reg = ref.regulizer_loss(z_mean=Tn(d['mean_cp']), z_logVar=Tn(d['lv_cp']), dist_in_z_space=3.0 * Lc) + \
            ref.regulizer_loss(z_mean=Tn(d['mean_ip']), z_logVar=Tn(d['lv_ip']), dist_in_z_space=3.0 * Li, class_input=Tn(d['cat_onehot']))
        store[k + 'kl'], store[k + 'reg'] = np.asarray(kl, dtype=np.float32), np.asarray(reg, dtype=np.float32)
        print('case %2d  B %3d Lc %2d Li %2d C %2d I %2d missing %.1f: acc %s' % (i, B, Lc, Li, C, I, mp, store[k + 'acc']))
    store['cases'] = np.asarray(len(CASES), dtype=np.int64)
    print('drawn %d, redrawn %d (%.1f %%)' % (drawn, redrawn, 100.0 * redrawn / drawn))
    assert redrawn <= 0.1 * drawn, 'more than 10 % of the cases were redrawn: the generator is wrong'
    np.savez_compressed(a.out, **store)
    print('wrote %s: %d bytes' % (a.out, os.path.getsize(a.out)))
    assert os.path.getsize(a.out) < 1000000


if __name__ == '__main__':
    main()
