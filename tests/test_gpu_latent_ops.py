"""GPU tests of the small kernels around the convolutions, through the C ABI (voxvae.lib), each against a float64 definition:
the latent-space ops of the missing-modality evaluation (vv_latent_mask_fill, vv_nearest_category, vv_latent_correct,
vv_category_accuracy), the stand-alone loss ops of src/module/function.py (vv_binary_loss, vv_voxel_precision_recall, vv_kl_loss,
vv_regulizer_loss, vv_sampling), vv_shape_metrics and vv_max_over_positions.

Every one of these kernels is a strided loop `for (i = lane; i < n; i += 64 or 256)` followed by a wave or block reduction, so the
sizes here make every such loop wrap and leave a ragged tail (more than 64 classes, latent above 64 and not a multiple of it, batch
above 64 / 256, voxel counts that are not a multiple of 256), and the inputs hold the values the comparisons turn on (exact ties,
-0.0, a probability exactly at the threshold, non-finite latents).  Every output buffer starts as NaN (int32 buffers as -1).

Error bounds are derived from the float32 operation count of the kernel's summation order and the reference's own intermediates
(U = 2^-24, the float32 unit roundoff); none is fitted to what the kernels give."""
import ctypes
import math

import numpy as np
import pytest
import torch

from oracle import numpy_oracle as no

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
U = 2.0 ** -24
NAN = float('nan')


@pytest.fixture(scope='module')
def L():
    from voxvae import lib
    lib.load()
    assert torch.cuda.is_available()
    return lib


def _st():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(DEV)


def _devi(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).to(DEV)


def _nan(*shape, dtype=torch.float32):
    return torch.full(shape, NAN, dtype=dtype, device=DEV)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


# ------------------------------------------------------------------------------------------- vv_nearest_category
def _nc_inputs(B, Lz, C, seed, kind, maskkind):
    rng = np.random.default_rng(seed)
    P = rng.standard_normal((C, Lz)).astype(np.float32)
    if kind == 'random':
        z = rng.standard_normal((B, Lz)).astype(np.float32)
    else:                                                  # clustered round a prototype
        z = (P[rng.integers(0, C, B)] + 0.1 * rng.standard_normal((B, Lz))).astype(np.float32)
    if maskkind == 'none':
        mask = None
    else:
        mask = (rng.random((B, Lz)) >= (0.9 if maskkind == 'sparse' else 0.5)).astype(np.float32)
        if maskkind == 'zero_rows':
            mask[::3] = 0.0
    return z, P, mask


def _nc_reference(z, P, mask):
    """(oracle index, float64 distances).  Asserts, on the reference alone, that no row is left to chance: with
    tol = (L + 2) 2^-23 (L sequential float32 adds of rounded products), every distance within tol * min of a row's minimum IS
    that minimum -- the row is either separated by more than tol, or an exact tie (distance 0, duplicated prototypes), where the
    float32 distances tie bit for bit as well.  On such rows a correct float32 kernel must give the oracle's (first) index."""
    z64, P64 = z.astype(np.float64), P.astype(np.float64)
    m64 = None if mask is None else mask.astype(np.float64)
    d = no.nearest_category_distances(z64, P64, m64)
    idx = no.nearest_category(z64, P64, m64)
    tol = (z.shape[1] + 2) * 2.0 ** -23
    dmin = d.min(axis=1, keepdims=True)
    near = d - dmin <= tol * dmin
    undecided = (near & (d != dmin)).any(axis=1)
    assert not undecided.any(), 'rows %s are closer than tol = %.2e: pick another seed' % (np.nonzero(undecided)[0][:8], tol)
    assert np.array_equal(idx, np.argmax(near, axis=1))
    return idx, d


def _nc_run(L, z, P, mask):
    B, Lz = z.shape
    zd, Pd, md = _dev(z), _dev(P), None if mask is None else _dev(mask)
    idx = torch.full((B,), -1, dtype=torch.int32, device=DEV)
    L.call('vv_nearest_category', L.ptr(zd), L.ptr(md), L.ptr(Pd), P.shape[0], L.ptr(idx), B, Lz, _st())
    torch.cuda.synchronize()
    return idx.cpu().numpy().astype(np.int64)


NC_CASES = [(256, 64, 200, 'random', 'none'), (256, 64, 200, 'clustered', 'half'), (300, 16, 40, 'random', 'half'),
            (300, 16, 40, 'clustered', 'none'), (65, 100, 129, 'random', 'none'), (65, 100, 129, 'random', 'zero_rows'),
            (256, 64, 64, 'random', 'sparse'), (256, 64, 64, 'clustered', 'zero_rows'), (1, 200, 65, 'random', 'none'),
            (1, 200, 65, 'clustered', 'half'), (65, 16, 1, 'random', 'half'), (300, 200, 200, 'clustered', 'zero_rows'),
            (65, 64, 40, 'random', 'none'), (1, 16, 129, 'clustered', 'none')]


@pytest.mark.parametrize('B,Lz,C,kind,maskkind', NC_CASES)
def test_nearest_category(L, B, Lz, C, kind, maskkind):
    z, P, mask = _nc_inputs(B, Lz, C, 1000 * B + 10 * Lz + C, kind, maskkind)
    ref, d = _nc_reference(z, P, mask)
    got = _nc_run(L, z, P, mask)
    assert got.min() >= 0 and got.max() < C
    bad = np.nonzero(got != ref)[0]
    assert bad.size == 0, 'rows %s: got %s, oracle %s' % (bad[:8], got[bad[:8]], ref[bad[:8]])
    if maskkind == 'zero_rows':
        assert np.all(d[::3] == 0) and np.all(got[::3] == 0)       # distance 0 to every class: the first


@pytest.mark.parametrize('maskkind', ['none', 'half'])
def test_nearest_category_exact_ties(L, maskkind):
    """Duplicated prototype rows tie exactly, in float64 and in float32 alike.  One class per lane step of 64: (6, 70) share a
    lane, (0, 128) share one two steps apart, (10, 21) sit in different lanes, and (50, 67) has its lower index in the higher
    lane (67 is lane 3).  The first index must win in every pair: inside a lane by the strict `<`, across lanes by the tie-break
    of the shuffle reduction."""
    C, Lz = 200, 64
    rng = np.random.default_rng(77)
    P = rng.standard_normal((C, Lz)).astype(np.float32)
    pairs = [(6, 70), (0, 128), (10, 21), (50, 67)]
    for lo, hi in pairs:
        P[hi] = P[lo]
    rows = np.repeat(np.arange(len(pairs)), 9)                      # nine latents round each duplicated prototype
    z = (P[[pairs[r][0] for r in rows]] + 0.1 * rng.standard_normal((rows.size, Lz))).astype(np.float32)
    mask = None if maskkind == 'none' else (rng.random(z.shape) >= 0.5).astype(np.float32)
    ref, d = _nc_reference(z, P, mask)
    first = np.array([pairs[r][0] for r in rows])
    second = np.array([pairs[r][1] for r in rows])
    assert np.array_equal(ref, first)                               # the reference itself: the pair is the minimum, the first wins
    assert np.all(d[np.arange(rows.size), first] == d[np.arange(rows.size), second])
    got = _nc_run(L, z, P, mask)
    assert np.array_equal(got, first), (got, first)


def _first_min_below_inf(d):
    """The contract for non-finite input, stated on the float64 distances: the first minimum over the distances below +inf
    (NaN is not), 0 for a row that has none."""
    valid = d < np.inf
    return np.where(valid.any(axis=1), np.argmin(np.where(valid, d, np.inf), axis=1), 0)


@pytest.mark.parametrize('masked', [False, True])
def test_nearest_category_non_finite(L, masked):
    """A diverged latent must give an index in [0, C), never the kernel's `nothing found yet` value.  The indices are read back and
    checked on the host only: nothing here hands them to vv_latent_correct."""
    C, Lz, B = 130, 64, 12
    rng = np.random.default_rng(5)
    P = rng.standard_normal((C, Lz)).astype(np.float32)
    z = (P[rng.integers(0, C, B)] + 0.1 * rng.standard_normal((B, Lz))).astype(np.float32)
    mask = (rng.random((B, Lz)) >= 0.3).astype(np.float32) if masked else None
    z[0, 3] = np.inf                                    # every distance +inf (NaN where the entry is masked: inf * 0)
    z[1, 70 % Lz] = np.nan                              # every distance NaN
    z[2, 0] = -np.inf
    z[3, :] = np.inf
    if masked:
        mask[0, 3], mask[2, 0] = 0.0, 1.0
    P[7, 5] = np.inf                                    # one +inf prototype entry: class 7 leaves the race, rows 4.. stay finite elsewhere
    z[4] = (P[7] + 0.01).astype(np.float32)             # ... also for the row that sat on it
    z[4, 5] = 0.0
    if masked:
        mask[4, 5] = 1.0
    with np.errstate(invalid='ignore', over='ignore'):
        d = no.nearest_category_distances(z.astype(np.float64), P.astype(np.float64), None if mask is None else mask.astype(np.float64))
    want = _first_min_below_inf(d)
    assert np.array_equal(want, no.nearest_category(z.astype(np.float64), P.astype(np.float64), None if mask is None else mask.astype(np.float64)))
    assert not (d[:4] < np.inf).any() and np.all(want[:4] == 0)
    assert not (d[:, 7] < np.inf).any() and (d[4:, :7] < np.inf).all() and np.all(want[4:] != 7)
    # the finite rows are decided by a margin no float32 rounding can close (clustered: a few percent of the runner-up)
    fin = np.where(d[4:] < np.inf, d[4:], np.inf)
    s = np.sort(fin, axis=1)
    assert np.all(s[:, 1] - s[:, 0] > 1e-3 * s[:, 0])
    got = _nc_run(L, z, P, mask)
    assert got.min() >= 0 and got.max() < C
    assert np.array_equal(got, want), (got, want)
    # every distance +inf through the prototypes instead: one +inf column
    P2 = P.copy()
    P2[:, 9] = np.inf
    z2 = z[4:].copy()
    m2 = None
    if masked:
        m2 = mask[4:].copy()
        m2[:, 9] = 1.0
    got2 = _nc_run(L, z2, P2, m2)
    assert np.all(got2 == 0), got2


# ------------------------------------------------------------------------------------------- vv_latent_mask_fill / vv_latent_correct
def _latent_inputs(B, Lz, C, seed):
    rng = np.random.default_rng(seed)
    z = rng.standard_normal((B, Lz)).astype(np.float32)
    r = rng.random((B, Lz))
    z[r < 0.05] = 0.0                                               # genuine zeros ...
    z[(r >= 0.05) & (r < 0.10)] = -0.0                              # ... of both signs
    mask = (rng.random((B, Lz)) >= 0.5).astype(np.float32)
    r = rng.random((B, Lz))
    mask[r < 0.05] = -0.0
    mask[(r >= 0.05) & (r < 0.10)] = 0.5                            # non-binary masks scale (fill) and count as `kept` (correct)
    mask[(r >= 0.10) & (r < 0.15)] = 2.0
    P = (1.0 + 3.0 * rng.standard_normal((C, Lz))).astype(np.float32)
    return rng, z, mask, P


def _act_buffer(L, act, B, Lz):
    if act == 'null':
        return None, L.VV_F32
    if act == 'f32':
        return _nan(B, Lz), L.VV_F32
    return _nan(B, Lz, dtype=torch.bfloat16), L.VV_BF16


def _check_act(act, buf, out):
    if act == 'f32':
        assert torch.equal(buf.view(torch.int32), out.view(torch.int32))
    elif act == 'bf16':
        assert torch.equal(buf.view(torch.int16), out.to(torch.bfloat16).view(torch.int16))


LATENT_SHAPES = [(8, 64, 40), (3, 100, 1), (65, 16, 200), (256, 200, 40), (1, 16, 40), (300, 64, 200)]    # B*L: 512, 300, 1040, 51200, 16, 19200


@pytest.mark.parametrize('act', ['null', 'f32', 'bf16'])
@pytest.mark.parametrize('B,Lz,C', LATENT_SHAPES)
def test_latent_mask_fill(L, B, Lz, C, act):
    rng, z, mask, P = _latent_inputs(B, Lz, C, 31 * B + Lz + C)
    zm = z * mask                                                   # float32; every mask value makes this product exact
    repl = zm == 0
    if B * Lz >= 256:
        assert ((z == 0) & (mask == 1)).any() and (np.signbit(zm) & repl).any() and (mask[~repl] == 0.5).any() and (mask[~repl] == 2.0).any()
    ref = no.latent_mask_fill(z.astype(np.float64), mask.astype(np.float64), P.astype(np.float64))
    assert np.array_equal(ref == P.astype(np.float64).mean(0)[None, :], repl)
    out = _nan(B, Lz)
    buf, adt = _act_buffer(L, act, B, Lz)
    zd, md, Pd = _dev(z), _dev(mask), _dev(P)
    L.call('vv_latent_mask_fill', L.ptr(zd), L.ptr(md), L.ptr(Pd), C, L.ptr(out), L.ptr(buf), adt, B, Lz, _st())
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    assert np.array_equal(_bits(got[~repl]), _bits(zm[~repl]))     # unreplaced: z * mask bit for bit
    # replaced (masked entries, -0.0, genuine zeros alike): the column mean of the prototypes, C sequential float32 adds and a division
    bound = np.broadcast_to((C + 1) * U * np.abs(P.astype(np.float64)).mean(0)[None, :], ref.shape)
    err = np.abs(got.astype(np.float64) - ref)
    assert np.all(err[repl] <= bound[repl]), (err[repl].max(), bound[repl].min())
    _check_act(act, buf, out)


@pytest.mark.parametrize('act', ['null', 'f32', 'bf16'])
@pytest.mark.parametrize('B,Lz,C', LATENT_SHAPES)
def test_latent_correct(L, B, Lz, C, act):
    rng, z, mask, P = _latent_inputs(B, Lz, C, 17 * B + Lz + C)
    idx = rng.integers(0, C, B).astype(np.int32)
    eps2 = rng.standard_normal((B, Lz)).astype(np.float32)
    corr = mask == 0                                                # 0.0 and -0.0; 0.5 and 2.0 keep z
    if B * Lz >= 256:
        assert (np.signbit(mask) & corr).any() and (~corr & (mask != 1)).any()
    out = _nan(B, Lz)
    buf, adt = _act_buffer(L, act, B, Lz)
    zd, md, Pd, id_, ed = _dev(z), _dev(mask), _dev(P), _devi(idx), _dev(eps2)
    L.call('vv_latent_correct', L.ptr(zd), L.ptr(md), L.ptr(Pd), L.ptr(id_), L.ptr(ed), L.ptr(out), L.ptr(buf), adt, B, Lz, _st())
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    assert np.array_equal(_bits(got[~corr]), _bits(z[~corr]))      # kept: z bit for bit (its zeros keep their sign)
    prior = P[idx] + eps2                                           # float32: P[idx] + sqrt(exp(0)) * eps2 is one rounded add
    assert np.array_equal(_bits(got[corr]), _bits(prior[corr]))
    ref = no.latent_correct(z.astype(np.float64), mask.astype(np.float64), P.astype(np.float64), idx, eps2.astype(np.float64))
    assert np.abs(got - ref).max() <= U * np.abs(ref).max()
    _check_act(act, buf, out)


# ------------------------------------------------------------------------------------------- vv_category_accuracy
@pytest.mark.parametrize('C', [1, 40, 200])
@pytest.mark.parametrize('B', [1, 63, 64, 65, 300])
def test_category_accuracy(L, B, C):
    for seed in range(3):
        rng = np.random.default_rng(100 * B + C + seed)
        oh = np.zeros((B, C), np.float32)
        oh[np.arange(B), rng.integers(0, C, B)] = 1.0
        oh[3::7] = 0.0                                              # all-zero rows: argmax 0
        if C > 1:
            for b in range(1, B, 5):                                # two equal maxima: the first wins
                a, c = sorted(rng.choice(C, 2, replace=False))
                oh[b] = 0.0
                oh[b, a] = oh[b, c] = 1.0
        label = np.argmax(oh, axis=1)
        idx = np.where(rng.random(B) < 0.5, label, rng.integers(0, C, B)).astype(np.int32)
        if B == 1 and C > 1:
            idx[0] = label[0] if seed else (label[0] + 1) % C       # one sample: a miss, then hits
        hits = int((idx == label).sum())
        assert no.category_accuracy(idx, oh) == hits / B
        acc = _nan(1)
        id_, od = _devi(idx), _dev(oh)
        L.call('vv_category_accuracy', L.ptr(id_), L.ptr(od), C, L.ptr(acc), B, _st())
        torch.cuda.synchronize()
        assert acc.cpu().numpy()[0] == np.float32(hits) / np.float32(B), (hits, B)     # a ratio of small integers: exact


# ------------------------------------------------------------------------------------------- composition through the model class
def test_getEval_missing_modality_100_classes():
    """One float32 getEval(missing_prob=0.5) at 16^3 with 100 category vectors and B = 9: the model path with more than 64
    classes, against the float64 definition with the same injected draws."""
    import voxvae
    from voxvae import synthetic as syn
    voxvae.set_default_dtype('f32')
    voxvae.set_default_device(DEV)
    import src.module.nolbo as nolbo
    D, Lz, B, C = 16, 64, 9, 100
    cfg = syn.make_config(D, Lz, True)
    ep, dp = syn.make_encoder_params(cfg['encoder']), syn.make_decoder_params(cfg['decoder'])
    m = nolbo.nolboSingleObject_modelnet_category_VAE(nolbo_structure=cfg)
    m._encoder.set_weights_dict(ep)
    m._decoder.set_weights_dict(dp)
    x, cats = syn.make_voxels(B, D, seed=21), syn.make_category_vectors(C, Lz, seed=23)
    oh = np.zeros((B, C), np.float32)
    eps, eps2, mask = syn.make_eps(B, Lz, seed=24), syn.make_eps(B, Lz, seed=25), syn.make_mask(B, Lz, 0.5, seed=26)
    ref, det = no.vae_get_eval(cfg, ep, dp, (x, x, oh), cats, eps, missing_prob=0.5, mask=mask, eps2=eps2, details=True)
    assert det['argmin_masked'].max() >= 64                         # classes that only a wrapped lane loop reaches
    # labels (they enter nothing but the two accuracies): some rows carry the class nearest to z, some the class nearest to z_corr, so
    # that neither accuracy is 0 or 1
    c64 = cats.astype(np.float64)
    near, near_c = no.nearest_category(det['z'], c64), no.nearest_category(det['z_corr'], c64)
    label = np.where(np.arange(B) % 2 == 0, near, np.where(np.arange(B) % 3 == 1, near_c, (near + 1) % C))
    oh[np.arange(B), label] = 1.0
    acc, acc_c = no.category_accuracy(near, oh), no.category_accuracy(near_c, oh)
    assert 0 < acc < 1 and 0 < acc_c < 1
    # the reference's own decisions are not marginal: a latent 2e-5 off cannot change a nearest class
    for zz, mm in ((det['z'], None), (det['z'], mask.astype(np.float64)), (det['z_corr'], None)):
        s = np.sort(no.nearest_category_distances(zz, cats.astype(np.float64), mm), axis=1)
        assert np.all(s[:, 1] - s[:, 0] > 1e-2)
    out = m.getEval(inputs=(x, x, oh), category_vectors=cats, missing_prob=0.5, _eps=eps, _mask=mask, _eps2=eps2)
    z, zc = np.array(m._z_category), np.array(m._z_category_corrected)
    np.testing.assert_allclose(z, det['z'], rtol=0, atol=2e-5)
    np.testing.assert_allclose(zc, det['z_corr'], rtol=0, atol=2e-5)
    # the masked argmin the model used, read off its corrected latent: the class whose prototype + eps2 sits in the masked entries
    prior = cats[None, :, :].astype(np.float64) + eps2[:, None, :]
    miss = (mask == 0)
    assert miss.any(axis=1).all()
    fits = np.array([[np.abs(prior[b, c][miss[b]] - zc[b][miss[b]]).max() <= 1e-6 for c in range(C)] for b in range(B)])
    assert np.all(fits.sum(axis=1) == 1)
    assert np.array_equal(np.argmax(fits, axis=1), det['argmin_masked'])
    assert np.float32(float(out[4])) == np.float32(acc) and np.float32(float(out[9])) == np.float32(acc_c)


# ------------------------------------------------------------------------------------------- vv_binary_loss / vv_voxel_precision_recall
def _probabilities(rng, B, V, thr, shift=0):
    """float32 probabilities: uniform, saturated sigmoids (logits N(0, 12)), and the values the clip and the threshold turn on."""
    p = rng.random((B, V)).astype(np.float32)
    sat = no.sigmoid(rng.normal(0.0, 12.0, (B, V)).astype(np.float32)).astype(np.float32)
    r = rng.random((B, V))
    p = np.where(r < 0.3, sat, p)
    t32 = np.float32(thr)
    special = [np.float32(0.0), np.float32(1.0), np.float32(1e-8), np.float32(1.0) - np.float32(1e-7), t32,
               np.nextafter(t32, np.float32(0.0)), np.nextafter(t32, np.float32(1.0))]
    for k, s in enumerate(special):
        p[(r >= 0.3 + 0.03 * k) & (r < 0.3 + 0.03 * (k + 1))] = s
    flat = p.reshape(-1)
    for k in range(min(flat.size, 2 * len(special))):              # also in the smallest cases
        flat[k] = special[(k + shift) % len(special)]
    return p


LOSS_PARAMS = [(0.5, 0, 0.5), (0.6, 0, 0.3), (1.0, 1, 0.5), (0.6, 1, 0.3)]         # gamma, b_range, threshold
# With b_range = 1 and target 0 the two products of a voxel have opposite signs and nearly cancel for q near 0.45 (gamma 0.6): the
# roundings of that voxel scale with the products, not with the term, so a bound in sum |term| holds only where one voxel does not carry
# the sample.  (256, 1) therefore skips that parameter set; at (1, 1) and (5, 1) the probabilities are the listed special values only.
LOSS_CASES = ([(B, V, k) for B, V in [(1, 1), (5, 1), (5, 255), (256, 257), (1, 1000), (5, 1000), (256, 1)] for k in range(4) if (B, V, k) != (256, 1, 3)]
              + [(256, 1000, 1), (5, 32 ** 3, 0), (5, 32 ** 3, 3), (256, 32 ** 3, 1), (1, 32 ** 3, 2), (5, 64 ** 3, 1), (1, 64 ** 3, 2),
                 (3, 64 ** 3, 0), (2, 64 ** 3, 3)])


@pytest.mark.parametrize('B,V,k', LOSS_CASES)
def test_binary_loss_and_counts(L, B, V, k):
    gamma, b_range, thr = LOSS_PARAMS[k]
    rng = np.random.default_rng(B * 7 + V + k)
    p = _probabilities(rng, B, V, thr, shift=B + V + k)
    y = (rng.random((B, V)) < 0.3).astype(np.float32)
    ref, terms = no.binary_loss_f32clip(p, y, epsilon=1e-7, gamma=gamma, b_range=bool(b_range))
    tp, fp, fn = no.voxel_precision_recall(y, p, prob=np.float32(thr))
    pd, yd = _dev(p), _dev(y)
    out, tpd, fpd, fnd = _nan(B), _nan(B), _nan(B), _nan(B)
    L.call('vv_binary_loss', L.ptr(pd), L.ptr(yd), 1e-7, gamma, float(b_range), L.ptr(out), B, V, _st())
    L.call('vv_voxel_precision_recall', L.ptr(yd), L.ptr(pd), thr, L.ptr(tpd), L.ptr(fpd), L.ptr(fnd), B, V, _st())
    torch.cuda.synchronize()
    # counts: integers below 2^24, exact in float32 whatever the order
    for name, g, r in (('tp', tpd, tp), ('fp', fpd, fp), ('fn', fnd, fn)):
        assert np.array_equal(g.cpu().numpy().astype(np.float64), r), name
    # loss: ceil(V/256) sequential adds per thread, eight tree steps, the roundings of one term, relative to sum |term| -- and
    # never looser than the rtol of 2e-5 the op has been held to: the factor is capped there (it exceeds it at 64^3).  The cap is on
    # sum |term| as well, which IS |loss| for b_range = 0; with b_range = 1 the terms have both signs and the loss can be a
    # thousandth of sum |term| (-0.89 against 1044 at B 256, V 257), where no summation is accurate relative to the loss itself.
    got = out.cpu().numpy().astype(np.float64)
    bound = min((math.ceil(V / 256) + 16) * U, 2e-5) * np.abs(terms).sum(-1)
    if not b_range:
        np.testing.assert_allclose(np.abs(terms).sum(-1), np.abs(ref), rtol=1e-12)
    err = np.abs(got - ref)
    print('\n[binary_loss B=%d V=%d gamma=%g b_range=%d] max err / bound = %.3f' % (B, V, gamma, b_range, (err / np.maximum(bound, 1e-300)).max()))
    assert np.all(err <= bound), (err.max(), bound[np.argmax(err)], ref[np.argmax(err)])


def _planted_positions(V):
    return [0, 255, 256, V - 257, V - 256, V - 1]


@pytest.mark.parametrize('V', [1000, 32 ** 3, 64 ** 3])
def test_binary_loss_planted_voxel(L, V):
    """The summation bound above is a few 1e-5 of the loss at 64^3 and would hide one dropped voxel among 262144.  With gamma = 1
    and a target that is 0 everywhere but at one voxel, every other term is exactly 0 (1 * 0 * log q + 0 * 1 * log(1 - q), both
    logarithms finite after the clip), so the loss IS -log(clip(p_v)): one logf, 4 ulp.  One sample per position: the first and
    last thread, the first wrap of the 256-thread loop, and both sides of the last full stride."""
    pos = _planted_positions(V)
    B = len(pos)
    rng = np.random.default_rng(V)
    p = _probabilities(rng, B, V, 0.5)
    y = np.zeros((B, V), np.float32)
    pv = np.array([0.37, 0.0, 0.9, 1e-3, 1.0, 0.5], np.float32)
    for b, v in enumerate(pos):
        y[b, v], p[b, v] = 1.0, pv[b]
    ref, terms = no.binary_loss_f32clip(p, y, epsilon=1e-7, gamma=1.0, b_range=False)
    assert np.all((terms != 0).sum(-1) == 1)
    q = np.clip(pv, np.float32(1e-7), np.float32(1.0) - np.float32(1e-7)).astype(np.float64)
    assert np.array_equal(ref, -np.log(q))
    pd, yd, out = _dev(p), _dev(y), _nan(B)
    L.call('vv_binary_loss', L.ptr(pd), L.ptr(yd), 1e-7, 1.0, 0.0, L.ptr(out), B, V, _st())
    torch.cuda.synchronize()
    got = out.cpu().numpy().astype(np.float64)
    ulp = np.spacing(np.abs(ref).astype(np.float32)).astype(np.float64)
    assert np.all(np.abs(got - ref) <= 4 * ulp), (got, ref)


@pytest.mark.parametrize('thr', [0.5, 0.3])
@pytest.mark.parametrize('V', [1000, 32 ** 3, 64 ** 3])
def test_precision_recall_planted_voxel(L, V, thr):
    """A single true positive, false positive and false negative at each of the positions above, nothing else set: the counts
    are (1, 0, 0), (0, 1, 0) and (0, 0, 1).  The false positive sits exactly at the threshold."""
    pos = _planted_positions(V)
    t32 = np.float32(thr)
    rng = np.random.default_rng(V + 1)
    for kind, want in (('tp', (1, 0, 0)), ('fp', (0, 1, 0)), ('fn', (0, 0, 1))):
        B = len(pos)
        p = (rng.random((B, V)) * thr * 0.999).astype(np.float32)
        p[:, ::5] = np.nextafter(t32, np.float32(0.0))              # just below the threshold: not occupied
        assert p.max() < t32
        y = np.zeros((B, V), np.float32)
        for b, v in enumerate(pos):
            y[b, v] = 0.0 if kind == 'fp' else 1.0
            p[b, v] = {'tp': np.float32(0.9), 'fp': t32, 'fn': np.nextafter(t32, np.float32(0.0))}[kind]
        r = no.voxel_precision_recall(y, p, prob=t32)
        assert all(np.all(a == w) for a, w in zip(r, want))
        pd, yd = _dev(p), _dev(y)
        outs = [_nan(B), _nan(B), _nan(B)]
        L.call('vv_voxel_precision_recall', L.ptr(yd), L.ptr(pd), thr, L.ptr(outs[0]), L.ptr(outs[1]), L.ptr(outs[2]), B, V, _st())
        torch.cuda.synchronize()
        for o, w in zip(outs, want):
            assert np.all(o.cpu().numpy() == np.float32(w)), (kind, [t.cpu().numpy() for t in outs])


# ------------------------------------------------------------------------------------------- vv_kl_loss / vv_sampling
@pytest.mark.parametrize('B', [1, 37, 256])
@pytest.mark.parametrize('Lz', [16, 64, 100, 200])
def test_kl_loss(L, B, Lz):
    rng = np.random.default_rng(B + Lz)
    m, mt = rng.standard_normal((B, Lz)).astype(np.float32), rng.standard_normal((B, Lz)).astype(np.float32)
    lv, lvt = rng.uniform(-10, 10, (B, Lz)).astype(np.float32), rng.uniform(-10, 10, (B, Lz)).astype(np.float32)
    lv.reshape(-1)[:4] = [-10.0, 10.0, -10.0, 10.0]                 # the corners of the clip range, on both sides
    lvt.reshape(-1)[:4] = [-10.0, 10.0, 10.0, -10.0]
    m64, mt64, lv64, lvt64 = (a.astype(np.float64) for a in (m, mt, lv, lvt))
    terms = 0.5 * (lvt64 - lv64) + (np.exp(lv64) + np.square(m64 - mt64)) / (2.0 * np.exp(lvt64)) - 0.5
    ref = no.kl_loss(m64, lv64, mt64, lvt64)
    np.testing.assert_allclose(terms.sum(-1), ref, rtol=1e-12)
    out = _nan(B)
    md, lvd, mtd, lvtd = _dev(m), _dev(lv), _dev(mt), _dev(lvt)
    L.call('vv_kl_loss', L.ptr(md), L.ptr(lvd), L.ptr(mtd), L.ptr(lvtd), L.ptr(out), B, Lz, _st())
    torch.cuda.synchronize()
    # ceil(L/64) sequential adds per lane, six tree steps, the roundings of one term (two expf, a division, four adds)
    bound = (math.ceil(Lz / 64) + 16) * U * np.abs(terms).sum(-1)
    err = np.abs(out.cpu().numpy().astype(np.float64) - ref)
    print('\n[kl_loss B=%d L=%d] max err / bound = %.3f' % (B, Lz, (err / bound).max()))
    assert np.all(err <= bound), (err.max(), bound[np.argmax(err)])


@pytest.mark.parametrize('n', [1, 255, 257, 256 * 64])
def test_sampling(L, n):
    rng = np.random.default_rng(n)
    mu, eps = rng.standard_normal(n).astype(np.float32), rng.standard_normal(n).astype(np.float32)
    lv = rng.uniform(-10, 10, n).astype(np.float32)
    lv[:2] = [-10.0, 10.0][:min(n, 2)]
    ref = no.sampling(mu.astype(np.float64), lv.astype(np.float64), eps.astype(np.float64))
    out = _nan(n)
    mud, lvd, ed = _dev(mu), _dev(lv), _dev(eps)
    L.call('vv_sampling', L.ptr(mud), L.ptr(lvd), L.ptr(ed), L.ptr(out), n, _st())
    torch.cuda.synchronize()
    mag = np.abs(mu.astype(np.float64)) + np.abs(np.sqrt(np.exp(lv.astype(np.float64))) * eps)
    ulp = np.spacing(mag.astype(np.float32)).astype(np.float64)
    err = np.abs(out.cpu().numpy().astype(np.float64) - ref)
    assert np.all(err <= 4 * ulp), (err / ulp).max()


# ------------------------------------------------------------------------------------------- vv_regulizer_loss
def _regulizer_reference(m, lv, cls, dist, S):
    """The oracle's loss and the bound its own intermediates allow.  S_ij = sum_l |m_i - m_j| / exp(lv_i / 2) is L float32 adds of
    quotients of three roundings each: e_ij = (L + 4) U S_ij.  With d = S - dist a pair inside the hinge contributes d^2, off by
    2 |d| e; the outer sum (ceil(B/256) adds per thread, eight tree steps, the roundings of d - dist and of the square) adds
    (ceil(B/256) + 16) U sum_j d^2.  Asserts that no pair sits within e of the hinge, where float32 and float64 could disagree on
    the side (exact duplicates aside: S = 0 on both sides)."""
    B, Lz = m.shape
    d = S - dist
    e = (Lz + 4) * U * S
    assert not ((np.abs(d) <= e) & (S != 0)).any(), 'a pair sits on the hinge: pick another dist'
    same = np.ones((B, B), bool) if cls is None else (np.abs(cls[:, None, :].astype(np.float64) - cls[None, :, :]).sum(-1) == 0)
    inside = same & (d <= 0)
    v = np.where(inside, d * d, 0.0)
    ref = no.regulizer_loss(m, lv, dist, cls)
    np.testing.assert_allclose(v.sum(-1), ref, rtol=1e-12, atol=0)
    bound = np.where(inside, 2 * np.abs(d) * e, 0.0).sum(-1) + (math.ceil(B / 256) + 16) * U * v.sum(-1)
    return ref, np.minimum(bound, 2e-5 * np.abs(ref) + 1e-4), inside         # never looser than rtol 2e-5, atol 1e-4


@pytest.mark.parametrize('B,Lz,cdim', [(1, 16, 0), (37, 64, 0), (37, 16, 5), (256, 16, 40), (256, 64, 0), (257, 64, 5), (257, 16, 0),
                                       (600, 16, 0), (600, 64, 40), (1, 64, 5)])
def test_regulizer_loss(L, B, Lz, cdim):
    rng = np.random.default_rng(B + Lz + cdim)
    m, lv = rng.standard_normal((B, Lz)).astype(np.float32), rng.standard_normal((B, Lz)).astype(np.float32)
    cls = None
    if cdim:
        cls = np.zeros((B, cdim), np.float32)
        cls[np.arange(B), rng.integers(0, cdim, B)] = 1.0
    if B > 1:                                                       # duplicated rows: distance 0, class included
        m[1], lv[1] = m[0], lv[0]
        m[B - 1], lv[B - 1] = m[B // 2], lv[B // 2]
        if cdim:
            cls[1], cls[B - 1] = cls[0], cls[B // 2]
    m64, lv64 = m.astype(np.float64), lv.astype(np.float64)
    S = (np.abs(m64[:, None, :] - m64[None, :, :]) / np.exp(0.5 * lv64)[:, None, :]).sum(-1)
    pos = np.sort(S[S > 0])
    dists = {'none': 0.0}
    if pos.size:
        # some: inside the widest gap of the lower tail of the pair distances, so that no pair sits on the hinge
        tail = pos[:max(2, pos.size // 50)]
        g = int(np.argmax(np.diff(tail)))
        dists['some'] = float(np.float32(0.5 * (tail[g] + tail[g + 1])))
        dists['all'] = float(np.float32(2.0 * pos[-1]))
    else:
        dists['all'] = 8.0
    md, lvd, cd = _dev(m), _dev(lv), None if cls is None else _dev(cls)
    for mode, dist in dists.items():
        ref, bound, inside = _regulizer_reference(m, lv, cls, dist, S)
        n_in = int(inside.sum())
        if mode == 'none':
            assert np.all(ref == 0)                                 # d = S > 0, or exactly 0 on the diagonal and the duplicates
        elif mode == 'all':
            assert n_in == (B * B if cls is None else int((np.abs(cls[:, None] - cls[None]).sum(-1) == 0).sum()))
        elif cls is None:
            assert B + 4 < n_in < B * B                             # some: more than the diagonal and the two duplicated pairs, not all
        out = _nan(B)
        L.call('vv_regulizer_loss', L.ptr(md), L.ptr(lvd), L.ptr(cd), dist, L.ptr(out), B, Lz, cdim, _st())
        torch.cuda.synchronize()
        err = np.abs(out.cpu().numpy().astype(np.float64) - ref)
        print('\n[regulizer_loss B=%d L=%d cdim=%d %s dist=%g] max err / bound = %.3f' % (B, Lz, cdim, mode, dist, (err / np.maximum(bound, 1e-300)).max()))
        assert np.all(err <= bound), (mode, err.max(), bound[np.argmax(err)], ref[np.argmax(err)])


# ------------------------------------------------------------------------------------------- vv_shape_metrics / vv_max_over_positions
@pytest.mark.parametrize('B', [1, 63, 64, 65, 256, 1000])
def test_shape_metrics(L, B):
    for seed in range(3):
        rng = np.random.default_rng(10 * B + seed)
        st = np.zeros((B, 4), np.float32)
        st[:, 0] = rng.uniform(100, 5000, B)
        st[:, 1:] = rng.integers(0, 3000, (B, 3))
        st[seed::4, 1:3] = 0.0                                      # TP + FP = 0: precision 0 through the 1e-10 guard, not NaN
        st[(seed + 1) % 5::5, 1] = 0.0
        st[(seed + 1) % 5::5, 3] = 0.0                              # TP + FN = 0
        st[(seed + 2) % 9::9, 1:] = 0.0                             # an empty target and an empty prediction: IoU 0 through max(., 1)
        s = st.astype(np.float64)
        tp, fp, fn = s[:, 1], s[:, 2], s[:, 3]
        terms = np.stack([s[:, 0], tp / (tp + fp + 1e-10), tp / (tp + fn + 1e-10), no.iou(tp, fp, fn)])
        assert np.isfinite(terms).all()
        ref = terms.mean(axis=1)
        assert abs(ref[1] - no.pr_rc(tp, fp, fn)[0]) < 1e-15 and abs(ref[2] - no.pr_rc(tp, fp, fn)[1]) < 1e-15
        out = _nan(4)
        sd = _dev(st)
        L.call('vv_shape_metrics', L.ptr(sd), L.ptr(out), B, _st())
        torch.cuda.synchronize()
        got = out.cpu().numpy().astype(np.float64)
        assert np.isfinite(got).all(), got
        # ceil(B/64) sequential adds per lane, six tree steps, the quotient, the guard and the division by B
        bound = (math.ceil(B / 64) + 10) * U * np.abs(terms).sum(axis=1) / B
        assert np.all(np.abs(got - ref) <= bound), (got, ref, bound)


@pytest.mark.parametrize('B,npos,C', [(37, 8, 128), (3, 64, 100), (1, 1, 7)])
@pytest.mark.parametrize('negative', [False, True])
def test_max_over_positions(L, B, npos, C, negative):
    rng = np.random.default_rng(B + npos + C)
    x = rng.standard_normal((B, npos, C)).astype(np.float32)
    if negative:
        x = -np.abs(x) - np.float32(0.5)                            # a running maximum that starts at 0 would show here
    out = _nan(B, C)
    xd = _dev(x)
    L.call('vv_max_over_positions', L.ptr(xd), L.ptr(out), B, npos, C, _st())
    torch.cuda.synchronize()
    assert np.array_equal(_bits(out.cpu().numpy()), _bits(x.max(axis=1)))


# ------------------------------------------------------------------------------------------- refusals
def _refusal_table(L):
    """name -> (arguments, indices of the required pointers, indices of the sizes, indices of the outputs).  Valid, tiny."""
    B, Lz, C, V = 2, 4, 3, 8
    f = lambda *s: torch.ones(*s, device=DEV)                       # noqa: E731
    i32 = lambda *s: torch.zeros(*s, dtype=torch.int32, device=DEV)  # noqa: E731
    iout = lambda *s: torch.full(s, -1, dtype=torch.int32, device=DEV)  # noqa: E731
    return {
        'vv_latent_mask_fill': ([f(B, Lz), f(B, Lz), f(C, Lz), C, _nan(B, Lz), _nan(B, Lz), L.VV_F32, B, Lz], [0, 1, 2, 4], [3, 7, 8], [4, 5]),
        'vv_nearest_category': ([f(B, Lz), f(B, Lz), f(C, Lz), C, iout(B), B, Lz], [0, 2, 4], [3, 5, 6], [4]),
        'vv_latent_correct': ([f(B, Lz), f(B, Lz), f(C, Lz), i32(B), f(B, Lz), _nan(B, Lz), _nan(B, Lz), L.VV_F32, B, Lz], [0, 1, 2, 3, 4, 5], [8, 9],
                              [5, 6]),
        'vv_category_accuracy': ([i32(B), f(B, C), C, _nan(1), B], [0, 1, 3], [2, 4], [3]),
        'vv_binary_loss': ([f(B, V) * 0.5, f(B, V), 1e-7, 0.6, 0.0, _nan(B), B, V], [0, 1, 5], [6, 7], [5]),
        'vv_voxel_precision_recall': ([f(B, V), f(B, V) * 0.5, 0.5, _nan(B), _nan(B), _nan(B), B, V], [0, 1, 3, 4, 5], [6, 7], [3, 4, 5]),
        'vv_kl_loss': ([f(B, Lz), f(B, Lz), f(B, Lz), f(B, Lz), _nan(B), B, Lz], [0, 1, 2, 3, 4], [5, 6], [4]),
        'vv_sampling': ([f(B * Lz), f(B * Lz), f(B * Lz), _nan(B * Lz), B * Lz], [0, 1, 2, 3], [4], [3]),
        'vv_regulizer_loss': ([f(B, Lz), f(B, Lz), f(B, C), 1.0, _nan(B), B, Lz, C], [0, 1, 4], [5, 6, 7], [4]),
        'vv_shape_metrics': ([f(B, 4), _nan(4), B], [0, 1], [2], [1]),
        'vv_max_over_positions': ([f(B, V, C), _nan(B, C), B, V, C], [0, 1], [2, 3, 4], [1]),
    }


def _raw(L, name, args):
    conv = [L.ptr(a) if isinstance(a, torch.Tensor) else a for a in args]
    return getattr(L.load(), name)(*conv, _st())


@pytest.mark.parametrize('name', ['vv_latent_mask_fill', 'vv_nearest_category', 'vv_latent_correct', 'vv_category_accuracy', 'vv_binary_loss',
                                  'vv_voxel_precision_recall', 'vv_kl_loss', 'vv_sampling', 'vv_regulizer_loss', 'vv_shape_metrics',
                                  'vv_max_over_positions'])
def test_refusals(L, name):
    """-1 for each required NULL pointer, -2 for each non-positive size, -3 for an activation dtype the two latent ops cannot
    write (anything but VV_F32 / VV_BF16 when z_act is given: an fp8-sized buffer would be overrun by float32 stores); nothing is
    launched, so the NaN-filled (-1 for int32) outputs are untouched."""
    args, ptrs, sizes, outs = _refusal_table(L)[name]
    for i in ptrs:
        a = list(args)
        a[i] = None
        assert _raw(L, name, a) == -1, (name, 'NULL argument', i)
    for i in sizes:
        for bad in (0, -1):
            a = list(args)
            a[i] = bad
            assert _raw(L, name, a) == -2, (name, 'size argument', i, bad)
    if name in ('vv_latent_mask_fill', 'vv_latent_correct'):
        k = {'vv_latent_mask_fill': 6, 'vv_latent_correct': 7}[name]
        assert args[k] == L.VV_F32 and isinstance(args[k - 1], torch.Tensor)      # z_act sits in front of act_dtype
        for bad in (L.VV_FP8, 3, -1):
            a = list(args)
            a[k] = bad
            assert _raw(L, name, a) == -3, (name, 'act_dtype', bad)
    torch.cuda.synchronize()
    for i in outs:
        o = args[i]
        assert bool(torch.isnan(o).all()) if o.dtype.is_floating_point else bool((o == -1).all()), (name, 'output', i)
    # the same arguments, unmodified, are accepted (the table is valid: each refusal above is due to the one argument changed)
    assert _raw(L, name, args) == 0
    torch.cuda.synchronize()
    for i in outs:
        o = args[i]
        assert not bool(torch.isnan(o.float()).any()) and (o.dtype.is_floating_point or bool((o >= 0).all())), (name, 'output', i)
