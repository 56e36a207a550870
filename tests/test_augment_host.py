"""CPU tests of the image pipeline's host twins (csrc/augment.h through vv_augment_images_host / vv_augment_draw_host): exact cases against
numpy expressions, seeded random images against the float64 restatement tests/_augment_ref.py, the random draws, the reference-named
src.dataset_loader.datasetUtils.imageRandomAugmentation, and the header as a stand-alone sanitizer program."""
import os

import numpy as np
import pytest
import torch

from _common import build_and_run_sanitized
import _augment_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

from voxvae import augment as A          # noqa: E402
from voxvae import lib as L              # noqa: E402


@pytest.fixture(scope='module', autouse=True)
def built():
    from voxvae import build as vb
    return vb.build()


def run(images, rows, out_size):
    arena = A.ImageArena.from_arrays(images, device=None)
    return A.augment_images(arena, np.stack(rows), out_size, host=True).numpy()


def f255(levels):
    return np.asarray(levels, dtype=np.float32) / np.float32(255.0)


# ---------------------------------------------------------------------------------------------------------------- 1. exact cases
def test_identity_is_the_source_over_255():
    img = R.random_images(1, [(9, 13)])
    out = run(img, [A.make_params(rows=9, cols=13)], (9, 13))[0]
    assert out.dtype == np.float32 and np.array_equal(out, f255(img[0]))


@pytest.mark.parametrize('d_row,d_col', [(2, -3), (-1, 4), (0, 1), (9, 0)])
def test_unit_scale_integer_translation_shifts_zeros_in(d_row, d_col):
    img = R.random_images(2, [(9, 13)])
    out = run(img, [A.make_params(rows=9, cols=13, d_row=d_row, d_col=d_col)], (9, 13))[0]
    want = np.zeros((9, 13, 3), dtype=np.uint8)
    ys, xs = np.arange(9) - d_row, np.arange(13) - d_col
    oky, okx = (ys >= 0) & (ys < 9), (xs >= 0) & (xs < 13)
    want[np.ix_(oky, okx)] = img[0][np.ix_(ys[oky], xs[okx])]
    assert np.array_equal(out, f255(want))


@pytest.mark.parametrize('flip', [1, 2, 3])
def test_each_flip_bit(flip):
    img = R.random_images(3, [(12, 10)])
    crop = img[0][2:9, 1:7]
    out = run(img, [A.make_params(row0=2, col0=1, rows=7, cols=6, flip=flip)], (7, 6))[0]
    want = crop[:, ::-1] if flip & 1 else crop
    want = want[::-1] if flip & 2 else want
    assert np.array_equal(out, f255(want))


def test_invert_and_add_on_a_ramp_hit_both_clamps():
    ramp = np.arange(256, dtype=np.uint8).reshape(16, 16)
    img = [np.stack([ramp, ramp, ramp], axis=-1)]
    out = run(img, [A.make_params(rows=16, cols=16, invert=0b010, add=(10, -10, -7))], (16, 16))[0]
    r = ramp.astype(np.int64)
    want = np.stack([np.clip(r + 10, 0, 255), np.clip(255 - r - 10, 0, 255), np.clip(r - 7, 0, 255)], axis=-1)
    assert want[..., 0].max() == 255 and want[..., 1].min() == 0 and (want[..., 0] == 255).sum() > 1 and (want[..., 1] == 0).sum() > 1
    assert np.array_equal(out, f255(want))


def test_a_pad_of_three_reads_zeros():
    img = R.random_images(4, [(5, 6)])
    out = run(img, [A.make_params(rows=11, cols=12, row_pad=3, col_pad=3)], (11, 12))[0]
    assert np.array_equal(out, f255(np.pad(img[0], ((3, 3), (3, 3), (0, 0)))))
    part = run(img, [A.make_params(row0=2, col0=4, rows=5, cols=7, row_pad=3, col_pad=3)], (5, 7))[0]
    assert np.array_equal(part, f255(np.pad(img[0], ((3, 3), (3, 3), (0, 0)))[2:7, 4:11]))


# ------------------------------------------------------------------------------------------------- 2. against the float64 restatement
ORACLE_CASES = [((5, 7), (8, 8)), ((37, 53), (16, 24)), ((200, 200), (8, 8))]


@pytest.mark.parametrize('src,dst', ORACLE_CASES)
@pytest.mark.parametrize('s,d_row,d_col', [(0.8, 1, -2), (1.2, -1, 2)])
def test_against_the_float64_restatement(src, dst, s, d_row, d_col):
    """No value more than one level off, at most 1e-3 of a case's values different at all.  Observed with the float64 header: none."""
    img = R.random_images(100 + src[0], [src])
    p = A.make_params(rows=src[0], cols=src[1], scale=s, d_row=d_row, d_col=d_col)
    worst, share = R.compare_levels(run(img, [p], dst)[0], R.chain_of_row(img, p, *dst))
    print('%s -> %s s %.1f: largest difference %g level(s), share of differing values %.2e' % (src, dst, s, worst, share))
    assert worst <= 1.0 and share <= 1e-3


def test_crop_flip_colour_and_pad_together_against_the_restatement():
    img = R.random_images(7, [(23, 31), (40, 17)])
    rows = [A.make_params(image=1, row0=3, col0=2, rows=30, cols=14, flip=3, scale=0.9, d_row=2, d_col=-1, invert=0b101, add=(5, -9, 0), row_pad=2, col_pad=4),
            A.make_params(image=0, row0=0, col0=5, rows=23, cols=20, flip=1, scale=1.1, d_row=-3, d_col=1)]
    out = run(img, rows, (12, 9))
    for got, p in zip(out, rows):
        worst, share = R.compare_levels(got, R.chain_of_row(img, p, 12, 9))
        assert worst <= 1.0 and share <= 1e-3


# ---------------------------------------------------------------------------------------------------------------------- 3. refusals
@pytest.mark.parametrize('field', [dict(image=2), dict(image=-1), dict(rows=0), dict(cols=0), dict(row0=1), dict(col0=-1), dict(cols=14),
                                   dict(scale=0.0), dict(scale=-1.0), dict(scale=float('nan')), dict(scale=float('inf'))])
def test_inadmissible_rows_are_refused_before_anything_is_written(field):
    img = R.random_images(5, [(9, 13), (4, 4)])
    arena = A.ImageArena.from_arrays(img, device=None)
    kw = dict(rows=9, cols=13)
    kw.update(field)
    rows = np.stack([A.make_params(rows=9, cols=13), A.make_params(**kw)])
    out = np.full((2, 4, 4, 3), -7.0, dtype=np.float32)
    hp = lambda a: a.ctypes.data_as(L.ctypes.c_void_p)
    rc = L.load().vv_augment_images_host(hp(arena.host_data), hp(arena.host_meta), 2, hp(rows), 2, 4, 4, hp(out))
    assert rc == -2 and bool((out == -7.0).all())
    assert L.load().vv_augment_check_host(hp(arena.host_meta), 2, hp(rows), 2) == -2
    for bad in ((0, 4), (4, 0)):
        assert L.load().vv_augment_images_host(hp(arena.host_data), hp(arena.host_meta), 2, hp(rows[:1].copy()), 1, bad[0], bad[1], hp(out)) == -2
    assert L.load().vv_augment_images_host(None, hp(arena.host_meta), 2, hp(rows), 2, 4, 4, hp(out)) == -1
    with pytest.raises(L.VoxVaeError):
        A.augment_images(arena, rows, (4, 4), host=True)


# ------------------------------------------------------------------------------------------------------------------------- 4. draws
N = 4096


def _objects(n, seed=11):
    rng = np.random.default_rng(seed)
    sizes = [(40, 60), (33, 21), (128, 96), (7, 9)]
    arena = A.ImageArena.from_arrays([np.zeros(s + (3,), dtype=np.uint8) for s in sizes], device=None)
    idx = rng.integers(0, len(sizes), n).astype(np.int32)
    ext = np.array(sizes)[idx]
    c0, r0 = rng.uniform(0, ext[:, 1] - 3), rng.uniform(0, ext[:, 0] - 3)
    c1, r1 = c0 + 2.5 + rng.uniform(0, 1, n) * (ext[:, 1] - 3 - c0), r0 + 2.5 + rng.uniform(0, 1, n) * (ext[:, 0] - 3 - r0)
    return arena, idx, np.stack([c0, r0, c1, r1], axis=1).astype(np.float32), ext


def test_no_augmentation_gives_the_fixed_values():
    arena, idx, boxes, ext = _objects(64)
    p = A.draw_params(arena, idx, boxes, False, step=3, host=True, seed=5).numpy()
    b = boxes.astype(np.float32)
    wd, ht = b[:, 2] - b[:, 0], b[:, 3] - b[:, 1]
    tenth = np.float32(0.1)
    cmin, cmax = np.maximum(0, b[:, 0] - wd * tenth), np.minimum(ext[:, 1].astype(np.float32), b[:, 2] + wd * tenth)
    rmin, rmax = np.maximum(0, b[:, 1] - ht * tenth), np.minimum(ext[:, 0].astype(np.float32), b[:, 3] + ht * tenth)
    assert np.array_equal(p[:, 0], idx)
    assert np.array_equal(p[:, 1], rmin.astype(np.int32)) and np.array_equal(p[:, 2], cmin.astype(np.int32))
    assert np.array_equal(p[:, 3], rmax.astype(np.int32) - rmin.astype(np.int32)) and np.array_equal(p[:, 4], cmax.astype(np.int32) - cmin.astype(np.int32))
    assert (p[:, 5] == 0).all() and (p[:, 6] == A.scale_bits(1.0)).all() and (p[:, 7:16] == 0).all()
    assert np.array_equal(p, A.draw_params(arena, idx, boxes, False, step=9, host=True, seed=77).numpy())      # nothing random in it


def _bounds(n, q):
    """[lo, hi] for a count of n Bernoulli(q) trials: five binomial standard deviations about the mean."""
    sd = np.sqrt(n * q * (1 - q))
    return n * q - 5 * sd, n * q + 5 * sd


def test_ranges_crops_and_gate_frequencies():
    arena, idx, boxes, ext = _objects(N)
    p = A.draw_params(arena, idx, boxes, True, step=0, host=True, seed=2024).numpy()
    assert p.shape == (N, 16) and np.array_equal(p[:, 0], idx)
    row0, col0, h, w = p[:, 1], p[:, 2], p[:, 3], p[:, 4]
    assert (row0 >= 0).all() and (col0 >= 0).all() and (h >= 1).all() and (w >= 1).all()
    assert (row0 + h <= ext[:, 0]).all() and (col0 + w <= ext[:, 1]).all()
    # the crop holds the box's whole pixels and at most the box widened by 0.2
    assert (col0 <= np.floor(boxes[:, 0])).all() and (col0 + w >= np.floor(boxes[:, 2])).all()
    assert (col0 >= np.floor(boxes[:, 0] - 0.2 * (boxes[:, 2] - boxes[:, 0]) - 1e-3).clip(0)).all()
    s = p[:, 6:7].copy().view(np.float32)[:, 0]
    assert (s >= np.float32(0.8)).all() and (s <= np.float32(1.2)).all()
    mr, mc = (np.float32(0.2) * h.astype(np.float32)).astype(np.int32), (np.float32(0.2) * w.astype(np.float32)).astype(np.int32)
    assert (p[:, 7] >= -mr).all() and (p[:, 7] <= np.maximum(mr - 1, 0)).all() and (p[:, 8] >= -mc).all() and (p[:, 8] <= np.maximum(mc - 1, 0)).all()
    assert ((p[:, 5] & ~3) == 0).all() and not ((p[:, 5] & 2) & ~((p[:, 5] & 1) << 1)).any()      # vertical only within horizontal
    assert ((p[:, 9] & ~7) == 0).all() and (np.abs(p[:, 10:13]) <= 10).all() and (p[:, 13:] == 0).all()
    assert p[:, 10:13].min() == -10 and p[:, 10:13].max() == 10
    assert p[:, 7].min() < 0 < p[:, 7].max() and p[:, 8].min() < 0 < p[:, 8].max()

    def inside(count, n, q):
        lo, hi = _bounds(n, q)
        return lo <= count <= hi

    hflip = (p[:, 5] & 1) != 0
    assert inside(hflip.sum(), N, 0.5)                                    # P(u > 0.5)
    assert inside(((p[:, 5] & 2) != 0).sum(), N, 0.25)                    # within the horizontal flip
    assert inside((s != 1.0).sum(), N, 0.5)                               # scalePr (s == 1 exactly has probability 2^-24 under the gate)
    big = (mr >= 3) & (mc >= 3)                                           # translation gate: P(d == (0, 0) | gated) <= 1 / 36 there
    moved = ((p[:, 7] != 0) | (p[:, 8] != 0)) & big
    lo, hi = _bounds(int(big.sum()), 0.5)
    assert lo * (1 - 1 / 36.0) - 1 <= moved.sum() <= hi
    # invert is enabled with probability 0.5 * 0.5 and then each channel with 0.05: per channel N independent trials at 0.0125
    for c in range(3):
        assert inside(((p[:, 9] >> c) & 1).sum(), N, 0.25 * 0.05)
    # Add is enabled with probability 0.25; a zero triple under it has probability 0.5 / 21 + 0.5 / 21^3
    q_add = 0.25 * (1 - (0.5 / 21 + 0.5 / 21 ** 3))
    assert inside((p[:, 10:13] != 0).any(axis=1).sum(), N, q_add)
    same = (p[:, 10] == p[:, 11]) & (p[:, 11] == p[:, 12]) & (p[:, 10] != 0)
    assert inside(same.sum(), N, 0.25 * (0.5 * 20 / 21 + 0.5 * 20 / 21 ** 3))       # one value for all channels


def test_a_sample_does_not_depend_on_the_batch_and_counters_repeat():
    arena, idx, boxes, _ = _objects(9)
    d = lambda n, step, seed=31: A.draw_params(arena, idx[:n], boxes[:n], True, step=step, host=True, seed=seed).numpy()
    p9, p5 = d(9, 4), d(5, 4)
    assert np.array_equal(p9[:5], p5)
    assert np.array_equal(p9, d(9, 4))
    assert not np.array_equal(p9, d(9, 5)) and not np.array_equal(p9, d(9, 4, seed=32))
    assert A.offset(4, rank=0) == 2 << 56 | 4 and A.offset(4, rank=3) == 2 << 56 | 3 << 40 | 4


def test_the_seed_follows_manual_seed():
    import voxvae
    arena, idx, boxes, _ = _objects(6)
    voxvae.manual_seed(99)
    try:
        a = A.draw_params(arena, idx, boxes, True, step=1, host=True).numpy()
        assert np.array_equal(a, A.draw_params(arena, idx, boxes, True, step=1, host=True, seed=99).numpy())
    finally:
        voxvae.manual_seed(None)


def test_draw_refuses_a_bad_index_and_an_empty_box():
    arena, idx, boxes, _ = _objects(4)
    bad = idx.copy()
    bad[2] = 4
    with pytest.raises(L.VoxVaeError):
        A.draw_params(arena, bad, boxes, True, step=0, host=True, seed=1)
    empty = boxes.copy()
    empty[1] = (5.2, 3.0, 5.4, 9.0)
    with pytest.raises(L.VoxVaeError):
        A.draw_params(arena, idx, empty, False, step=0, host=True, seed=1)


# --------------------------------------------------------------------------------------------------- 5. datasetUtils (reference names)
def test_image_random_augmentation_returns_the_six_tuple():
    import src.dataset_loader.datasetUtils as U
    img = R.random_images(8, [(20, 44)])[0]
    np.random.seed(3)
    out = U.imageRandomAugmentation(img, 16, 24)
    assert len(out) == 6
    image, row_pad, d_row, col_pad, d_col, s = out
    assert image.shape == (16, 24, 3) and image.dtype == np.uint8
    assert row_pad >= 0 and col_pad >= 0 and 0.8 <= s <= 1.2 and isinstance(d_row, int) and isinstance(d_col, int)
    np.random.seed(3)
    again = U.imageRandomAugmentation(img, 16, 24)
    assert np.array_equal(image, again[0]) and out[1:] == again[1:]
    # the padding=True geometry (datasetUtils.py:105-126): 20 x 44 into 16 x 24 expects 29.33 x 44, so int(9.33 / 2) rows on each side
    assert (row_pad, col_pad) == (4, 0)
    assert U.natural_keys('img12_3.png') == ['img', 12, '_', 3, '.png']


@pytest.mark.parametrize('padding', [False, True])
def test_image_random_augmentation_without_randomness_is_a_cubic_resize(padding):
    import src.dataset_loader.datasetUtils as U
    img = R.random_images(9, [(37, 53)])[0]
    image, row_pad, d_row, col_pad, d_col, s = U.imageRandomAugmentation(img, 16, 24, padding=padding, imAugPr=0.0, transPr=0.0, scalePr=0.0)
    assert (d_row, d_col, s) == (0, 0, 1.0)
    if not padding:
        assert (row_pad, col_pad) == (0, 0)
    want = R.resize_cubic(np.pad(img, ((row_pad, row_pad), (col_pad, col_pad), (0, 0))).astype(np.float64), 16, 24)
    d = np.abs(image.astype(np.float64) - want)
    assert d.max() <= 1.0 and (d > 0).mean() <= 1e-3


# ---------------------------------------------------------------------------------------------------------------------- 6. sanitizers
@pytest.mark.skipif(torch.cuda.is_available(), reason='sanitizer programs run on CPU-only machines')
def test_standalone_sanitizer_build(tmp_path):
    """csrc/augment.h and tests/augment_main.cpp as ONE program of its own under the address and undefined-behaviour sanitizers, run on the CPU."""
    build_and_run_sanitized('augment_main.cpp', tmp_path, 'augment_asan')
