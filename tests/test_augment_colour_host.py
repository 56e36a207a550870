"""CPU tests of the two opt-in colour stages of the image pipeline (csrc/augment.h 1a, 1b through vv_augment_images_ex_host /
vv_augment_draw_ex_host): the blur against scipy, hue/saturation against the numpy restatements of tests/_augment_colour_ref.py, the
order of the four stages, the draws, refusals, datasetUtils.imgAug, and the new host loops as a stand-alone sanitizer program."""
import ctypes
import os

import numpy as np
import pytest
import torch
from scipy import ndimage

from _common import build_and_run_sanitized
import _augment_colour_ref as C
import _augment_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

from voxvae import augment as A          # noqa: E402
from voxvae import lib as L              # noqa: E402


@pytest.fixture(scope='module', autouse=True)
def built():
    from voxvae import build as vb
    return vb.build()


def levels_of(images, rows, colour, out_size):
    arena = A.ImageArena.from_arrays(images, device=None)
    out = A.augment_images(arena, np.stack(rows), out_size, colour=None if colour is None else np.stack(colour), host=True).numpy()
    lev = np.rint(out.astype(np.float64) * 255.0)
    assert np.array_equal((lev.astype(np.float32) / np.float32(255.0)), out)          # the output is level / 255 exactly
    return lev.astype(np.int64)


def identity(img, colour, **kw):
    """Identity warp, output size = crop size: the output levels are the source levels."""
    h, w = img.shape[:2]
    return levels_of([img], [A.make_params(rows=h, cols=w, **kw)], [colour], (h, w))[0]


# -------------------------------------------------------------------------------------------------------------- 1. blur against scipy
# (rows, cols, sigma): the issue's five, sigma on both sides of 0.125 where the radius goes from 0 to 1, one tile plus one pixel
BLUR_CASES = [(48, 64, 3.0), (2, 5, 3.0), (1, 1, 1.3), (7, 3, 0.4), (33, 17, 0.0011), (9, 11, 0.1249), (9, 11, 0.1251), (33, 33, 2.0)]


@pytest.mark.parametrize('h,w,sigma', BLUR_CASES)
def test_blur_against_scipy(h, w, sigma):
    """The twin's level is floor(v + 0.5) of scipy's float64 gaussian_filter(mode='mirror', truncate=4.0), except where v is within 1e-6
    of a tie; at most one value in 1000 may be excluded.  Observed: no exclusion and no difference in any case."""
    img = R.random_images(1000 * h + w, [(h, w)])[0]
    got = identity(img, A.make_colour(sigma=sigma, blur=True))
    sd = float(np.float32(sigma))
    want = np.stack([ndimage.gaussian_filter(img[..., c].astype(np.float64), sd, mode='mirror', truncate=4.0) for c in range(3)], axis=-1)
    tie = np.abs((want - np.floor(want)) - 0.5) < 1e-6
    print('%dx%d sigma %g: %d of %d values excluded, largest |restatement - scipy| %.3g' % (h, w, sigma, tie.sum(), tie.size,
                                                                                             np.abs(C.blur_real(img, sigma) - want).max()))
    assert tie.sum() * 1000 <= tie.size
    assert np.array_equal(got[~tie], np.clip(np.floor(want + 0.5), 0, 255).astype(np.int64)[~tie])
    assert C.radius(0.1249) == 0 and C.radius(0.1251) == 1
    if C.radius(sigma) == 0:
        assert np.array_equal(got, img)


def test_blur_acts_on_the_flipped_crop_with_its_pad_zeros():
    img = R.random_images(77, [(12, 10)])[0]
    kw = dict(row0=1, col0=2, rows=14, cols=9, flip=1, row_pad=2, col_pad=3)
    got = levels_of([img], [A.make_params(**kw)], [A.make_colour(sigma=1.5, blur=True)], (14, 9))[0]
    crop = R.source(img, 1, 2, 14, 9, flip=1, row_pad=2, col_pad=3)
    assert (crop == 0).any() and np.array_equal(got, C.blur(crop, 1.5))


# ------------------------------------------------------------------------------------------------- 2., 3. hue / saturation
def colour_set():
    """256 x 256 seeded random colours, with structured rows written over the first ones: all greys, v == r == g ties (and the other
    pairs), pure primaries and secondaries at every level."""
    img = np.random.default_rng(2024).integers(0, 256, (256, 256, 3), dtype=np.uint8)
    k = np.arange(256, dtype=np.uint8)
    z = np.zeros(256, dtype=np.uint8)
    low = (k // 3).astype(np.uint8)
    rows = [np.stack([k, k, k], -1), np.stack([k, k, low], -1), np.stack([k, low, k], -1), np.stack([low, k, k], -1),
            np.stack([k, z, z], -1), np.stack([z, k, z], -1), np.stack([z, z, k], -1), np.stack([k, k, z], -1), np.stack([z, k, k], -1),
            np.stack([k, z, k], -1)]
    for i, r in enumerate(rows):
        img[i] = r
    return img


# value 20 and -20 as drawn (hue = trunc(value * 180 / 255)); hue adds that wrap below 0 and past 179; saturation clamped at both ends
HUE_SAT = [(0, 0), (14, 20), (-14, -20), (179, 0), (-179, 0), (100, 255), (-100, -255), (7, -255), (90, 130)]


@pytest.fixture(scope='module')
def hue_sat_results():
    img = colour_set()
    return img, dict(((h, s), identity(img, A.make_colour(hue=h, sat=s, hue_sat=True))) for h, s in HUE_SAT)


@pytest.mark.parametrize('hue,sat', HUE_SAT)
def test_hue_saturation_against_the_numpy_restatement_exactly(hue, sat, hue_sat_results):
    img, res = hue_sat_results
    got, want = res[(hue, sat)], C.hue_sat(img, hue, sat)
    assert np.array_equal(got, want), '%d value(s) differ' % int((got != want).sum())
    h8, s8, _ = C.to_hsv8(img)
    if hue > 0:
        assert (h8 + hue > 179).any()
    if hue < 0:
        assert (h8 + hue < 0).any()
    if sat:
        assert ((s8 + sat > 255).any() if sat > 0 else (s8 + sat < 0).any())
    assert np.array_equal(got[0, :, 0], got[0, :, 1]) or sat > 0                      # greys stay grey unless saturation is added


F64_BOUND = 6.0


@pytest.mark.parametrize('hue,sat', HUE_SAT)
def test_hue_saturation_against_a_float64_hsv_chain(hue, sat, hue_sat_results):
    """Against colorsys arithmetic in float64 with the same adds and no 8-bit h, s.  Measured on this test's own colour set on the CPU,
    largest deviation in levels (mean) per (hue, sat): (0, 0) 5.0000 (0.33); (14, 20) 5.2153 (0.47); (-14, -20) 4.6873 (0.42);
    (179, 0) 5.2333 (0.36); (-179, 0) 5.3000 (0.36); (100, 255) 5.5089 (0.52); (-100, -255) and (7, -255) 0 (saturation 0: grey on both
    sides); (90, 130) 5.2965 (0.52).  The largest, 5.5089, rounded up to the next half level is the bound: 6.0.  It is H's quantum of
    2 degrees: a sixth of the hue circle is 30 H units for up to 255 levels."""
    img, res = hue_sat_results
    d = np.abs(res[(hue, sat)] - C.hue_sat64(img, hue, sat))
    print('hue %d sat %d: largest deviation %.4f levels, mean %.4f' % (hue, sat, d.max(), d.mean()))
    assert d.max() <= F64_BOUND


# ---------------------------------------------------------------------------------------------------------------------------- 4. order
def test_the_four_stages_compose_in_the_reference_order():
    img = R.random_images(31, [(21, 18)])[0]
    kw = dict(sigma=1.2, invert=0b011, add=(9, -10, 4), hue=-14, sat=-20)
    got = identity(img, A.make_colour(sigma=1.2, hue=-14, sat=-20, blur=True, hue_sat=True), invert=0b011, add=(9, -10, 4))
    assert np.array_equal(got, C.levels(img, 'biah', **kw))
    for other in ('biha', 'hbia', 'baih', 'iabh'):          # (invert alone commutes with the blur: both are affine in the levels)
        assert not np.array_equal(got, C.levels(img, other, **kw)), other


# ---------------------------------------------------------------------------------------------------------------------------- 5. draws
N = 20000


def _objects(n, seed=11):
    rng = np.random.default_rng(seed)
    sizes = [(40, 60), (33, 21), (128, 96), (7, 9)]
    arena = A.ImageArena.from_arrays([np.zeros(s + (3,), dtype=np.uint8) for s in sizes], device=None)
    idx = rng.integers(0, len(sizes), n).astype(np.int32)
    ext = np.array(sizes)[idx]
    c0, r0 = rng.uniform(0, ext[:, 1] - 3), rng.uniform(0, ext[:, 0] - 3)
    c1, r1 = c0 + 2.5 + rng.uniform(0, 1, n) * (ext[:, 1] - 3 - c0), r0 + 2.5 + rng.uniform(0, 1, n) * (ext[:, 0] - 3 - r0)
    return arena, idx, np.stack([c0, r0, c1, r1], axis=1).astype(np.float32)


def _bounds(n, q):
    """[lo, hi] for a count of n Bernoulli(q) trials: five binomial standard deviations about the mean (tests/test_augment_host.py)."""
    sd = np.sqrt(n * q * (1 - q))
    return n * q - 5 * sd, n * q + 5 * sd


def test_draw_ex_rows_flags_and_ranges():
    arena, idx, boxes = _objects(N)
    p, c = (t.numpy() for t in A.draw_params(arena, idx, boxes, True, step=0, host=True, seed=2024, colour=True))
    assert p.shape == (N, 16) and c.shape == (N, 4) and c.dtype == np.int32
    assert np.array_equal(p, A.draw_params(arena, idx, boxes, True, step=0, host=True, seed=2024).numpy())
    assert ((c[:, 0] & ~3) == 0).all()
    blur, hs = (c[:, 0] & 1) != 0, (c[:, 0] & 2) != 0
    for flag, q in ((blur, 0.25), (hs, 0.25), (blur & hs, 0.125)):               # the gate of slot 3 at 0.5, then each choice at 0.5
        lo, hi = _bounds(N, q)
        assert lo <= flag.sum() <= hi, (flag.sum(), lo, hi, q)
    sigma = c[:, 1:2].copy().view(np.float32)[:, 0]
    assert (sigma[~blur] == 0).all() and (c[~blur, 1] == 0).all() and (sigma >= 0).all() and (sigma < 3.0).all() and sigma[blur].max() > 2.9
    value = c[:, 3]
    assert (value[~hs] == 0).all() and (c[~hs, 2] == 0).all() and value[hs].min() == -20 and value[hs].max() == 20
    assert np.array_equal(c[:, 2], np.trunc(value * 180 / 255.0).astype(np.int32))
    counts = np.bincount(value[hs] + 20, minlength=41)
    lo, hi = _bounds(int(hs.sum()), 1 / 41.0)
    assert (counts >= lo).all() and (counts <= hi).all()


def test_draw_ex_without_augmentation_and_batch_independence():
    arena, idx, boxes = _objects(64)
    p, c = (t.numpy() for t in A.draw_params(arena, idx, boxes, False, step=3, host=True, seed=5, colour=True))
    assert (c == 0).all() and np.array_equal(p, A.draw_params(arena, idx, boxes, False, step=3, host=True, seed=5).numpy())
    d = lambda n, step, seed=31: A.draw_params(arena, idx[:n], boxes[:n], True, step=step, host=True, seed=seed, colour=True)[1].numpy()
    c9, c5 = d(9, 4), d(5, 4)
    assert np.array_equal(c9[:5], c5) and np.array_equal(c9, d(9, 4))
    c64 = d(64, 4)
    assert c64.any() and not np.array_equal(c64, d(64, 5)) and not np.array_equal(c64, d(64, 4, seed=32))
    bad = idx.copy()
    bad[2] = 4
    col = np.full((64, 4), 9, dtype=np.int32)
    par = np.zeros((64, 16), dtype=np.int32)
    hp = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    rc = L.load().vv_augment_draw_ex_host(hp(arena.host_meta), len(arena), hp(bad), hp(boxes), 64, 1, 31, A.offset(4, rank=0), hp(par), hp(col))
    assert rc == -2 and (col[2] == 0).all() and par[2, 0] == -1 and np.array_equal(np.delete(col, 2, 0), np.delete(c64, 2, 0))


# ------------------------------------------------------------------------------------------------------ 6. refusals and compatibility
def _ex_host(arena, rows, colour, out, max_rows, max_cols, ws_words=None):
    hp = lambda a: None if a is None else a.ctypes.data_as(ctypes.c_void_p)
    B = rows.shape[0]
    if ws_words is None:
        need = L.load().vv_augment_colour_workspace_bytes(max_rows, max_cols, B)
        assert need == 4 * max_rows * max_cols * B
        ws_words = need // 4
    ws = np.full(ws_words, 0x5A5A5A5A, dtype=np.uint32)
    return L.load().vv_augment_images_ex_host(hp(arena.host_data), hp(arena.host_meta), len(arena), hp(rows), B, out.shape[1], out.shape[2],
                                              hp(out), hp(colour), hp(ws), ws.nbytes, max_rows, max_cols)


BAD_COLOUR = [np.array([4, 0, 0, 0]), np.array([-1, 0, 0, 0]), A.make_colour(sigma=float('nan'), blur=True), A.make_colour(sigma=float('nan')),
              A.make_colour(sigma=-0.5, blur=True), A.make_colour(sigma=16.5, blur=True), A.make_colour(sigma=float('inf')),
              A.make_colour(hue=180, hue_sat=True), A.make_colour(hue=-180), A.make_colour(sat=256, hue_sat=True), A.make_colour(sat=-256)]


@pytest.mark.parametrize('k', range(len(BAD_COLOUR)))
def test_inadmissible_colour_rows_are_refused_before_anything_is_written(k):
    arena = A.ImageArena.from_arrays(R.random_images(5, [(9, 13)]), device=None)
    rows = np.stack([A.make_params(rows=9, cols=13)] * 2)
    colour = np.stack([A.make_colour(sigma=1.0, blur=True), BAD_COLOUR[k].astype(np.int32)])
    out = np.full((2, 4, 4, 3), -7.0, dtype=np.float32)
    assert _ex_host(arena, rows, colour, out, 9, 13) == -2 and bool((out == -7.0).all())
    with pytest.raises(L.VoxVaeError):
        A.augment_images(arena, rows, (4, 4), colour=colour, host=True)


def test_slab_size_workspace_size_and_null_arguments():
    arena = A.ImageArena.from_arrays(R.random_images(5, [(9, 13)]), device=None)
    rows = np.stack([A.make_params(rows=9, cols=13), A.make_params(rows=4, cols=5)])
    colour = np.stack([A.make_colour(hue=3, sat=4, hue_sat=True), A.make_colour(sigma=0.8, blur=True)])
    out = np.full((2, 4, 4, 3), -7.0, dtype=np.float32)
    assert _ex_host(arena, rows, colour, out, 9, 13) == 0 and bool((out != -7.0).all())                   # a slab exactly full
    want = out.copy()
    out[:] = -7.0
    assert _ex_host(arena, rows, colour, out, 13, 9) == 0 and np.array_equal(out, want)                   # the product counts, not the shape
    out[:] = -7.0
    assert _ex_host(arena, rows, colour, out, 29, 4) == -2 and bool((out == -7.0).all())                  # 116 words: one word too small
    assert _ex_host(arena, rows, colour, out, 4, 29) == -2 and bool((out == -7.0).all())
    unflagged = np.stack([A.make_colour(), A.make_colour(sigma=0.8, blur=True)])                          # an unflagged crop needs no slab
    assert _ex_host(arena, rows, unflagged, out, 4, 5) == 0
    out[:] = -7.0
    assert _ex_host(arena, rows, colour, out, 9, 13, ws_words=2 * 117 - 1) == -5 and bool((out == -7.0).all())
    assert _ex_host(arena, rows, colour, out, 0, 13, ws_words=8) == -2 and _ex_host(arena, rows, colour, out, 9, 40000, ws_words=8) == -2
    lib, hp = L.load(), lambda a: a.ctypes.data_as(ctypes.c_void_p)
    assert lib.vv_augment_images_ex_host(hp(arena.host_data), hp(arena.host_meta), 1, hp(rows), 2, 4, 4, hp(out), hp(colour), None, 0, 9, 13) == -1
    assert lib.vv_augment_colour_workspace_bytes(0, 4, 1) == 0 and lib.vv_augment_colour_workspace_bytes(4, 4, 0) == 0
    assert lib.vv_augment_colour_workspace_bytes(32767, 32767, 3) == 3 * 4 * 32767 * 32767


def test_no_table_and_a_table_of_zeros_are_the_existing_entry_bit_for_bit():
    img = R.random_images(7, [(23, 31), (40, 17)])
    arena = A.ImageArena.from_arrays(img, device=None)
    rows = np.stack([A.make_params(image=1, row0=3, col0=2, rows=30, cols=14, flip=3, scale=0.9, d_row=2, d_col=-1, invert=0b101, add=(5, -9, 0), row_pad=2, col_pad=4),
                     A.make_params(image=0, row0=0, col0=5, rows=23, cols=20, flip=1, scale=1.1, d_row=-3, d_col=1)])
    want = A.augment_images(arena, rows, (12, 9), host=True).numpy()
    zeros = np.zeros((2, 4), dtype=np.int32)
    assert np.array_equal(A.augment_images(arena, rows, (12, 9), colour=zeros, host=True).numpy(), want)
    out = np.full_like(want, -7.0)
    hp = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    assert L.load().vv_augment_images_ex_host(hp(arena.host_data), hp(arena.host_meta), 2, hp(rows), 2, 12, 9, hp(out), None, None, 0, 0, 0) == 0
    assert np.array_equal(out, want)
    # one flagged sample beside an unflagged one: the unflagged one keeps its bits
    mixed = np.stack([A.make_colour(), A.make_colour(sigma=2.0, hue=5, sat=7, blur=True, hue_sat=True)])
    got = A.augment_images(arena, rows, (12, 9), colour=mixed, host=True).numpy()
    assert np.array_equal(got[0], want[0]) and not np.array_equal(got[1], want[1])


def test_warped_and_resized_output_reads_the_finished_source_levels():
    """Scale and translation after the colour stages: the float64 restatement of warp and resize on the restated source levels."""
    img = R.random_images(12, [(37, 53)])
    p = A.make_params(rows=37, cols=53, flip=1, scale=0.8, d_row=1, d_col=-2, invert=0b100, add=(3, 0, -8))
    got = levels_of(img, [p], [A.make_colour(sigma=1.7, hue=9, sat=-12, blur=True, hue_sat=True)], (16, 24))[0]
    src = C.levels(R.source(img[0], 0, 0, 37, 53, flip=1), 'biah', sigma=1.7, invert=0b100, add=(3, 0, -8), hue=9, sat=-12)
    want = R.resize_cubic(R.warp(src.astype(np.float64), np.float32(0.8), 1, -2), 16, 24)
    d = np.abs(got - want)
    assert d.max() <= 1.0 and (d > 0).mean() <= 1e-3                                  # the bound of test_against_the_float64_restatement


# ---------------------------------------------------------------------------------------------------------------------- 7. datasetUtils
def test_imgAug_equals_the_twin_for_injected_choices():
    import src.dataset_loader.datasetUtils as U
    img = R.random_images(8, [(20, 44)])[0]
    ch = dict(sigma=1.25, invert=0b010, add=(4, 4, 4), value=-17)
    out = U.imgAug(img, crop=False, flip=False, choices=ch)
    assert out.dtype == np.uint8 and out.shape == img.shape
    hue = int(np.trunc(-17 * 180 / 255.0))
    assert np.array_equal(out, identity(img, A.make_colour(sigma=1.25, hue=hue, sat=-17, blur=True, hue_sat=True), invert=0b010, add=(4, 4, 4)))
    assert np.array_equal(out, C.levels(img, 'biah', sigma=1.25, invert=0b010, add=(4, 4, 4), hue=hue, sat=-17))
    only = U.imgAug(img, crop=False, flip=False, gaussianBlur=False, channelInvert=False, brightness=False, hueSat=True, choices=dict(value=20))
    assert np.array_equal(only, C.hue_sat(img, 14, 20))
    none = U.imgAug(img, crop=False, flip=False, gaussianBlur=False, channelInvert=False, brightness=False, hueSat=False)
    assert np.array_equal(none, img)
    np.random.seed(4)
    a = U.imgAug(img, crop=False, flip=False)
    np.random.seed(4)
    assert np.array_equal(a, U.imgAug(img, crop=False, flip=False)) and a.shape == img.shape and not np.array_equal(a, img)
    for kw in (dict(), dict(crop=False), dict(flip=False)):
        with pytest.raises(NotImplementedError):
            U.imgAug(img, **kw)


def test_image_random_augmentation_routes_through_imgAug_when_asked():
    import src.dataset_loader.datasetUtils as U
    img = R.random_images(8, [(20, 44)])[0]
    differ = 0
    for seed in range(12):
        np.random.seed(seed)
        base = U.imageRandomAugmentation(img, 16, 24)
        np.random.seed(seed)
        again = U.imageRandomAugmentation(img, 16, 24, colour_ops='invert_add')
        assert np.array_equal(base[0], again[0]) and base[1:] == again[1:]
        np.random.seed(seed)
        full = U.imageRandomAugmentation(img, 16, 24, colour_ops='all')
        assert full[0].shape == (16, 24, 3) and full[0].dtype == np.uint8 and full[1] == base[1] and full[3] == base[3]
        differ += not np.array_equal(full[0], base[0])
    assert differ >= 1
    with pytest.raises(ValueError):
        U.imageRandomAugmentation(img, 16, 24, colour_ops='blur')


# ---------------------------------------------------------------------------------------------------------------------- 8. sanitizers
@pytest.mark.skipif(torch.cuda.is_available(), reason='sanitizer programs run on CPU-only machines')
def test_standalone_sanitizer_build_of_the_colour_loops(tmp_path):
    """csrc/augment.h and tests/augment_colour_main.cpp as ONE program of its own under the address and undefined-behaviour sanitizers, run on the CPU."""
    build_and_run_sanitized('augment_colour_main.cpp', tmp_path, 'augment_colour_asan')
