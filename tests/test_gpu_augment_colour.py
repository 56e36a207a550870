"""GPU tests of the colour pre-pass (csrc/augment.hip: vv_augment_images_ex, vv_augment_draw_ex): both device entries against their host
twins bit for bit, memory discipline between sentinels with a poisoned workspace, what the two launches do with a row they must refuse,
and the colour_ops='all' setting of src.dataset_loader.pascal3D.deviceDataLoaderSingleObject and train_pascal.py."""
import ctypes

import numpy as np
import pytest
import torch

import _augment_ref as R

pytestmark = pytest.mark.gpu
DEV = 'cuda'
OUT = (20, 24)                           # two ragged 16 x 16 output tiles in each direction

from voxvae import augment as A          # noqa: E402
from voxvae import lib as L              # noqa: E402


def _blur(sigma, **kw):
    return A.make_colour(sigma=sigma, blur=True, **kw)


def _p(src, image, **kw):
    return A.make_params(image=image, rows=src[0], cols=src[1], **kw)


# name -> (image sizes, params rows, colour rows): batches of at most 8
def _cases():
    one = [(48, 64), (2, 5), (1, 1), (7, 3), (33, 17), (9, 11), (9, 11), (33, 33)]          # the host test's blur cases
    sig = [3.0, 3.0, 1.3, 0.4, 0.0011, 0.1249, 0.1251, 2.0]
    more = [(70, 33), (40, 29), (37, 53), (37, 53), (37, 45), (23, 31)]
    return {
        'blur cases': (one, [_p(s, i) for i, s in enumerate(one)], [_blur(g) for g in sig]),
        'halos, flip, warp, direct': (more, [
            _p(more[0], 0),                                                                  # sigma 3: halos of 12 cross the tile edges
            _p(more[1], 1, flip=3),                                                          # both flips under the blur
            _p(more[2], 2, scale=0.8, d_row=1, d_col=-2, invert=0b101, add=(5, -9, 0)),
            _p(more[3], 3, scale=1.2, d_row=-1, d_col=2, flip=1),
            _p(more[4], 4, scale=0.9, d_row=2, d_col=1),                                     # radius 14 > 12: the direct form
            A.make_params(image=5, row0=3, col0=2, rows=24, cols=30, row_pad=2, col_pad=4, flip=2, add=(0, 10, -10)),
        ], [_blur(3.0), _blur(2.2, hue=-14, sat=-20, hue_sat=True), _blur(1.1, hue=14, sat=20, hue_sat=True),
            A.make_colour(hue=100, sat=-60, hue_sat=True), _blur(3.5, hue=3, sat=3, hue_sat=True), _blur(0.8)]),
        'flagged beside unflagged': ([(37, 53), (64, 64), (23, 31)], [
            _p((37, 53), 0, scale=0.9, d_row=2, d_col=3, invert=1), _p((64, 64), 1), _p((23, 31), 2, flip=1, add=(3, 3, 3)),
            _p((64, 64), 1, scale=1.1), _p((37, 53), 0)],
            [A.make_colour(), _blur(2.9, hue=-3, sat=9, hue_sat=True), A.make_colour(), A.make_colour(sigma=2.0), _blur(16.0)]),   # radius 64
    }


@pytest.fixture(scope='module')
def host_results():
    """The host twin's output for every case, computed once."""
    out = {}
    for k, (name, (sizes, rows, colour)) in enumerate(_cases().items()):
        arena = A.ImageArena.from_arrays(R.random_images(60 + k, sizes), device=DEV)
        rows, colour = np.stack(rows), np.stack(colour)
        out[name] = (arena, rows, colour, A.augment_images(arena, rows, OUT, colour=colour, host=True))
    return out


@pytest.mark.parametrize('name', list(_cases()))
def test_images_ex_device_against_the_host_twin_bit_for_bit(name, host_results):
    arena, rows, colour, want = host_results[name]
    got = A.augment_images(arena, torch.from_numpy(rows).to(DEV), OUT, colour=torch.from_numpy(colour).to(DEV))
    torch.cuda.synchronize()
    assert got.shape == want.shape and got.dtype == torch.float32
    diff = (got.cpu() != want).reshape(len(rows), -1).sum(1)
    assert torch.equal(got.cpu(), want), 'device and host differ, values per sample: %s' % diff.tolist()


def _sizes_and_boxes(n, seed):
    rng = np.random.default_rng(seed)
    sizes = [(40, 60), (33, 21), (128, 96), (7, 9)]
    idx = rng.integers(0, len(sizes), n).astype(np.int32)
    ext = np.array(sizes)[idx]
    c0, r0 = rng.uniform(0, ext[:, 1] - 3), rng.uniform(0, ext[:, 0] - 3)
    c1, r1 = c0 + 2.5 + rng.uniform(0, 1, n) * (ext[:, 1] - 3 - c0), r0 + 2.5 + rng.uniform(0, 1, n) * (ext[:, 0] - 3 - r0)
    arena = A.ImageArena.from_arrays(R.random_images(seed, sizes), device=DEV)
    return arena, idx, np.stack([c0, r0, c1, r1], axis=1).astype(np.float32)


@pytest.mark.parametrize('n,augmentation', [(1, True), (3, True), (257, True), (257, False)])
def test_draw_ex_device_against_the_host_twin_bit_for_bit(n, augmentation):
    arena, idx, boxes = _sizes_and_boxes(n, 21)
    want_p, want_c = A.draw_params(arena, idx, boxes, augmentation, step=6, host=True, seed=1234, colour=True)
    got_p, got_c = A.draw_params(arena, idx, boxes, augmentation, step=6, seed=1234, colour=True)
    assert got_c.is_cuda and got_c.dtype == torch.int32 and tuple(got_c.shape) == (n, 4)
    assert torch.equal(got_p.cpu(), want_p) and torch.equal(got_c.cpu(), want_c)
    assert torch.equal(got_p, A.draw_params(arena, idx, boxes, augmentation, step=6, seed=1234))          # the existing launch's rows
    assert bool(want_c.any()) == augmentation or n < 257
    # and the drawn tables drive the image launches to the host twin's bits
    img = A.augment_images(arena, got_p[:8], OUT, colour=got_c[:8])
    assert torch.equal(img.cpu(), A.augment_images(arena, want_p[:8], OUT, colour=want_c[:8], host=True))


# ------------------------------------------------------------------------------------------------------------------ memory discipline
SENTINEL = 0x5A
POISON = 0xC3


def _between_sentinels(nbytes, pad=4096, fill=SENTINEL):
    raw = torch.full((nbytes + 2 * pad,), SENTINEL, dtype=torch.uint8, device=DEV)
    raw[pad:pad + nbytes] = fill
    return raw, raw[pad:pad + nbytes]


def _clean(raw, pad=4096):
    return bool((raw[:pad] == SENTINEL).all()) and bool((raw[-pad:] == SENTINEL).all())


def test_everything_sits_between_sentinels_and_the_workspace_is_written_before_it_is_read(host_results):
    arena, rows, colour, want = host_results['halos, flip, warp, direct']
    B = rows.shape[0]
    mr, mc = int(rows[:, 3].max()), int(rows[:, 4].max())
    need = L.load().vv_augment_colour_workspace_bytes(mr, mc, B)
    assert need == 4 * mr * mc * B
    raw_out, out_b = _between_sentinels(B * OUT[0] * OUT[1] * 3 * 4)
    raw_par, par_b = _between_sentinels(B * 64)
    raw_col, col_b = _between_sentinels(B * 16)
    par_b.copy_(torch.from_numpy(rows.view(np.uint8).reshape(-1)).to(DEV))
    col_b.copy_(torch.from_numpy(colour.view(np.uint8).reshape(-1)).to(DEV))
    out, par, col = out_b.view(torch.float32).view(B, OUT[0], OUT[1], 3), par_b.view(torch.int32).view(B, 16), col_b.view(torch.int32).view(B, 4)
    before = [t.clone() for t in (arena.data, arena.meta, raw_par, raw_col)]
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    results = []
    for extra in (0, 4096 + 12):                                            # the minimum, then a larger workspace_bytes
        raw_ws, ws = _between_sentinels(need + extra, fill=POISON)
        L.call('vv_augment_images_ex', L.ptr(arena.data), L.ptr(arena.meta), len(arena), L.ptr(par), B, OUT[0], OUT[1], L.ptr(out), L.ptr(col),
               L.ptr(ws), need + extra, mr, mc, st)
        torch.cuda.synchronize()
        assert _clean(raw_out) and _clean(raw_ws)
        assert bool((ws[need:] == POISON).all())                             # nothing beyond the minimum is touched
        results.append(out.clone())
    for t, b in zip((arena.data, arena.meta, raw_par, raw_col), before):
        assert torch.equal(t, b)
    assert torch.equal(results[0].cpu(), want) and torch.equal(results[0], results[1])

    # the draw launch: both tables between sentinels, its inputs untouched, a second run identical
    arena2, idx, boxes = _sizes_and_boxes(5, 33)
    idx_t, box_t = torch.from_numpy(idx).to(DEV), torch.from_numpy(boxes).to(DEV)
    raw_p, p_b = _between_sentinels(5 * 64)
    raw_c, c_b = _between_sentinels(5 * 16)
    p, c = p_b.view(torch.int32).view(5, 16), c_b.view(torch.int32).view(5, 4)
    keep = [t.clone() for t in (arena2.meta, idx_t, box_t)]
    want_p, want_c = A.draw_params(arena2, idx, boxes, True, step=2, host=True, seed=77, rank=0, colour=True)
    for _ in range(2):
        L.call('vv_augment_draw_ex', L.ptr(arena2.meta), len(arena2), L.ptr(idx_t), L.ptr(box_t), 5, 1, 77, A.offset(2, rank=0), L.ptr(p), L.ptr(c), st)
        torch.cuda.synchronize()
        assert _clean(raw_p) and _clean(raw_c)
        assert torch.equal(p.cpu(), want_p) and torch.equal(c.cpu(), want_c)
    for t, b in zip((arena2.meta, idx_t, box_t), keep):
        assert torch.equal(t, b)


@pytest.mark.parametrize('mr,mc', [(10, 100), (20, 50), (100, 10)])
def test_a_crop_taller_than_the_slab_rectangle_is_fully_written(mr, mc):
    """Only h * w decides whether a crop fits its slab: 100 x 10 crops in slabs of 10 x 100 (four workgroups per sample in one row of
    tiles), 20 x 50 (two workgroups for four tiles: each walks two) and 100 x 10.  Poisoned workspace: every word of every slab is
    written, and the output is the host twin's -- in the staged form, the per-pixel form (no blur) and the direct form."""
    arena = A.ImageArena.from_arrays(R.random_images(9, [(100, 10), (40, 40)]), device=DEV)
    rows = np.stack([_p((100, 10), 0, scale=0.9, d_row=3), A.make_params(image=1, row0=0, col0=15, rows=100, cols=10, row_pad=30, flip=2),
                     _p((100, 10), 0, flip=1)])
    colour = np.stack([_blur(2.5, hue=5, sat=-9, hue_sat=True), A.make_colour(hue=-20, sat=40, hue_sat=True), _blur(3.5)])
    want = A.augment_images(arena, rows, OUT, colour=colour, host=True)
    rows_d, colour_d = torch.from_numpy(rows).to(DEV), torch.from_numpy(colour).to(DEV)
    out = torch.full((3,) + OUT + (3,), -7.0, device=DEV)
    raw_ws, ws = _between_sentinels(3 * 1000 * 4, fill=POISON)
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    L.call('vv_augment_images_ex', L.ptr(arena.data), L.ptr(arena.meta), 2, L.ptr(rows_d), 3, OUT[0], OUT[1], L.ptr(out), L.ptr(colour_d),
           L.ptr(ws), ws.numel(), mr, mc, st)
    torch.cuda.synchronize()
    words = ws.view(torch.int32)
    poison = int(np.array([POISON] * 4, dtype=np.uint8).view(np.int32)[0])
    assert _clean(raw_ws) and not bool((words == poison).any())               # a written word's top byte is 0
    assert torch.equal(out.cpu(), want)


def test_an_injected_padded_crop_through_the_python_surface():
    """Rows that stay on the device get slabs of the arena's largest image (40 x 40): a padded 100 x 10 crop has fewer pixels, is
    admitted, and gives the host twin's bits."""
    arena = A.ImageArena.from_arrays(R.random_images(10, [(40, 40)]), device=DEV)
    rows = np.stack([A.make_params(row0=0, col0=15, rows=100, cols=10, row_pad=30), A.make_params(rows=40, cols=40, flip=1)])
    colour = np.stack([_blur(3.0, hue=3, sat=3, hue_sat=True), _blur(1.0)])
    got = A.augment_images(arena, torch.from_numpy(rows).to(DEV), OUT, colour=torch.from_numpy(colour).to(DEV))
    torch.cuda.synchronize()
    assert torch.equal(got.cpu(), A.augment_images(arena, rows, OUT, colour=colour, host=True))


# ------------------------------------------------------------------------------------------------------------------------- refusals
def test_statuses_of_the_device_entries_leave_everything_untouched():
    arena = A.ImageArena.from_arrays(R.random_images(5, [(9, 13)]), device=DEV)
    rows = torch.from_numpy(np.stack([A.make_params(rows=9, cols=13)])).to(DEV)
    col = torch.from_numpy(np.stack([_blur(1.0)])).to(DEV)
    out = torch.full((1, 4, 4, 3), -7.0, device=DEV)
    ws = torch.full((4 * 117,), POISON, dtype=torch.uint8, device=DEV)
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    lib = L.load()

    def img(c=col, w=ws, nbytes=4 * 117, mr=9, mc=13, r=4):
        return lib.vv_augment_images_ex(L.ptr(arena.data), L.ptr(arena.meta), 1, L.ptr(rows), 1, r, 4, L.ptr(out), L.ptr(c), L.ptr(w), nbytes, mr, mc, st)

    assert img(w=None) == -1 and img(nbytes=4 * 117 - 1) == -5 and img(mr=0) == -2 and img(mc=40000) == -2 and img(r=0) == -2
    idx, box = torch.zeros(1, dtype=torch.int32, device=DEV), torch.tensor([[1.0, 1.0, 5.0, 5.0]], device=DEV)
    par = torch.full((1, 16), 12345, dtype=torch.int32, device=DEV)
    cc = torch.full((1, 4), 12345, dtype=torch.int32, device=DEV)
    drw = lambda p=par, c=cc, b=1: lib.vv_augment_draw_ex(L.ptr(arena.meta), 1, L.ptr(idx), L.ptr(box), b, 1, 1, 0, L.ptr(p), L.ptr(c), st)
    assert drw(c=None) == -1 and drw(p=None) == -1 and drw(b=0) == -2
    torch.cuda.synchronize()
    assert bool((out == -7.0).all()) and bool((par == 12345).all()) and bool((cc == 12345).all()) and bool((ws == POISON).all())
    assert img(c=None) == 0                                                  # colour == NULL is vv_augment_images
    torch.cuda.synchronize()
    assert torch.equal(out.cpu(), A.augment_images(arena, rows.cpu(), (4, 4), host=True)) and bool((ws == POISON).all())


BAD = [np.array([4, 0, 0, 0], dtype=np.int32), A.make_colour(sigma=float('nan'), blur=True), A.make_colour(sigma=-1.0, blur=True),
       A.make_colour(sigma=17.0, blur=True), A.make_colour(hue=180, hue_sat=True), A.make_colour(sat=-256, hue_sat=True), 'slab', 'params']


@pytest.mark.parametrize('k', range(len(BAD)))
def test_rows_the_two_launches_must_refuse(k):
    """A refused sample's output rows and slab stay untouched, in both launches, and its neighbours are computed."""
    images = R.random_images(5, [(9, 13), (12, 12)])
    arena = A.ImageArena.from_arrays(images, device=DEV)
    rows = np.stack([_p((9, 13), 0), _p((9, 13), 0), _p((9, 13), 0, scale=0.9)])
    colour = np.stack([_blur(1.0), _blur(2.0, hue=4, sat=4, hue_sat=True), A.make_colour(hue=-9, sat=30, hue_sat=True)])
    mr, mc = 9, 13
    if isinstance(BAD[k], str) and BAD[k] == 'slab':
        rows[1] = _p((12, 12), 1)                                            # 144 pixels against slabs of 117 words
    elif isinstance(BAD[k], str):
        rows[1] = _p((9, 14), 0)                                             # a crop outside its image
    else:
        colour[1] = BAD[k]
    if not isinstance(BAD[k], str):
        with pytest.raises(L.VoxVaeError):
            A.augment_images(arena, rows, (4, 4), colour=colour, host=True)
    out = torch.full((3, 4, 4, 3), -7.0, device=DEV)
    ws = torch.full((3, mr * mc * 4), POISON, dtype=torch.uint8, device=DEV)
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    rows_d, colour_d = torch.from_numpy(rows).to(DEV), torch.from_numpy(colour).to(DEV)         # named: they must outlive the launches
    L.call('vv_augment_images_ex', L.ptr(arena.data), L.ptr(arena.meta), 2, L.ptr(rows_d), 3, 4, 4, L.ptr(out), L.ptr(colour_d), L.ptr(ws),
           ws.numel(), mr, mc, st)
    torch.cuda.synchronize()
    assert bool((out[1] == -7.0).all()) and bool((ws[1] == POISON).all())
    want = A.augment_images(arena, rows[[0, 2]], (4, 4), colour=colour[[0, 2]], host=True)
    assert torch.equal(out[[0, 2]].cpu(), want)
    words = ws.view(torch.int32)                                             # a written word's top byte is 0: never the poison word
    assert not bool((words[0] == words[1, 0]).any()) and not bool((words[2] == words[1, 0]).any())     # slabs exactly full, every word written


# --------------------------------------------------------------------------------------------------------------------------- loader
@pytest.fixture
def seeded():
    import voxvae
    voxvae.manual_seed(2468)
    yield
    voxvae.manual_seed(None)


def _loader(**kw):
    import src.dataset_loader.pascal3D as P
    return P.deviceDataLoaderSingleObject('train', 'synthetic:8:32:3', device=DEV, **kw)


def test_loader_with_all_colour_ops(seeded):
    base, full = _loader(), _loader(colour_ops='all')
    assert base.colour_ops == 'invert_add' and full.colour_ops == 'all'
    flagged_differs = 0
    for _ in range(4):
        a, b = base.getNextBatch(8, (24, 20)), full.getNextBatch(8, (24, 20))
        assert len(a) == len(b) == 6 and base.last_colour is None
        for x, y in zip(a, b):
            assert torch.is_tensor(y) and y.is_cuda and y.dtype == x.dtype and y.shape == x.shape
        for k in (0, 1, 2, 3, 5):
            assert torch.equal(a[k], b[k])
        assert torch.equal(base.last_params, full.last_params)
        c = full.last_colour
        assert tuple(c.shape) == (8, 4) and c.dtype == torch.int32
        plain = c[:, 0] == 0
        assert torch.equal(a[4][plain], b[4][plain])
        flagged_differs += int((a[4][~plain] != b[4][~plain]).flatten(1).any(1).sum())
        assert torch.equal(b[4].cpu(), A.augment_images(full._arena, full.last_params.cpu(), (20, 24), colour=c.cpu(), host=True))
        assert float(b[4].min()) >= 0.0 and float(b[4].max()) <= 1.0
    assert flagged_differs >= 1
    full.getNextBatch(8, (24, 20), augmentation=False)
    assert not bool(full.last_colour.any())
    import src.dataset_loader.pascal3D as P
    with pytest.raises(ValueError):
        _loader(colour_ops='blur')
    with pytest.raises(ValueError):
        P.loader_factory('host', 'all')
    assert P.loader_factory('device', 'invert_add') is P.deviceDataLoaderSingleObject


def test_from_arrays_takes_colour_ops():
    import src.dataset_loader.pascal3D as P
    images = R.random_images(1, [(20, 30), (16, 16)])
    grids = (np.random.default_rng(0).random((2, 8, 8, 8)) > 0.7).astype(np.float32)
    ld = P.deviceDataLoaderSingleObject.from_arrays(images=images, boxes=[[2.0, 3.0, 20.5, 15.0], [0.0, 0.0, 16.0, 16.0]], classes=[1, 4], cad_index=[1, 0],
                                                    euler=np.zeros((2, 3)), cad_grids=grids, device=DEV, seed=1, shuffle=False, colour_ops='all')
    img = ld.getNextBatch(2, (12, 12))[4]
    assert tuple(img.shape) == (2, 12, 12, 3) and tuple(ld.last_colour.shape) == (2, 4)


def test_train_pascal_with_all_colour_ops():
    """train_pascal.py --loader device --colour-ops all --max-iter 1 on the synthetic photos."""
    import os
    import subprocess
    import sys
    pkg = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'anytime-3d-reconstruction_amd')
    cmd = [sys.executable, 'train_pascal.py', '--max-iter', '1', '--batch', '2', '--image', '64', '--voxel', '16', '--latent', '8',
           '--dataset-path', 'synthetic:4:16', '--loader', 'device', '--colour-ops', 'all']
    r = subprocess.run(cmd, cwd=pkg, capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
