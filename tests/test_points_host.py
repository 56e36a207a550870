"""CPU tests of the point-cloud step's host side: the three C entries (include/voxvae.h: vv_voxel_points_workspace_bytes / _count / _emit)
are declared, exported and bound alike and refuse bad arguments before any launch, so they need no GPU; and the float64 definition the
GPU tests compare against (tests/_points_ref.py) is itself checked on a hand-written example and on an exactness property."""
import ctypes
import os
import re

import numpy as np
import pytest

import _points_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, 'include', 'voxvae.h')
ENTRIES = {'vv_voxel_points_workspace_bytes': 2, 'vv_voxel_points_count': 12, 'vv_voxel_points_emit': 15}


@pytest.fixture(scope='module')
def lib():
    from voxvae import build as vb
    vb.build()
    from voxvae import lib as L
    return L.load()


# ------------------------------------------------------------------------------------------------ the ABI
def test_entries_are_declared_exported_and_bound_with_equal_argument_counts(lib):
    from voxvae import lib as L
    src = re.sub(r'/\*.*?\*/', '', open(HEADER).read(), flags=re.S)
    for name, nargs in ENTRIES.items():
        m = re.search(r'\b(?:int|size_t)\s+%s\s*\(([^;]*?)\)\s*;' % name, src, flags=re.S)
        assert m, '%s is not declared in include/voxvae.h' % name
        assert len([a for a in m.group(1).split(',') if a.strip()]) == nargs, name
        assert hasattr(lib, name), 'libvoxvae.so does not export %s' % name
        assert len(L.SIGNATURES[name][1]) == nargs, name
    assert L.SIGNATURES['vv_voxel_points_workspace_bytes'][0] is ctypes.c_size_t
    assert L.SIGNATURES['vv_voxel_points_emit'][1][9] is ctypes.c_longlong           # capacity: 64 bits


def _count(lib, occ=64, packed=0, batch=2, side=8, counts=64, bbox=64, offsets=64, ws=64, ws_bytes=1 << 30):
    """The pointers are never dereferenced by a call that is refused: small aligned integers stand in for device addresses."""
    return lib.vv_voxel_points_count(occ, packed, 0.5, 0, batch, side, counts, bbox, offsets, ws, ws_bytes, None)


def _emit(lib, occ=64, packed=0, dims=64, pose=None, offsets=64, bbox=64, points=64, capacity=10, ws=64, ws_bytes=1 << 30, batch=2, side=8):
    return lib.vv_voxel_points_emit(occ, packed, 0.5, 0, dims, pose, offsets, bbox, points, capacity, ws, ws_bytes, batch, side, None)


def test_count_refuses_before_any_launch(lib):
    for name in ('occ', 'counts', 'bbox', 'offsets', 'ws'):
        assert _count(lib, **{name: None}) == -1, name
    assert _count(lib, batch=0) == -2 and _count(lib, batch=-1) == -2
    assert _count(lib, side=0) == -2 and _count(lib, side=129) == -2 and _count(lib, side=-4) == -2
    assert _count(lib, packed=1, side=5) == -2                    # 125 cells: not whole bytes
    assert _count(lib, offsets=68) == -4                          # int64 at a 4-byte address
    assert _count(lib, occ=66) == -4 and _count(lib, counts=65) == -4 and _count(lib, bbox=62) == -4 and _count(lib, ws=66) == -4
    need = lib.vv_voxel_points_workspace_bytes(2, 8)
    assert need > 0 and _count(lib, ws_bytes=need - 1) == -5 and _count(lib, ws_bytes=0) == -5
    # the order of the refusals: null, shape, alignment, workspace
    assert _count(lib, occ=None, side=0, offsets=68, ws_bytes=0) == -1
    assert _count(lib, side=0, offsets=68, ws_bytes=0) == -2
    assert _count(lib, offsets=68, ws_bytes=0) == -4


def test_emit_refuses_before_any_launch(lib):
    for name in ('occ', 'dims', 'offsets', 'bbox', 'points', 'ws'):
        assert _emit(lib, **{name: None}) == -1, name
    assert _emit(lib, batch=0) == -2 and _emit(lib, batch=-1) == -2
    assert _emit(lib, side=0) == -2 and _emit(lib, side=129) == -2
    assert _emit(lib, packed=1, side=5) == -2
    assert _emit(lib, capacity=-1) == -2
    assert _emit(lib, offsets=68) == -4
    assert _emit(lib, occ=66) == -4 and _emit(lib, dims=66) == -4 and _emit(lib, pose=66) == -4 and _emit(lib, points=65) == -4
    need = lib.vv_voxel_points_workspace_bytes(2, 8)
    assert _emit(lib, ws_bytes=need - 1) == -5 and _emit(lib, ws_bytes=0) == -5
    assert _emit(lib, occ=None, side=0, offsets=68, ws_bytes=0) == -1
    assert _emit(lib, side=0, offsets=68, ws_bytes=0) == -2
    assert _emit(lib, offsets=68, ws_bytes=0) == -4
    assert lib.vv_status_string(-5) == b'workspace missing or too small'


def test_workspace_bytes_is_monotone_and_zero_for_refused_shapes(lib):
    w = lib.vv_voxel_points_workspace_bytes
    assert w(0, 8) == 0 and w(-1, 8) == 0 and w(2, 0) == 0 and w(2, 129) == 0 and w(2, -3) == 0
    prev = 0
    for side in range(1, 129):
        cur = w(3, side)
        assert cur >= prev > 0 or (side == 1 and cur > 0), side
        prev = cur
    assert w(1, 16) == w(1, 1) < w(1, 17)                         # one piece up to 4096 cells, two from 17^3 on
    for side in (5, 16, 20, 64, 128):
        sizes = [w(b, side) for b in (1, 2, 3, 64, 256, 4096)]
        assert all(b > a > 0 for a, b in zip(sizes, sizes[1:])), side
    assert w(256, 32) == 256 * 8 * w(1, 16) and w(64, 64) == 64 * 64 * w(1, 16)


def test_voxel_points_without_a_gpu_is_an_error_not_a_fallback(monkeypatch):
    import voxvae
    from voxvae import lib as L
    from voxvae.points import voxel_points
    monkeypatch.setitem(voxvae._DEFAULTS, 'device', 'cpu')
    with pytest.raises(L.VoxVaeError):
        voxel_points(np.zeros((1, 4, 4, 4, 1), np.float32), [[1.0, 1.0, 1.0]])


# ------------------------------------------------------------------------------------------------ the float64 definition
def test_definition_on_a_hand_written_example():
    """3^3 grid, cells (0,0,1), (0,2,1), (1,0,2) in that (row-major) order: lo = (0,0,1), hi = (1,2,2), ext = (1,2,1), E = 2;
    (h, w, l) = (1, 4, 2) -> scale = 4 / 2 = 2; q = (cell - lo) 2 - ext = (-1,-2,-1), (-1,2,-1), (1,-2,1)."""
    p = np.zeros((3, 3, 3), dtype=np.float32)
    p[0, 0, 1], p[0, 2, 1], p[1, 0, 2] = 0.9, 0.51, 1.0
    p[2, 2, 2] = 0.5                                              # exactly the threshold: not occupied
    p[2, 0, 0] = np.nan                                           # neither is a NaN
    m = R.occupancy(p)
    assert m.sum() == 3
    pts, box = R.object_points(m, 1.0, 4.0, 2.0)
    assert box.tolist() == [0, 0, 1, 1, 2, 2]
    assert pts.tolist() == [[-1.0, -2.0, -1.0], [-1.0, 2.0, -1.0], [1.0, -2.0, 1.0]]
    # the pose: a quarter turn about the first axis and a shift
    P = np.array([[1, 0, 0, 10], [0, 0, -1, 20], [0, 1, 0, 30], [0, 0, 0, 1]], dtype=np.float64)
    pts2, _ = R.object_points(m, 1.0, 4.0, 2.0, P)
    assert pts2.tolist() == [[9.0, 21.0, 28.0], [9.0, 21.0, 32.0], [11.0, 19.0, 28.0]]
    # every cell of a 3^3 grid touches the boundary except the centre
    full = np.ones((3, 3, 3), dtype=bool)
    assert R.surface_mask(full).sum() == 26 and not R.surface_mask(full)[1, 1, 1]
    s, sbox = R.object_points(full, 2.0, 2.0, 2.0, surface_only=True)
    a, abox = R.object_points(full, 2.0, 2.0, 2.0)
    assert np.array_equal(sbox, abox) and np.array_equal(s, np.delete(a, 13, axis=0))
    # the two defined edge cases
    e, ebox = R.object_points(np.zeros((3, 3, 3), dtype=bool), 1.0, 1.0, 1.0)
    assert e.shape == (0, 3) and ebox.tolist() == [3, 3, 3, -1, -1, -1]
    one = np.zeros((3, 3, 3), dtype=bool)
    one[1, 2, 0] = True
    o, obox = R.object_points(one, 1.0, 2.0, 3.0, P)
    assert o.tolist() == [[10.0, 20.0, 30.0]] and obox.tolist() == [1, 2, 0, 1, 2, 0]
    out = R.batch_points(np.stack([m, np.zeros((3, 3, 3), dtype=bool), one]), [[1, 4, 2], [1, 1, 1], [1, 2, 3]])
    assert out['counts'].tolist() == [3, 0, 1] and out['offsets'].tolist() == [0, 3, 3, 4] and out['points'].shape == (4, 3)


@pytest.mark.parametrize('side', [5, 8, 16, 20, 32])
def test_with_unit_scale_every_coordinate_is_a_float32_multiple_of_one_half(side):
    """dims = (E, ., .) with E the largest extent and the identity pose: scale == 1, q = (cell - lo) - ext / 2, so every coordinate is a
    multiple of 0.5 below 2^7 and the float64 definition cast to float32 is exact -- what the bit-for-bit GPU tests rest on."""
    rng = np.random.default_rng(side)
    for fill in (0.02, 0.3, 0.9):
        m = rng.random((side, side, side)) < fill
        E = R.extent(m)
        assert E >= 1
        for surface in (False, True):
            pts, _ = R.object_points(m, float(E), 1.0, 0.5, surface_only=surface)
            assert len(pts) == (R.surface_mask(m) if surface else m).sum()
            assert np.array_equal(pts * 2, np.round(pts * 2)) and np.abs(pts).max() <= side / 2.0
            assert np.array_equal(pts.astype(np.float32).astype(np.float64), pts)


def test_affine_bound_is_the_brackets_sixteen_units():
    P = np.zeros((1, 4, 4))
    P[0, :3, :3] = [[1, -1, 0], [0, 0.5, 0], [0, 0, 0]]
    P[0, :3, 3] = [3, -4, 0]
    b = R.affine_bound([[2.0, 5.0, 1.0]], P)
    assert np.array_equal(b, 16 * 2.0 ** -24 * np.array([[2 * 5.0 + 3, 0.5 * 5.0 + 4, 0.0]]))
    rot = R.random_poses(np.random.default_rng(0), 4)
    assert rot.dtype == np.float32 and np.allclose(rot[:, :3, :3] @ rot[:, :3, :3].transpose(0, 2, 1), np.eye(3), atol=1e-6)
    assert np.abs(rot[:, :3, 3]).max() <= 20.0
