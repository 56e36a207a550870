"""CPU tests of the detection -> world-pose step (csrc/pose_solve.h, csrc/object_pose.hip, voxvae/pose.py, src/visualizer): the C entries
are declared, exported and bound alike and refuse bad arguments before any launch; and the NUMERICS are checked without a GPU through
vv_object_pose_host -- the same header compiled for the CPU -- against tests/golden/pose_kitti.npz, which holds what the reference's own
getObjectInRealWorld / getTranslation returned for 401 seeded KITTI-like detections (tests/golden/make_pose_golden.py).

keep, candidate, index, count and the pixel box are compared EXACTLY.  The float fields are compared within
    half a float32 unit of the value  +  GATE x (the field's sensitivity to the translation),
GATE = 16 x SOLVER_TERM, where SOLVER_TERM is MEASURED, not chosen: the largest relative difference (max-norm over the translation's
max-norm) between the host entry's float64 translation and the reference's over all fitted fixture rows,

    SOLVER_TERM = 2.58e-13        (one-sided Jacobi in pose_solve.h vs LAPACK's SVD in the reference; median 1.9e-15.  The same row
                                   separates our numpy statement of the step, which calls LAPACK too, from the reference by 2.2e-13: it
                                   is that row's conditioning, the rotation entering with a last-bit difference, not the solver)

and the factor 16 absorbs builds that contract multiply-adds differently.  The winner is stable under that: the smallest IoU gap between
a fixture row's winner and its best candidate with a different translation is 4.9e-6.
"""
import ctypes
import os
import re

import numpy as np
import pytest

import _pose_ref as PR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, 'include', 'voxvae.h')
GOLDEN = os.path.join(ROOT, 'tests', 'golden', 'pose_kitti.npz')
ENTRIES = {'vv_object_pose_workspace_bytes': 1, 'vv_object_pose': 21, 'vv_object_pose_host': 20, 'vv_pose_translation_host': 7,
           'vv_pose_ray_host': 4, 'vv_pose_ray_rotation_host': 2, 'vv_pose_box_projection_host': 7}
SOLVER_TERM = 2.58e-13
GATE = 16 * SOLVER_TERM
F32 = np.float32


@pytest.fixture(scope='module')
def lib():
    from voxvae import build as vb
    vb.build()
    from voxvae import lib as L
    return L.load()


@pytest.fixture(scope='module')
def golden():
    g = dict(np.load(GOLDEN))
    g['proj_inv'] = np.linalg.inv(g['proj_mat'])
    g['kept'] = np.nonzero(g['keep'])[0]
    return g


def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def host_entry(lib, b2, b3, sn, cs, image, P, Pinv, sweeps=0):
    """vv_object_pose_host on numpy inputs -> dict of numpy outputs (compacted fields cut to count) + the float64 translations."""
    n = len(b2)
    ins = [np.ascontiguousarray(a, dtype=F32) for a in (b2, b3, sn, cs)]
    o = dict(keep=np.zeros(n, np.int32), candidate=np.zeros(n, np.int32), iou=np.zeros(n, F32), count=np.zeros(1, np.int32),
             index=np.zeros(n, np.int32), pose=np.zeros((n, 16), F32), size=np.zeros((n, 3), F32), box2d=np.zeros((n, 4), np.int32),
             proj=np.zeros((n, 16), F32), translation=np.zeros((n, 3)))
    P, Pinv = np.ascontiguousarray(P, dtype=np.float64), np.ascontiguousarray(Pinv, dtype=np.float64)
    rc = lib.vv_object_pose_host(*[_p(a) for a in ins], n, float(image[0]), float(image[1]), _p(P), _p(Pinv), _p(o['keep']), _p(o['candidate']),
                                 _p(o['iou']), _p(o['count']), _p(o['index']), _p(o['pose']), _p(o['size']), _p(o['box2d']), _p(o['proj']),
                                 _p(o['translation']), sweeps)
    assert rc == 0, rc
    M = int(o['count'][0])
    o['count'] = M
    for k in ('index', 'pose', 'size', 'box2d', 'proj'):
        o[k] = o[k][:M]
    return o


@pytest.fixture(scope='module')
def host(lib, golden):
    g = golden
    return host_entry(lib, g['bbox2d'], g['bbox3d'], g['sin'], g['cos'], g['image_size'], g['proj_mat'], g['proj_inv'])


def half_ulp32(*values):
    """Half a float32 unit at the largest of the given magnitudes (elementwise)."""
    m = np.maximum.reduce([np.abs(np.asarray(v, dtype=np.float64)) for v in values])
    return np.spacing(m.astype(F32)).astype(np.float64) / 2.0


def float_field_bounds(g, rows, roundings=1):
    """Allowed |got - reference| for pose [M,16], size [M,3] and proj [M,16] of the fixture rows `rows` (kept ones): `roundings` half
    float32 units of the value, plus GATE times the field's sensitivity to a relative perturbation of the translation:
        rotation entries   1 (they carry no translation; a last-bit difference of the float64 rotation is far below GATE)
        translation        max |X|
        size               0: the inputs, copied
        projected corner   u = (P_row . x) / z_c with x = R d + X: a perturbation dX moves the numerator by at most sum |P_row| |dX| and the
                           depth by |dX|, so |du| <= (sum |P_row| + |u|) |dX| / z_c, with z_c >= X_z - half the box diagonal."""
    pose, proj, P = g['pose'][rows].reshape(-1, 16), g['proj'][rows].reshape(-1, 16), g['proj_mat']
    X = pose[:, [3, 7, 11]]
    xmax = np.abs(X).max(axis=1)
    sens = np.ones_like(pose)
    sens[:, [3, 7, 11]] = xmax[:, None]
    sens[:, 12:] = 0.0
    b_pose = roundings * half_ulp32(pose) + GATE * sens
    zc = X[:, 2] - np.sqrt((g['bbox3d'][rows].astype(np.float64) ** 2).sum(axis=1)) / 2.0
    assert (zc > 0.5).all()                                             # the fixtures' kept objects lie wholly in front of the camera
    rowsum = np.tile([np.abs(P[0]).sum(), np.abs(P[1]).sum()], 8)
    b_proj = roundings * half_ulp32(proj) + GATE * (rowsum[None, :] + np.abs(proj)) * (xmax / zc)[:, None]
    return b_pose, np.zeros((len(rows), 3)), b_proj


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
    assert L.SIGNATURES['vv_object_pose_workspace_bytes'][0] is ctypes.c_size_t
    assert L.SIGNATURES['vv_object_pose'][1][5] is ctypes.c_double and L.SIGNATURES['vv_object_pose'][1][6] is ctypes.c_double


PTRS = ('bbox2d', 'bbox3d', 'sin', 'cos', 'proj', 'proj_inv', 'keep', 'candidate', 'iou', 'count', 'index', 'pose', 'size', 'box2d', 'proj3d')


def _device(lib, n=4, col=1242.0, row=375.0, ws=64, ws_bytes=1 << 30, **over):
    """A call that is refused dereferences nothing: small aligned integers stand in for the addresses."""
    a = dict((k, 64) for k in PTRS)
    a.update(over)
    return lib.vv_object_pose(a['bbox2d'], a['bbox3d'], a['sin'], a['cos'], n, col, row, a['proj'], a['proj_inv'], a['keep'], a['candidate'],
                              a['iou'], a['count'], a['index'], a['pose'], a['size'], a['box2d'], a['proj3d'], ws, ws_bytes, None)


def _host(lib, n=4, col=1242.0, row=375.0, translation=None, sweeps=0, **over):
    a = dict((k, 64) for k in PTRS)
    a.update(over)
    return lib.vv_object_pose_host(a['bbox2d'], a['bbox3d'], a['sin'], a['cos'], n, col, row, a['proj'], a['proj_inv'], a['keep'], a['candidate'],
                                   a['iou'], a['count'], a['index'], a['pose'], a['size'], a['box2d'], a['proj3d'], translation, sweeps)


def test_device_entry_refuses_before_any_launch(lib):
    for name in PTRS:
        assert _device(lib, **{name: None}) == -1, name
    assert _device(lib, ws=None) == -1
    assert _device(lib, n=0) == -2 and _device(lib, n=-1) == -2 and _device(lib, n=65537) == -2
    assert _device(lib, col=0.0) == -2 and _device(lib, row=-375.0) == -2 and _device(lib, col=float('nan')) == -2
    for name in PTRS:
        assert _device(lib, **{name: 66}) == -4, name
    assert _device(lib, proj=68) == -4 and _device(lib, proj_inv=68) == -4     # doubles at a 4-byte address
    assert _device(lib, ws=65) == -4
    need = lib.vv_object_pose_workspace_bytes(4)
    assert need > 0 and _device(lib, ws_bytes=need - 1) == -5 and _device(lib, ws_bytes=0) == -5
    # the order of the refusals: null, shape, alignment, workspace
    assert _device(lib, bbox2d=None, n=0, pose=66, ws_bytes=0) == -1
    assert _device(lib, n=0, pose=66, ws_bytes=0) == -2
    assert _device(lib, pose=66, ws_bytes=0) == -4
    assert _device(lib, ws_bytes=0) == -5


def test_host_entry_refuses_like_the_device_entry(lib):
    for name in PTRS:
        assert _host(lib, **{name: None}) == -1, name
    assert _host(lib, n=0) == -2 and _host(lib, n=65537) == -2 and _host(lib, row=0.0) == -2 and _host(lib, sweeps=65) == -2
    for name in PTRS:
        assert _host(lib, **{name: 66}) == -4, name
    assert _host(lib, translation=68) == -4
    assert _host(lib, keep=None, n=0, pose=66) == -1 and _host(lib, n=0, pose=66) == -2
    assert lib.vv_pose_translation_host(None, 64, 64, 64, 64, None, None) == -1 and lib.vv_pose_translation_host(64, 64, 68, 64, 64, None, None) == -4
    assert lib.vv_pose_ray_host(None, 1.0, 1.0, 64) == -1 and lib.vv_pose_ray_rotation_host(64, None) == -1
    assert lib.vv_pose_box_projection_host(64, 64, None, 1.0, 1.0, 1.0, 64) == -1


def test_workspace_bytes_is_monotone_and_zero_for_refused_counts(lib):
    w = lib.vv_object_pose_workspace_bytes
    assert w(0) == 0 and w(-1) == 0 and w(65537) == 0
    sizes = [w(n) for n in (1, 2, 63, 64, 65, 4096, 65536)]
    assert all(b > a > 0 for a, b in zip(sizes, sizes[1:])) and w(64) == 64 * w(1)


def test_object_poses_without_a_gpu_is_an_error_not_a_fallback(monkeypatch, golden):
    import voxvae
    from voxvae import lib as L
    from voxvae.pose import object_poses
    monkeypatch.setitem(voxvae._DEFAULTS, 'device', 'cpu')
    g = golden
    with pytest.raises(L.VoxVaeError):
        object_poses(g['bbox2d'][:3], g['bbox3d'][:3], g['sin'][:3], g['cos'][:3], g['image_size'])
    empty = object_poses(np.zeros((0, 5), F32), np.zeros((0, 3), F32), np.zeros((0, 3), F32), np.zeros((0, 3), F32), g['image_size'], host=True)
    assert len(empty) == 0 and empty.count() == 0 and empty.numpy()[0].shape == (0, 4, 4)


# ------------------------------------------------------------------------------------------------ the fixture itself
def test_fixture_covers_every_way_a_detection_leaves(golden):
    g = golden
    N = len(g['bbox2d'])
    assert N >= 400 and os.path.getsize(GOLDEN) < 1 << 20
    assert g['bbox2d'].dtype == F32 and g['sin'].dtype == F32
    assert (~g['ran']).sum() == 1 and np.isnan(g['bbox3d'][~g['ran']]).any()              # the NaN row, never shown to the reference
    ran = g['ran']
    assert g['keep'].sum() >= 300 and (g['candidate'][ran] == -2).sum() >= 5 and (g['candidate'] == -1).sum() >= 1
    assert not g['keep'][g['candidate'] < 0].any()
    assert (g['gap'] >= 1e-9).all()                                                       # nothing near an IoU tie of distinct poses
    general = (g['sin'][:, 1] != 0) & g['keep']
    assert general.sum() >= 50                                                            # elevation and in-plane angles, not only yaw
    d = np.diff(g['keep'].astype(int))
    assert (d != 0).sum() >= 40                                                           # kept and dropped rows interleave


# ------------------------------------------------------------------------------------------------ numerics through the host entry
def test_host_entry_exact_fields_are_the_references(golden, host):
    g, h, ran = golden, host, golden['ran']
    assert np.array_equal(h['keep'][ran] != 0, g['keep'][ran])
    assert np.array_equal(h['candidate'][ran], g['candidate'][ran])
    assert h['keep'][~ran].tolist() == [0] and h['candidate'][~ran].tolist() == [-2]       # the NaN row: not kept, never fitted
    assert h['count'] == len(g['kept']) and np.array_equal(h['index'], g['kept'])
    assert np.array_equal(h['box2d'], g['box2d'][g['kept']])
    assert set(np.unique(h['keep'])) <= {0, 1}


def test_host_entry_solver_term_and_float_fields(golden, host):
    g, h = golden, host
    fitted = g['candidate'] >= 0
    ref = g['translation'][fitted]
    rel = np.abs(h['translation'][fitted] - ref).max(axis=1) / np.abs(ref).max(axis=1)
    print('\n[pose host] solver term: max relative translation difference %.3e (median %.1e) over %d rows; documented %.2e, gate %.2e'
          % (rel.max(), np.median(rel), fitted.sum(), SOLVER_TERM, GATE))
    assert rel.max() <= GATE
    assert not h['translation'][~fitted].any()                                            # no winner / not fitted: zeros
    np.testing.assert_allclose(h['iou'][fitted], g['iou'][fitted], rtol=0, atol=2.0 ** -24 + 1e-9)
    assert (h['iou'][~fitted] == -1).all()
    kept = g['kept']
    b_pose, b_size, b_proj = float_field_bounds(g, kept)
    e_pose = np.abs(h['pose'].astype(np.float64) - g['pose'][kept].reshape(-1, 16))
    e_proj = np.abs(h['proj'].astype(np.float64) - g['proj'][kept].reshape(-1, 16))
    print('[pose host] pose error / bound %.3f, projected corners error / bound %.3f' % ((e_pose / np.maximum(b_pose, 1e-300)).max(), (e_proj / b_proj).max()))
    assert (e_pose <= b_pose).all() and (e_proj <= b_proj).all()
    assert np.array_equal(h['size'].astype(np.float64), g['size'][kept])                  # (h, l, w): copies of float32 inputs
    assert np.array_equal(h['size'], g['bbox3d'][kept][:, [1, 2, 0]])


def test_a_further_sweep_changes_no_bit(lib, golden, host):
    """VV_POSE_SWEEPS = 6: the fixture set is converged after 4 sweeps (3 leave up to 7e-9), so 5, 6, 7 and 12 give the default's bits."""
    g = golden
    args = (g['bbox2d'], g['bbox3d'], g['sin'], g['cos'], g['image_size'], g['proj_mat'], g['proj_inv'])
    for sweeps in (4, 5, 6, 7, 12):
        o = host_entry(lib, *args, sweeps=sweeps)
        for k in ('keep', 'candidate', 'iou', 'index', 'pose', 'size', 'box2d', 'proj', 'translation'):
            assert np.array_equal(o[k], host[k]), (sweeps, k)
    three = host_entry(lib, *args, sweeps=3)
    assert not np.array_equal(three['translation'], host['translation'])                  # the argument does reach the solver


def test_python_surface_host_mode_and_the_visualizer_helpers(golden, host):
    from voxvae.pose import KITTI_PROJ_MAT, object_poses
    import src.visualizer.visualizer as vis
    g = golden
    assert np.array_equal(KITTI_PROJ_MAT, g['proj_mat']) and np.array_equal(vis.kitti_proj_mat_inv, g['proj_inv'])
    o = object_poses(g['bbox2d'], g['bbox3d'], g['sin'], g['cos'], tuple(g['image_size']), host=True)
    assert o.count() == host['count'] and np.array_equal(o.index[:o.count()].numpy(), host['index'])
    pose, size, box, proj = o.numpy()
    assert pose.shape == (o.count(), 4, 4) and proj.shape == (o.count(), 2, 2, 2, 2) and box.dtype == np.int32
    assert np.array_equal(pose.reshape(-1, 16), host['pose']) and np.array_equal(proj.reshape(-1, 16), host['proj'])
    assert np.array_equal(size, host['size']) and np.array_equal(box, host['box2d'])
    assert np.array_equal(o.candidate.numpy(), host['candidate'])
    # the single-object helpers reproduce one kept fixture row step by step
    i = int(g['kept'][7])
    px = g['bbox2d'][i, :4].astype(np.float64) * np.array([1242, 375, 1242, 375])
    ray = vis.getRay(vis.kitti_proj_mat_inv, ((px[0] + px[2]) / 2, (px[1] + px[3]) / 2))
    assert abs(np.linalg.norm(ray) - 1) < 1e-15
    R = vis.getRayRotation(ray) @ PR.object_rotation(g['sin'][i], g['cos'][i])
    assert np.abs(R - g['pose'][i][:3, :3]).max() < 1e-14
    X = vis.getTranslation(vis.kitti_proj_mat, g['pose'][i][:3, :3], px, g['bbox3d'][i])
    assert X.shape == (3, 1) and np.abs(X.ravel() - g['translation'][i]).max() <= GATE * np.abs(g['translation'][i]).max()
    w, h, l = g['bbox3d'][i].astype(np.float64)
    a = vis.get3DbboxProjection(vis.kitti_proj_mat, g['pose'][i][:3, :3], g['translation'][i], h, w, l)
    assert a.shape == (2, 2, 2, 2) and np.abs(a - g['proj'][i]).max() < 1e-9


# ------------------------------------------------------------------------------------------------ our float64 statement
def test_pose_ref_against_the_fixtures(golden):
    """tests/_pose_ref.py serves the shapes the fixtures do not cover; here it is held to the fixtures like the host entry (every 4th row)."""
    g = golden
    rows = np.arange(0, len(g['bbox2d']), 4)
    r = PR.batch(g['bbox2d'][rows], g['bbox3d'][rows], g['sin'][rows], g['cos'][rows], g['image_size'], g['proj_mat'], g['proj_inv'])
    ran = g['ran'][rows]
    assert np.array_equal(r['keep'][ran], g['keep'][rows][ran]) and np.array_equal(r['candidate'][ran], g['candidate'][rows][ran])
    assert not r['keep'][~ran].any() and (r['candidate'][~ran] == -2).all()
    kept = rows[g['keep'][rows]]
    assert r['count'] == len(kept) and np.array_equal(rows[r['index']], kept) and np.array_equal(r['box2d'], g['box2d'][kept])
    b_pose, _, b_proj = float_field_bounds(g, kept, roundings=0)
    assert (np.abs(r['pose'].reshape(-1, 16) - g['pose'][kept].reshape(-1, 16)) <= b_pose + 1e-15).all()
    assert (np.abs(r['proj'].reshape(-1, 16) - g['proj'][kept].reshape(-1, 16)) <= b_proj).all()
    assert np.array_equal(r['size'], g['size'][kept])


# ------------------------------------------------------------------------------------------------ by hand
def test_hand_written_case_identity_rotation_on_the_optical_axis(lib):
    """P = focal 100, principal point 0; R = identity; a cube of side 2 centred at (0, 2, 10): below the optical axis (y points down),
    so the box's top edge comes from the FAR top corners (y = 1, z = 11: v = 100 / 11), its bottom edge from the NEAR bottom corners
    (y = 3, z = 9: v = 300 / 9), its sides from the near face (x = -+1, z = 9: u = -+100 / 9).  In getTranslation's tables every ymin
    corner has +dz and every ymax corner -dz, so candidate k = 0 -- xmin (-,-,-), ymin (-,-,+), xmax (+,+,-), ymax (-,+,-) -- is exactly
    this assignment and is the lowest k of its tie class.  The detected box is that box pulled in by half a pixel per edge (an exact fit
    has IoU 1 to the last bit, which the reference's `iou < 1` may reject), so the fit lands a little behind (0, 2, 10)."""
    import src.visualizer.visualizer as vis
    P = np.array([[100.0, 0, 0, 0], [0, 100.0, 0, 0], [0, 0, 1, 0], [0, 0, 0, 1]])
    R = np.eye(3)
    box = np.array([-100 / 9 + 0.5, 100 / 11 + 0.5, 100 / 9 - 0.5, 300 / 9 - 0.5])
    whl = np.array([2.0, 2.0, 2.0])
    X, k, iou = np.zeros(3), ctypes.c_int(-5), ctypes.c_double(0)
    assert lib.vv_pose_translation_host(_p(P), _p(R), _p(box), _p(whl), _p(X), ctypes.byref(k), ctypes.byref(iou)) == 0
    assert k.value == 0 and PR.candidate_corners(0) == ((-1, -1, -1), (-1, -1, 1), (1, 1, -1), (-1, 1, -1))
    assert 0.9 < iou.value < 1.0
    assert abs(X[0]) < 1e-9 and X[2] > 10.0 and abs(X[2] - 10.0) < 1.0 and abs(X[1] - 2.0) < 0.3      # in front of the camera: the sign
    assert np.array_equal(vis.getTranslation(P, R, box, whl).ravel(), X)
    f = PR.fit(P, R, box, 2.0, 2.0, 2.0)
    assert f['candidate'] == 0 and np.abs(f['X'] - X).max() < 1e-9
    # the projected corners of the exact pose, by hand: index 0 = +1, index 1 = -1 along (x, y, z)
    a = vis.get3DbboxProjection(P, R, np.array([0.0, 2.0, 10.0]), 2.0, 2.0, 2.0)
    want = np.zeros((2, 2, 2, 2))
    for i, x in enumerate((1.0, -1.0)):
        for j, y in enumerate((3.0, 1.0)):
            for kk, z in enumerate((11.0, 9.0)):
                want[i, j, kk] = 100 * x / z, 100 * y / z
    assert np.abs(a - want).max() < 1e-12
    assert a[0, 0, 1].tolist() == [100 / 9, 300 / 9]


def test_ties_go_to_the_lowest_k(lib, golden, host):
    """Every candidate tied with the winner has an index >= `candidate`.  Fixture rows first (with a general rotation exact ties are rare);
    then getTranslation itself with a rotation about the vertical axis alone, where they are the rule: an x-row of the constraint matrix
    does not see the corner's vertical offset then, so the loop nest visits bit-identical matrices under different k."""
    g = golden
    for i in g['kept'][:8]:
        r = PR.object_pose(g['bbox2d'][i], g['bbox3d'][i], g['sin'][i], g['cos'][i], g['image_size'], g['proj_mat'], g['proj_inv'])
        tied = np.nonzero(r['fit']['ious'] == r['fit']['iou'])[0]
        assert tied.min() == host['candidate'][i] == g['candidate'][i] and (tied >= host['candidate'][i]).all()
    rng = np.random.default_rng(5)
    P = np.ascontiguousarray(g['proj_mat'])
    for _ in range(6):
        w, h, l = rng.uniform([1.4, 1.3, 3.0], [2.0, 1.9, 5.0])
        t = np.array([rng.uniform(-4, 4), rng.uniform(0.8, 1.8), rng.uniform(10, 40)])
        yaw = rng.uniform(-np.pi, np.pi)
        R = np.array([[np.cos(yaw), 0, np.sin(yaw)], [0, 1, 0], [-np.sin(yaw), 0, np.cos(yaw)]])
        uv = PR.corners_projection(P, R, t, w, h, l).reshape(-1, 2)
        box = np.array([uv[:, 0].min(), uv[:, 1].min(), uv[:, 0].max(), uv[:, 1].max()]) + rng.normal(0, 2, 4)
        f = PR.fit(P, R, box, w, h, l)
        tied = np.nonzero(f['ious'] == f['iou'])[0]
        assert len(tied) > 1 and f['candidate'] == tied.min()
        X, k = np.zeros(3), ctypes.c_int(-5)
        assert lib.vv_pose_translation_host(_p(P), _p(np.ascontiguousarray(R)), _p(box), _p(np.array([w, h, l])), _p(X), ctypes.byref(k), None) == 0
        assert k.value == tied.min() and np.abs(X - f['X']).max() <= GATE * np.abs(f['X']).max()
