"""GPU tests of the detection -> world-pose step (csrc/object_pose.hip, voxvae/pose.py, src/visualizer.getObjectInRealWorld,
getSampledObjects).  The numerics are pinned on the CPU (tests/test_pose_host.py: vv_object_pose_host against the reference's recorded
results); here the DEVICE entry is held to the host entry, which is the same header compiled for the other side:

    keep, candidate, count, index, box2d    identical
    iou, pose, size, box3d_proj             within one float32 unit (both sides round once) + GATE x sensitivity, GATE and the
                                            sensitivities those of test_pose_host.py (16 x the measured solver term 2.58e-13)
    two runs                                bit-identical;  rows at or past `count` untouched (sentinel fill);  a non-default stream

n in {1, 2, 63, 64, 65, 257, 1025}: one detection (a dropped one: nothing kept), two kept ones (everything kept), a wave short of / equal
to / one past a quarter compaction piece, one past a piece of 256 (kept rows straddle it), one past four pieces (tiled fixture rows; the
fixture's order interleaves kept and dropped rows).
"""
import ctypes
import functools
import os

import numpy as np
import pytest
import torch

import _points_ref as PTS
import _pose_ref as PR
from test_pose_host import F32, GATE, GOLDEN, float_field_bounds, host_entry

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
SIZES = [1, 2, 63, 64, 65, 257, 1025]
SENT_F, SENT_I = -12345.0, -777


@pytest.fixture(scope='module')
def L():
    import voxvae
    from voxvae import lib
    lib.load()
    assert torch.cuda.is_available()
    voxvae.set_default_device(DEV)
    return lib


@functools.lru_cache(maxsize=None)
def golden():
    g = dict(np.load(GOLDEN))
    g['proj_inv'] = np.linalg.inv(g['proj_mat'])
    g['kept'] = np.nonzero(g['keep'])[0]
    return g


@functools.lru_cache(maxsize=None)
def case_rows(n):
    g = golden()
    if n == 1:
        return np.array([np.nonzero(~g['keep'] & (g['candidate'] == -1))[0][0]])       # fitted, no winner: not kept
    if n == 2:
        return g['kept'][:2].copy()
    return (np.arange(n) + 3 * n) % len(g['keep'])


def device_entry(L, rows, stream=None):
    """vv_object_pose on fixture rows, outputs pre-filled with sentinels -> dict of numpy arrays (NOT cut to count)."""
    g = golden()
    n = len(rows)
    ins = [torch.from_numpy(np.ascontiguousarray(g[k][rows])).to(DEV) for k in ('bbox2d', 'bbox3d', 'sin', 'cos')]
    i32 = lambda *s: torch.full(s, SENT_I, dtype=torch.int32, device=DEV)
    f32 = lambda *s: torch.full(s, SENT_F, dtype=torch.float32, device=DEV)
    o = dict(keep=i32(n), candidate=i32(n), iou=f32(n), count=i32(1), index=i32(n), pose=f32(n, 16), size=f32(n, 3), box2d=i32(n, 4), proj=f32(n, 16))
    need = L.load().vv_object_pose_workspace_bytes(n)
    ws = torch.empty(need, dtype=torch.uint8, device=DEV)
    P, Pinv = np.ascontiguousarray(g['proj_mat']), np.ascontiguousarray(g['proj_inv'])
    s = stream if stream is not None else torch.cuda.current_stream()
    torch.cuda.synchronize()
    L.call('vv_object_pose', *[L.ptr(t) for t in ins], n, float(g['image_size'][0]), float(g['image_size'][1]), P.ctypes.data_as(ctypes.c_void_p),
           Pinv.ctypes.data_as(ctypes.c_void_p), L.ptr(o['keep']), L.ptr(o['candidate']), L.ptr(o['iou']), L.ptr(o['count']), L.ptr(o['index']),
           L.ptr(o['pose']), L.ptr(o['size']), L.ptr(o['box2d']), L.ptr(o['proj']), L.ptr(ws), need, ctypes.c_void_p(s.cuda_stream))
    s.synchronize()
    return {k: v.cpu().numpy() for k, v in o.items()}


@pytest.mark.parametrize('n', SIZES)
def test_device_entry_is_the_host_entry(L, n):
    g = golden()
    rows = case_rows(n)
    h = host_entry(L.load(), g['bbox2d'][rows], g['bbox3d'][rows], g['sin'][rows], g['cos'][rows], g['image_size'], g['proj_mat'], g['proj_inv'])
    side = torch.cuda.Stream(device=DEV)
    d = device_entry(L, rows, stream=side)                         # a non-default stream
    M = int(d['count'][0])
    print('\n[pose n %d] kept %d, pre-filtered / NaN %d, no winner %d' % (n, M, (d['candidate'] == -2).sum(), (d['candidate'] == -1).sum()))
    if n == 1:
        assert M == 0
    elif n == 2:
        assert M == 2
    else:
        assert 0 < M < n and (g['keep'][rows][:-1] != g['keep'][rows][1:]).sum() >= 4
    # exact fields
    assert M == h['count'] and np.array_equal(d['keep'], h['keep']) and np.array_equal(d['candidate'], h['candidate'])
    assert np.array_equal(d['index'][:M], h['index']) and np.array_equal(d['box2d'][:M], h['box2d'])
    ran = g['ran'][rows]
    assert np.array_equal(d['keep'][ran] != 0, g['keep'][rows][ran]) and np.array_equal(d['candidate'][ran], g['candidate'][rows][ran])
    # float fields: one float32 unit (each side rounds once) + the gate
    kept = rows[h['index']]
    b_pose, _, b_proj = float_field_bounds(g, kept, roundings=2)
    e_pose = np.abs(d['pose'][:M].astype(np.float64) - h['pose'].astype(np.float64))
    e_proj = np.abs(d['proj'][:M].astype(np.float64) - h['proj'].astype(np.float64))
    same = np.array_equal(d['pose'][:M], h['pose']) and np.array_equal(d['proj'][:M], h['proj']) and np.array_equal(d['iou'], h['iou'])
    print('[pose n %d] device vs host: bit-identical %s; pose error / bound %.3f, corners %.3f'
          % (n, same, (e_pose / np.maximum(b_pose, 1e-300)).max() if M else 0.0, (e_proj / b_proj).max() if M else 0.0))
    assert (e_pose <= b_pose).all() and (e_proj <= b_proj).all()
    assert np.array_equal(d['size'][:M], h['size'])
    np.testing.assert_allclose(d['iou'], h['iou'], rtol=0, atol=2.0 ** -23 + 16 * GATE)
    # against the reference's recorded values too
    b_pose, _, b_proj = float_field_bounds(g, kept, roundings=1)
    assert (np.abs(d['pose'][:M].astype(np.float64) - g['pose'][kept].reshape(-1, 16)) <= b_pose).all()
    assert (np.abs(d['proj'][:M].astype(np.float64) - g['proj'][kept].reshape(-1, 16)) <= b_proj).all()
    # rows at or past count are untouched
    assert (d['index'][M:] == SENT_I).all() and (d['box2d'][M:] == SENT_I).all()
    assert (d['pose'][M:] == F32(SENT_F)).all() and (d['size'][M:] == F32(SENT_F)).all() and (d['proj'][M:] == F32(SENT_F)).all()
    # a second run, on the default stream: the same bytes
    d2 = device_entry(L, rows)
    assert all(d[k].tobytes() == d2[k].tobytes() for k in d)


def test_python_surface_on_the_device(L):
    from voxvae.pose import object_poses
    from voxvae.tensor import DeviceArray
    g = golden()
    rows = case_rows(65)
    o = object_poses(DeviceArray(torch.from_numpy(g['bbox2d'][rows]).to(DEV)), g['bbox3d'][rows], torch.from_numpy(g['sin'][rows]).to(DEV),
                     g['cos'][rows], g['image_size'])
    d = device_entry(L, rows)
    M = o.count()
    assert M == int(d['count'][0]) and o.pose.is_cuda and o.index.dtype == torch.int32
    pose, size, box, proj = o.numpy()
    assert np.array_equal(pose.reshape(M, 16), d['pose'][:M]) and np.array_equal(proj.reshape(M, 16), d['proj'][:M])
    assert np.array_equal(size, d['size'][:M]) and np.array_equal(box, d['box2d'][:M]) and np.array_equal(o.keep.cpu().numpy(), d['keep'])
    empty = object_poses(np.zeros((0, 5), F32), np.zeros((0, 3), F32), np.zeros((0, 3), F32), np.zeros((0, 3), F32), g['image_size'])
    assert empty.count() == 0 and empty.points(np.zeros((0, 4, 4, 4), F32)) is None


def _grids(rng, n, D):
    """Seeded probabilities confined to a random box per object (at least two cells apart in some axis)."""
    p = rng.random((n, D, D, D)).astype(F32)
    for b in range(n):
        a, z = rng.integers(0, D // 4, 3), D - rng.integers(0, D // 4, 3)
        keep = np.zeros((D,) * 3, dtype=bool)
        keep[a[0]:z[0], a[1]:z[1], a[2]:z[2]] = True
        p[b][~keep] *= F32(0.25)
    return p


def test_getObjectInRealWorld_end_to_end(L):
    """D = 16, 5 detections (3 kept, one pre-filtered, one without a winner) against the fixture poses and tests/_points_ref.py."""
    import src.visualizer.visualizer as vis
    g = golden()
    pre = np.nonzero((g['candidate'] == -2) & g['ran'])[0][0]
    none = np.nonzero(g['candidate'] == -1)[0][0]
    rows = np.array([g['kept'][3], pre, g['kept'][40], none, g['kept'][200]])
    p = _grids(np.random.default_rng(16), 5, 16)
    shapes = [p[i].reshape(16, 16, 16, 1) for i in range(5)]
    objsPose, objsSize, objsPoints, objsBox, objsProj = vis.getObjectInRealWorld(g['bbox2d'][rows], g['bbox3d'][rows], g['sin'][rows], g['cos'][rows],
                                                                                 shapes, tuple(g['image_size']))
    kept = rows[[0, 2, 4]]
    assert objsPose.shape == (3, 4, 4) and objsSize.shape == (3, 3) and objsBox.shape == (3, 4) and objsProj.shape == (3, 2, 2, 2, 2)
    assert isinstance(objsPoints, list) and len(objsPoints) == 3
    assert np.array_equal(objsBox, g['box2d'][kept]) and np.array_equal(objsSize.astype(np.float64), g['size'][kept])
    b_pose, _, b_proj = float_field_bounds(g, kept)
    assert (np.abs(objsPose.reshape(3, 16).astype(np.float64) - g['pose'][kept].reshape(3, 16)) <= b_pose).all()
    assert (np.abs(objsProj.reshape(3, 16).astype(np.float64) - g['proj'][kept].reshape(3, 16)) <= b_proj).all()
    for j, src in enumerate((0, 2, 4)):
        h, l, w = g['size'][kept[j]]
        pose32 = objsPose[j].astype(np.float64)                   # the points are posed with the float32 pose the call returned
        want, _ = PTS.object_points(PTS.occupancy(p[src]), h, w, l, pose32)
        assert objsPoints[j].shape == want.shape and len(want) > 0
        bound = PTS.affine_bound([[h, w, l]], pose32[None])[0]
        assert (np.abs(objsPoints[j].astype(np.float64) - want) <= bound).all()
    # the same grids as one device tensor: the same bytes
    again = vis.getObjectInRealWorld(g['bbox2d'][rows], g['bbox3d'][rows], g['sin'][rows], g['cos'][rows], torch.from_numpy(p).to(DEV),
                                     tuple(g['image_size']))
    assert all(np.array_equal(a, b) for a, b in zip(again[2], objsPoints)) and np.array_equal(again[0], objsPose)
    nothing = vis.getObjectInRealWorld(g['bbox2d'][rows[[1, 3]]], g['bbox3d'][rows[[1, 3]]], g['sin'][rows[[1, 3]]], g['cos'][rows[[1, 3]]],
                                       shapes[:2], tuple(g['image_size']))
    assert nothing[0].shape == (0, 4, 4) and nothing[2] == [] and nothing[4].shape == (0, 2, 2, 2, 2)


def test_getSampledObjects_is_getSampledShape_then_poses_then_points(L):
    """The 16^3 model of the existing goldens (vae_d16_l64_b3): three detections, the middle one pre-filtered."""
    import voxvae
    from voxvae import synthetic as syn
    from voxvae.points import voxel_points
    from voxvae.pose import object_poses
    import src.module.nolbo as nolbo
    voxvae.set_default_dtype('f32')
    voxvae.set_default_device(DEV)
    cfg = syn.make_config(16, 64, True)
    m = nolbo.nolboSingleObject_modelnet_category_VAE(nolbo_structure=cfg)
    m._encoder.set_weights_dict(syn.make_encoder_params(cfg['encoder']))
    m._decoder.set_weights_dict(syn.make_decoder_params(cfg['decoder']))
    B, K = 3, 4
    mean, logvar = m._posterior(torch.from_numpy(syn.make_voxels(B, 16)).to(DEV))
    eps = syn.make_eps(B * K, 64, seed=11).reshape(B, K, 64)
    g = golden()
    pre = np.nonzero((g['candidate'] == -2) & g['ran'])[0][0]
    rows = np.array([g['kept'][5], pre, g['kept'][6]])
    det = (g['bbox2d'][rows], g['bbox3d'][rows], g['sin'][rows], g['cos'][rows], tuple(g['image_size']))
    grid = m.getSampledShape(mean, logvar, K, _eps=eps)
    prob = float(np.median(np.array(grid)))                        # about half the cells, whatever the weights make of 0.5
    poses, cloud = m.getSampledObjects(mean, logvar, *det, sampling_num=K, prob=prob, _eps=eps)
    assert poses.count() == 2 and poses.index[:2].tolist() == [0, 2] and poses.keep.tolist() == [1, 0, 1]
    sep = object_poses(*det)
    pick = grid.t.index_select(0, torch.tensor([0, 2], device=DEV))
    want = voxel_points(pick, sep.size[:2], sep.pose[:2].reshape(2, 4, 4), prob=prob)
    assert len(cloud) == 2 and cloud.total() == want.total() > 0
    for a, b in ((cloud.points, want.points), (cloud.offsets, want.offsets), (cloud.counts, want.counts), (cloud.bbox, want.bbox),
                 (poses.pose[:2], sep.pose[:2]), (poses.box3d_proj[:2], sep.box3d_proj[:2])):
        assert a.shape == b.shape and a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes()
    assert np.array_equal(cloud.counts.cpu().numpy(), (np.array(grid)[[0, 2]].reshape(2, -1) > F32(prob)).sum(axis=1))
