"""GPU tests of the detection decode (csrc/detect_decode.hip, voxvae/detect.py, src/module/nolbo_test.py).  The numerics and the
decisions are pinned on the CPU (tests/test_detect_host.py: vv_detect_decode_host against what the reference's getPred selected); here
the DEVICE entry is held to the host entry, which is the same header compiled for the other side: every output equal bit for bit (a NaN
matching any NaN: the sign and payload of a NaN are not part of the contract), on every case, and every case also checks that rows at
or past `count` keep the sentinel they were filled with.
"""
import ctypes

import numpy as np
import pytest
import torch

import _detect_ref as R
import _guarded as G
from test_detect_host import assert_same, same

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
P, Z, W = 5, 16, 49
SENT = 0x5A
WIDTHS = dict(index=1, bbox2d=5, bbox3d=3, inst_mean=None, inst_log_var=None, sin=3, cos=3, rad_log_var=3)


@pytest.fixture(scope='module')
def L():
    import voxvae
    from voxvae import lib
    lib.load()
    assert torch.cuda.is_available()
    voxvae.set_default_device(DEV)
    return lib


@pytest.fixture(scope='module')
def D(L):
    from voxvae import detect
    return detect


def host_entry(D, head, P_, Z_, obj, iou, top_1):
    return R.detections_as_dicts(D.decode_detections(torch.as_tensor(head).cpu(), P_, Z_, obj, iou, top_1, host=True))


def device_entry(L, D, head, P_=P, Z_=Z, obj=0.5, iou=0.5, top_1=True, stream=None):
    """vv_detect_decode on `head` (numpy, or a torch tensor in one of the two layouts) with the outputs pre-filled with a sentinel
    -> a list of per-frame dicts cut to count, after checking that nothing at or past count was written."""
    t, layout = D._as_head(head, torch.device(DEV), P_ * R.width(Z_))
    B, Rr, C = int(t.shape[0]), int(t.shape[1]), int(t.shape[2])
    N = Rr * C * (1 if top_1 else P_)
    fill = lambda n, dt: torch.full((n * 4,), SENT, dtype=torch.uint8, device=DEV).view(dt)
    count = fill(B, torch.int32)
    outs = {k: fill(B * N * (w or Z_), torch.int32 if k == 'index' else torch.float32) for k, w in WIDTHS.items()}
    st = stream if stream is not None else torch.cuda.current_stream(DEV)
    with torch.cuda.stream(st):
        L.call('vv_detect_decode', L.ptr(t), layout, B, Rr, C, P_, Z_, P_ * R.width(Z_), float(obj), float(iou), 1 if top_1 else 0, L.ptr(count),
               *[L.ptr(outs[k]) for k in WIDTHS], ctypes.c_void_p(st.cuda_stream))
    st.synchronize()
    counts = count.cpu().tolist()
    host = {k: outs[k].cpu().numpy().reshape(B, N, w or Z_) for k, w in WIDTHS.items()}      # one copy per output
    res = []
    for b in range(B):
        M = counts[b]
        assert 0 <= M <= N
        d = dict(count=M)
        for k, w in WIDTHS.items():
            rows = host[k][b]
            assert bool((rows[M:].view(np.uint8) == SENT).all()), '%s: a row at or past count was written' % k
            d[k] = rows[:M].reshape((M,) if k == 'index' else (M, w or Z_))
        res.append(d)
    return res


def check(L, D, head, P_=P, Z_=Z, obj=0.5, iou=0.5, top_1=True, stream=None):
    got = device_entry(L, D, head, P_, Z_, obj, iou, top_1, stream)
    assert_same(got, host_entry(D, head, P_, Z_, obj, iou, top_1), 'device against host')
    return got


# ------------------------------------------------------------------------------------------------------------ equality with the host
def test_fixture_frames(L, D):
    for i, g in enumerate(R.golden_frames()):
        got = check(L, D, g['head'], obj=g['obj_thresh'], iou=g['iou_thresh'], top_1=g['top_1'])[0]
        assert np.array_equal(got['index'], g['index']), 'frame %d: the device picks differ from the reference' % i


@pytest.mark.parametrize('case', [(1, 1, 1, 5, 16), (1, 3, 5, 5, 16), (1, 13, 13, 5, 16), (1, 11, 38, 5, 16), (2, 7, 9, 1, 1), (2, 2, 2, 16, 64)],
                         ids=lambda c: 'B%d-%dx%d-P%d-Z%d' % c)
@pytest.mark.parametrize('top_1', [True, False])
def test_seeded_frames(L, D, case, top_1):
    """11x38 is 418 cells: more than one piece of 256, so the carry is exercised; without top_1 it has 2090 slots."""
    B, Rr, C, P_, Z_ = case
    head = R.seeded_head(100 + sum(case), B, Rr, C, P_, Z_, lit=0.15 if Rr * C > 4 else 0.7)
    got = check(L, D, head, P_, Z_, top_1=top_1)
    assert sum(d['count'] for d in got) > 0
    if case == (1, 11, 38, 5, 16):
        lit = (head.reshape(418, P_, -1)[..., 0] > 0).sum()
        assert (not top_1 and lit > 256) or top_1                           # candidates themselves cross a piece of 256
        check(L, D, head, P_, Z_, obj=0.3, iou=0.9, top_1=top_1)            # a high IoU threshold: many picks


def test_batch_of_three_with_an_empty_frame(L, D):
    head = R.seeded_head(3, 3, 6, 9, P, Z, lit=0.3)
    head.reshape(3, 6, 9, P, W)[1, ..., 0] = -6.0
    got = check(L, D, head, top_1=False)
    assert got[1]['count'] == 0 and got[0]['count'] > 0 and got[2]['count'] > 0 and got[0]['count'] != got[2]['count']


# ------------------------------------------------------------------------------------------------------------ stress and edges
def _grid_32x32(identical):
    rng = np.random.default_rng(32)
    f = np.zeros((1, 32, 32, 4, W), np.float32)
    f[..., 0] = rng.uniform(1.0, 4.0, (1, 32, 32, 4))                       # every objectness above the threshold
    f[..., 1:3] = 5.0 if identical else -8.0                                # boxes 148 wide (every IoU ~ 1), or 0.0003 wide
    f[..., 3] = np.float32([-2.0, -0.7, 0.7, 2.0])                          # four centres across the cell: disjoint when small
    f[..., 5:] = rng.normal(0, 1, (1, 32, 32, 4, W - 5))
    return f.reshape(1, 32, 32, 4 * W)


def test_4096_picks_the_scan_worst_case(L, D):
    got = check(L, D, _grid_32x32(False), 4, Z, top_1=False)[0]
    assert got['count'] == 4096 and sorted(got['index'].tolist()) == list(range(4096))
    assert (np.diff(got['bbox2d'][:, 4]) <= 0).all()


def test_identical_boxes_one_pick(L, D):
    head = _grid_32x32(True)
    got = check(L, D, head, 4, Z, top_1=False)[0]
    assert got['count'] == 1
    s = head.reshape(4096, W)[:, 0]
    assert got['index'][0] == np.nonzero(s == s.max())[0].max()


def test_ties(L, D):
    cell = np.zeros((P, W), np.float32)
    cell[:, 0] = -9
    cell[1, :5] = [2.5, -4.0, -4.0, 0.3, -0.3]                              # boxes 0.018 wide, cells 0.053: disjoint
    cell[3, :5] = [2.5, -4.0, -4.0, -0.3, 0.3]
    f = np.tile(cell.reshape(1, 1, 1, -1), (1, 17, 19, 1))                  # 323 cells, two equal predictors each: 646 equal scores
    got = check(L, D, f, top_1=True)[0]
    assert list(got['index']) == [c * P + 1 for c in range(322, -1, -1)]    # lower predictor in the cell, higher candidate first
    got = check(L, D, f, top_1=False, iou=2.0)[0]
    assert list(got['index'][:4]) == [322 * P + 3, 322 * P + 1, 321 * P + 3, 321 * P + 1] and got['count'] == 646
    check(L, D, f, top_1=False, iou=0.1)


def test_on_the_dot_thresholds(L, D):
    head = R.seeded_head(8, 1, 6, 9, P, Z, lit=0.4)
    base = host_entry(D, head, P, Z, 0.5, 2.0, False)[0]                    # nothing suppressed: every candidate's score and box
    scores = base['bbox2d'][:, 4]
    for s in (scores[0], scores[len(scores) // 2], scores[-1]):
        a = check(L, D, head, obj=float(s), iou=2.0, top_1=False)[0]        # equal to a value's objectness: that one is out
        b = check(L, D, head, obj=float(np.nextafter(s, np.float32(0))), iou=2.0, top_1=False)[0]
        assert not (a['bbox2d'][:, 4] == s).any() and (b['bbox2d'][:, 4] == s).any()
    f32, b = np.float32, base['bbox2d']
    ious = []
    js = []
    for j in range(1, min(len(b), 40)):                                     # IoUs the scan evaluates for the first pick
        x, y = b[0, :4], b[j, :4]
        w, h = max(f32(0), f32(min(x[2], y[2]) - max(x[0], y[0]))), max(f32(0), f32(min(x[3], y[3]) - max(x[1], y[1])))
        inter = f32(w * h)
        ious.append(f32(inter / f32(f32(f32(f32(x[3] - x[1]) * f32(x[2] - x[0])) + f32(f32(y[3] - y[1]) * f32(y[2] - y[0]))) - inter)))
        js.append(j)
    pairs = [(v, j) for v, j in zip(ious, js) if 0.02 < v < 0.98][:3]
    assert pairs
    for v, j in pairs:
        check(L, D, head, iou=float(v), top_1=False)                        # equal to this IoU: the first pick does not suppress j
        c = check(L, D, head, iou=float(np.nextafter(v, f32(0))), top_1=False)[0]
        assert base['index'][j] not in c['index']                           # one unit below: it does


def test_nan_and_inf(L, D):
    head = R.seeded_head(77, 2, 6, 9, P, Z, lit=0.4).reshape(2, 6, 9, P, W)
    rng = np.random.default_rng(5)
    for value in (np.nan, np.inf, -np.inf, 100.0, -100.0, 88.8, -104.0, -87.2, 88.7):
        for _ in range(16):
            head[rng.integers(2), rng.integers(6), rng.integers(9), rng.integers(P), rng.integers(8)] = value
            head[rng.integers(2), rng.integers(6), rng.integers(9), rng.integers(P), W - 9 + rng.integers(9)] = value
    head = head.reshape(2, 6, 9, -1)
    for top_1 in (True, False):
        got = check(L, D, head, top_1=top_1, iou=0.3)
    assert np.isinf(got[0]['bbox2d']).any() or np.isinf(got[1]['bbox2d']).any()
    assert check(L, D, np.full((1, 3, 5, P * W), np.nan, np.float32))[0]['count'] == 0
    assert check(L, D, R.seeded_head(1, 1, 3, 5, P, Z), obj=float('nan'))[0]['count'] == 0


def test_activations_agree_with_the_host_on_a_bit_pattern_sweep(L, D):
    """Every activation the kernel applies, through 1x1 frames: h / w = exp, x / y and objectness = sigmoid, sin / cos = tanh, on a
    sweep of bit patterns over every exponent and both signs (the NaNs among them included)."""
    bits = np.arange(0, 2 ** 32, 1048583, dtype=np.uint64).astype(np.uint32)
    assert bits.size == 4096
    x = bits.view(np.float32)
    f = np.zeros((4096, 1, 1, 1, R.width(1)), np.float32)
    f[:, 0, 0, 0, 0] = 30.0                                                 # objectness 1: every frame has its one candidate
    f[:, 0, 0, 0, 1], f[:, 0, 0, 0, 2], f[:, 0, 0, 0, 3], f[:, 0, 0, 0, 4] = x, x[::-1], x, x[::-1]
    f[:, 0, 0, 0, 10:16] = x[:, None]
    got = check(L, D, f.reshape(4096, 1, 1, -1), 1, 1, obj=0.5)
    assert all(d['count'] == 1 for d in got)
    f[:, 0, 0, 0, 0] = x                                                    # and the objectness itself
    check(L, D, f.reshape(4096, 1, 1, -1), 1, 1, obj=0.25)


# ------------------------------------------------------------------------------------------------------------ other checks
def test_two_runs_are_bit_identical_and_a_side_stream_works(L, D):
    head = torch.from_numpy(R.seeded_head(21, 2, 11, 38, P, Z)).to(DEV)
    a = device_entry(L, D, head, top_1=False)
    b = device_entry(L, D, head, top_1=False)
    side = torch.cuda.Stream(device=DEV)
    side.wait_stream(torch.cuda.current_stream(DEV))
    c = check(L, D, head, top_1=False, stream=side)
    for x, y, z in zip(a, b, c):
        for k in R.FIELDS:
            assert x[k].tobytes() == y[k].tobytes() == z[k].tobytes(), k


def _small_structure():
    import src.module.nolbo_test as NT
    from voxvae import synthetic as syn
    s = {k: dict(v) for k, v in NT.config.items()}
    s['encoder_head'].update(filter_num_list=[64], filter_size_list=[3])
    s['decoder'] = syn.make_config(32, 16, True)['decoder']
    return NT, s


def test_both_layouts_and_the_real_head_view(L, D):
    import src.net_core.darknet as darknet
    head = R.seeded_head(5, 2, 6, 9, P, Z, lit=0.3)
    t = torch.from_numpy(head).to(DEV)
    planes = t.permute(0, 3, 1, 2).contiguous().permute(0, 2, 3, 1)
    assert D._as_head(planes, torch.device(DEV), 245)[0].data_ptr() == planes.data_ptr() and D._as_head(planes, torch.device(DEV), 245)[1] == D.NCHW
    assert_same(check(L, D, planes, top_1=False), check(L, D, t, top_1=False), 'planes against channels-innermost')
    torch.manual_seed(2)
    h2d = darknet.head2D('h', (None, None, 32), 245, [32], [3], last_pooling=None, activation='elu', device=DEV)
    with torch.no_grad():
        h2d.last.weight.mul_(6.0)
    out = h2d(torch.randn(2, 4, 7, 32, device=DEV), training=False)        # [2,4,7,245], a permuted view of the conv's result
    # (whichever memory format the convolution chose for its result, the view is one of the two layouts and is read where it is)
    assert D._as_head(out, torch.device(DEV), 245)[0].data_ptr() == out.data_ptr()
    got = check(L, D, out, obj=0.4, top_1=False)
    assert sum(d['count'] for d in got) > 0
    assert_same(R.detections_as_dicts(D.decode_detections(out, obj_thresh=0.4, top_1_pred=False)), got, 'decode_detections on the view')


@pytest.mark.parametrize('layout', ['nhwc', 'nchw'])
@pytest.mark.parametrize('case', [(1, 11, 38, 5, 16, False), (3, 3, 5, 5, 16, True), (2, 2, 2, 16, 64, False)], ids=lambda c: '-'.join(map(str, c)))
def test_guard_banded_buffers(L, D, case, layout):
    """The entry reads and writes only inside what it was given: inputs and outputs between guard bands (tests/_guarded.py), outputs
    pre-filled with 0xFF -- so rows at or past count must still be 0xFF afterwards."""
    B, Rr, C, P_, Z_, top_1 = case
    head = R.seeded_head(sum(case[:5]), B, Rr, C, P_, Z_, lit=0.3)
    want = host_entry(D, head, P_, Z_, 0.5, 0.5, top_1)
    N, CH = Rr * C * (1 if top_1 else P_), P_ * R.width(Z_)
    t = torch.from_numpy(head).to(DEV)
    stored = t.permute(0, 3, 1, 2).contiguous() if layout == 'nchw' else t   # the bytes the kernel reads
    arena = G.Arena(DEV)
    src = arena.input(stored, 'head')
    count = arena.output((B,), torch.int32, 'count')
    outs = {k: arena.output((B, N, w or Z_), torch.int32 if k == 'index' else torch.float32, k) for k, w in WIDTHS.items()}
    arena.commit()
    st = L.load().vv_detect_decode(src.ptr, 1 if layout == 'nchw' else 0, B, Rr, C, P_, Z_, CH, 0.5, 0.5, 1 if top_1 else 0, count.ptr,
                                   *[outs[k].ptr for k in WIDTHS], ctypes.c_void_p(torch.cuda.current_stream(DEV).cuda_stream))
    torch.cuda.synchronize()
    assert st == 0
    arena.check()
    counts = count.tensor.cpu().tolist()
    assert counts == [w['count'] for w in want] and sum(counts) > 0
    for b, M in enumerate(counts):
        for k in WIDTHS:
            rows = outs[k].tensor[b]
            assert same(rows[:M].cpu().numpy().reshape(want[b][k].shape), want[b][k]), k
            assert bool((rows[M:].contiguous().view(torch.uint8) == G.POISON).all()), k


# ------------------------------------------------------------------------------------------------------------ end to end
def test_getpred_and_getobjects_end_to_end(L, D):
    """A Darknet19 + head2D on a 64x96 image (grid 2x3) and a small decoder: getPred = decode_detections(host=True) followed by the
    existing sampled-mean path; getObjects = getSampledObjects fed with the detections."""
    import src.net_core.darknet as darknet
    NT, s = _small_structure()
    torch.manual_seed(7)
    m = NT.nolbo_test(s, backbone_style=darknet.Darknet19)
    with torch.no_grad():
        m._encoder_head.last.weight.mul_(4.0)
    image = np.random.default_rng(9).uniform(0, 1, (1, 64, 96, 3)).astype(np.float32)
    kw = dict(obj_thresh=0.3, IOU_thresh=0.5, top_1_pred=False)
    head = m._head_output(image)[1]
    assert tuple(head.shape) == (1, 2, 3, 245) and head.is_cuda
    # two forward passes of the torch encoder need not give the same bits (the convolution library picks its algorithm per call): the
    # comparisons below are about what follows the head, so every later call sees THIS head output
    m._encoder_backbone = lambda x, training=False: x
    m._encoder_head = lambda x, training=False: head
    hd = D.decode_detections(head.cpu(), P, Z, 0.3, 0.5, False, host=True)
    M = hd.counts()[0]
    assert M >= 1
    b2, b3, sn, cs, rad, mean, lv = hd.numpy(0)
    eps = torch.randn(M, 32, Z, generator=torch.Generator().manual_seed(1)).numpy()
    out = m.getPred(image, get_3D_shape=True, is_sampling=True, _eps=eps, **kw)
    assert len(out) == 7 and out[0].shape == (64, 96, 3)
    for got, want in zip(out[1:6], (b2, b3, sn, cs, rad)):
        assert same(got, want)
    shapes = np.array(m.getSampledShape(mean, lv, 32, _eps=eps)).reshape(M, 32, 32, 32)
    assert out[6].shape == (M, 32, 32, 32) and np.array_equal(out[6], shapes)
    plain = m.getPred(image, get_3D_shape=True, is_sampling=False, **kw)
    assert np.array_equal(plain[6], np.array(m._decoder(mean)).reshape(M, 32, 32, 32))
    assert len(m.getPred(image, get_3D_shape=False, **kw)) == 6
    none = m.getPred(image, obj_thresh=1.0)
    assert none[1].shape == (0, 5) and none[6].size == 0
    # the whole chain: nothing but the counts comes back before the points
    det, poses, cloud = m.getObjects(image, sampling_num=32, _eps=eps, **kw)
    assert det.bbox2d.is_cuda and det.inst_mean.is_cuda and det.counts() == [M]
    want_poses, want_cloud = m.getSampledObjects(mean, lv, b2, b3, sn, cs, (96, 64), 32, _eps=eps)
    for k in ('keep', 'candidate', 'iou', 'count_', 'index', 'pose', 'size', 'box2d', 'box3d_proj'):
        kept = want_poses.count() if k in ('index', 'pose', 'size', 'box2d', 'box3d_proj') else None
        assert torch.equal(getattr(poses, k)[:kept], getattr(want_poses, k)[:kept]), k
    assert (cloud is None) == (want_cloud is None)
    if cloud is not None:
        for x, y in zip(cloud.split(), want_cloud.split()):
            assert np.array_equal(np.asarray(x), np.asarray(y))
    assert m.getObjects(image, obj_thresh=1.0)[1:] == (None, None)
