"""CPU tests of the detection decode: the host entry vv_detect_decode_host -- the code the kernel runs, compiled for the CPU --
against what the reference's own getPred selected (tests/golden/detect_frames.npz, recorded by tests/golden/make_detect_golden.py) and,
where the fixture has no frame, against our numpy statement tests/_detect_ref.py, which is held to the fixture in the same way.

Figures (measured here, recorded in tests/_detect_ref.py and DESIGN 4h):
  host entry against the reference's float fields over the fixture: at most 1.19e-7 (one float32 unit at 1); the gate is 4 x that.
  activations against float64 numpy over 2^20 random bit patterns each plus ends and clamp points: exp 0.987, sigmoid 2.223, tanh 1.254
  float32 units (tests/_detect_ref.ACT_MAX_ULP); the gate is 2 x those.
"""
import ctypes
import os

import numpy as np
import pytest
import torch

from _common import build_and_run_sanitized
import _detect_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P, Z, W = 5, 16, 49


@pytest.fixture(scope='module')
def D():
    from voxvae import build as vb
    vb.build()
    from voxvae import detect
    return detect


@pytest.fixture(scope='module')
def golden():
    return R.golden_frames()


def host(D, head, P_=P, Z_=Z, obj=0.5, iou=0.5, top_1=True):
    return R.detections_as_dicts(D.decode_detections(head, P_, Z_, obj, iou, top_1, host=True))


def same(a, b):
    """Bit for bit, a NaN matching any NaN (sign and payload of a NaN are not part of the contract)."""
    a, b = np.asarray(a), np.asarray(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    if a.dtype.kind != 'f':
        return bool(np.array_equal(a, b))
    na, nb = np.isnan(a), np.isnan(b)
    return bool(np.array_equal(na, nb) and np.array_equal(a.view(np.uint32)[~na], b.view(np.uint32)[~nb]))


def assert_same(got, want, what=''):
    assert len(got) == len(want), what
    for b, (g, w) in enumerate(zip(got, want)):
        assert g['count'] == w['count'], '%s frame %d: count %d, expected %d' % (what, b, g['count'], w['count'])
        for k in R.FIELDS:
            assert same(g[k], w[k]), '%s frame %d: %s differs' % (what, b, k)


def frame_1x1(rows):
    """[1,1,1,P*W] with predictor p's (objectness logit, h, w, x, y logits) = rows[p]; everything else zero."""
    f = np.zeros((1, 1, 1, len(rows), W), np.float32)
    for p, r in enumerate(rows):
        f[0, 0, 0, p, :len(r)] = r
    return f.reshape(1, 1, 1, -1)


# ------------------------------------------------------------------------------------------------------------------ 1. the fixture
def test_host_entry_against_the_fixture(D, golden):
    worst = 0.0
    for i, g in enumerate(golden):
        got = host(D, g['head'], obj=g['obj_thresh'], iou=g['iou_thresh'], top_1=g['top_1'])[0]
        n = len(g['index'])
        assert got['count'] == n, 'frame %d: %d picks, the reference %d' % (i, got['count'], n)
        assert np.array_equal(got['index'], g['index']), 'frame %d: picks or their order differ' % i
        raw = g['head'].reshape(-1, W)[g['index']]                         # the picked predictors' raw channels
        assert same(got['inst_mean'], raw[:, 8:8 + Z]) and same(got['inst_log_var'], raw[:, 8 + Z:8 + 2 * Z]), i
        assert same(got['rad_log_var'], g['rad']) and same(got['rad_log_var'], raw[:, W - 3:]), i
        assert same(got['bbox3d'], np.maximum(raw[:, [6, 5, 7]], np.float32(0))), 'frame %d: bbox3D is (field 1, field 0, field 2), relu' % i
        assert same(got['bbox3d'], g['bbox3D']), i
        for ours, theirs in ((got['bbox2d'], g['bbox2D']), (got['sin'], g['sin']), (got['cos'], g['cos'])):
            assert ours.shape == theirs.shape
            if ours.size:
                d = float(np.abs(ours.astype(np.float64) - theirs).max())
                worst = max(worst, d)
                assert d <= R.FIXTURE_TOL, 'frame %d: %.3e' % (i, d)
    print('\nhost entry against the reference over %d frames: largest float difference %.4e (recorded %.4e, gate 4 x)' % (
        len(golden), worst, R.FIXTURE_MAX_DIFF))
    assert sum(len(g['index']) for g in golden) > 40


def test_fixture_holds_what_the_issue_lists(golden):
    grids = {g['head'].shape[1:3] for g in golden}
    assert grids == {(1, 1), (3, 5), (6, 9), (13, 13)}
    assert {(g['obj_thresh'], g['iou_thresh'], g['top_1']) for g in golden} == {(0.5, 0.5, True), (0.5, 0.5, False), (0.3, 0.4, False), (0.7, 0.2, True)}
    hostile = golden[-1]['head']
    assert np.isnan(hostile).any() and (hostile == 100.0).any()
    assert np.isinf(golden[-1]['held_bbox2D']).any()                       # exp(100) = inf in the reference's activated field too
    assert os.path.getsize(R.GOLDEN) < 1000000


def test_numpy_statement_against_the_fixture(golden):
    """tests/_detect_ref.py is held to the reference like the host entry (its activations are numpy's: decisions have margins)."""
    for i, g in enumerate(golden):
        got = R.decode_frame(g['head'][0], P, Z, g['obj_thresh'], g['iou_thresh'], g['top_1'])
        assert np.array_equal(got['index'], g['index']), i
        assert same(got['bbox3d'], g['bbox3D']) and same(got['rad_log_var'], g['rad'])
        for ours, theirs in ((got['bbox2d'], g['bbox2D']), (got['sin'], g['sin']), (got['cos'], g['cos'])):
            assert ours.size == 0 or float(np.abs(ours.astype(np.float64) - theirs).max()) <= R.FIXTURE_TOL, i


# ------------------------------------------------------------------------------------------------------------------ 2. layouts
@pytest.mark.parametrize('shape', [(1, 1, 1, 5, 16, True), (2, 3, 5, 5, 16, False), (1, 13, 13, 5, 16, True), (1, 11, 38, 5, 16, False),
                                   (2, 4, 3, 1, 1, False), (1, 2, 2, 16, 64, False)])
def test_both_layouts_identical_and_equal_to_the_numpy_statement(D, shape):
    B, Rr, C, P_, Z_, top_1 = shape
    head = R.seeded_head(sum(shape), B, Rr, C, P_, Z_, lit=0.15 if Rr * C > 4 else 0.7)
    t = torch.from_numpy(head)
    planes = t.permute(0, 3, 1, 2).contiguous().permute(0, 2, 3, 1)         # what the torch head returns: an NCHW tensor, permuted
    if Rr * C > 1:                                                          # (one cell: the two layouts are the same bytes)
        assert not planes.is_contiguous() and D._as_head(planes, torch.device('cpu'), head.shape[-1])[1] == D.NCHW
    assert D._as_head(t, torch.device('cpu'), head.shape[-1])[1] == D.NHWC
    assert D._as_head(planes, torch.device('cpu'), head.shape[-1])[0].data_ptr() == planes.data_ptr()       # no copy
    a, b = host(D, t, P_, Z_, top_1=top_1), host(D, planes, P_, Z_, top_1=top_1)
    assert_same(a, b, 'NHWC against NCHW')
    assert_same(a, R.decode(head, P_, Z_, 0.5, 0.5, top_1, act='entry'), 'against tests/_detect_ref.py')
    assert sum(d['count'] for d in a) > 0
    sliced = t[:, :, :, :].transpose(1, 2)                                  # neither layout: copied
    if Rr != C and Rr > 1 and C > 1:
        assert D._as_head(sliced, torch.device('cpu'), head.shape[-1])[0].data_ptr() != sliced.data_ptr()


# ------------------------------------------------------------------------------------------------------------------ 3. decisions
def test_objectness_threshold_is_strict(D):
    f = frame_1x1([[1.25, -2, -2, 0, 0]] + [[-9]] * 4)
    s = float(D.activation_host(np.float32([1.25]), 'sigmoid')[0])
    assert host(D, f, obj=s)[0]['count'] == 0                               # equal: not a candidate
    below = float(np.nextafter(np.float32(s), np.float32(0)))
    got = host(D, f, obj=below)[0]
    assert got['count'] == 1 and got['index'][0] == 0 and got['bbox2d'][0, 4] == np.float32(s)
    assert host(D, f, obj=float('nan'))[0]['count'] == 0


def test_iou_threshold_is_strict(D):
    # two cells, one candidate each, overlapping boxes
    f = np.zeros((1, 1, 2, P, W), np.float32)
    f[..., 0] = -9
    f[0, 0, 0, 0, :5] = [2.0, -0.5, -0.6, 1.5, 0.2]
    f[0, 0, 1, 0, :5] = [1.0, -0.4, -0.7, -1.5, -0.1]
    f = f.reshape(1, 1, 2, -1)
    both = host(D, f, iou=2.0)[0]
    assert both['count'] == 2 and list(both['index']) == [0, 5]
    a, b = both['bbox2d'][0, :4], both['bbox2d'][1, :4]
    f32 = np.float32
    area = lambda v: f32(f32(v[3] - v[1]) * f32(v[2] - v[0]))
    w, h = max(f32(0), f32(min(a[2], b[2]) - max(a[0], b[0]))), max(f32(0), f32(min(a[3], b[3]) - max(a[1], b[1])))
    inter = f32(w * h)
    iou = f32(inter / f32(f32(area(a) + area(b)) - inter))
    assert 0.05 < iou < 0.95
    assert host(D, f, iou=float(iou))[0]['count'] == 2                      # equal: not suppressed
    assert host(D, f, iou=float(np.nextafter(iou, f32(0))))[0]['count'] == 1
    assert R.suppresses(a, b, np.nextafter(iou, f32(0))) and not R.suppresses(a, b, iou)


def test_ties_inside_a_cell_go_to_the_lower_predictor(D):
    f = frame_1x1([[-9], [2.5, -2, -2, 0, 0], [-9], [2.5, -1, -1, 1, 1], [0.5]])
    got = host(D, f, top_1=True)[0]
    assert got['count'] == 1 and got['index'][0] == 1
    # without top_1 both are candidates, in the cell's order 1, 3; among equal candidates the HIGHER candidate index is picked first
    got = host(D, f, top_1=False, iou=2.0)[0]
    assert list(got['index']) == [3, 1, 4]
    assert_same([got], R.decode(f, P, Z, 0.5, 2.0, False, act='entry'))


def test_ties_across_cells_go_to_the_higher_candidate(D):
    cell = np.zeros((P, W), np.float32)
    cell[:, 0] = -9
    cell[2, :5] = [1.75, -2.0, -2.0, 0.3, -0.3]
    f = np.tile(cell.reshape(1, 1, 1, -1), (1, 2, 3, 1))                    # six cells with the same logits: six equal scores
    got = host(D, f, iou=0.5)[0]                                            # boxes 0.135 wide on a 2 x 3 grid: disjoint
    assert list(got['index']) == [c * P + 2 for c in (5, 4, 3, 2, 1, 0)]
    wide = f.copy().reshape(1, 2, 3, P, W)
    wide[..., 2, 1:3] = 2.0                                                 # boxes 7.4 wide: every pair overlaps with IoU > 0.5
    got = host(D, wide.reshape(f.shape), iou=0.5)[0]
    assert list(got['index']) == [5 * P + 2]
    assert_same([got], R.decode(wide.reshape(f.shape), P, Z, 0.5, 0.5, True, act='entry'))


def test_nan_and_inf_frames(D):
    head = R.seeded_head(77, 1, 6, 9, P, Z, lit=0.4).reshape(1, 6, 9, P, W)
    rng = np.random.default_rng(5)
    for value in (np.nan, np.inf, -np.inf, 100.0, -100.0, 88.8, -104.0):
        for _ in range(12):
            head[0, rng.integers(6), rng.integers(9), rng.integers(P), rng.integers(8)] = value        # objectness and box fields
        head[0, rng.integers(6), rng.integers(9), rng.integers(P), W - 9 + rng.integers(9)] = value    # angles
    head = head.reshape(1, 6, 9, -1)
    for top_1 in (True, False):
        got = host(D, head, top_1=top_1, iou=0.3)
        assert_same(got, R.decode(head, P, Z, 0.5, 0.3, top_1, act='entry'), 'top_1 %s' % top_1)
        b = got[0]['bbox2d']
        assert not np.isnan(b[:, 4]).any() and (b[:, 4] > 0.5).all()        # a NaN is never a candidate
    assert np.isinf(got[0]['bbox2d'][:, :4]).any() and np.isnan(got[0]['bbox2d'][:, :4]).any()   # such candidates exist and are kept
    allnan = np.full((1, 3, 5, P * W), np.nan, np.float32)
    assert host(D, allnan)[0]['count'] == 0 and host(D, allnan, top_1=False)[0]['count'] == 0


def test_an_infinite_box_suppresses_nothing(D):
    """IoU of an infinite box with anything is inf / inf = NaN: both stay."""
    f = np.zeros((1, 1, 2, P, W), np.float32)
    f[..., 0] = -9
    f[0, 0, 0, 0, :5] = [3.0, 100.0, 100.0, 0, 0]
    f[0, 0, 1, 0, :5] = [1.0, -1.0, -1.0, 0, 0]
    got = host(D, f.reshape(1, 1, 2, -1), iou=0.0)[0]
    assert got['count'] == 2 and np.isinf(got['bbox2d'][0, :4]).all()


def test_empty_frame_and_unequal_counts(D):
    head = R.seeded_head(3, 3, 3, 5, P, Z, lit=0.3)
    head.reshape(3, 3, 5, P, W)[1, ..., 0] = -6.0                           # frame 1: nothing above the threshold
    got = host(D, head, top_1=False)
    assert got[1]['count'] == 0 and got[0]['count'] > 0 and got[2]['count'] > 0 and got[0]['count'] != got[2]['count']
    assert_same(got, R.decode(head, P, Z, 0.5, 0.5, False, act='entry'))
    det = D.decode_detections(head, host=True, top_1_pred=False)
    b2, b3, sn, cs, rad, mean, lv = det.numpy(1)
    assert b2.shape == (0, 5) and b3.shape == (0, 3) and mean.shape == (0, Z) and rad.shape == (0, 3)


def test_rows_past_count_are_not_written(D):
    from voxvae import lib as L
    head = torch.from_numpy(R.seeded_head(9, 2, 3, 5, P, Z))
    N = 15
    outs = [torch.full(s, 0x5A, dtype=torch.uint8).view(dt) for s, dt in (((2 * 4,), torch.int32), ((2 * N * 4,), torch.int32),
            ((2 * N * 5 * 4,), torch.float32), ((2 * N * 3 * 4,), torch.float32), ((2 * N * Z * 4,), torch.float32), ((2 * N * Z * 4,), torch.float32),
            ((2 * N * 3 * 4,), torch.float32), ((2 * N * 3 * 4,), torch.float32), ((2 * N * 3 * 4,), torch.float32))]
    L.call('vv_detect_decode_host', L.ptr(head), 0, 2, 3, 5, P, Z, P * W, 0.5, 0.5, 1, *[L.ptr(o) for o in outs])
    counts = outs[0].tolist()
    for o, width_ in zip(outs[1:], (1, 5, 3, Z, Z, 3, 3, 3)):
        rows = o.view(torch.uint8).view(2, N, width_ * 4)
        for b in range(2):
            assert 0 < counts[b] < N and bool((rows[b, counts[b]:] == 0x5A).all()) and not bool((rows[b, :counts[b]] == 0x5A).all())


# ------------------------------------------------------------------------------------------------------------------ 4. activations
def _ulp_error(got, want64):
    """|got - want| in units of the float32 spacing at want (the normal range; the clamps keep results out of the subnormals)."""
    want32 = want64.astype(np.float32)
    spacing = np.spacing(np.maximum(np.abs(want32), np.float32(1.1754944e-38))).astype(np.float64)
    return np.abs(got.astype(np.float64) - want64) / spacing


def test_activations_against_float64(D):
    rng = np.random.default_rng(2024)
    figures = {}
    for which, lo, hi, fn in (('exp', -87.3, 88.72283, np.exp), ('sigmoid', -87.0, 30.0, lambda v: 1.0 / (1.0 + np.exp(-v))),
                              ('tanh', -12.0, 12.0, np.tanh)):
        # 2^20 random float32 BIT PATTERNS in range: a random sign, exponent and mantissa, so that tiny arguments are covered as well
        bits = rng.integers(0, 2 ** 32, size=3 * 2 ** 20, dtype=np.uint64).astype(np.uint32)
        x = bits.view(np.float32)
        x = x[np.isfinite(x) & (x >= np.float32(lo)) & (x <= np.float32(hi))][:2 ** 20]
        assert x.size == 2 ** 20
        ends = np.float32([lo, hi, 0.0, -0.0, 0.625, -0.625, np.nextafter(np.float32(0.625), np.float32(0)), 10.0, -10.0, 1e-30, -1e-30,
                           0.34657359, -0.34657359, 1.0, -1.0])
        ends = ends[(ends >= np.float32(lo)) & (ends <= np.float32(hi))]
        x = np.concatenate([x, ends, rng.uniform(lo, hi, 2 ** 18).astype(np.float32)])
        got = D.activation_host(x, which)
        with np.errstate(all='ignore'):
            err = _ulp_error(got, fn(x.astype(np.float64)))
        figures[which] = float(err.max())
        assert figures[which] <= 2 * R.ACT_MAX_ULP[which], '%s: %.3f float32 units at x = %r' % (which, figures[which], float(x[err.argmax()]))
    print('\nactivations against float64, largest error in float32 units: ' + ', '.join('%s %.3f' % kv for kv in figures.items()))


def test_activation_ends_and_clamps(D):
    f32 = np.float32
    act = lambda v, which: D.activation_host(f32(v), which)
    big = f32(88.72283)                                                     # the largest float whose exponential is finite
    e = act([big, np.nextafter(big, f32(100)), 100.0, np.inf, -87.3, np.nextafter(f32(-87.3), f32(-100)), -200.0, -np.inf, 0.0, np.nan], 'exp')
    assert np.isfinite(e[0]) and abs(float(e[0]) / float(np.exp(np.float64(big))) - 1) < 3e-7
    with np.errstate(all='ignore'):
        assert np.isinf(np.exp(np.nextafter(big, f32(100))))               # numpy's float32 exp overflows at the same argument
    assert np.isinf(e[1]) and np.isinf(e[2]) and np.isinf(e[3]) and e[4] > 1.17549435e-38 and e[5] == 0 and e[6] == 0 and e[7] == 0
    assert e[8] == 1 and np.isnan(e[9])
    s = act([-87.0, np.nextafter(f32(-87.0), f32(-100)), -1000.0, -np.inf, 0.0, 17.0, 1000.0, np.inf, np.nan], 'sigmoid')
    assert s[0] > 1.17549435e-38 and s[1] == 0 and s[2] == 0 and s[3] == 0 and s[4] == 0.5 and s[5] == 1 and s[6] == 1 and s[7] == 1 and np.isnan(s[8])
    t = act([0.0, -0.0, 10.0, np.nextafter(f32(10.0), f32(11)), -50.0, np.inf, -np.inf, np.nan, 1e-20, -1e-20], 'tanh')
    assert t[0] == 0 and not np.signbit(t[0]) and t[1] == 0 and np.signbit(t[1]) and t[2] == 1 and t[3] == 1 and t[4] == -1 and t[5] == 1 and t[6] == -1
    assert np.isnan(t[7]) and t[8] == f32(1e-20) and t[9] == f32(-1e-20)
    x = np.linspace(-12, 12, 4001).astype(np.float32)
    assert np.array_equal(act(-x, 'tanh'), -act(x, 'tanh'))                 # odd, bit for bit
    assert (np.diff(act(np.sort(x), 'tanh')) >= 0).all() and (np.diff(act(np.sort(x), 'sigmoid')) >= 0).all()


# ------------------------------------------------------------------------------------------------------------------ 5. error codes
def test_error_codes(D):
    from voxvae import lib as L
    lib = L.load()
    head = np.zeros((1, 2, 2, 16 * (17 + 2 * 64)), np.float32)
    outs = [np.zeros(4096 * 64 + 8, np.float32) for _ in range(9)]
    ptr = lambda a, off=0: ctypes.c_void_p(a.ctypes.data + off)

    def call(fn, head_ptr=None, layout=0, B=1, Rr=2, C=2, P_=5, Z_=16, CH=None, top_1=1, outs_=None, drop=None):
        o = [ptr(a) for a in outs] if outs_ is None else outs_
        if drop is not None:
            o[drop] = None
        extra = (None,) if fn == 'vv_detect_decode' else ()
        return getattr(lib, fn)(ptr(head) if head_ptr is None else head_ptr, layout, B, Rr, C, P_, Z_, P_ * (17 + 2 * Z_) if CH is None else CH,
                                0.5, 0.5, top_1, *o, *extra)

    for fn in ('vv_detect_decode_host', 'vv_detect_decode'):                # validation comes before any launch: no GPU needed
        if fn == 'vv_detect_decode_host':
            assert call(fn) == 0
        assert call(fn, head_ptr=ctypes.c_void_p(None)) == -1
        for k in range(9):
            assert call(fn, drop=k) == -1, k
        assert call(fn, P_=0, CH=0) == -2 and call(fn, P_=17) == -2 and call(fn, Z_=65) == -2 and call(fn, Z_=0) == -2
        assert call(fn, B=0) == -2 and call(fn, Rr=0) == -2 and call(fn, layout=2) == -2
        assert call(fn, CH=244) == -2 and call(fn, CH=246) == -2            # channels != P * W
        if fn == 'vv_detect_decode_host':
            assert call(fn, Rr=64, C=64, P_=1, Z_=1, top_1=0) == 0          # 4096 slots: the limit itself
        assert call(fn, Rr=4097, C=1, top_1=1) == -2 and call(fn, Rr=64, C=64, P_=2, Z_=1, top_1=0) == -2      # 4097 / 8192 slots
        assert call(fn, head_ptr=ptr(head, 2)) == -4                        # a misaligned float pointer
        o = [ptr(a) for a in outs]
        o[3] = ptr(outs[3], 1)
        assert call(fn, outs_=o) == -4
    with pytest.raises(ValueError):
        D.decode_detections(np.zeros((1, 2, 2, 244), np.float32), host=True)
    with pytest.raises(ValueError):
        D.decode_detections(np.zeros((1, 65, 64, 245), np.float32), host=True)


@pytest.mark.skipif(torch.cuda.is_available(), reason='checks the no-GPU failure mode')
def test_no_silent_fallback_without_a_gpu(D):
    from voxvae import lib as L
    with pytest.raises(L.VoxVaeError):
        D.decode_detections(np.zeros((1, 2, 2, 245), np.float32))


# ------------------------------------------------------------------------------------------------------------------ 6. nolbo_test
class _TinyBackbone(object):
    """images [B,H,W,3] -> features [B,H/32,W/32,8] on the CPU: stands where Darknet19 stands."""
    output_shape = (None, None, None, 8)

    def __call__(self, x, training=False):
        x = torch.as_tensor(np.asarray(x), dtype=torch.float32)
        pooled = torch.nn.functional.avg_pool2d(x.permute(0, 3, 1, 2), 32)
        return torch.cat([pooled, pooled * 0.5, pooled[:, :2] - 0.3], 1).permute(0, 2, 3, 1)


def _structure(P_, Z_):
    import src.module.nolbo_test as NT
    s = {k: dict(v) for k, v in NT.config.items()}
    s['encoder_backbone'].update(predictor_num=P_, z_inst_dim=Z_)
    s['encoder_head'].update(output_dim=P_ * (17 + 2 * Z_), filter_num_list=[16], filter_size_list=[3])
    return NT, s


def test_partition_widths(D):
    for P_, Z_ in ((5, 16), (3, 7), (1, 1), (16, 64)):
        part = D.partition(P_, Z_)
        assert D.channel_width(Z_) == 17 + 2 * Z_
        assert part['objness'][0] == (0, 1) and part['rad_log_var'][-1][1] == P_ * (17 + 2 * Z_)
        assert [b - a for a, b in part['inst_mean']] == [Z_] * P_ and [b - a for a, b in part['sin']] == [3] * P_
        flat = sorted(r for v in part.values() for r in v)
        assert all(flat[i][1] == flat[i + 1][0] for i in range(len(flat) - 1))      # the fields tile the channels in order
        p1 = [part[k][P_ - 1] for k in ('objness', 'bbox2D', 'bbox3D', 'inst_mean', 'inst_log_var', 'sin', 'cos', 'rad_log_var')]
        assert p1 == sorted(p1)
    import src.module.nolbo_test as NT
    assert NT.config['encoder_head']['output_dim'] == 245 and NT.config['encoder_backbone']['z_inst_dim'] == 16
    assert NT.config['decoder']['output_shape'] == [64, 64, 64, 1] and NT.config['decoder']['name'] == 'docoder'


@pytest.mark.parametrize('P_,Z_', [(5, 16), (3, 7)])
def test_getpred_tuple_through_the_host_entry(D, P_, Z_):
    NT, s = _structure(P_, Z_)
    torch.manual_seed(11)
    m = NT.nolbo_test(s, encoder_backbone=_TinyBackbone())
    with torch.no_grad():
        m._encoder_head.last.weight.mul_(8.0)                               # objectness logits of a few units either way
    image = np.random.default_rng(4).uniform(0, 1, (64, 160, 3)).astype(np.float32)        # grid 2 x 5; no batch axis, as callers pass it
    out = m.getPred(image, obj_thresh=0.4, IOU_thresh=0.5, top_1_pred=False, get_3D_shape=False, host=True)
    assert len(out) == 6
    img, b2, b3, sn, cs, rad = out
    n = len(b2)
    assert 0 < n <= 2 * 5 * P_ and img.shape == (64, 160, 3) and m._gridSize == [5, 2]
    assert b2.shape == (n, 5) and b3.shape == (n, 3) and sn.shape == (n, 3) and cs.shape == (n, 3) and rad.shape == (n, 3)
    assert all(a.dtype == np.float32 for a in (b2, b3, sn, cs, rad))
    assert (np.diff(b2[:, 4]) <= 0).all() and (b2[:, 4] > 0.4).all()        # pick order: descending objectness
    head = m._enc_output.detach().cpu().numpy()
    want = R.decode(head[:1], P_, Z_, 0.4, 0.5, False, act='entry')[0]
    assert same(b2, want['bbox2d']) and same(b3, want['bbox3d']) and same(sn, want['sin']) and same(cs, want['cos']) and same(rad, want['rad_log_var'])
    gray = m.getPred(image[..., 0], obj_thresh=0.4, top_1_pred=True, get_3D_shape=False, host=True)
    assert gray[0].shape == (64, 160, 3) and len(gray[1]) <= 10
    assert m._encOutPartitioning() == D.partition(P_, Z_)
    with pytest.raises(ValueError):
        m.getPred(image, get_3D_shape=False, host=True, image_reduced=16)   # the head's grid is not the image's / 16


# ------------------------------------------------------------------------------------------------------------------ 7. sanitizers
@pytest.mark.skipif(torch.cuda.is_available(), reason='sanitizer programs run on CPU-only machines')
def test_standalone_sanitizer_build(tmp_path):
    """The header and tests/detect_asan_main.cpp as ONE program of its own under the address and undefined-behaviour sanitizers, run on the CPU."""
    build_and_run_sanitized('detect_asan_main.cpp', tmp_path, 'detect_asan')
