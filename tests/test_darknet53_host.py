"""CPU tests of the Darknet53 / Darknet53Tiny additions: the float64 statement of the new operations against torch's own, the graphs of
the torch modules, the new entries' validation and size queries, the strided index arithmetic under the host sanitizers, and the
classifier's loss, accuracies and training step."""
import ctypes
import os

import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from _common import build_and_run_sanitized
import _conv2d_ref as R
import _darknet53_ref as R53

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32, BF16 = 0, 1
NULL, SHAPE, DTYPE, ALIGN, WORKSPACE = -1, -2, -3, -4, -5


@pytest.fixture(scope='module')
def lib():
    from voxvae import build as vb
    vb.build()
    from voxvae import lib as L
    return L.load()


# ------------------------------------------------------------------------------------------------------------ the reference statement
@pytest.mark.parametrize('grid', [(1, 2, 2), (2, 5, 7), (1, 3, 9), (2, 6, 4)], ids=lambda g: 'x'.join(map(str, g)))
def test_strided_statement_is_torchs_padded_valid_convolution(grid):
    rng = np.random.default_rng(sum(grid))
    x, w = rng.standard_normal(grid + (4,)), rng.standard_normal((3, 3, 4, 5))
    xt, wt = torch.from_numpy(x).permute(0, 3, 1, 2), torch.from_numpy(w).permute(3, 2, 0, 1)
    want = F.conv2d(F.pad(xt, (1, 0, 1, 0)), wt, stride=2).permute(0, 2, 3, 1).numpy()         # ZeroPadding2D(((1,0),(1,0))) + 'valid'
    got = R53.conv_ex_direct(x, w, 2)
    assert got.shape == want.shape == (grid[0], grid[1] // 2, grid[2] // 2, 5)
    assert np.abs(got - want).max() < 1e-12
    for k in (1, 3):                                                                            # stride 1 is the 'same' convolution
        assert np.abs(R53.conv_ex_direct(x, w[:k, :k], 1) - R.conv2d_direct(x, w[:k, :k])).max() < 1e-12
    for tr in range(3):
        for tc in range(3):
            sel = R.selector_kernel(3, 4, 5, tr, tc, 2, 3)
            assert np.array_equal(R53.conv_ex_direct(x, sel, 2)[..., 3], R53.shifted_s2(x, tr, tc, 2))


def test_residual_statement_adds_behind_the_activation():
    rng = np.random.default_rng(5)
    x, w = rng.standard_normal((2, 5, 7, 32)).astype(np.float32), rng.standard_normal((3, 3, 32, 8)).astype(np.float32)
    scale, shift = rng.uniform(0.5, 2, 8).astype(np.float32), rng.uniform(-1, 1, 8).astype(np.float32)
    for stride in (1, 2):
        Ro, Co = R53.out_grid(5, 7, stride)
        res = rng.standard_normal((2, Ro, Co, 8)).astype(np.float32)
        y, pre = R53.conv_ex_ref(x, w, scale, shift, res, 'elu', 0.0, stride, 'bf16')
        xt = torch.from_numpy(R.round_to(x, 'bf16')).permute(0, 3, 1, 2)
        wt = torch.from_numpy(R.round_to(w, 'bf16')).permute(3, 2, 0, 1)
        conv = (F.conv2d(F.pad(xt, (1, 0, 1, 0)), wt, stride=2) if stride == 2 else F.conv2d(xt, wt, padding=1)).permute(0, 2, 3, 1)
        want = F.elu(conv * torch.from_numpy(scale).double() + torch.from_numpy(shift).double()) + torch.from_numpy(R.round_to(res, 'bf16'))
        assert np.abs(y - want.numpy()).max() < 1e-12
        assert pre.shape == (2,) + y.shape and np.array_equal(pre[1], R.round_to(res, 'bf16'))
        y0, pre0 = R53.conv_ex_ref(x, w, scale, shift, None, 'elu', 0.0, stride, 'bf16')
        assert np.array_equal(pre0, pre[0]) and np.abs(y0 + pre[1] - y).max() < 1e-12
    y1, _ = R53.conv_ex_ref(x, w, scale, shift, None, 'lrelu', 0.1, 1, 'f32')
    assert np.abs(y1 - R.conv2d_ref(x, w, scale, shift, 'lrelu', 0.1, 'f32')[0]).max() < 1e-12


@pytest.mark.parametrize('grid', [(2, 5, 7), (1, 1, 1), (1, 1, 9), (2, 2, 2)], ids=lambda g: 'x'.join(map(str, g)))
def test_pool_statement_is_torchs_end_padded_pool(grid):
    x = np.random.default_rng(sum(grid)).standard_normal(grid + (3,)) - 3.0
    xt = torch.from_numpy(x).permute(0, 3, 1, 2)
    want = F.max_pool2d(F.pad(xt, (0, 1, 0, 1), value=float('-inf')), 2, 1).permute(0, 2, 3, 1).numpy()
    assert np.array_equal(R53.pool1_ref(x), want)


# ------------------------------------------------------------------------------------------------------------ the torch modules
def _convs(m):
    import src.net_core.darknet as darknet
    return [l for l in m.layers if isinstance(l, darknet._ConvBNAct)]


def _grids(m, rows, cols):
    with torch.no_grad():
        outs = m(np.zeros((1, rows, cols, 3), np.float32))
    return [tuple(o.shape[1:]) for o in outs]


def test_darknet53_graph():
    import src.net_core.darknet as darknet
    from voxvae import conv2d as C
    m = darknet.Darknet53(name='b', activation='lrelu', device='cpu')
    convs = _convs(m)
    assert len(convs) == 52 and len(m.layers) == 52
    assert [c.conv.out_channels for c in convs if c.stride == 2] == [64, 128, 256, 512, 1024]
    assert all(c.conv.kernel_size == (3, 3) and c.conv.padding == (0, 0) for c in convs if c.stride == 2)
    assert all(c.conv.bias is None and c.bn.eps == 1e-3 and c.l2 == 0.0005 for c in convs)
    assert len(m._res) == 23 == 1 + 2 + 8 + 8 + 4
    for i, src in m._res.items():
        one, three = m.layers[i - 1], m.layers[i]
        assert src == i - 2 and one.conv.kernel_size == (1, 1) and three.conv.kernel_size == (3, 3)
        assert one.conv.out_channels * 2 == three.conv.out_channels == m.layers[src].conv.out_channels
        assert isinstance(three.act, nn.ELU)                               # the reference's quirk: no activation argument there
        assert isinstance(one.act, nn.LeakyReLU) and one.act.negative_slope == pytest.approx(0.1)
    assert all(isinstance(c.act, nn.LeakyReLU) for i, c in enumerate(convs) if i not in m._res)
    assert _grids(m, 416, 416) == [(52, 52, 256), (26, 26, 512), (13, 13, 1024)]
    assert _grids(m, 65, 33) == [(8, 4, 256), (4, 2, 512), (2, 1, 1024)]                  # floor at every stride
    assert m.output_shape == (None, None, None, 1024)
    assert m.output_shapes == [(None, None, None, 256), (None, None, None, 512), (None, None, None, 1024)]
    assert len(m.losses) == 52
    assert float(m.losses[0].detach()) == pytest.approx(0.0005 * float((convs[0].conv.weight.detach() ** 2).sum()))
    # the engine's plan of it
    plan = C.module_plan(m)
    shapes = C.plan_shapes(plan, 416, 416)
    assert [s[1] for s in shapes if s[0] == 'conv'][::1][:3] == [416, 416, 208]
    assert sorted({s[1] for s in shapes}) == [13, 26, 52, 104, 208, 416]
    assert sum(1 for s in plan if len(s) > 5 and s[5] == 2) == 5 and sum(1 for s in plan if len(s) > 5 and s[6] is not None) == 23
    assert C.plan_taps(m) == m._taps and [shapes[t + 1][1] if t + 1 < len(shapes) else None for t in m._taps] == [52, 26]
    assert C.plan_shapes(plan, 65, 33)[-1][:3] == ('conv', 2, 1)
    elu = darknet.Darknet53(name='b', device='cpu')
    assert all(isinstance(c.act, nn.ELU) for c in _convs(elu))


def test_darknet53tiny_graph():
    import src.net_core.darknet as darknet
    from voxvae import conv2d as C
    m = darknet.Darknet53Tiny(name='t', activation='lrelu', device='cpu')
    convs = _convs(m)
    assert [(c.conv.in_channels, c.conv.out_channels) for c in convs] == [(3, 16), (16, 32), (32, 64), (64, 128), (128, 256), (256, 512), (512, 1024)]
    assert all(c.stride == 1 and c.conv.kernel_size == (3, 3) and c.l2 == 0.0005 and c.bn.eps == 1e-3 for c in convs)
    kinds = ['conv' if isinstance(l, darknet._ConvBNAct) else ('pool1' if isinstance(l, darknet._Pool1Same) else 'pool') for l in m.layers]
    assert kinds == ['conv', 'pool'] * 5 + ['conv', 'pool1', 'conv']
    assert [s[0] for s in C.module_plan(m)] == kinds
    assert _grids(m, 416, 416) == [(26, 26, 256), (13, 13, 1024)]
    assert _grids(m, 96, 160) == [(6, 10, 256), (3, 5, 1024)]
    assert _grids(m, 65, 33) == [(5, 3, 256), (3, 2, 1024)]                              # ceil at every pool
    assert m.output_shape == (None, None, None, 1024) and m.output_shapes[0] == (None, None, None, 256)
    assert len(m.losses) == 7 and not m._res
    assert C.plan_shapes(C.module_plan(m), 416, 416)[-2:] == [('pool1', 13, 13, 512, 512, 2), ('conv', 13, 13, 512, 1024, 3)]


def test_old_plans_keep_their_form():
    import src.net_core.darknet as darknet
    from voxvae import conv2d as C
    plan = C.module_plan(darknet.Darknet19(name='b', device='cpu'))
    assert all(len(s) == (1 if s[0] == 'pool' else 5) for s in plan) and C.plan_taps(darknet.Darknet19(name='b', device='cpu')) is None
    assert all(len(s) == 6 for s in C.plan_shapes(plan, 64, 64))


def test_heads_take_the_last_output():
    import src.net_core.darknet as darknet
    a, b = torch.zeros(1), torch.ones(1)
    assert darknet.last_output((a, b)) is b and darknet.last_output(a) is a
    m = darknet.Darknet53Tiny(name='t', device='cpu')
    h = darknet.head2D('h', m.output_shape[1:], 7, [32], [1], last_pooling='average', device='cpu')
    feats = m(np.zeros((2, 64, 64, 3), np.float32))
    assert tuple(h(darknet.last_output(feats)).shape) == (2, 7)
    assert torch.equal(h(feats), h(feats[-1]))                              # a head called on the tuple itself, as nolbo_test calls it
    assert torch.equal(h(feats, training=True), h(feats[-1], training=True))


# ------------------------------------------------------------------------------------------------------------ validation, size queries
def _ex(lib, x, w, y, res=None, batch=1, rows=4, cols=4, cin=32, cout=32, k=3, stride=2, act=0, dt=F32, odt=F32, ws=None, ws_bytes=0):
    return lib.vv_conv2d_ex_fwd(x, w, None, None, res, y, batch, rows, cols, cin, cout, k, stride, act, 0.1, dt, odt, ws, ws_bytes, None)


def test_null_is_refused_everywhere(lib):
    assert _ex(lib, None, None, None) == NULL
    assert lib.vv_maxpool2d_s1_same_fwd(None, None, 1, 4, 4, 32, F32, None) == NULL


@pytest.mark.skipif(torch.cuda.is_available(), reason='pointers that are never dereferenced: validation precedes the launch, so this runs only where no launch can follow')
def test_new_entries_refuse_before_the_launch(lib):
    p = ctypes.c_void_p(4096)
    assert _ex(lib, None, p, p) == NULL and _ex(lib, p, None, p) == NULL and _ex(lib, p, p, None) == NULL
    assert _ex(lib, p, p, p, stride=0) == SHAPE and _ex(lib, p, p, p, stride=3) == SHAPE and _ex(lib, p, p, p, stride=-1) == SHAPE
    assert _ex(lib, p, p, p, k=1) == SHAPE                                  # stride 2 is k3 only
    assert _ex(lib, p, p, p, rows=1) == SHAPE and _ex(lib, p, p, p, cols=1) == SHAPE
    assert _ex(lib, p, p, p, cin=3) == SHAPE                                # no image layer has stride 2
    assert _ex(lib, p, p, p, cin=16) == SHAPE and _ex(lib, p, p, p, cin=48) == SHAPE
    assert _ex(lib, p, p, p, cin=16, stride=1) == SHAPE and _ex(lib, p, p, p, k=2, stride=1) == SHAPE
    assert _ex(lib, p, p, p, act=9) == SHAPE and _ex(lib, p, p, p, batch=0) == SHAPE and _ex(lib, p, p, p, cout=0) == SHAPE
    assert _ex(lib, p, p, p, dt=2) == DTYPE and _ex(lib, p, p, p, odt=2) == DTYPE
    assert _ex(lib, p, p, p, rows=65536, cols=1024) == SHAPE               # the input holds 2^31 elements
    assert _ex(lib, p, p, p, rows=65536, cols=1024, stride=1) == SHAPE
    assert _ex(lib, p, p, p, batch=1 << 20, rows=1 << 10, cols=1 << 10) == SHAPE
    assert _ex(lib, p, p, p, batch=2, rows=4096, cols=4096, cin=32, cout=256) == SHAPE    # the OUTPUT (a quarter of the pixels) is past it
    assert _ex(lib, p, p, p, res=ctypes.c_void_p(4100)) == ALIGN and _ex(lib, ctypes.c_void_p(4100), p, p) == ALIGN
    assert _ex(lib, p, p, p, res=ctypes.c_void_p(4100), stride=1) == ALIGN
    assert _ex(lib, p, p, p, rows=26, cols=26, cin=512, cout=1024) == WORKSPACE          # 13 x 13 output: split-K, and no workspace given
    assert _ex(lib, p, p, p, res=p, rows=26, cols=26, cin=512, cout=1024, ws=p, ws_bytes=15) == WORKSPACE
    q = lib.vv_maxpool2d_s1_same_fwd
    assert q(None, p, 1, 4, 4, 32, F32, None) == NULL and q(p, None, 1, 4, 4, 32, F32, None) == NULL
    assert q(p, p, 1, 0, 4, 32, F32, None) == SHAPE and q(p, p, 1, 4, 4, 0, F32, None) == SHAPE and q(p, p, 0, 4, 4, 32, F32, None) == SHAPE
    assert q(p, p, 1, 65536, 1024, 32, F32, None) == SHAPE and q(p, p, 1, 4, 4, 32, 2, None) == DTYPE


def test_ex_queries(lib):
    assert lib.vv_conv2d_ex_supported(3, 2, 32, 64, BF16, BF16) == 1 and lib.vv_conv2d_ex_supported(3, 2, 512, 1024, F32, BF16) == 1
    for bad in [(1, 2, 32, 64, 0, 0), (3, 2, 3, 32, 0, 0), (3, 0, 32, 32, 0, 0), (3, 3, 32, 32, 0, 0), (3, 2, 16, 32, 0, 0), (3, 2, 48, 32, 0, 0),
                (3, 2, 32, 32, 2, 0), (3, 2, 32, 32, 0, 2), (3, 2, 32, 0, 0, 0), (2, 1, 32, 32, 0, 0)]:
        assert lib.vv_conv2d_ex_supported(*bad) == 0, bad
    # stride 1: the old queries
    for cin, cout, k in [(3, 32, 3), (32, 64, 3), (128, 64, 1), (1024, 1024, 3), (1024, 245, 1), (64, 40, 3)]:
        for dt in (F32, BF16):
            assert lib.vv_conv2d_ex_supported(k, 1, cin, cout, dt, F32) == lib.vv_conv2d_supported(k, cin, cout, dt, F32) == 1
        for B, r, c in [(1, 13, 13), (1, 3, 5), (4, 8, 8), (72, 8, 8), (1, 416, 416), (0, 4, 4)]:
            assert lib.vv_conv2d_ex_splits(B, r, c, k, 1, cin, cout) == lib.vv_conv2d_splits(B, r, c, k, cin, cout)
            assert lib.vv_conv2d_ex_workspace_bytes(B, r, c, k, 1, cin, cout, BF16) == lib.vv_conv2d_workspace_bytes(B, r, c, k, cin, cout, BF16)
    # stride 2: the halved grid decides
    for cin, cout in [(32, 64), (64, 128), (256, 512), (512, 1024)]:
        for B, r, c in [(1, 26, 26), (1, 27, 27), (2, 13, 9), (1, 416, 416), (1, 2, 2)]:
            s = lib.vv_conv2d_ex_splits(B, r, c, 3, 2, cin, cout)
            assert s == lib.vv_conv2d_splits(B, r // 2, c // 2, 3, cin, cout) >= 1
            assert lib.vv_conv2d_ex_workspace_bytes(B, r, c, 3, 2, cin, cout, F32) == (s * B * (r // 2) * (c // 2) * cout * 4 if s > 1 else 0)
    assert lib.vv_conv2d_ex_splits(1, 26, 26, 3, 2, 512, 1024) == lib.vv_conv2d_splits(1, 13, 13, 3, 512, 1024) > 1
    assert lib.vv_conv2d_ex_splits(1, 1, 8, 3, 2, 32, 32) == 0 and lib.vv_conv2d_ex_splits(1, 8, 8, 1, 2, 32, 32) == 0
    assert lib.vv_conv2d_ex_workspace_bytes(1, 1, 8, 3, 2, 32, 32, F32) == 0


@pytest.mark.skipif(torch.cuda.is_available(), reason='sanitizer programs run on CPU-only machines')
def test_strided_plan_under_the_host_sanitizers(tmp_path):
    build_and_run_sanitized('conv2d_s2_plan_main.cpp', tmp_path, 'conv2d_s2_plan_main')


# ------------------------------------------------------------------------------------------------------------ the classifier
def _classifier(**kw):
    import src.module.classifier as CL
    import src.net_core.darknet as darknet
    torch.manual_seed(0)
    args = dict(backbone_style=lambda name, activation: darknet.Darknet53Tiny(name=name, activation=activation, device='cpu'), name='c',
                BATCH_SIZE_PER_REPLICA=8, output_dim=10, last_filter_num_list=[32], last_filter_size_list=[1], learning_rate=1e-3)
    args.update(kw)
    return CL.classifier(**args)


def test_classifier_loss_and_accuracy_formulas():
    c = _classifier()
    rng = np.random.default_rng(0)
    pred = rng.standard_normal((6, 10)) * 3
    gt = np.eye(10)[rng.integers(0, 10, 6)]
    soft = np.exp(pred - pred.max(-1, keepdims=True))
    soft /= soft.sum(-1, keepdims=True)
    want = (-(gt * np.log(soft + 1e-9)).sum(-1)).sum() / 8                                # the GLOBAL batch, not the batch at hand
    got = c._lossObject(torch.from_numpy(gt), torch.from_numpy(pred))
    assert float(got) == pytest.approx(want, rel=1e-12)
    top1, top5 = c._evaluation(torch.from_numpy(gt), torch.from_numpy(pred))
    order = np.argsort(-pred, -1)
    label = gt.argmax(-1)
    assert float(top1) == pytest.approx((order[:, 0] == label).sum() / 8)
    assert float(top5) == pytest.approx(sum(l in o[:5] for l, o in zip(label, order)) / 8)
    assert 0 < float(top1) <= float(top5) or float(top1) == 0
    sure = torch.from_numpy(gt) * 50.0
    assert c._evaluation(torch.from_numpy(gt), sure)[0] == pytest.approx(6 / 8) and float(c._lossObject(torch.from_numpy(gt), sure)) < 1e-6


def test_classifier_fit_lowers_the_loss(tmp_path):
    c = _classifier()
    assert isinstance(c.model_backbone(np.zeros((1, 32, 32, 3), np.float32)), tuple)       # the tuple backbone: fit takes its last element
    rng = np.random.default_rng(1)
    labels = rng.integers(0, 10, 8)
    images = rng.uniform(0, 1, (8, 32, 32, 3)).astype(np.float32)
    images[np.arange(8), :, :, labels % 3] += 0.1 * labels[:, None, None]
    onehot = np.eye(10, dtype=np.float32)[labels]
    before = [p.detach().clone() for p in c.model_backbone.trainable_variables]
    want_reg = float((sum(c.model_backbone.losses) + sum(c.model_head.losses)).detach())       # of the weights the first step sees
    out = [c.fit((images, onehot)) for _ in range(6)]
    reg, pred, total, a1, a5 = out[0]
    assert total == pred and reg > 0 and 0 <= a1 <= a5 <= 1
    assert reg == pytest.approx(want_reg, rel=1e-5)
    assert out[-1][1] < out[0][1]
    assert any(not torch.equal(a, b) for a, b in zip(before, c.model_backbone.trainable_variables))
    assert len(c.distributed_fit((images, onehot))) == 5
    scores = c.predict(images)
    assert tuple(scores.shape) == (8, 10)
    c.saveModel(str(tmp_path))
    other = _classifier()
    other.fit((images, onehot))
    other.loadModel(str(tmp_path))
    assert torch.equal(other.predict(images), scores)
    other.loadBackbone(str(tmp_path)), other.loadHead(str(tmp_path)), other.saveBackbone(str(tmp_path)), other.saveHead(str(tmp_path))

    class Two:
        num_replicas_in_sync = 2
    with pytest.raises(NotImplementedError):
        _classifier(strategy=Two())
