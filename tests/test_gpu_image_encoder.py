"""GPU tests of the image encoder on the HIP 2D convolution (voxvae/conv2d.py, src/net_core/darknet.py with engine='hip').
Darknet19 and a small head2D are built twice over one state dict -- engine 'hip' and 'torch' -- with randomised BatchNormalization
parameters and statistics, and held to the float64 CPU run of the same module (tests/_conv2d_ref.py layer by layer, the module itself
in float64 end to end)."""
import copy

import numpy as np
import pytest
import torch
import torch.nn as nn

import _conv2d_ref as R
import _tol

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
HEAD = dict(output_dim=245, filter_num_list=[64, 64], filter_size_list=[3, 1])
IMAGES = [(2, 64, 64), (1, 96, 160)]


@pytest.fixture(scope='module')
def L():
    import voxvae
    from voxvae import lib
    lib.load()
    assert torch.cuda.is_available()
    voxvae.set_default_device(DEV)
    return lib


@pytest.fixture
def dtype():
    import voxvae
    saved = voxvae.default_dtype()
    yield voxvae.set_default_dtype
    voxvae.set_default_dtype(saved)


def randomise_bn(module, seed):
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for m in module.modules():
            if isinstance(m, nn.BatchNorm2d):
                n = m.num_features
                m.weight.copy_(torch.empty(n).uniform_(0.5, 1.5, generator=g))
                m.bias.copy_(torch.empty(n).uniform_(-0.5, 0.5, generator=g))
                m.running_mean.copy_(torch.empty(n).uniform_(-0.5, 0.5, generator=g))
                m.running_var.copy_(torch.empty(n).uniform_(0.5, 2.0, generator=g))


def build_pair(seed=0, activation='lrelu', last_pooling=None, cin=None):
    """(backbone, head) for each engine over the same state dict; cin: a head alone on that many channels (no backbone)."""
    import src.net_core.darknet as darknet
    out = {}
    for engine in ('hip', 'torch'):
        torch.manual_seed(seed)
        b = None if cin else darknet.Darknet19(name='b', activation=activation, device=DEV, engine=engine)
        h = darknet.head2D('h', (None, None, cin or 1024), last_pooling=last_pooling, activation=activation, device=DEV, engine=engine, **HEAD)
        out[engine] = (b, h)
    for i in (0, 1):
        if out['hip'][i] is not None:
            randomise_bn(out['hip'][i], seed + i)
            out['torch'][i].load_state_dict(out['hip'][i].state_dict())
    return out


def f64_run(module, x):
    """The module's own torch forward, on the CPU in float64 (inference form)."""
    m = copy.copy(module)                                  # a shallow copy: deepcopy below must not drag the chain's device buffers along
    m.__dict__ = {k: v for k, v in module.__dict__.items() if k != '_chain'}
    m = copy.deepcopy(m).cpu().double().eval()
    with torch.no_grad():
        return nn.Module.__call__(m, torch.as_tensor(x).detach().cpu().double()).numpy()


def image(shape, seed=3):
    return np.random.default_rng(seed).uniform(0, 1, shape + (3,)).astype(np.float32)


# ------------------------------------------------------------------------------------------------------------ layer by layer, bf16
@pytest.mark.parametrize('shape', IMAGES, ids=lambda s: 'x'.join(map(str, s)))
def test_every_layer_meets_one_rounding_in_bf16(L, dtype, shape):
    """Each step of the chain against the float64 definition applied to the PREVIOUS HIP activation: this is the gate for bf16."""
    from voxvae import conv2d as C
    dtype('bf16')
    (b, h), _ = build_pair(activation='lrelu')['hip'], None
    x = torch.from_numpy(image(shape)).to(DEV)
    feats = b(x)
    for name, module, inp in (('backbone', b, x), ('head', h, feats)):
        chain, outs = module._chain, []
        assert chain.dt == L.VV_BF16
        chain(inp, layer_outputs=outs)
        prev = inp.float().cpu().numpy()
        for i, (step, y) in enumerate(zip(chain.plan, outs)):
            what = '%s step %d %s' % (name, i, shape)
            if step[0] == 'pool':
                _tol.check_exact(y, R.pool_ref(prev), what)
            else:
                _, conv, bn, act, alpha = step
                scale, shift = (None, None) if bn is None else R.fold_ref(*(t.detach().cpu().numpy() for t in (bn.weight, bn.bias, bn.running_mean, bn.running_var)), eps=bn.eps)
                ref, pre = R.conv2d_ref(prev, C.keras_kernel(conv.weight).cpu().numpy(), scale, shift, act, alpha, 'bf16')
                odt = 'f32' if y.dtype == torch.float32 else 'bf16'
                assert (odt == 'f32') == (i == len(outs) - 1)
                worst = _tol.check_one_rounding(y, ref, pre, odt, what)
                print('%s k%d %d->%d %s: worst err / bound %.3f' % (what, conv.kernel_size[0], conv.in_channels, conv.out_channels, odt, worst))
            prev = y.float().cpu().numpy()
    # not gated (no bound can be derived for 22 chained roundings): the end-to-end bf16 difference to float64
    ref = f64_run(h, f64_run(b, x))
    got = h(feats).cpu().numpy()
    print('bf16 end to end %s: max|hip - f64| %.3e, max|f64| %.3e' % (shape, np.abs(got - ref).max(), np.abs(ref).max()))


# ------------------------------------------------------------------------------------------------------------ end to end, f32
@pytest.mark.parametrize('shape', IMAGES, ids=lambda s: 'x'.join(map(str, s)))
def test_f32_end_to_end_is_as_close_to_float64_as_the_torch_path(L, dtype, shape):
    dtype('f32')
    pair = build_pair(activation='lrelu')
    x = image(shape)
    ref = f64_run(pair['hip'][1], f64_run(pair['hip'][0], x))
    assert ref.shape == (shape[0], shape[1] // 32, shape[2] // 32, 245)
    got = {e: pair[e][1](pair[e][0](x)).cpu().numpy() for e in ('hip', 'torch')}
    e_hip, e_torch, top = np.abs(got['hip'] - ref).max(), np.abs(got['torch'] - ref).max(), np.abs(ref).max()
    print('f32 end to end %s: e_hip %.3e e_torch %.3e max|f64| %.3e' % (shape, e_hip, e_torch, top))
    assert e_hip <= 4 * e_torch + 1e-6 * top


# ------------------------------------------------------------------------------------------------------------ staleness
def _follows(module, x, what):
    """The HIP output against float64 of the module's CURRENT state, judged like the end-to-end test: against the module's own torch ops."""
    ref = f64_run(module, x)
    hip = module(x).cpu().numpy()
    with torch.no_grad():
        module.eval()
        tor = nn.Module.__call__(module, x).cpu().numpy()
    e_hip, e_torch, top = np.abs(hip - ref).max(), np.abs(tor - ref).max(), np.abs(ref).max()
    print('%s: e_hip %.3e e_torch %.3e max|f64| %.3e' % (what, e_hip, e_torch, top))
    assert e_hip <= 4 * e_torch + 1e-6 * top, what
    return hip


def test_pack_follows_every_kind_of_update(L, dtype, tmp_path):
    dtype('f32')
    h = build_pair(cin=64)['hip'][1]
    x = torch.randn(2, 3, 5, 64, generator=torch.Generator().manual_seed(4)).to(DEV)
    y0 = _follows(h, x, 'as built')
    assert not h._chain.stale()
    opt = torch.optim.Adam(h.trainable_variables, lr=1e-2)
    h(x, training=True).square().mean().backward()
    assert h._chain.stale()                                                # the training forward moved the running statistics
    y1 = _follows(h, x, 'after a training-mode forward')
    assert np.abs(y1 - y0).max() > 1e-4
    opt.step()
    assert h._chain.stale()
    y2 = _follows(h, x, 'after an Adam step')
    assert np.abs(y2 - y1).max() > 1e-4
    other = build_pair(seed=9, cin=64)['torch'][1]
    other.save_weights(str(tmp_path / 'w'))
    h.load_weights(str(tmp_path / 'w'))
    assert h._chain.stale()
    y3 = _follows(h, x, 'after load_weights')
    assert np.abs(y3 - y2).max() > 1e-4
    assert np.array_equal(y3, h(x).cpu().numpy()) and not h._chain.stale()


# ------------------------------------------------------------------------------------------------------------ routing
def test_routing(L, dtype, monkeypatch):
    dtype('f32')
    calls = []
    real = L.call
    monkeypatch.setattr(L, 'call', lambda name, *a: (calls.append(name), real(name, *a))[1])
    x = torch.randn(2, 3, 5, 64, generator=torch.Generator().manual_seed(5)).to(DEV)
    for pooling in (None, 'max', 'average'):
        pair = build_pair(cin=64, last_pooling=pooling)
        hip, tor = pair['hip'][1], pair['torch'][1]
        del calls[:]
        t = tor(x)
        assert not [c for c in calls if 'conv2d' in c or 'maxpool2d' in c or c == 'vv_fold_bn'], calls       # 'torch': not one entry of ours
        hip(x, training=True)
        assert not [c for c in calls if 'conv2d' in c], calls                                                  # training never enters the engine
        hip.load_state_dict(tor.state_dict())                                                                 # (the training forward moved the statistics)
        del calls[:]
        y = hip(x)
        assert calls.count('vv_conv2d_fwd') == 3 and calls.count('vv_pack_conv2d') == 3 and calls.count('vv_fold_bn') == 2
        assert ('vv_max_over_positions' in calls) == (pooling == 'max')
        assert y.dtype == torch.float32 and y.is_cuda and y.is_contiguous()
        assert tuple(y.shape) == ((2, 245) if pooling else (2, 3, 5, 245)) == tuple(t.shape)
        ref = f64_run(tor, x)
        assert np.abs(y.cpu().numpy() - ref).max() <= 4 * np.abs(t.cpu().numpy() - ref).max() + 1e-6 * np.abs(ref).max()
        del calls[:]
        hip(x)
        assert calls.count('vv_pack_conv2d') == 0 and calls.count('vv_conv2d_fwd') == 3                        # packed once
    # numpy in, host in, the full backbone: float32 CUDA out, channels innermost
    b = build_pair()['hip'][0]
    out = b(image((1, 64, 96)))
    assert tuple(out.shape) == (1, 2, 3, 1024) and out.is_cuda and out.dtype == torch.float32 and out.is_contiguous()


# ------------------------------------------------------------------------------------------------------------ the chain
def test_nolbo_test_runs_on_the_hip_engine(L, dtype):
    import voxvae
    import src.module.nolbo_test as NT
    import src.net_core.darknet as darknet
    from voxvae import detect as D
    from voxvae import synthetic as syn
    from test_detect_host import assert_same
    import _detect_ref as DR
    dtype('f32')
    s = {k: dict(v) for k, v in NT.config.items()}
    s['encoder_head'].update(filter_num_list=HEAD['filter_num_list'], filter_size_list=HEAD['filter_size_list'])
    s['decoder'] = syn.make_config(32, 16, True)['decoder']
    voxvae.set_image_engine('hip')
    try:
        torch.manual_seed(7)
        m = NT.nolbo_test(s, backbone_style=darknet.Darknet19)
    finally:
        voxvae.set_image_engine('torch')
    assert m._encoder_backbone._chain is not None and m._encoder_head._chain is not None
    with torch.no_grad():
        m._encoder_head.last.weight.mul_(4.0)
    img = image((1, 64, 96), seed=9)
    head = m._head_output(img)[1]
    assert tuple(head.shape) == (1, 2, 3, 245) and head.is_cuda and head.dtype == torch.float32
    t, layout = D._as_head(head, torch.device(DEV), 245)
    assert t.data_ptr() == head.data_ptr() and layout == D.NHWC                      # read where the engine left it
    kw = dict(obj_thresh=0.3, iou_thresh=0.5, top_1_pred=False)
    dev = D.decode_detections(head, 5, 16, kw['obj_thresh'], kw['iou_thresh'], kw['top_1_pred'])
    host = D.decode_detections(head.cpu(), 5, 16, kw['obj_thresh'], kw['iou_thresh'], kw['top_1_pred'], host=True)
    assert_same(DR.detections_as_dicts(dev), DR.detections_as_dicts(host), 'device decode against host decode of the HIP head output')
    # two calls give the same bits (no algorithm choice, no atomics), so getObjects sees the head output decoded above
    assert torch.equal(head, m._head_output(img)[1])
    M = host.counts()[0]
    assert M >= 1
    eps = torch.randn(M, 32, 16, generator=torch.Generator().manual_seed(1)).numpy()
    det, poses, cloud = m.getObjects(img, sampling_num=32, _eps=eps, obj_thresh=0.3, IOU_thresh=0.5, top_1_pred=False)
    assert det.counts() == [M] and det.bbox2d.is_cuda
    assert poses is not None and 0 <= poses.count() <= M
    b2, b3, sn, cs, _, mean, lv = host.numpy(0)
    want_poses, want_cloud = m.getSampledObjects(mean, lv, b2, b3, sn, cs, (96, 64), 32, _eps=eps)
    assert poses.count() == want_poses.count() and (cloud is None) == (want_cloud is None)
