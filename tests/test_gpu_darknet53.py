"""GPU tests of Darknet53 / Darknet53Tiny on the HIP image engine (src/net_core/darknet.py with engine='hip', voxvae/conv2d.py).
Each module is built twice over one state dict -- engine 'hip' and 'torch' -- with randomised BatchNormalization parameters and
statistics.  bf16: every step of the chain is held to the float64 definition applied to the PREVIOUS HIP activation.  f32: every element
of the output tuple is as close to the float64 CPU run as the torch engine's.  Then the callers: nolbo_test, classifier, staleness."""
import copy

import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

import _conv2d_ref as R
import _darknet53_ref as R53
import _tol
from test_gpu_image_encoder import DEV, image, randomise_bn

pytestmark = pytest.mark.gpu

IMAGES = [(2, 64, 64), (1, 96, 160), (1, 65, 33)]
BUILDERS = ['Darknet53', 'Darknet53Tiny']


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


def build_pair(builder, seed=0, activation='lrelu'):
    import src.net_core.darknet as darknet
    out = {}
    for engine in ('hip', 'torch'):
        torch.manual_seed(seed)
        out[engine] = getattr(darknet, builder)(name='b', activation=activation, device=DEV, engine=engine)
    randomise_bn(out['hip'], seed)
    out['torch'].load_state_dict(out['hip'].state_dict())
    return out


def f64_run(module, x):
    """The module's own torch forward on the CPU in float64 (inference form) -> a tuple of numpy arrays."""
    m = copy.copy(module)
    m.__dict__ = {k: v for k, v in module.__dict__.items() if k != '_chain'}
    m = copy.deepcopy(m).cpu().double().eval()
    with torch.no_grad():
        out = nn.Module.__call__(m, torch.as_tensor(x).detach().cpu().double())
    return tuple(o.numpy() for o in (out if isinstance(out, tuple) else (out,)))


def conv_step_ref(prev, wk, scale, shift, res, act, alpha, stride, dt):
    """_darknet53_ref.conv_ex_ref with the sum done by torch's float64 convolution (tests/test_darknet53_host.py shows the two are the
    same statement): a 1024-channel layer tap by tap in numpy is minutes."""
    xt = torch.from_numpy(R.round_to(prev, dt)).permute(0, 3, 1, 2)
    wt = torch.from_numpy(R.round_to(wk, dt)).permute(3, 2, 0, 1)
    y = (F.conv2d(F.pad(xt, (1, 0, 1, 0)), wt, stride=2) if stride == 2 else F.conv2d(xt, wt, padding=wk.shape[0] // 2)).permute(0, 2, 3, 1).numpy()
    y = y * scale + shift
    out = R.act_ref(y, act, alpha)
    if res is None:
        return out, y
    rr = R.round_to(res, dt)
    return out + rr, np.stack([y, rr])


# ------------------------------------------------------------------------------------------------------------ step by step, bf16
@pytest.mark.parametrize('shape', IMAGES, ids=lambda s: 'x'.join(map(str, s)))
@pytest.mark.parametrize('builder', BUILDERS)
def test_every_step_meets_one_rounding_in_bf16(L, dtype, builder, shape):
    from voxvae import conv2d as C
    dtype('bf16')
    pair = build_pair(builder)
    b = pair['hip']
    x = torch.from_numpy(image(shape)).to(DEV)
    chain, outs = b._chain, []
    assert chain.dt == L.VV_BF16
    got = chain(x, layer_outputs=outs)
    assert isinstance(got, tuple) and len(got) == len(b.output_shapes) and all(g.dtype == torch.float32 and g.is_contiguous() for g in got)
    prev, real, worst_all, padded = x.float().cpu().numpy(), [], 0.0, 0
    for i, (step, y) in enumerate(zip(chain.plan, outs)):
        what = '%s step %d %s' % (builder, i, shape)
        yh = y.float().cpu().numpy()
        n = step[1].out_channels if step[0] == 'conv' else real[-1].shape[-1]
        if yh.shape[-1] != n:                                   # Darknet53Tiny's 16-channel layer runs as 32: the padding is exactly zero
            assert builder == 'Darknet53Tiny' and yh.shape[-1] == 32 and n == 16
            assert not yh[..., n:].any(), what + ': padded channels'
            padded += 1
            yh = yh[..., :n]
        if step[0] == 'pool':
            _tol.check_exact(yh, R.pool_ref(prev), what)
        elif step[0] == 'pool1':
            _tol.check_exact(yh, R53.pool1_ref(prev), what)
        else:
            _, conv, bn, act, alpha = step[:5]
            stride, res = C.step_stride_res(step)
            scale, shift = R.fold_ref(*(t.detach().cpu().numpy() for t in (bn.weight, bn.bias, bn.running_mean, bn.running_var)), eps=bn.eps)
            ref, pre = conv_step_ref(prev, C.keras_kernel(conv.weight).cpu().numpy(), scale, shift, None if res is None else real[res], act, alpha, stride, 'bf16')
            odt = 'f32' if y.dtype == torch.float32 else 'bf16'
            assert (odt == 'f32') == (i == len(outs) - 1)
            worst = _tol.check_one_rounding(yh, ref, pre, odt, what)
            worst_all = max(worst_all, worst)
            print('%s k%d s%d %d->%d res %s %s: worst err / bound %.3f' % (what, conv.kernel_size[0], stride, conv.in_channels, conv.out_channels, res, odt, worst))
        real.append(yh)
        prev = yh
    assert padded == (2 if builder == 'Darknet53Tiny' else 0)   # the first convolution and the pool behind it
    # the outputs are those activations, converted exactly
    for g, t in zip(got, list(chain.taps) + [len(outs) - 1]):
        assert np.array_equal(g.cpu().numpy(), real[t])
    # not gated (no bound can be derived for that many chained roundings): the end-to-end bf16 difference to float64
    ref = f64_run(b, x)
    for j, (g, r) in enumerate(zip(got, ref)):
        print('%s bf16 end to end %s output %d: max|hip - f64| %.3e, max|f64| %.3e, worst step %.3f' % (builder, shape, j, np.abs(g.cpu().numpy() - r).max(), np.abs(r).max(), worst_all))


# ------------------------------------------------------------------------------------------------------------ end to end, f32
@pytest.mark.parametrize('shape', IMAGES, ids=lambda s: 'x'.join(map(str, s)))
@pytest.mark.parametrize('builder', BUILDERS)
def test_f32_outputs_are_as_close_to_float64_as_the_torch_path(L, dtype, builder, shape):
    dtype('f32')
    pair = build_pair(builder)
    x = image(shape)
    ref = f64_run(pair['hip'], x)
    got = {e: pair[e](x) for e in ('hip', 'torch')}
    assert isinstance(got['hip'], tuple) and len(got['hip']) == len(got['torch']) == len(ref) == (3 if builder == 'Darknet53' else 2)
    for j, r in enumerate(ref):
        h, t = got['hip'][j].cpu().numpy(), got['torch'][j].cpu().numpy()
        assert h.shape == t.shape == r.shape
        e_hip, e_torch, top = np.abs(h - r).max(), np.abs(t - r).max(), np.abs(r).max()
        print('%s f32 end to end %s output %d %s: e_hip %.3e e_torch %.3e max|f64| %.3e' % (builder, shape, j, r.shape, e_hip, e_torch, top))
        assert e_hip <= 4 * e_torch + 1e-6 * top


# ------------------------------------------------------------------------------------------------------------ callers
def test_nolbo_test_runs_getpred_on_darknet53(L, dtype):
    import voxvae
    import src.module.nolbo_test as NT
    import src.net_core.darknet as darknet
    from voxvae import synthetic as syn
    dtype('f32')
    s = {k: dict(v) for k, v in NT.config.items()}
    s['encoder_head'].update(filter_num_list=[64, 64], filter_size_list=[3, 1])
    s['decoder'] = syn.make_config(32, 16, True)['decoder']
    voxvae.set_image_engine('hip')
    try:
        torch.manual_seed(7)
        m = NT.nolbo_test(s, backbone_style=darknet.Darknet53)
    finally:
        voxvae.set_image_engine('torch')
    assert m._encoder_backbone._chain is not None and m._encoder_head._chain is not None and m._encoder_backbone._chain.taps
    with torch.no_grad():
        m._encoder_head.last.weight.mul_(4.0)
    img = image((1, 64, 96), seed=9)
    head = m._head_output(img)[1]
    assert tuple(head.shape) == (1, 2, 3, 245) and head.is_cuda and head.dtype == torch.float32
    assert torch.equal(head, m._head_output(img)[1])
    out = m.getPred(img, obj_thresh=0.3, IOU_thresh=0.5, top_1_pred=False, get_3D_shape=False)
    assert len(out) == 6 and all(isinstance(o, np.ndarray) for o in out[1:])
    assert out[1].shape[0] == out[2].shape[0] == out[3].shape[0] >= 1 and out[2].shape[-1] == 3          # bbox2D rows, bbox3D [M,3]
    assert out[0].shape == (64, 96, 3) and np.isfinite(out[1]).all() and np.isfinite(out[2]).all()


def test_classifier_inference_follows_the_engine(L, dtype, monkeypatch):
    import voxvae
    import src.module.classifier as CL
    import src.net_core.darknet as darknet
    dtype('f32')
    calls = []
    real = L.call
    monkeypatch.setattr(L, 'call', lambda name, *a: (calls.append(name), real(name, *a))[1])
    made = {}
    for engine in ('hip', 'torch'):
        torch.manual_seed(3)
        backbone = darknet.Darknet53Tiny(name='t', activation='lrelu', device=DEV, engine=engine)
        voxvae.set_image_engine(engine)                      # the head is built by the classifier, on the engine of the moment
        try:
            made[engine] = CL.classifier(model_backbone=backbone, name='c', BATCH_SIZE_PER_REPLICA=4, output_dim=10, last_filter_num_list=[64],
                                         last_filter_size_list=[1], learning_rate=1e-3)
        finally:
            voxvae.set_image_engine('torch')
    hip, tor = made['hip'], made['torch']
    tor.model_backbone.load_state_dict(hip.model_backbone.state_dict())
    tor.model_head.load_state_dict(hip.model_head.state_dict())
    x = image((4, 64, 64), seed=2)
    del calls[:]
    t = tor.predict(x)
    assert not [c for c in calls if 'conv2d' in c or 'maxpool2d' in c], calls
    y = hip.predict(x)
    assert calls.count('vv_conv2d_fwd') == 7 + 2 and calls.count('vv_conv2d_ex_fwd') == 0          # Tiny has neither a stride nor a residual
    assert calls.count('vv_maxpool2d_same_fwd') == 5 and calls.count('vv_maxpool2d_s1_same_fwd') == 1
    assert tuple(y.shape) == (4, 10) == tuple(t.shape)
    ref = f64_run(tor.model_head, f64_run(tor.model_backbone, x)[-1])[0]
    e_hip, e_torch = np.abs(y.cpu().numpy() - ref).max(), np.abs(t.cpu().numpy() - ref).max()
    print('classifier scores: e_hip %.3e e_torch %.3e max|f64| %.3e' % (e_hip, e_torch, np.abs(ref).max()))
    assert e_hip <= 4 * e_torch + 1e-6 * np.abs(ref).max()
    # training never enters the engine, and the next inference call packs the stepped weights again
    labels = np.eye(10, dtype=np.float32)[[1, 3, 5, 7]]
    del calls[:]
    hip.fit((x, labels))
    assert not [c for c in calls if 'conv2d' in c or 'maxpool2d' in c], calls
    assert hip.model_backbone._chain.stale() and hip.model_head._chain.stale()
    y2 = hip.predict(x)
    assert calls.count('vv_pack_conv2d') == 7 + 2 and not hip.model_backbone._chain.stale()
    assert np.abs((y2 - y).cpu().numpy()).max() > 1e-6


def test_chain_repacks_after_load_weights_and_an_optimizer_step(L, dtype, tmp_path):
    dtype('f32')
    pair = build_pair('Darknet53Tiny')
    b = pair['hip']
    x = image((1, 64, 64), seed=4)

    def follows(what):
        ref = f64_run(b, x)
        hip = b(x)
        with torch.no_grad():
            b.eval()
            tor = nn.Module.__call__(b, torch.from_numpy(x).to(DEV))
        for h, t, r in zip(hip, tor, ref):
            e_hip, e_torch = np.abs(h.cpu().numpy() - r).max(), np.abs(t.cpu().numpy() - r).max()
            print('%s: e_hip %.3e e_torch %.3e' % (what, e_hip, e_torch))
            assert e_hip <= 4 * e_torch + 1e-6 * np.abs(r).max(), what
        return hip[-1].cpu().numpy()

    y0 = follows('as built')
    assert not b._chain.stale()
    opt = torch.optim.Adam(b.trainable_variables, lr=1e-2)
    b(x, training=True)[-1].square().mean().backward()
    opt.step()
    assert b._chain.stale()
    y1 = follows('after an Adam step')
    assert np.abs(y1 - y0).max() > 1e-4
    other = build_pair('Darknet53Tiny', seed=9)['torch']
    other.save_weights(str(tmp_path / 'w'))
    b.load_weights(str(tmp_path / 'w'))
    assert b._chain.stale()
    y2 = follows('after load_weights')
    assert np.abs(y2 - y1).max() > 1e-4 and not b._chain.stale()
