"""The training step at the reference's native 64^3 grid (train_modelnet_category_VAE.py: make_config(latent_dim, 64, True)) and at two
other depths, launch by launch.

At 64^3 the trainer runs another set of kernel forms than at 32^3 (NATIVE_ROUTES below), and the bf16 whole-step test allows 6 % per
gradient tensor: one wrong boundary plane of one layer passes that.  Here ONE bf16 step is taken with Trainer.debug = {} and every
launch is recomputed in float64 from the operands the trainer held (tests/_train_layer_ref.py: teacher forcing, per-element bounds).
The route tables are asserted first, so that a routing change fails a test instead of emptying it."""
import copy

import numpy as np
import pytest
import torch

import _train_layer_ref as LR

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
LZ = 64

# form of every stride-2 launch of a bf16 step: layer -> (forward, data gradient).  'E2' is enc/conv1, 'D2' dec/convT1.
NATIVE_ROUTES = {'E2': ('direct', 'direct'),        # conv 32^3 x 64 -> 128 | convT 16^3 x 128 -> 64
                 'E3': ('igemm', 'igemm'),          # conv 16^3 x 128 -> 256 | convT 8^3 x 256 -> 128
                 'E4': ('skip', 'skip'),            # conv 8^3 x 256 -> 512 | convT 4^3 x 512 -> 256
                 'D2': ('skip', 'skip'),            # convT 4^3 x 512 -> 256 | conv 8^3 x 256 -> 512
                 'D3': ('igemm', 'igemm'),          # convT 8^3 x 256 -> 128 | conv 16^3 x 128 -> 256
                 'D4': ('direct', 'direct')}        # convT 16^3 x 128 -> 64 (plain statistics sweep) | conv 32^3 x 64 -> 128
SIX_ROUTES = {'E2': ('direct', 'whole'), 'E3': ('skip', 'skip'), 'E4': ('pos', 'pos'), 'E5': ('igemm', 'igemm'),     # E5: side 2 behind a pos layer
              'D2': ('igemm', 'igemm'), 'D3': ('pos', 'pos'), 'D4': ('skip', 'skip'), 'D5': ('whole', 'direct')}
FOUR_ROUTES = {'E2': ('skip', 'igemm'), 'E3': ('pos', 'pos'), 'D2': ('pos', 'pos'), 'D3': ('igemm', 'skip')}
W192_ROUTES = {'E2': ('direct', 'whole'), 'E3': ('skip', 'skip'), 'E4': ('pos', 'pos'),                              # E4: 256 -> 192, three 64-tiles
               'D2': ('pos', 'pos'), 'D3': ('skip', 'skip'), 'D4': ('whole', 'direct')}

CONFIGS = {  # name -> (D, B, encoder filters without the output width, decoder filters, routes)
    'six layers': (32, 3, [64, 128, 256, 512, 512], [512, 512, 256, 128, 64, 1], SIX_ROUTES),
    'four layers': (16, 4, [64, 128, 256], [256, 128, 64, 1], FOUR_ROUTES),
    'width 192': (32, 4, [64, 128, 256, 192], [512, 256, 128, 64, 1], W192_ROUTES),
}


def _config(D, var, enc_filters=None, dec_filters=None):
    from voxvae import synthetic as syn
    cfg = copy.deepcopy(syn.make_config(D, LZ, var))
    for side, filters in (('encoder', None if enc_filters is None else list(enc_filters) + [2 * LZ if var else LZ]), ('decoder', dec_filters)):
        if filters is not None:
            n = len(filters)
            cfg[side]['filter_num_list'] = list(filters)
            cfg[side]['filter_size_list'] = [4] * n
            cfg[side]['strides_list'] = [2] * (n - 1) + [1] if side == 'encoder' else [1] + [2] * (n - 1)
    return cfg


def _build(cfg, var, B, dtype, seed=0):
    """test_gpu_train._setup for any filter lists."""
    import voxvae
    from voxvae import synthetic as syn
    voxvae.set_default_dtype(dtype)
    voxvae.set_default_device(DEV)
    import src.module.nolbo as nolbo
    ep = syn.make_encoder_params(cfg['encoder'], seed=42, nontrivial_affine=True)
    dp = syn.make_decoder_params(cfg['decoder'], seed=43, nontrivial_affine=True, final_gain=2.0)
    cls = nolbo.nolboSingleObject_modelnet_category_VAE if var else nolbo.nolboSingleObject_modelnet_category_AE
    model = cls(nolbo_structure=cfg, learning_rate=1e-3)
    model._encoder.set_weights_dict(ep)
    model._decoder.set_weights_dict(dp)
    D = cfg['encoder']['input_shape'][0]
    return ep, dp, model, syn.make_voxels(B, D, seed=100 + seed), syn.make_eps(B, LZ, seed=200 + seed)


def _routes_of(tr):
    """{layer: (forward form, data-gradient form)} through Trainer._route, what _stride2 asks at every launch."""
    from voxvae import routes as R
    tr.sw = R.switches()
    got = {}
    fe, side = tr.enc.filters, tr.enc.D // 2
    for i in range(1, len(fe) - 1):
        got['E%d' % (i + 1)] = (tr._route(R.CONV, side, fe[i - 1], fe[i]), tr._route(R.CONVT, side // 2, fe[i], fe[i - 1]))
        side //= 2
    fd, side = tr.dec.filters, tr.dec.S
    for i in range(1, len(fd) - 1):
        got['D%d' % (i + 1)] = (tr._route(R.CONVT, side, fd[i - 1], fd[i]), tr._route(R.CONV, 2 * side, fd[i], fd[i - 1]))
        side *= 2
    return got


def _prepack_jobs(tr):
    """The (direction, cin, cout) list of the step's batched weight images (Trainer._prepack), sorted."""
    from voxvae import routes as R
    tr.sw = R.switches()
    for e in (tr.enc, tr.dec):
        e.ensure_packed(fold=False)                  # the engines' plans: which images they hold themselves
    tr._prepack()
    torch.cuda.synchronize()
    jobs = sorted((k, cin, cout) for k, _, cin, cout in tr._prepacked)
    tr._prepacked = {}
    return jobs


def _trainer(cfg, var, B, monkeypatch=None, wgrad_stream='0'):
    from voxvae import train as T
    if monkeypatch is not None:
        monkeypatch.setenv('VOXVAE_WGRAD_STREAM', wgrad_stream)
    ep, dp, model, x, eps = _build(cfg, var, B, 'bf16')
    tr = T.Trainer(model._enc_eng, model._dec_eng, var, 1e-3)
    assert (tr.wgrad_stream is not None) == (wgrad_stream == '1')
    return tr, model, x, eps


def _report(F, label):
    print('\n[%s] worst err / bound per check:' % label)
    for k, v in F.ratios.items():
        print('    %-64s %.3f' % (k, v))
    F.raise_if_any()


# ------------------------------------------------------------------------------------------------ bf16, 64^3, layer by layer
@pytest.fixture(scope='module')
def native():
    """One bf16 step of the reference config at 64^3, B = 2, on one stream: (routes, batched image list, capture).  Read-only."""
    mp = pytest.MonkeyPatch()
    try:
        tr, model, x, eps = _trainer(_config(64, True), True, 2, mp, '0')
        routes, jobs = _routes_of(tr), _prepack_jobs(tr)
        cap = LR.capture(tr, x, eps)
    finally:
        mp.undo()
    return routes, jobs, cap


def test_native_grid_runs_the_forms_it_is_tested_on(native):
    from voxvae import routes as R
    routes, jobs, cap = native
    assert routes == NATIVE_ROUTES
    # encoder tail and D1 as dense panels over a 4^3 map: vv_pack_conv_k4s1_meanpool / vv_unpack_meanpool_grad and
    # vv_pack_convT_k4s1_dense / vv_unpack_convT_dense_grad with side 4
    assert cap['Se'] == 4 and cap['Se'] ** 3 * cap['fe'][-2] == 32768
    assert cap['Sd'] == 4 and cap['Sd'] ** 3 * cap['fd'][0] == 32768
    assert tuple(cap['dpanel_enc'].shape) == (128, 32768) and tuple(cap['dpanel_dec'].shape) == (32768, 512)
    # D4 is the direct form: no column sums of its own, the statistics sweep runs
    assert cap['fused_stats'] == [False, False, False, False]
    # final layer, vv_bce_bwd, the last weight gradient and the first-conv-form data gradient at side 64
    assert tuple(cap['probs'].shape) == (2, 64, 64, 64, 1) and tuple(cap['dlogit'].shape) == (2, 64, 64, 64, 1)
    assert tuple(cap['dh_dec'][3].shape) == (2, 32, 32, 32, 64) and cap['grads']['dec/convT4/kernel'].shape == (4, 4, 4, 1, 64)
    # the batched weight images: the four 'skip' launches (nine images at 32^3)
    assert jobs == sorted([(R.CONV, 256, 512), (R.CONVT, 512, 256), (R.CONVT, 512, 256), (R.CONV, 256, 512)])


def test_native_grid_encoder_launches_against_float64(native):
    _report(LR.check_step(native[2], ('encoder',)), 'bf16 64^3 encoder')


def test_native_grid_decoder_launches_against_float64(native):
    _report(LR.check_step(native[2], ('decoder',)), 'bf16 64^3 decoder')


def _same(a, b, what):
    if isinstance(a, dict):
        assert a.keys() == b.keys(), what
        for k in a:
            _same(a[k], b[k], '%s[%s]' % (what, k))
    elif isinstance(a, (list, tuple)):
        assert len(a) == len(b), what
        for i, (u, v) in enumerate(zip(a, b)):
            _same(u, v, '%s[%d]' % (what, i))
    elif isinstance(a, torch.Tensor):
        assert a.dtype == b.dtype and torch.equal(a.view(torch.int16) if a.dtype == torch.bfloat16 else a, b.view(torch.int16) if b.dtype == torch.bfloat16 else b), what
    elif isinstance(a, np.ndarray):
        assert np.array_equal(a, b), what
    else:
        assert a == b, what


def test_native_grid_step_with_the_weight_gradient_stream(native, monkeypatch):
    """The same step with the weight gradients on their own stream (VOXVAE_WGRAD_STREAM=1): every tensor the layer-wise tests above
    checked -- activations, their gradients, statistics, weight gradients, losses -- is the same bits, so their references hold here."""
    tr, model, x, eps = _trainer(_config(64, True), True, 2, monkeypatch, '1')
    assert _routes_of(tr) == NATIVE_ROUTES
    _same(LR.capture(tr, x, eps), native[2], 'capture')


# ------------------------------------------------------------------------------------------------------------- other depths
@pytest.mark.parametrize('name', ['six layers', 'four layers'])
def test_fit_step_matches_autograd_oracle_at_other_depths(name):
    """f32 whole-step oracle parity (the assertions of test_gpu_train.py::test_fit_step_matches_autograd_oracle) at six layers (S = 1: a
    side-2 layer behind the 4^3 -> 2^3 one) and four (S = 2 at 16^3)."""
    from test_gpu_train import _assert_fit_step_matches_oracle
    D, B, fe, fd, _ = CONFIGS[name]
    cfg = _config(D, True, fe, fd)
    ep, dp, model, x, eps = _build(cfg, True, B, 'f32')
    _assert_fit_step_matches_oracle(cfg, ep, dp, model, x, eps, True, name)


@pytest.mark.parametrize('name', ['six layers', 'four layers', 'width 192'])
def test_bf16_step_layer_by_layer_at_other_depths_and_widths(name):
    """Route table, then every launch of one bf16 step against float64.  'width 192': the last stride-2 encoder layer is the
    position-major form with cout = 192 -- three 64-tiles in vv_pack_skip_images -- and its data gradient that form with cin = 192."""
    from voxvae import routes as R
    D, B, fe, fd, want = CONFIGS[name]
    tr, model, x, eps = _trainer(_config(D, True, fe, fd), True, B)
    assert _routes_of(tr) == want
    if name == 'width 192':
        assert (R.CONV, 256, 192) in _prepack_jobs(tr) and (R.CONVT, 192, 256) in _prepack_jobs(tr)
    cap = LR.capture(tr, x, eps)
    assert cap['fused_stats'] == [False] + [f == 'whole' for f, _ in (want['D%d' % (i + 1)] for i in range(1, len(fd) - 1))]
    _report(LR.check_step(cap), 'bf16 ' + name)


# ------------------------------------------------------------------- a width the engines evaluate and the trainer cannot fit
def test_trainer_refuses_a_stride2_width_without_a_data_gradient_form():
    """The 4^3 -> 2^3 position-major form admits any output width that is a multiple of 8 (136 here), so such an encoder evaluates.  Its
    data gradient is a transposed convolution with 136 INPUT channels, which no form takes (position-major and whole-sample forms:
    multiples of 64; implicit GEMM: 64 * 2^k).  The Trainer says so when it is built -- naming the layer and the rule -- instead of
    failing inside step() with the layer half trained; evaluation of the same model is untouched."""
    from oracle import torch_oracle as to
    from voxvae import lib as L
    from voxvae import routes as R
    from voxvae import synthetic as syn
    from voxvae import train as T
    lib = L.load()
    assert lib.vv_conv3d_k4s2_pos_supported(4, 256, 136, L.VV_BF16) and not lib.vv_convT3d_k4s2_pos_supported(2, 136, 256, L.VV_BF16)
    assert not R.igemm_admits(136, 256, L.VV_BF16) and R.igemm_admits(128, 256, L.VV_BF16) and R.igemm_admits(256, 136, L.VV_BF16)
    B = 4
    cfg = _config(32, True, [64, 128, 256, 136])
    ep, dp, model, x, eps = _build(cfg, True, B, 'bf16')
    with pytest.raises(ValueError) as e:
        T.Trainer(model._enc_eng, model._dec_eng, True, 1e-3)
    msg = str(e.value)
    assert 'enc/conv3/kernel' in msg and 'data gradient' in msg and '136' in msg and 'multiple of 64' in msg
    with pytest.raises(ValueError):
        model.fit((x, x), _eps=eps)
    # the widths the trainer does take are not refused: a decoder-only trainer of the same model, and width 192 (tested above)
    T.Trainer(None, model._dec_eng, True, 1e-3)
    # evaluation: the bf16 tolerance of test_gpu_api.py::test_getLatent_and_bf16_api (loss within 2 %), against the float32 forward
    oh, cats = syn.make_onehot(B, 40), syn.make_category_vectors(40, LZ)
    out = model.getEval(inputs=(x, x, oh), category_vectors=cats, missing_prob=0.0, _eps=eps)
    torch.cuda.synchronize()
    logits, bce, tp, fp, fn = to.eval_forward_f32(cfg, ep, dp, x, eps)
    want = float(bce.mean())
    print('\n[width 136 getEval] loss_shape %.4f, float32 forward %.4f' % (float(out[1]), want))
    assert abs(float(out[1]) - want) < 0.02 * want
    assert np.array(out[0]).shape == (B, 32, 32, 32, 1)
