"""Host logic of the one-prior model classes, CPU only, with the recorder of tests/test_call_trace.py: which library calls
nolboSingleObject_instOnly, nolboSingleObject_category_only and nolboSingleObject_modelnet_category_only.fit(latent='hip') issue for
their latent stage, with which constants and for which branch of the decoder-input draw; the return arities; and a save / load round
trip of the prior network."""
import contextlib
import ctypes

import numpy as np
import pytest
import torch

from test_call_trace import _recording, _zeros

B, LZ, C, I, D = 4, 8, 12, 10, 16
OLDER = {'vv_latent_mask_fill', 'vv_nearest_category', 'vv_latent_correct', 'vv_category_accuracy', 'vv_reparam_kl_fwd', 'vv_reparam_kl_bwd',
         'vv_mm_latent_eval', 'vv_mm_latent_train_fwd', 'vv_mm_latent_train_bwd'}
FWD, BWD, EVAL = 'vv_prior_latent_train_fwd', 'vv_prior_latent_train_bwd', 'vv_inst_latent_eval'
#          structure keys                      one-hot width   dist      reg_weight   l2 terms
CLASSES = {'nolboSingleObject_instOnly': ('z_inst_dim', 'prior_inst', I, 10.0 * LZ, 1.0, True),
           'nolboSingleObject_category_only': ('z_category_dim', 'prior_class', C, 3.0 * LZ, 0.01, False)}


def config(name):
    from voxvae import synthetic as syn
    z_key, prior_key, n = CLASSES[name][:3]
    return {'encoder_backbone': {'name': 'bb', z_key: LZ}, 'encoder_head': None, 'decoder': syn.make_config(D, LZ, True)['decoder'],
            prior_key: {'name': 'priornet', 'input_dim': n, 'unit_num_list': [16, LZ], 'core_activation': 'elu', 'const_log_var': 0.0}}


@contextlib.contextmanager
def recording(trace, dtype, build):
    import voxvae
    import src.module.nolbo as nolbo
    from voxvae import prior_latent as PL
    saved = nolbo._st, PL._st, voxvae.default_device(), voxvae.default_dtype()
    nolbo._st = PL._st = lambda: ctypes.c_void_p(0)
    voxvae.set_default_device('cpu')
    voxvae.set_default_dtype(dtype)
    try:
        with _recording(trace):
            m = build(nolbo)
            _zeros(m._dec_eng)
            if getattr(m, '_enc_eng', None) is not None:
                _zeros(m._enc_eng)
            yield m
    finally:
        nolbo._st, PL._st = saved[:2]
        voxvae.set_default_device(saved[2])
        voxvae.set_default_dtype(saved[3])


def _image_model(name):
    return lambda nolbo: getattr(nolbo, name)(nolbo_structure=config(name))              # fed head outputs [B, 2 L]: no backbone


def _inputs(name):
    n = CLASSES[name][2]
    return torch.zeros(B, 2 * LZ), torch.zeros(B, D, D, D, 1), np.eye(n, dtype=np.float32)[np.arange(B) % n]


def _names(trace):
    return [t.split('(')[0] for t in trace if not t.startswith('#')]


def _args(trace, entry):
    """The rendered arguments of the first call of `entry` (a pointer renders as dtype[shape]: commas inside brackets do not split)."""
    import re
    return re.split(r', (?![^\[]*\])', [t for t in trace if t.startswith(entry + '(')][0][len(entry) + 1:-1])


@pytest.mark.parametrize('dtype', ['f32', 'bf16'])
@pytest.mark.parametrize('name,rand,keep_given', [
    ('nolboSingleObject_instOnly', dict(from_prior=False), False),                   # rand < 0.5: decoder(z)
    ('nolboSingleObject_instOnly', dict(from_prior=True), True),                     # else decoder(z_prior): an all-zero keep
    ('nolboSingleObject_category_only', dict(mix=False), False),                     # rand > 0.5: decoder(z)
    ('nolboSingleObject_category_only', dict(mix=True, noise=np.ones((B, LZ), np.float32)), True),
])
def test_fit_is_one_train_fwd_and_one_train_bwd_with_the_class_constants(name, rand, keep_given, dtype):
    dist, reg_weight, l2 = CLASSES[name][3:]
    trace = []
    zl = torch.zeros(B, LZ)
    with recording(trace, dtype, _image_model(name)) as m:
        out = m.fit(_inputs(name), _rand=dict(rand, eps=zl, eps_prior=zl))
        assert m._dist_per_dim * LZ == dist and m._reg_weight == reg_weight and m._network_l2 == l2
    names = _names(trace)
    assert len(out) == 5
    assert names.count(FWD) == 1 and names.count(BWD) == 1 and not OLDER & set(names), names
    fwd, bwd, dec, adam = (names.index(n) for n in (FWD, BWD, 'vv_convT3d_final_bce_fwd', 'vv_adam_step_multi'))
    assert fwd < dec < bwd and names.index('vv_bce_bwd') < bwd                            # the decoder's step sits between the two
    assert names.count('vv_adam_step_multi') == 1 and adam > dec
    f, b = _args(trace, FWD), _args(trace, BWD)
    # enc_out, eps, mean_p, lv_p, eps_p, keep, dist, ...
    assert (f[5] != 'None') == keep_given and (b[5] != 'None') == keep_given
    assert f[6] == float(dist).hex() and b[6] == float(dist).hex()
    assert (f[8] != 'None') == (dtype == 'bf16')                                          # the bfloat16 twin only where the decoder wants one
    assert f[-3:] == [str(B), str(LZ), 'stream']
    # ..., dz_in, inv_batch, reg_weight, d_enc_out, d_mean_p, d_lv_p, B, L, stream: a constant log-variance has no gradient
    assert b[8:10] == [(1.0 / B).hex(), float(reg_weight).hex()] and b[10] != 'None' and b[11] != 'None' and b[12] == 'None'


@pytest.mark.parametrize('name', sorted(CLASSES))
def test_uninjected_draws_take_the_reference_branches(name, monkeypatch):
    """instOnly: rand < 0.5 -> z (nolbo.py:383); category_only: rand > 0.5 -> z (:1042), else a Bernoulli(0.7) keep drawn with the
    reference's call."""
    zl = torch.zeros(B, LZ)
    for u, expect_keep in ((0.25, name == 'nolboSingleObject_category_only'), (0.75, name == 'nolboSingleObject_instOnly')):
        trace = []
        monkeypatch.setattr(np.random, 'rand', lambda *a, u=u: u)
        with recording(trace, 'f32', _image_model(name)) as m:
            m.fit(_inputs(name), _rand=dict(eps=zl, eps_prior=zl))
        assert (_args(trace, FWD)[5] != 'None') == expect_keep, (u, _args(trace, FWD)[5])


@pytest.mark.parametrize('name', sorted(CLASSES))
def test_fit_torch_form_issues_neither(name):
    trace = []
    zl = torch.zeros(B, LZ)
    with recording(trace, 'f32', _image_model(name)) as m:
        out = m.fit(_inputs(name), latent='torch', _rand=dict(eps=zl, eps_prior=zl, from_prior=True, mix=True, noise=np.ones((B, LZ), np.float32)))
        with pytest.raises(ValueError):
            m.fit(_inputs(name), latent='eager')
    names = _names(trace)
    assert len(out) == 5 and FWD not in names and BWD not in names and names.count('vv_adam_step_multi') == 1


@pytest.mark.parametrize('dtype', ['f32', 'bf16'])
@pytest.mark.parametrize('training', [False, True])
@pytest.mark.parametrize('missing_prob', [0.0, 0.5])
def test_instOnly_getEval_is_one_inst_latent_eval(missing_prob, training, dtype):
    name = 'nolboSingleObject_instOnly'
    trace = []
    with recording(trace, dtype, _image_model(name)) as m:
        x, y, _ = _inputs(name)
        out = m.getEval(x, y, np.identity(I), missing_prob, training, _eps=torch.zeros(B, LZ), _mask=torch.ones(B, LZ) if missing_prob > 0 else None,
                        _fill=torch.zeros(B, LZ) if missing_prob > 0 else None)
    names = _names(trace)
    assert len(out) == 8
    assert names.count(EVAL) == 1 and not OLDER & set(names), names
    assert sum(n.startswith('vv_convT3d_final_bce') for n in names) == 2                  # the decoder on z and on the corrected latent
    a = _args(trace, EVAL)
    assert (a[2] != 'None') == (a[3] != 'None') == (missing_prob > 0)
    assert (a[7] != 'None') == (a[8] != 'None') == (dtype == 'bf16' and not training)
    assert a[-4:] == [str(B), str(LZ), str(I), 'stream']


def test_instOnly_getEval_keeps_the_reference_defaults():
    import inspect
    import src.module.nolbo as nolbo
    p = inspect.signature(nolbo.nolboSingleObject_instOnly.getEval).parameters
    assert list(p)[:6] == ['self', 'input_images', 'output_images', 'inst_list', 'missing_prob', 'training']
    assert p['training'].default is True and p['missing_prob'].default == 0.1 and p['inst_list'].default.shape == (10, 10)
    p = inspect.signature(nolbo.nolboSingleObject_category_only.getEval).parameters
    assert list(p)[:5] == ['self', 'inputs', 'category_indices', 'training', 'missing_prob'] and p['category_indices'].default.shape == (12, 12)
    for cls in (nolbo.nolboSingleObject_instOnly, nolbo.nolboSingleObject_category_only):
        assert issubclass(cls, nolbo.nolboSingleObject_VAE)
        assert list(inspect.signature(cls.__init__).parameters) == ['self', 'nolbo_structure', 'backbone_style', 'encoder_backbone', 'learning_rate']


@pytest.mark.parametrize('missing_prob', [0.0, 0.5])
def test_category_only_getEval_is_the_VAE_form_on_the_prior_means(missing_prob):
    name = 'nolboSingleObject_category_only'
    trace = []
    with recording(trace, 'f32', _image_model(name)) as m:
        out = m.getEval(_inputs(name), np.identity(C), missing_prob=missing_prob, _eps=torch.zeros(B, LZ),
                        _mask=torch.ones(B, LZ) if missing_prob > 0 else None, _eps2=torch.zeros(B, LZ) if missing_prob > 0 else None)
    names = _names(trace)
    assert len(out) == 10 and (out[5:] == (0, 0, 0, 0, 0)) == (missing_prob == 0.0)
    assert 'vv_reparam_kl_fwd' in names and EVAL not in names and FWD not in names
    call = [t for t in trace if t.startswith('vv_nearest_category(')][0]
    assert ', float32[%d, %d], %d, ' % (C, LZ, C) in call                                  # classified against the prior network's means


@pytest.mark.parametrize('name,save,load', [('nolboSingleObject_instOnly', 'savePriorInst', 'loadPriorInst'),
                                            ('nolboSingleObject_category_only', 'savePriorCategory', 'loadPriorCategory')])
def test_prior_network_save_load_round_trip(name, save, load, tmp_path):
    trace = []
    with recording(trace, 'f32', _image_model(name)) as m:
        net = m._priornet_inst if name.endswith('instOnly') else m._priornet_class
        assert net is m._priornet and getattr(m, '_%s_str' % CLASSES[name][1])['name'] == 'priornet'
        onehot = _inputs(name)[2]
        before = net(onehot)[0].clone()
        getattr(m, save)(str(tmp_path))
        with torch.no_grad():
            for p in net.parameters():
                p.add_(1.0)
        assert not torch.equal(net(onehot)[0], before)
        getattr(m, load)(str(tmp_path))
        assert torch.equal(net(onehot)[0], before)
        assert callable(m.saveModel) and callable(m.loadModel)


@pytest.mark.parametrize('dropout', [False, True])
@pytest.mark.parametrize('mix', [False, True])
def test_modelnet_fit_hip_is_two_launches_inside_the_step(mix, dropout):
    """nolboSingleObject_modelnet_category_only.fit(latent='hip'): ONE vv_prior_latent_train_fwd after the encoder and ONE
    vv_prior_latent_train_bwd after the decoder's backward, dist 2 L and weight 0.01 as the torch leg; dropout adds one vv_mask_scale
    on z_in and one on dz.  The default leg issues none of them, and its trace is what it was."""
    from voxvae import synthetic as syn
    import src.net_core.priornet as priornet
    cfg = syn.make_config(D, LZ, True)
    cfg['prior_class'] = dict(priornet.priornet_structure, unit_num_list=[16, LZ])
    build = lambda nolbo: nolbo.nolboSingleObject_modelnet_category_only(nolbo_structure=cfg)
    x, oh = torch.zeros(B, D, D, D, 1), np.eye(40, dtype=np.float32)[np.arange(B)]
    zl = torch.zeros(B, LZ)
    rand = dict(eps=zl, eps_prior=zl, mix=mix, noise=torch.ones(B, LZ), drop_rate=0.25, drop_keep=torch.ones(B, LZ))
    traces = {}
    for latent in ('hip', 'torch', None):
        trace = []
        with recording(trace, 'f32', build) as m:
            out = m.fit((x, x, oh), dropout, _rand=rand, **({} if latent is None else {'latent': latent}))
            assert len(out) == 5
        traces[latent] = trace
    assert traces[None] == traces['torch']                                               # the default stays the torch leg
    names = _names(traces['hip'])
    assert names.count(FWD) == 1 and names.count(BWD) == 1 and names.count('vv_mask_scale') == (2 if dropout else 0)
    assert FWD not in _names(traces['torch']) and BWD not in _names(traces['torch']) and 'vv_mask_scale' not in _names(traces['torch'])
    fwd, bwd, dec, bce = (names.index(n) for n in (FWD, BWD, 'vv_convT3d_final_bce_fwd', 'vv_bce_bwd'))
    assert fwd < dec < bce < bwd
    if dropout:
        ms = [i for i, n in enumerate(names) if n == 'vv_mask_scale']
        assert fwd < ms[0] < dec and bce < ms[1] < bwd
    f, b = _args(traces['hip'], FWD), _args(traces['hip'], BWD)
    assert (f[5] != 'None') == mix and f[6] == (2.0 * LZ).hex() and b[9] == 0.01.hex()
    # apart from the latent stage the two legs issue the same library calls in the same order
    other = lambda t: [n for n in _names(t) if n not in (FWD, BWD, 'vv_mask_scale')]
    assert other(traces['hip']) == other(traces['torch'])
