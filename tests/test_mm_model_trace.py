"""Which library calls nolboSingleObject issues for its latent stage, CPU only, with the recorder of tests/test_call_trace.py:
getEval is exactly one vv_mm_latent_eval and none of the older latent entries, in both missing_prob forms and both activation dtypes;
fit is exactly one vv_mm_latent_train_fwd and one vv_mm_latent_train_bwd around the decoder's step; fit(latent='torch') issues neither."""
import contextlib
import ctypes

import numpy as np
import pytest
import torch

from test_call_trace import _recording, _zeros

B, LC, LI, C, I, D = 8, 4, 4, 12, 10, 16
OLDER = {'vv_latent_mask_fill', 'vv_nearest_category', 'vv_latent_correct', 'vv_category_accuracy', 'vv_reparam_kl_fwd', 'vv_reparam_kl_bwd'}


def config():
    from voxvae import synthetic as syn
    prior = lambda name, n: {'name': name, 'input_dim': n, 'unit_num_list': [16, 8, 4], 'core_activation': 'elu', 'const_log_var': 0.0}
    return {'encoder_backbone': {'name': 'bb', 'z_category_dim': LC, 'z_inst_dim': LI}, 'encoder_head': None,
            'decoder': syn.make_config(D, LC + LI, True)['decoder'], 'prior_class': prior('priornet_class', C), 'prior_inst': prior('priornet_inst', C + I)}


@contextlib.contextmanager
def recording(trace, dtype):
    import voxvae
    import src.module.nolbo as nolbo
    saved = nolbo._st, voxvae.default_device(), voxvae.default_dtype()
    nolbo._st = lambda: ctypes.c_void_p(0)
    voxvae.set_default_device('cpu')
    voxvae.set_default_dtype(dtype)
    try:
        with _recording(trace):
            m = nolbo.nolboSingleObject(nolbo_structure=config())          # fed head outputs [B, 2 Lc + 2 Li]: no backbone
            _zeros(m._dec_eng)
            yield m
    finally:
        nolbo._st = saved[0]
        voxvae.set_default_device(saved[1])
        voxvae.set_default_dtype(saved[2])


def _inputs():
    return (torch.zeros(B, 2 * LC + 2 * LI), torch.zeros(B, D, D, D, 1), np.eye(C, dtype=np.float32)[np.arange(B) % C],
            np.eye(I, dtype=np.float32)[np.arange(B) % I])


def _names(trace):
    return [t.split('(')[0] for t in trace if not t.startswith('#')]


@pytest.mark.parametrize('dtype', ['f32', 'bf16'])
@pytest.mark.parametrize('training', [False, True])
@pytest.mark.parametrize('missing_prob', [0.0, 0.5])
def test_getEval_is_one_mm_latent_eval(missing_prob, training, dtype):
    trace = []
    with recording(trace, dtype) as m:
        out = m.getEval(_inputs(), np.identity(C), np.identity(I), training=training, missing_prob=missing_prob, _eps=torch.zeros(B, LC + LI),
                        _mask=torch.ones(B, LC) if missing_prob > 0 else None, _eps2=torch.zeros(B, LC) if missing_prob > 0 else None)
    names = _names(trace)
    assert len(out) == (11 if missing_prob > 0 else 6)
    assert names.count('vv_mm_latent_eval') == 1 and not OLDER & set(names), names
    assert sum(n.startswith('vv_convT3d_final_bce') for n in names) == (2 if missing_prob > 0 else 1)   # the decoder once or twice
    call = [t for t in trace if t.startswith('vv_mm_latent_eval(')][0]
    assert call.endswith('%d, %d, %d, %d, %d, stream)' % (B, LC, LI, C, I))


@pytest.mark.parametrize('dtype', ['f32', 'bf16'])
@pytest.mark.parametrize('mix', [False, True])
def test_fit_is_one_train_fwd_and_one_train_bwd(mix, dtype):
    trace = []
    zl = torch.zeros(B, LC + LI)
    with recording(trace, dtype) as m:
        out = m.fit(_inputs(), _rand=dict(eps=zl, eps_prior=zl, mix=mix, noise=torch.ones(B, LC + LI)))
    names = _names(trace)
    assert len(out) == 5
    assert names.count('vv_mm_latent_train_fwd') == 1 and names.count('vv_mm_latent_train_bwd') == 1 and not OLDER & set(names), names
    fwd, bwd, dec, adam = (names.index(n) for n in ('vv_mm_latent_train_fwd', 'vv_mm_latent_train_bwd', 'vv_convT3d_final_bce_fwd', 'vv_adam_step_multi'))
    assert fwd < dec < bwd and names.index('vv_bce_bwd') < bwd                            # the decoder's step sits between the two
    assert names.count('vv_adam_step_multi') == 1 and adam > dec
    # a constant log-variance (const_log_var: 0.0) has no gradient: its two outputs are NULL
    call = [t for t in trace if t.startswith('vv_mm_latent_train_bwd(')][0]
    assert call.count('None') == (2 if mix else 3)                                         # and the noise pointer without the mix


def test_fit_torch_form_issues_neither():
    trace = []
    zl = torch.zeros(B, LC + LI)
    with recording(trace, 'f32') as m:
        m.fit(_inputs(), latent='torch', _rand=dict(eps=zl, eps_prior=zl, mix=True, noise=torch.ones(B, LC + LI)))
        with pytest.raises(ValueError):
            m.fit(_inputs(), latent='eager')
    names = _names(trace)
    assert 'vv_mm_latent_train_fwd' not in names and 'vv_mm_latent_train_bwd' not in names and names.count('vv_adam_step_multi') == 1
