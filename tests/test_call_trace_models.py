"""Which library calls the MODEL classes of src/module/nolbo.py issue -- getEval in every form, getLatent, fit, getSampledEval,
eval_forward_device -- in which order and with which arguments.  CPU only, with the recorder of tests/test_call_trace.py and one more
name replaced (nolbo._st: stream 0); the engines' parameters and every input are zero and every draw (_eps, _mask, _eps2, _rand) is
injected, so nothing depends on a generator.  tests/golden/model_call_traces.json was recorded from the commit BEFORE the classes'
evaluation algorithm was written once, with one exception: the ten 3-input getEval(training=True) cases of the three voxel classes were
re-recorded from the single body (--only), which issues vv_nearest_category / vv_category_accuracy in front of the decoder pass, as the
evaluation-mode body and the reference do, where the training-mode copy issued them behind it.  Each of the ten is a permutation of the
parent's trace that moves those two entry points only.  The cases of the rest of the image family (nolboSingleObject, _instOnly,
_category_only, _AE, the dropout and latent='hip' fits) were recorded from the commit BEFORE their training step was written once and
the two-prior stage's callers moved to voxvae/mm_latent.py.  The file changes only with a deliberate change of what a method launches:
    python tests/test_call_trace_models.py --write [--package DIR] [--only REGEX]   (DIR: another checkout's anytime-3d-reconstruction_amd)
"""
import contextlib
import ctypes
import functools
import json
import os
import re
import sys

import pytest

from test_call_trace import LATENT, ROOT, _golden as _load_golden, _recording, _store, _zeros

GOLDEN = os.path.join(ROOT, 'tests', 'golden', 'model_call_traces.json')
BATCH, CLASSES, SAMPLES = 8, 40, 4
MODELS = {'VAE': 'nolboSingleObject_modelnet_category_VAE', 'AE': 'nolboSingleObject_modelnet_category_AE',
          'only': 'nolboSingleObject_modelnet_category_only', 'image': 'nolboSingleObject_VAE', 'imageAE': 'nolboSingleObject_AE',
          'mm': 'nolboSingleObject', 'inst': 'nolboSingleObject_instOnly', 'cat': 'nolboSingleObject_category_only'}
LC, INSTS = LATENT // 2, 10          # the multi-modal model's category half (the instance half is the rest); instance one-hot width


INPUTS = {'mm': ('x', 'y', 'cat', 'inst'), 'inst': ('x', 'y', 'inst'), 'cat': ('x', 'y', 'cat')}       # what fit's `inputs` holds


def _cases():
    """name -> dict(model, dtype, side, method, args): args = (inputs, missing_prob, training) for getEval."""
    cases = {}

    def add(model, dtype, side, method, *args):
        name = '-'.join([model, dtype, str(side), method] + [str(a) for a in args])
        assert name not in cases
        cases[name] = dict(model=model, dtype=dtype, side=side, method=method, args=args)

    for model, dtypes in (('VAE', ('f32', 'bf16')), ('AE', ('f32', 'bf16')), ('only', ('f32',)), ('image', ('f32',))):
        for dtype in dtypes:
            for training in (False, True):
                for inputs in (3, 2) if model != 'image' else (3,):       # the image -> 3D model has no 2-input form
                    for missing_prob in (0.0, 0.5):
                        add(model, dtype, 16, 'getEval', inputs, missing_prob, training)
            add(model, dtype, 16, 'getLatent')
            add(model, dtype, 16, 'fit')
            if model == 'VAE':
                add(model, dtype, 16, 'fit_dropout')
            if model != 'AE':
                add(model, dtype, 16, 'getSampledEval', SAMPLES)
    for model in ('VAE', 'AE'):                                           # side 32: the fused latent tail
        add(model, 'bf16', 32, 'getEval', 3, 0.0, False)
        add(model, 'bf16', 32, 'eval_forward_device')
    # the rest of the image family: fit on either latent leg with each branch of the decoder-input draw, and the getEval forms of their own
    for model, getEval in (('mm', [(d, t) for d in ('f32', 'bf16') for t in (False, True)]), ('inst', [('f32', False), ('bf16', False), ('f32', True)]),
                           ('cat', [])):
        for dtype in ('f32', 'bf16'):
            for draw in (False, True):                                    # mix (mm, cat) / from_prior (inst)
                add(model, dtype, 16, 'fit_hip', draw)
        add(model, 'f32', 16, 'fit_torch', True)
        for dtype, training in getEval:
            for missing_prob in (0.0, 0.5):
                add(model, dtype, 16, 'getEval', len(INPUTS[model]), missing_prob, training)
    add('imageAE', 'f32', 16, 'fit')
    add('imageAE', 'f32', 16, 'fit_dropout')
    add('image', 'f32', 16, 'fit_dropout')
    for mix in (True, False):
        add('only', 'f32', 16, 'fit_hip', mix)
    for latent in ('hip', 'torch'):
        add('only', 'f32', 16, 'fit_dropout_' + latent, True)
    return cases


CASES = _cases()


@contextlib.contextmanager
def _model_recording(trace, dtype):
    import importlib
    import voxvae
    import src.module.nolbo as nolbo
    mods = [nolbo]
    for name in ('voxvae.prior_latent', 'voxvae.mm_latent'):          # a --package checkout from before a module existed has none to replace
        with contextlib.suppress(ImportError):
            mods.append(importlib.import_module(name))
    saved = [m._st for m in mods], voxvae.default_device(), voxvae.default_dtype()
    for m in mods:
        m._st = lambda: ctypes.c_void_p(0)
    voxvae.set_default_device('cpu')
    voxvae.set_default_dtype(dtype)
    try:
        with _recording(trace):
            yield nolbo
    finally:
        for m, st in zip(mods, saved[0]):
            m._st = st
        voxvae.set_default_device(saved[1])
        voxvae.set_default_dtype(saved[2])


def _build(nolbo, c):
    from voxvae import synthetic as syn
    import src.net_core.priornet as priornet
    model, side = c['model'], c['side']
    cfg = syn.make_config(side, LATENT, model != 'AE')
    prior = lambda n, width, **kw: dict(priornet.priornet_structure, input_dim=n, unit_num_list=[64, 32, width], **kw)
    if model in ('image', 'imageAE'):      # fed head outputs [B, 2L] (the autoencoder: latents [B, L]): no backbone
        cfg = {'encoder_backbone': {'name': 'nolbo_backbone', 'z_dim': LATENT}, 'decoder': cfg['decoder']}
    elif model == 'only':
        cfg['prior_class'] = dict(priornet.priornet_structure, unit_num_list=[64, 32, LATENT])
    elif model == 'mm':       # a learned log-variance for the category prior, a constant one for the instance prior: one NULL pair in the backward
        cfg = {'encoder_backbone': {'name': 'nolbo_backbone', 'z_category_dim': LC, 'z_inst_dim': LATENT - LC}, 'decoder': cfg['decoder'],
               'prior_class': prior(CLASSES, LC), 'prior_inst': prior(CLASSES + INSTS, LATENT - LC, const_log_var=0.0)}
    elif model == 'inst':
        cfg = {'encoder_backbone': {'name': 'nolbo_backbone', 'z_inst_dim': LATENT}, 'decoder': cfg['decoder'], 'prior_inst': prior(INSTS, LATENT, const_log_var=0.0)}
    elif model == 'cat':
        cfg = {'encoder_backbone': {'name': 'nolbo_backbone', 'z_category_dim': LATENT}, 'decoder': cfg['decoder'], 'prior_class': prior(CLASSES, LATENT)}
    kw = {'dropout': True} if c['method'] == 'fit_dropout' else {}
    m = getattr(nolbo, MODELS[model])(nolbo_structure=cfg, **kw)
    for eng in (getattr(m, '_enc_eng', None), m._dec_eng):
        if eng is not None:
            _zeros(eng)
    return m


def record(case):
    """The trace of one case: a list of 'name(arg, ...)' strings."""
    import numpy as np
    import torch
    c, B, L = case, BATCH, LATENT
    trace = []
    with _model_recording(trace, c['dtype']) as nolbo:
        m = _build(nolbo, c)
        D, model, method = c['side'], c['model'], c['method']
        y = torch.zeros(B, D, D, D, 1)
        x = torch.zeros(B, L) if model == 'imageAE' else torch.zeros(B, 2 * L) if model in ('image', 'mm', 'inst', 'cat') else y
        oh, cats, zl = torch.zeros(B, CLASSES), torch.zeros(CLASSES, L), torch.zeros(B, L)
        ones, rand = torch.ones(B, L), dict(eps=zl, eps_prior=zl)
        if model in INPUTS:
            inputs = tuple(dict(x=x, y=y, cat=oh, inst=torch.zeros(B, INSTS))[k] for k in INPUTS[model])
            if method == 'getEval':
                _, missing_prob, training = c['args']
                if model == 'mm':
                    m.getEval(inputs, np.identity(CLASSES), np.identity(INSTS), training=training, missing_prob=missing_prob, _eps=zl,
                              _mask=torch.ones(B, LC), _eps2=torch.zeros(B, LC))
                else:
                    m.getEval(x, y, missing_prob=missing_prob, training=training, _eps=zl, _mask=ones, _fill=zl)
            else:
                draw = dict(from_prior=c['args'][0]) if model == 'inst' else dict(mix=c['args'][0], noise=ones)
                m.fit(inputs, latent=method[len('fit_'):], _rand=dict(rand, **draw))
        elif model == 'only' and method != 'fit' and method.startswith('fit'):
            drop = method.startswith('fit_dropout')
            m.fit((x, y, oh), drop, latent=method.rsplit('_', 1)[1], _rand=dict(rand, mix=c['args'][0], noise=ones, drop_rate=0.25, drop_keep=ones))
        elif model in ('image', 'imageAE') and method.startswith('fit'):
            kw = dict(_dropout=(0.25, ones)) if method == 'fit_dropout' else {}
            m.fit((x, y), **(kw if model == 'imageAE' else dict(kw, _eps=zl)))
        elif method == 'getEval':
            n, missing_prob, training = c['args']
            kw = dict(training=training, missing_prob=missing_prob, _eps=zl, _mask=torch.ones(B, L))
            if n == 2:
                m.getEval((x, y), **kw)
            elif model == 'only':
                m.getEval((x, y, oh), _eps2=zl, **kw)
            else:
                m.getEval((x, y, oh), cats, _eps2=zl, **kw)
        elif method == 'getLatent':
            m.getLatent(x, _eps=zl)
        elif method == 'getSampledEval':
            m.getSampledEval((x, y), c['args'][0], _eps=torch.zeros(B, c['args'][0], L))
        elif method == 'eval_forward_device':
            m.eval_forward_device(x, y, zl)
        elif method == 'fit_dropout':
            m.fit((x, y), _eps=zl, _mask=torch.ones(B, L), _rate=0.25)
        elif model == 'only':
            m.fit((x, y, oh), _rand=dict(eps=zl, eps_prior=zl, mix=True, noise=torch.ones(B, L)))
        elif model == 'AE':
            m.fit((x, y))
        else:
            m.fit((x, y), _eps=zl)
    return trace


_golden = functools.partial(_load_golden, GOLDEN)


def test_golden_covers_exactly_the_cases():
    assert sorted(_golden()) == sorted(CASES)


@pytest.mark.parametrize('name', sorted(CASES))
def test_model_call_trace(name):
    want, got = _golden()[name], record(CASES[name])
    for i, (w, g) in enumerate(zip(want, got)):
        assert w == g, '%s: call %d differs\n  recorded from the parent: %s\n  now:                      %s' % (name, i, w, g)
    assert len(want) == len(got), '%s: %d calls recorded from the parent, %d now; first extra: %s' % (
        name, len(want), len(got), (want + got)[min(len(want), len(got))])


if __name__ == '__main__':
    import argparse
    ap = argparse.ArgumentParser()
    ap.add_argument('--write', action='store_true', required=True)
    ap.add_argument('--package', default=os.path.join(ROOT, 'anytime-3d-reconstruction_amd'))
    ap.add_argument('--only', default='', help='re-record the cases whose name matches this regular expression; the others keep their golden trace')
    a = ap.parse_args()
    sys.path.insert(0, a.package)
    traces = dict(_golden()) if a.only else {}
    traces.update({name: record(CASES[name]) for name in sorted(CASES) if re.search(a.only, name)})
    with open(GOLDEN, 'w') as f:
        json.dump(_store(traces), f, indent=0, sort_keys=True)
        f.write('\n')
    print('%d cases, %d calls -> %s' % (len(traces), sum(len(t) for t in traces.values()), GOLDEN))
