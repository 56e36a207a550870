"""Which library calls the MODEL classes of src/module/nolbo.py issue -- getEval in every form, getLatent, fit, getSampledEval,
eval_forward_device -- in which order and with which arguments.  CPU only, with the recorder of tests/test_call_trace.py and one more
name replaced (nolbo._st: stream 0); the engines' parameters and every input are zero and every draw (_eps, _mask, _eps2, _rand) is
injected, so nothing depends on a generator.  tests/golden/model_call_traces.json was recorded from the commit BEFORE the classes'
evaluation algorithm was written once, with one exception: the ten 3-input getEval(training=True) cases of the three voxel classes were
re-recorded from the single body (--only), which issues vv_nearest_category / vv_category_accuracy in front of the decoder pass, as the
evaluation-mode body and the reference do, where the training-mode copy issued them behind it.  Each of the ten is a permutation of the
parent's trace that moves those two entry points only.  The file changes only with a deliberate change of what a method launches:
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
          'only': 'nolboSingleObject_modelnet_category_only', 'image': 'nolboSingleObject_VAE'}


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
    return cases


CASES = _cases()


@contextlib.contextmanager
def _model_recording(trace, dtype):
    import voxvae
    import src.module.nolbo as nolbo
    saved = nolbo._st, voxvae.default_device(), voxvae.default_dtype()
    nolbo._st = lambda: ctypes.c_void_p(0)
    voxvae.set_default_device('cpu')
    voxvae.set_default_dtype(dtype)
    try:
        with _recording(trace):
            yield nolbo
    finally:
        nolbo._st = saved[0]
        voxvae.set_default_device(saved[1])
        voxvae.set_default_dtype(saved[2])


def _build(nolbo, c):
    from voxvae import synthetic as syn
    import src.net_core.priornet as priornet
    model, side = c['model'], c['side']
    cfg = syn.make_config(side, LATENT, model != 'AE')
    if model == 'image':      # fed head outputs [B, 2L]: no backbone
        cfg = {'encoder_backbone': {'name': 'nolbo_backbone', 'z_dim': LATENT}, 'decoder': cfg['decoder']}
    elif model == 'only':
        cfg['prior_class'] = dict(priornet.priornet_structure, unit_num_list=[64, 32, LATENT])
    kw = {'dropout': True} if c['method'] == 'fit_dropout' else {}
    m = getattr(nolbo, MODELS[model])(nolbo_structure=cfg, **kw)
    for eng in (getattr(m, '_enc_eng', None), m._dec_eng):
        if eng is not None:
            _zeros(eng)
    return m


def record(case):
    """The trace of one case: a list of 'name(arg, ...)' strings."""
    import torch
    c, B, L = case, BATCH, LATENT
    trace = []
    with _model_recording(trace, c['dtype']) as nolbo:
        m = _build(nolbo, c)
        D, model, method = c['side'], c['model'], c['method']
        y = torch.zeros(B, D, D, D, 1)
        x = torch.zeros(B, 2 * L) if model == 'image' else y
        oh, cats, zl = torch.zeros(B, CLASSES), torch.zeros(CLASSES, L), torch.zeros(B, L)
        if method == 'getEval':
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
