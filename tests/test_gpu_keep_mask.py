"""GPU tests of the keep masks drawn on the device (csrc/keep_mask.hip): vv_keep_mask against its host twin bit for bit, vv_mask_scale
against numpy float32 as bits, both on guard-banded buffers, and voxvae.masks.KeepMasks through getEval(missing_prob > 0)."""
import ctypes

import numpy as np
import pytest
import torch

import _guarded as G

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
SHAPES = [(1, 1), (1, 3), (3, 5), (5, 64), (256, 64), (257, 63)]      # (257, 63): 16191 elements, a 3-element tail in the last workgroup
RATES = [0.0, 0.1, 0.35, 0.5, 0.9, float(np.nextafter(np.float32(1), np.float32(0)))]
SEEDS = [0, 1, 2 ** 63 + 5]
OFFSETS = [0, 1, 2 ** 40, 2 ** 56 + 7]


def _st():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _host_mask(B, Lz, rate, seed, offset):
    from voxvae import lib as L
    keep = np.full((B, Lz), np.nan, dtype=np.float32)
    L.call('vv_keep_mask_host', keep.ctypes.data_as(ctypes.c_void_p), B, Lz, rate, seed, offset)
    return keep


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


@pytest.fixture
def device_masks():
    """Models built inside draw their masks on the device; the process goes back to what it was."""
    import voxvae
    from voxvae import masks as M
    before, seed = voxvae.mask_source(), M._SEED['value']
    voxvae.set_mask_source('device')
    yield M
    voxvae.set_mask_source(before)
    M.manual_seed(seed)


@pytest.mark.parametrize('B,Lz', SHAPES)
def test_device_mask_equals_the_host_entry_bit_for_bit(B, Lz):
    from voxvae import lib as L
    keep = torch.empty(B, Lz, dtype=torch.float32, device=DEV)
    for rate in RATES:
        for seed in SEEDS:
            for offset in OFFSETS:
                keep.fill_(float('nan'))
                L.call('vv_keep_mask', L.ptr(keep), B, Lz, rate, seed, offset, _st())
                got = keep.cpu().numpy()
                assert np.array_equal(_bits(got), _bits(_host_mask(B, Lz, rate, seed, offset))), (rate, seed, offset)


def _mask_scale_inputs(B, Lz):
    rng = np.random.default_rng(1000 * B + Lz)
    x = rng.standard_normal((B, Lz)).astype(np.float32)
    special = np.array([0.0, -0.0, 1e-40, -1e-40, 3e38, -3e38, 1e30, -1e30], dtype=np.float32)      # +-0, a denormal, +-large
    flat = x.reshape(-1)
    flat[:min(flat.size, special.size)] = special[:flat.size]
    keep = (rng.random((B, Lz)) >= 0.35).astype(np.float32)
    keep.reshape(-1)[:8:2] = 1.0                                      # the special values meet a kept and a dropped element
    return x, keep


@pytest.mark.parametrize('B,Lz', [(1, 1), (3, 5), (5, 64), (256, 64), (7, 321)])
@pytest.mark.parametrize('scale', [1.0, 1.0 / (1.0 - 0.35), 1.0 / (1.0 - 0.999)])
def test_mask_scale_equals_numpy_float32_as_bits(B, Lz, scale):
    from voxvae import lib as L
    x, keep = _mask_scale_inputs(B, Lz)
    with np.errstate(over='ignore'):
        want = (x * keep) * np.float32(scale)
    assert want.dtype == np.float32
    xd, kd = torch.from_numpy(x).to(DEV), torch.from_numpy(keep).to(DEV)
    y = torch.full((B, Lz), float('nan'), dtype=torch.float32, device=DEV)
    L.call('vv_mask_scale', L.ptr(xd), L.ptr(kd), scale, L.ptr(y), B, Lz, _st())
    got = y.cpu().numpy()
    assert np.array_equal(_bits(got), _bits(want)), np.flatnonzero(_bits(got) != _bits(want))[:8]


def test_both_launching_entries_keep_inside_their_buffers():
    """Inputs between NaN guards, outputs pre-poisoned inside sentinel guards: nothing outside the payload is written, no input is
    touched, every output element is written, and the result is the plain run's."""
    from voxvae import lib as L
    B, Lz, rate, seed, offset = 257, 63, 0.35, 2 ** 63 + 5, 2 ** 56 + 7
    a = G.Arena('cuda')
    out = a.output((B, Lz), torch.float32, 'keep')
    a.commit()
    L.call('vv_keep_mask', out.ptr, B, Lz, rate, seed, offset, _st())
    torch.cuda.synchronize()
    a.check()
    plain = torch.empty(B, Lz, dtype=torch.float32, device=DEV)
    L.call('vv_keep_mask', L.ptr(plain), B, Lz, rate, seed, offset, _st())
    assert torch.equal(out.tensor.view(torch.int32), plain.view(torch.int32))

    B, Lz, scale = 7, 321, 1.0 / (1.0 - 0.35)
    x, keep = _mask_scale_inputs(B, Lz)
    a = G.Arena('cuda')
    bx, bk = a.input(torch.from_numpy(x), 'x'), a.input(torch.from_numpy(keep), 'keep')
    by = a.output((B, Lz), torch.float32, 'y')
    a.commit()
    L.call('vv_mask_scale', bx.ptr, bk.ptr, scale, by.ptr, B, Lz, _st())
    torch.cuda.synchronize()
    a.check()
    xd, kd = torch.from_numpy(x).to(DEV), torch.from_numpy(keep).to(DEV)
    plain = torch.empty(B, Lz, dtype=torch.float32, device=DEV)
    L.call('vv_mask_scale', L.ptr(xd), L.ptr(kd), scale, L.ptr(plain), B, Lz, _st())
    assert not bool(torch.isnan(by.tensor).any())
    assert torch.equal(by.tensor.view(torch.int32), plain.view(torch.int32))


def test_keepmasks_on_the_device_equal_their_host_twin():
    from voxvae import masks as M
    km = M.KeepMasks(DEV, seed=5, rank=0)
    for step in range(4):
        assert np.array_equal(_bits(km.dropout(5, 64, 0.35).cpu().numpy()), _bits(km.host('dropout', 5, 64, 0.35, step))), step
        assert np.array_equal(_bits(km.missing(3, 5, 0.5).cpu().numpy()), _bits(km.host('missing', 3, 5, 0.5, step))), step
    assert km.steps == {'dropout': 4, 'missing': 4}
    r0, r1 = M.KeepMasks(DEV, seed=5, rank=0), M.KeepMasks(DEV, seed=5, rank=1)
    m0, m1 = r0.dropout(256, 64, 0.5), r1.dropout(256, 64, 0.5)
    agree = float((m0 == m1).float().mean())
    assert not torch.equal(m0, m1) and 0.45 <= agree <= 0.55, agree


def test_getEval_with_a_device_mask_is_reproduced_by_injecting_the_host_twin(device_masks):
    import voxvae
    from voxvae import synthetic as syn
    voxvae.set_default_dtype('f32')
    voxvae.set_default_device(DEV)
    device_masks.manual_seed(21)
    import src.module.nolbo as nolbo
    D, Lz, B = 16, 64, 5
    cfg = syn.make_config(D, Lz, True)
    model = nolbo.nolboSingleObject_modelnet_category_VAE(nolbo_structure=cfg)
    model._encoder.set_weights_dict(syn.make_encoder_params(cfg['encoder']))
    model._decoder.set_weights_dict(syn.make_decoder_params(cfg['decoder']))
    assert model._keep_masks is not None
    x, eps, eps2 = syn.make_voxels(B, D), syn.make_eps(B, Lz), syn.make_eps(B, Lz, seed=8)
    oh, cats = syn.make_onehot(B, 40), syn.make_category_vectors(40, Lz)
    drawn = model.getEval(inputs=(x, x, oh), category_vectors=cats, missing_prob=0.5, _eps=eps, _eps2=eps2)
    assert model._keep_masks.steps['missing'] == 1
    mask = model._keep_masks.host('missing', B, Lz, 0.5, 0)
    assert 0.3 < mask.mean() < 0.7
    injected = model.getEval(inputs=(x, x, oh), category_vectors=cats, missing_prob=0.5, _eps=eps, _mask=mask, _eps2=eps2)
    assert model._keep_masks.steps['missing'] == 1                    # an injected mask draws nothing
    assert len(drawn) == len(injected) == 10
    for i, (a, b) in enumerate(zip(drawn, injected)):
        assert np.array_equal(_bits(np.array(a)), _bits(np.array(b))), i
