"""The folded form of the 4^3 <-> 2^3 position GEMMs (posgemm.hip, pg_kernel<MODE, true>; VV_SCHED_THROUGHPUT of the *_ex entries): one
workgroup walks all K shares of its output position and adds them up in registers.  It must give the bytes of the split-K form
(pg_kernel<MODE, false> + pg_reduce_kernel, the plain entries) -- same float32 sums in the same order -- so every comparison between the
forms here is `torch.equal` on the raw bits; the split form's result is also held to the float64 numpy definition at the tolerances of
tests/test_gpu_ops.py (its own helpers), once per case.

Cases.  A position is cut into shares only when it has more than 8 chunks of 64 input channels, so the transposed layer needs cin >= 128
to have anything to fold.  conv (27 taps per position): (5, 64, 64) 4 shares, a ragged single sample tile, half a channel tile;
(300, 64, 128) two sample tiles, the second ragged; (20, 128, 136) cout % 8 with a ragged second channel tile; (20, 256, 512) the 32^3
model's layer, 7 shares.  convT (1 .. 8 taps): the same four with cin 128 / the model's (512, 256): positions of 1, 2 and 4 shares in
one launch.  Activations ELU and none."""
import ctypes

import numpy as np
import pytest
import torch

import _guarded as G
import _layer_calls as LC
import test_gpu_ops as O
from oracle import numpy_oracle as no

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
BT = torch.bfloat16

CONV_CASES = [(5, 64, 64), (300, 64, 128), (20, 128, 136), (20, 256, 512)]
CONVT_CASES = [(5, 128, 64), (300, 128, 128), (20, 128, 136), (20, 512, 256)]
LAYER_CASES = [('conv',) + c for c in CONV_CASES] + [('convT',) + c for c in CONVT_CASES]


@pytest.fixture(scope='module')
def L():
    from voxvae import lib
    lib.load()
    assert torch.cuda.is_available()
    return lib


def _bits(t):
    return t.contiguous().view(torch.uint8 if t.element_size() == 1 else torch.int16 if t.element_size() == 2 else torch.int32)


_LAYER = {}


def _layer(L, mode, B, cin, cout):
    """Inputs, packed weights and the float64 pre-activation of one case, computed once and shared (never written to)."""
    key = (mode, B, cin, cout)
    if key not in _LAYER:
        rng = np.random.default_rng(B * 13 + cin + (7 if mode == 'convT' else 0))
        side, taps = (4, 27) if mode == 'conv' else (2, 4)
        x = O._bf16_round(rng.standard_normal((B, side, side, side, cin)).astype(np.float32))
        wshape = (4, 4, 4, cin, cout) if mode == 'conv' else (4, 4, 4, cout, cin)
        w = O._bf16_round((rng.standard_normal(wshape) / np.sqrt(taps * cin)).astype(np.float32))
        scale = rng.uniform(0.5, 1.5, cout).astype(np.float32)
        shift = rng.normal(0, 0.3, cout).astype(np.float32)
        if mode == 'conv':
            conv = no.conv3d_same(x.astype(np.float64), w.astype(np.float64), 2)
            wp = LC.pack_conv_k4_skip(L, LC.dev(w), cin, cout)
        else:
            conv = no.conv3d_transpose_same(x.astype(np.float64), w.astype(np.float64), 2)
            wp = LC.pack_convT_k4s2_skip(L, LC.dev(w), cin, cout)
        _LAYER[key] = dict(conv=conv, scale=scale, shift=shift, xd=LC.dev(x, BT), wp=wp, scd=LC.dev(scale), shd=LC.dev(shift))
    return _LAYER[key]


def _entry(mode):
    return 'vv_conv3d_k4s2_pos' if mode == 'conv' else 'vv_convT3d_k4s2_pos'


def _out_shape(mode, B, cout):
    return (B, 2, 2, 2, cout) if mode == 'conv' else (B, 4, 4, 4, cout)


def _run_ex(L, mode, c, B, cin, cout, act, schedule, ws=None):
    lib = L.load()
    if ws is None:
        ws = torch.empty(max(getattr(lib, _entry(mode) + '_workspace_bytes')(B, cin, cout), 16), dtype=torch.uint8, device=DEV)
    y = LC.nan_out(_out_shape(mode, B, cout), BT)
    L.call(_entry(mode) + '_fwd_ex', L.ptr(c['xd']), L.ptr(c['wp']), L.ptr(c['scd']), L.ptr(c['shd']), L.ptr(y), B, 4 if mode == 'conv' else 2,
           cin, cout, act, schedule, L.ptr(ws), ws.numel(), LC.st())
    torch.cuda.synchronize()
    return y


@pytest.mark.parametrize('act', [1, 0])
@pytest.mark.parametrize('mode,B,cin,cout', LAYER_CASES)
def test_folded_form_gives_the_bytes_of_the_split_form(L, mode, B, cin, cout, act):
    c = _layer(L, mode, B, cin, cout)
    plain = (LC.conv3d_k4s2_pos if mode == 'conv' else LC.convT3d_k4s2_pos)(L, c['xd'], c['wp'], c['scd'], c['shd'], B, cin, cout, act)
    pre, ref = O._epilogue(c['conv'], c['scale'], c['shift'], act)
    O._check(plain, ref, 'bf16', _entry(mode) + '_fwd', pre)                      # the split form against float64
    split = _run_ex(L, mode, c, B, cin, cout, act, L.VV_SCHED_LATENCY)
    fold = _run_ex(L, mode, c, B, cin, cout, act, L.VV_SCHED_THROUGHPUT)
    assert not torch.isnan(fold.float()).any()
    assert torch.equal(_bits(split), _bits(plain))
    assert torch.equal(_bits(fold), _bits(plain)), '%d of %d elements differ' % ((_bits(fold) != _bits(plain)).sum().item(), plain.numel())
    O._check(fold, ref, 'bf16', _entry(mode) + '_fwd_ex folded', pre)             # ... and the folded form on its own


def test_schedule_codes_outside_the_enum_are_refused(L):
    c = _layer(L, 'conv', 5, 64, 64)
    lib = L.load()
    ws = torch.empty(lib.vv_conv3d_k4s2_pos_workspace_bytes(5, 64, 64), dtype=torch.uint8, device=DEV)
    y = LC.nan_out((5, 2, 2, 2, 64), BT)
    for name, side in (('vv_conv3d_k4s2_pos_fwd_ex', 4), ('vv_convT3d_k4s2_pos_fwd_ex', 2)):
        for code in (-1, 2, 7):
            assert getattr(lib, name)(L.ptr(c['xd']), L.ptr(c['wp']), None, None, L.ptr(y), 5, side, 64, 64, 0, code, L.ptr(ws), ws.numel(), LC.st()) == -2
    torch.cuda.synchronize()
    assert torch.isnan(y.float()).all()                                          # nothing was launched


# ------------------------------------------------------------------------------------------------ guard bands, workspace independence
def _guarded_layer(L, mode, c, B, cin, cout, act, schedule, fill, short=0, extra=0):
    """One *_ex call on guard-banded buffers (tests/_guarded.Arena): the workspace is what the query returns, pre-filled with `fill`,
    plus `extra` announced bytes, minus `short` announced bytes.  -> (status, output tensor)."""
    lib = L.load()
    need = getattr(lib, _entry(mode) + '_workspace_bytes')(B, cin, cout)
    assert need > 0
    a = G.Arena(DEV)
    x, w = a.input(c['xd'], 'x'), a.input(c['wp'], 'w_skip')
    sc, sh = a.input(c['scd'], 'scale'), a.input(c['shd'], 'shift')
    y = a.output(_out_shape(mode, B, cout), BT, 'y')
    ws = a.workspace(need, fill, extra=extra)
    a.commit()
    rc = getattr(lib, _entry(mode) + '_fwd_ex')(x.ptr, w.ptr, sc.ptr, sh.ptr, y.ptr, B, 4 if mode == 'conv' else 2, cin, cout, act, schedule,
                                                ws.ptr, need + extra - short, LC.st())
    torch.cuda.synchronize()
    a.check()
    return rc, y.tensor.clone()


@pytest.mark.parametrize('mode,B,cin,cout', [('conv', 5, 64, 64), ('conv', 300, 64, 128), ('conv', 20, 128, 136),
                                             ('convT', 5, 128, 64), ('convT', 300, 128, 128), ('convT', 20, 128, 136)])
def test_layer_entries_stay_inside_their_buffers_and_ignore_the_workspace_contents(L, mode, B, cin, cout, act=1):
    c = _layer(L, mode, B, cin, cout)
    plain = (LC.conv3d_k4s2_pos if mode == 'conv' else LC.convT3d_k4s2_pos)(L, c['xd'], c['wp'], c['scd'], c['shd'], B, cin, cout, act)
    for schedule in (L.VV_SCHED_THROUGHPUT, L.VV_SCHED_LATENCY):
        for fill, extra in ((0x00, 0), (0xFF, 0), (0xFF, 4096)):               # 0xFF: a slab element read before it is written is a NaN
            rc, y = _guarded_layer(L, mode, c, B, cin, cout, act, schedule, fill, extra=extra)
            assert rc == 0
            assert torch.equal(_bits(y), _bits(plain)), (schedule, fill, extra)
        rc, y = _guarded_layer(L, mode, c, B, cin, cout, act, schedule, 0x00, short=1)
        assert rc == G.VV_ERR_WORKSPACE and torch.isnan(y.float()).all()         # one byte short: refused, nothing launched, for either form


# ------------------------------------------------------------------------------------------------ the fused E4 + latent tail entry
def _tail_case(L, B, cin, cout, Lz):
    rng = np.random.default_rng(B * 7 + cin)
    E, K5, lin, n1 = 2 * Lz, 8 * cout, 64, 4096
    assert L.load().vv_conv_pos_latent_tail_supported(cin, cout, E, Lz, lin, n1, 1, L.VV_BF16)
    r = O._bf16_round
    w4 = r((rng.standard_normal((4, 4, 4, cin, cout)) / np.sqrt(27 * cin)).astype(np.float32))
    t = dict(x=LC.dev(r(rng.standard_normal((B, 4, 4, 4, cin)).astype(np.float32)), BT), wp=LC.pack_conv_k4_skip(L, LC.dev(w4), cin, cout),
             sc4=LC.dev(rng.uniform(0.5, 1.5, cout)), sh4=LC.dev(rng.normal(0, 0.3, cout)),
             w5=LC.dev(r((rng.standard_normal((E, K5)) / np.sqrt(K5)).astype(np.float32) * 3), BT), eps=LC.dev(rng.standard_normal((B, Lz))),
             wd=LC.dev(r((rng.standard_normal((lin, Lz)) / np.sqrt(Lz)).astype(np.float32)), BT), scd=LC.dev(rng.uniform(0.5, 1.5, lin)),
             shd=LC.dev(rng.normal(0, 0.3, lin)), w1=LC.dev(r((rng.standard_normal((n1, lin)) / np.sqrt(lin)).astype(np.float32)), BT),
             sc1=LC.dev(rng.uniform(0.5, 1.5, n1)), sh1=LC.dev(rng.normal(0, 0.3, n1)))
    return t, (E, lin, n1)


_TAIL_IN = ('x', 'wp', 'sc4', 'sh4', 'w5', 'eps', 'wd', 'scd', 'shd', 'w1', 'sc1', 'sh1')


def _tail_run(L, t, B, cin, cout, Lz, dims, schedule, fill, plain=False):
    """vv_conv_pos_latent_tail_fwd (plain) or _fwd_ex(schedule) on guard-banded buffers -> the five outputs."""
    E, lin, n1 = dims
    lib = L.load()
    need = lib.vv_conv_pos_latent_tail_workspace_bytes(B, cin, cout, E)
    assert need > 0
    a = G.Arena(DEV)
    i = {k: a.input(t[k], k) for k in _TAIL_IN}
    o = dict(enc_out=a.output((B, E), torch.float32, 'enc_out'), z=a.output((B, Lz), torch.float32, 'z'), z_act=a.output((B, Lz), BT, 'z_act'),
             kl=a.output((B,), torch.float32, 'kl'), h1=a.output((B, n1), BT, 'h1'))
    ws = a.workspace(need, fill)
    a.commit()
    head = (i['x'].ptr, i['wp'].ptr, i['sc4'].ptr, i['sh4'].ptr, cin, cout, i['w5'].ptr, None, i['eps'].ptr, i['wd'].ptr, i['scd'].ptr, i['shd'].ptr,
            i['w1'].ptr, i['sc1'].ptr, i['sh1'].ptr, o['enc_out'].ptr, o['z'].ptr, o['z_act'].ptr, o['kl'].ptr, o['h1'].ptr, B, E, Lz, lin, n1, 1, 1)
    if plain:
        rc = lib.vv_conv_pos_latent_tail_fwd(*head, L.VV_BF16, ws.ptr, need, LC.st())
    else:
        rc = lib.vv_conv_pos_latent_tail_fwd_ex(*head, schedule, ws.ptr, need, LC.st())
    torch.cuda.synchronize()
    assert rc == 0
    a.check()
    return {k: b.tensor.clone() for k, b in o.items()}


@pytest.mark.parametrize('B,cin,cout,Lz', [(5, 64, 256, 64), (40, 256, 512, 64)])
def test_fused_tail_entry_folded_against_split(L, B, cin, cout, Lz):
    """Every output of the fused entry, byte for byte; the split form itself is held to the float64 definition by
    tests/test_gpu_ops.py::test_conv_pos_latent_tail_fused."""
    t, dims = _tail_case(L, B, cin, cout, Lz)
    want = _tail_run(L, t, B, cin, cout, Lz, dims, None, 0x00, plain=True)
    assert not any(torch.isnan(v.float()).any() for v in want.values())
    for schedule in (L.VV_SCHED_THROUGHPUT, L.VV_SCHED_LATENCY):
        for fill in (0x00, 0xFF):
            got = _tail_run(L, t, B, cin, cout, Lz, dims, schedule, fill)
            for k in want:
                assert torch.equal(_bits(got[k]), _bits(want[k])), (k, schedule, fill)


# ------------------------------------------------------------------------------------------------ end to end
def test_streamed_submit_is_the_direct_call_bit_for_bit(monkeypatch):
    """StreamedEvaluator(streams=3).submit asks for the folded form, model.eval_forward_device keeps the latency plan: the same bytes in
    pred, stats, metrics and kl at batch 8, on every one of the three streams."""
    import contextlib
    import sys
    import voxvae
    from voxvae import lib as L
    from voxvae import synthetic as syn
    from voxvae.streams import StreamedEvaluator
    voxvae.set_default_dtype('bf16')
    voxvae.set_default_device(DEV)
    import src.module.nolbo as nolbo
    cfg = syn.make_config(32, 64, True)
    ep, dp = syn.make_encoder_params(cfg['encoder']), syn.make_decoder_params(cfg['decoder'])

    def build():
        with contextlib.redirect_stdout(sys.stderr):
            m = nolbo.nolboSingleObject_modelnet_category_VAE(nolbo_structure=cfg)
        m._encoder.set_weights_dict(ep)
        m._decoder.set_weights_dict(dp)
        return m

    names, call = [], L.call
    monkeypatch.setattr(L, 'call', lambda fn, *a: (names.append(fn), call(fn, *a))[1])
    ev = StreamedEvaluator(build, streams=3, device=DEV)
    B = 8
    x = torch.from_numpy(syn.make_voxels(B, 32, seed=11)).to(DEV)
    eps = torch.from_numpy(syn.make_eps(B, 64, seed=3)).to(DEV)
    want = ev.models[0].eval_forward_device(x, x, eps)
    torch.cuda.synchronize()
    direct = [n for n in names if 'pos' in n and n.endswith(('_fwd', '_fwd_ex'))]
    assert direct and not any(n.endswith('_ex') for n in direct), direct        # the latency plan, through the plain entries
    del names[:]
    outs = [ev.submit(x, x, eps) for _ in range(3)]
    ev.synchronize()
    streamed = [n for n in names if 'pos' in n and n.endswith(('_fwd', '_fwd_ex'))]
    assert len(streamed) == 3 * len(direct) and all(n.endswith('_ex') for n in streamed), streamed
    assert all(e.schedule == L.VV_SCHED_LATENCY for m in ev.models for e in (m._enc_eng, m._dec_eng))   # restored after every submit
    for got in outs:
        for g, w, what in zip(got, want, ('pred', 'stats', 'metrics', 'kl')):
            assert torch.equal(_bits(g), _bits(w)), what
