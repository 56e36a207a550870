"""Exact GPU tests of every stride-2 convolution / transposed-convolution forward entry: inputs on which each output element receives at
most one non-zero product (tests/_exact_inputs.py), an epilogue of exact operations (scale +-2^k, shift 0 or a value of the output
type, no activation or ReLU).  The result is then independent of summation order, MFMA shape and split-K, and must EQUAL the float64
oracle on the same inputs -- every element, no tolerance (tests/_tol.check_exact).  A dropped, duplicated or misplaced tap, a padding,
sample-index or per-channel-scale error shows as an inequality; outputs are pre-filled with NaN, so does an unwritten element.

  selector   one non-zero weight per output channel (conv) / per output channel and parity class (transposed conv), dense random x
  impulse    one non-zero voxel and channel per sample (8 corners, an edge, a face, the interior; the last sample always), dense w
  zero       x = 0, shift non-zero: the output is act(shift_c)

Each entry runs at the smallest shape of the existing parameter lists that reaches its code; kernel forms are chosen with
monkeypatch.setenv as in tests/test_gpu_ops.py, launches go through tests/_layer_calls.py."""
from collections import namedtuple

import numpy as np
import pytest
import torch

import _exact_inputs as XI
import _layer_calls as LC
import _tol as T
from oracle import numpy_oracle as no

pytestmark = pytest.mark.gpu

OP = {'conv': no.conv3d_same, 'convT': no.conv3d_transpose_same}


@pytest.fixture(scope='module')
def L():
    from voxvae import lib
    lib.load()
    assert torch.cuda.is_available()
    return lib


# op: operand type; out: type of the stored output; env: kernel-form overrides; run(L, c, xd, wd, scd, shd, act) -> output tensor
Case = namedtuple('Case', 'id kind B side cin cout op out env run epilogue xf32 families')


def _case(id, kind, B, side, cin, cout, op, out, run, env=None, epilogue=True, xf32=False, families=('selector', 'impulse', 'zero')):
    return Case(id, kind, B, side, cin, cout, op, out, env or {}, run, epilogue, xf32, families)


def _igemm_conv(L, c, xd, wd, scd, shd, act):
    wp = LC.pack_conv_k4(L, wd, c.cin, c.cout, c.op)
    return LC.conv3d_k4s2(L, xd, wp, scd, shd, c.B, c.side, c.cin, c.cout, act, c.op, c.out if c.op == 'fp8' else None)


def _igemm_convT(L, c, xd, wd, scd, shd, act):
    wp = LC.pack_convT_k4s2(L, wd, c.cin, c.cout, c.op)
    return LC.convT3d_k4s2(L, xd, wp, scd, shd, c.B, c.side, c.cin, c.cout, act, c.op, c.out if c.op == 'fp8' else None)


def _skip_conv(L, c, xd, wd, scd, shd, act):
    assert L.load().vv_conv3d_k4s2_skip_supported(8, c.cin, c.cout, L.VV_BF16)
    return LC.conv3d_k4s2_skip(L, xd, LC.pack_conv_k4_skip(L, wd, c.cin, c.cout), scd, shd, c.B, c.cin, c.cout, act)


def _skip_convT(L, c, xd, wd, scd, shd, act):
    assert L.load().vv_convT3d_k4s2_skip_supported(4, c.cin, c.cout, L.VV_BF16)
    return LC.convT3d_k4s2_skip(L, xd, LC.pack_convT_k4s2_skip(L, wd, c.cin, c.cout), scd, shd, c.B, c.cin, c.cout, act)


def _pos_conv(L, c, xd, wd, scd, shd, act):
    return LC.conv3d_k4s2_pos(L, xd, LC.pack_conv_k4_skip(L, wd, c.cin, c.cout), scd, shd, c.B, c.cin, c.cout, act)


def _pos_convT(L, c, xd, wd, scd, shd, act):
    return LC.convT3d_k4s2_pos(L, xd, LC.pack_convT_k4s2_skip(L, wd, c.cin, c.cout), scd, shd, c.B, c.cin, c.cout, act)


def _whole(L, c, xd, wd, scd, shd, act):
    return LC.convT3d_k4s2_whole(L, xd, LC.pack_convT_k4s2_skip(L, wd, c.cin, c.cout), scd, shd, c.B, act)


def _direct_conv(L, c, xd, wd, scd, shd, act):
    return LC.conv3d_k4s2_direct(L, xd, LC.pack_conv_k4(L, wd, c.cin, c.cout, 'bf16'), scd, shd, c.B, c.side, act)


def _direct_convT(L, c, xd, wd, scd, shd, act):
    return LC.convT3d_k4s2_direct(L, xd, LC.pack_convT_k4s2_frag(L, wd, c.cin, c.cout), scd, shd, c.B, c.side, act)


def _direct_conv_fp8(L, c, xd, wd, scd, shd, act):
    return LC.conv3d_k4s2_direct_fp8(L, xd, LC.pack_conv_k4(L, wd, c.cin, c.cout, 'fp8'), scd, shd, c.B, c.side, act, c.out)


def _direct_convT_fp8(L, c, xd, wd, scd, shd, act):
    return LC.convT3d_k4s2_direct_fp8(L, xd, LC.pack_convT_k4s2_frag_fp8(L, wd, c.cin, c.cout), scd, shd, c.B, c.side, act, c.out)


def _first(L, c, xd, wd, scd, shd, act):
    return LC.conv3d_first(L, xd, LC.pack_conv_k4(L, wd, 1, 64, c.op), scd, shd, c.B, c.side, act, c.op)


def _final_logits(L, c, xd, wd, scd, shd, act):
    D = 2 * c.side
    yd = torch.zeros(c.B, D, D, D, 1, dtype=torch.float32, device=LC.DEV)
    return LC.convT3d_final_bce(L, xd, wd, yd, c.B, c.side, c.op)[1]


CASES = [_case('igemm_conv-%s-%d-%d-%d-%d' % ((dt,) + s), 'conv', *s, dt, dt, _igemm_conv)
         for dt in ('f32', 'bf16') for s in ((3, 4, 128, 64), (32, 4, 128, 64), (5, 2, 256, 512))]      # B >= 32: position-major rows; last: split-K
CASES += [_case('igemm_convT-%s-%d-%d-%d-%d' % ((dt,) + s), 'convT', *s, dt, dt, _igemm_convT)
          for dt in ('f32', 'bf16') for s in ((2, 4, 128, 64), (33, 2, 64, 128), (3, 2, 512, 256))]
CASES += [
    # fp8 operands: conv with Cin 64 (tap-pair rows) and 128; the transposed conv admits multiples of 128 only
    _case('igemm_conv-fp8-cin64-bf16out', 'conv', 3, 8, 64, 128, 'fp8', 'bf16', _igemm_conv),
    _case('igemm_conv-fp8-cin128-fp8out', 'conv', 2, 8, 128, 256, 'fp8', 'fp8', _igemm_conv),
    _case('igemm_convT-fp8-cin128-bf16out', 'convT', 3, 8, 128, 64, 'fp8', 'bf16', _igemm_convT),
    _case('igemm_convT-fp8-cin256-fp8out', 'convT', 2, 4, 256, 128, 'fp8', 'fp8', _igemm_convT),
    _case('skip_conv-B5', 'conv', 5, 8, 64, 64, 'bf16', 'bf16', _skip_conv),                             # ragged last quad
    _case('skip_convT-B9', 'convT', 9, 4, 64, 128, 'bf16', 'bf16', _skip_convT),
    _case('pos_conv-B33', 'conv', 33, 4, 64, 64, 'bf16', 'bf16', _pos_conv),
    _case('pos_convT-B33', 'convT', 33, 2, 64, 64, 'bf16', 'bf16', _pos_convT),
]
CASES += [_case('whole-shape%d-ps%d' % (sh, ps), 'convT', 3, 8, 128, 64, 'bf16', 'bf16', _whole,
                dict(VV_CTW_SHAPE=str(sh), **({'VV_CTW_PS': str(ps)} if ps else {}))) for sh in (16, 32, 4) for ps in (0, 4)]
CASES += [_case('direct_conv-shape%d' % sh, 'conv', 2, 16, 64, 128, 'bf16', 'bf16', _direct_conv, {'VV_CD_SHAPE': str(sh)}) for sh in (16, 32, 8)]
CASES += [_case('direct_convT-mt%s' % v, 'convT', 2, 8, 128, 64, 'bf16', 'bf16', _direct_convT, {'VV_DIRECT_MT': v}) for v in ('8', '4', '2')]
CASES += [
    _case('direct_conv_fp8-bf16out', 'conv', 1, 16, 64, 128, 'fp8', 'bf16', _direct_conv_fp8),
    _case('direct_conv_fp8-fp8out', 'conv', 1, 16, 64, 128, 'fp8', 'fp8', _direct_conv_fp8),
    _case('direct_convT_fp8-bf16out', 'convT', 1, 8, 128, 64, 'fp8', 'bf16', _direct_convT_fp8),
    _case('direct_convT_fp8-fp8out', 'convT', 1, 8, 128, 64, 'fp8', 'fp8', _direct_convT_fp8),
    _case('first-plane-D32', 'conv', 2, 32, 1, 64, 'bf16', 'bf16', _first, xf32=True),
    # 70 samples are the fewest that chain (1,120 plane items over 1,024 persistent workgroups) and cost the float64 oracle seconds per
    # call: the chained kernel gets the family that exercises every tap on dense data; impulses and zeros go through the plane form
    _case('first-chained-B70', 'conv', 70, 32, 1, 64, 'bf16', 'bf16', _first, xf32=True, families=('selector',)),
    _case('final_logits-box', 'convT', 2, 8, 64, 1, 'bf16', 'f32', _final_logits, {'VV_FINAL_BCE': 'box'}, epilogue=False),
    _case('final_logits-sweep', 'convT', 2, 8, 64, 1, 'bf16', 'f32', _final_logits, {'VV_FINAL_BCE': 'sweep'}, epilogue=False),
    _case('direct_conv-chunked', 'conv', 5, 16, 64, 128, 'bf16', 'bf16', _direct_conv, {'VV_CHUNK_SAMPLES': '2'}),
]


def _family(name):
    cs = [c for c in CASES if name in c.families]
    return pytest.mark.parametrize('c', cs, ids=[c.id for c in cs])


def _fp8(c):
    return c.op == 'fp8' or c.out == 'fp8'


def _shapes(c):
    x = (c.B, c.side, c.side, c.side, c.cin)
    return x, ((4, 4, 4, c.cin, c.cout) if c.kind == 'conv' else (4, 4, 4, c.cout, c.cin))


def _launch_and_check(L, c, x, w, scale, shift, act, what):
    """One launch of the entry on (x, w) against the float64 oracle on the same arrays, exactly."""
    conv = OP[c.kind](x.astype(np.float64), w.astype(np.float64), 2)
    if c.epilogue:
        ref = conv * scale + shift
        ref = np.maximum(ref, 0) if act == 2 else ref
    else:
        ref, act = conv, 0
    xd = LC.dev(x, torch.float32 if c.xf32 else LC.TDT[c.op])
    wd = LC.dev(w)
    scd, shd = (LC.dev(scale), LC.dev(shift)) if c.epilogue else (None, None)
    y = c.run(L, c, xd, wd, scd, shd, act)
    T.check_exact(y, ref, '%s %s' % (c.id, what))
    return ref


F8_MISSING = LC.F8 is None


def _setenv(c, monkeypatch):
    if F8_MISSING and _fp8(c):
        pytest.skip('torch.float8_e4m3fn not available')
    for v in ('VV_CTW_PS', 'VV_CTW_SHAPE', 'VV_CD_SHAPE', 'VV_DIRECT_MT', 'VV_FINAL_BCE', 'VV_CHUNK_SAMPLES'):
        monkeypatch.delenv(v, raising=False)
    for k, v in c.env.items():
        monkeypatch.setenv(k, v)


@_family('selector')
def test_selector_weights(L, c, monkeypatch):
    """Dense random x, selector weights (all 64 taps over the launches): every output is one x value times its channel's scale, or 0."""
    _setenv(c, monkeypatch)
    rng = np.random.default_rng(len(c.id) + c.B)
    xs, _ = _shapes(c)
    x = XI.grid_values(rng, xs, _fp8(c))
    scale, shift = XI.exact_scale(c.cout), np.zeros(c.cout, np.float32)
    sel, n = ((XI.selector_conv_weights, XI.selector_conv_launches(c.cout)) if c.kind == 'conv'
              else (XI.selector_convT_weights, XI.selector_convT_launches(c.cout)))
    for l in range(n):
        ref = _launch_and_check(L, c, x, sel(c.cin, c.cout, l), scale, shift, 0, 'selector launch %d' % l)
        assert (ref != 0).any()


@_family('impulse')
def test_impulse_input(L, c, monkeypatch):
    """One impulse per sample, dense random w: the output is a slice of the weights times the channel's scale and exactly zero elsewhere
    (launches alternate between no activation and ReLU)."""
    _setenv(c, monkeypatch)
    rng = np.random.default_rng(len(c.id) + c.cin)
    _, ws = _shapes(c)
    w = XI.grid_values(rng, ws, _fp8(c))
    scale, shift = XI.exact_scale(c.cout), np.zeros(c.cout, np.float32)
    for l in range(XI.impulse_launches(c.B)):
        ref = _launch_and_check(L, c, XI.impulse_input(c.B, c.side, c.cin, l), w, scale, shift, 2 * (l % 2), 'impulse launch %d' % l)
        assert (ref[-1] != 0).any()


@_family('zero')
def test_zero_input(L, c, monkeypatch):
    """x = 0, dense w, shift a non-zero value of the output type: the output is act(shift_c) (0 for the last layer's logits)."""
    _setenv(c, monkeypatch)
    rng = np.random.default_rng(len(c.id))
    xs, ws = _shapes(c)
    w = XI.grid_values(rng, ws, _fp8(c))
    scale, shift = XI.exact_scale(c.cout), XI.grid_values(rng, (c.cout,), _fp8(c))
    for act in ((2, 0) if c.epilogue else (0,)):
        _launch_and_check(L, c, np.zeros(xs, np.float32), w, scale, shift, act, 'zero input act %d' % act)
