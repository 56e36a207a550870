"""GPU tests of the 2D convolution and the 2x2 SAME max-pool (csrc/conv2d.hip) against the float64 definition of
tests/_conv2d_ref.py.  Selector cases are exact; random cases meet tests/_tol.check_one_rounding on every element; the contract checks
(same bits twice, side stream, workspace, guard bands) run on the ragged shapes.  Which form ran -- one launch or split-K slabs -- is
read from vv_conv2d_splits and forced through the VV_C2_SPLITS hook where a small shape has to reach the other one."""
import ctypes

import numpy as np
import pytest
import torch

import _conv2d_ref as R
import _guarded as G
import _tol

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
DT = {'f32': 0, 'bf16': 1}
TT = {'f32': torch.float32, 'bf16': torch.bfloat16}
ACT = {None: 0, 'elu': 1, 'relu': 2, 'lrelu': 3}


@pytest.fixture(scope='module')
def L():
    import voxvae
    from voxvae import lib
    lib.load()
    assert torch.cuda.is_available()
    voxvae.set_default_device(DEV)
    return lib


def _stream_ptr(st=None):
    st = st if st is not None else torch.cuda.current_stream(DEV)
    return ctypes.c_void_p(st.cuda_stream)


def pack(L, wk, dt):
    k, _, cin, cout = wk.shape
    w = torch.from_numpy(np.ascontiguousarray(wk, dtype=np.float32)).to(DEV)
    packed = torch.empty(L.load().vv_conv2d_packed_bytes(k, cin, cout, DT[dt]), dtype=torch.uint8, device=DEV)
    L.call('vv_pack_conv2d', L.ptr(w), L.ptr(packed), k, cin, cout, DT[dt], _stream_ptr())
    return packed


def device_input(x, dt):
    """The bytes the entry reads: the float32 image for cin = 3, else the operand type."""
    t = torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).to(DEV)
    return t if x.shape[-1] == 3 else t.to(TT[dt])


def conv(L, x, wk, scale=None, shift=None, act=None, alpha=0.0, dt='f32', odt=None, stream=None, extra_ws=0):
    odt = odt or dt
    B, Rr, C, cin = x.shape
    k, cout = wk.shape[0], wk.shape[3]
    xd, packed = device_input(x, dt), pack(L, wk, dt)
    sc = None if scale is None else torch.from_numpy(np.asarray(scale, dtype=np.float32)).to(DEV)
    sh = None if shift is None else torch.from_numpy(np.asarray(shift, dtype=np.float32)).to(DEV)
    need = L.load().vv_conv2d_workspace_bytes(B, Rr, C, k, cin, cout, DT[dt])
    ws = torch.full((need + extra_ws + 16,), 0xA5, dtype=torch.uint8, device=DEV)
    y = torch.empty(B, Rr, C, cout, dtype=TT[odt], device=DEV)
    torch.cuda.synchronize()
    st = stream if stream is not None else torch.cuda.current_stream(DEV)
    with torch.cuda.stream(st):
        L.call('vv_conv2d_fwd', L.ptr(xd), L.ptr(packed), L.ptr(sc), L.ptr(sh), L.ptr(y), B, Rr, C, cin, cout, k, ACT[act], float(alpha), DT[dt], DT[odt],
               L.ptr(ws), need + extra_ws, _stream_ptr(st))
    st.synchronize()
    return y


def splits_of(L, x, wk):
    B, Rr, C, cin = x.shape
    return L.load().vv_conv2d_splits(B, Rr, C, wk.shape[0], cin, wk.shape[3])


def small_ints(rng, shape):
    return rng.integers(-4, 5, shape).astype(np.float32)


# ------------------------------------------------------------------------------------------------------------ exact selector cases
@pytest.mark.parametrize('force', [None, 1], ids=['default', 'direct'])
@pytest.mark.parametrize('grid', [(2, 5, 7), (1, 1, 1), (1, 1, 9)], ids=lambda g: 'x'.join(map(str, g)))
@pytest.mark.parametrize('cin', [3, 32, 64])
@pytest.mark.parametrize('k', [1, 3])
@pytest.mark.parametrize('dt', ['f32', 'bf16'])
def test_selector_kernels_are_exact(L, dt, k, cin, grid, force, monkeypatch):
    """One 1 in the kernel: every output is one input value or a zero from the padding.  A tap at column -1 reads a VALID address (the
    previous row's last pixel, or the previous image's), so a kernel that decides validity by address fails here."""
    if force is not None:                                # (cin = 3 has one form: the hook changes nothing there)
        monkeypatch.setenv('VV_C2_SPLITS', str(force))
    rng = np.random.default_rng(k * 100 + cin)
    B, Rr, C = grid
    x = small_ints(rng, (B, Rr, C, cin)) + 5.0          # no zero in the input: a zero in the output is a padded tap
    for tr in range(k):
        for tc in range(k):
            ci, co = int(rng.integers(cin)), int(rng.integers(32))
            y = conv(L, x, R.selector_kernel(k, cin, 32, tr, tc, ci, co), dt=dt)
            want = np.zeros((B, Rr, C, 32))
            want[..., co] = R.shifted(x, k, tr, tc, ci)
            _tol.check_exact(y, want, 'selector %s k%d cin%d tap (%d,%d) %s' % (dt, k, cin, tr, tc, grid))
    if force == 1:
        assert splits_of(L, x, R.selector_kernel(k, cin, 32, 0, 0, 0, 0)) == 1


# ------------------------------------------------------------------------------------------------------------ one rounding
CASES = [  # (B, R, C, cin, cout, k)
    (2, 6, 10, 3, 32, 3),
    (1, 13, 13, 32, 64, 3),
    (1, 13, 13, 32, 64, 1),
    (3, 13, 13, 64, 128, 3),
    (1, 13, 13, 128, 245, 1),
    (2, 6, 10, 256, 40, 3),
]
ACTS = [(None, 0.0), ('elu', 0.0), ('relu', 0.0), ('lrelu', 0.1), ('lrelu', 0.3)]


def random_case(case, seed=0):
    B, Rr, C, cin, cout, k = case
    rng = np.random.default_rng(seed + sum(case))
    x = rng.uniform(0, 1, (B, Rr, C, cin)).astype(np.float32) if cin == 3 else rng.standard_normal((B, Rr, C, cin)).astype(np.float32)
    wk = (rng.standard_normal((k, k, cin, cout)) / np.sqrt(k * k * cin)).astype(np.float32)
    scale = rng.uniform(0.5, 2.0, cout).astype(np.float32) * rng.choice([-1.0, 1.0], cout).astype(np.float32)
    shift = rng.uniform(-1, 1, cout).astype(np.float32)
    return x, wk, scale, shift


@pytest.mark.parametrize('force', [None, 1, 3], ids=['default', 'direct', 'split3'])
@pytest.mark.parametrize('case', CASES, ids=lambda c: '-'.join(map(str, c)))
@pytest.mark.parametrize('dt,odt', [('f32', 'f32'), ('bf16', 'bf16'), ('bf16', 'f32')])
def test_one_rounding(L, dt, odt, case, force, monkeypatch):
    x, wk, scale, shift = random_case(case)
    if force is not None:
        monkeypatch.setenv('VV_C2_SPLITS', str(force))
        want_splits = 1 if case[3] == 3 else min(force, -(-case[5] ** 2 * case[3] // 32))      # cin = 3 has one form
        assert splits_of(L, x, wk) == want_splits
    for act, alpha in ACTS:
        y = conv(L, x, wk, scale, shift, act, alpha, dt, odt)
        ref, pre = R.conv2d_ref(x, wk, scale, shift, act, alpha, dt)
        worst = _tol.check_one_rounding(y, ref, pre, odt, 'conv2d %s %s %s alpha %g' % (case, dt, act, alpha))
        print('conv2d %s %s->%s %s alpha %g splits %d: worst err / bound %.3f' % (case, dt, odt, act, alpha, splits_of(L, x, wk), worst))


def test_reference_matches_its_numpy_statement():
    x, wk, _, _ = random_case((2, 5, 7, 32, 8, 3))
    assert np.abs(R.conv2d_ref(x, wk)[0] - R.conv2d_direct(x, wk)).max() < 1e-12


@pytest.mark.parametrize('dt', ['f32', 'bf16'])
def test_head_layer_runs_split_k(L, dt):
    """The real head layer on one 13 x 13 frame: 169 rows against K = 9216.  It must take the split-K form, and meet the same bound."""
    case = (1, 13, 13, 1024, 1024, 3)
    x, wk, scale, shift = random_case(case)
    assert splits_of(L, x, wk) > 1
    assert L.load().vv_conv2d_workspace_bytes(1, 13, 13, 3, 1024, 1024, DT[dt]) == splits_of(L, x, wk) * 169 * 1024 * 4
    y = conv(L, x, wk, scale, shift, 'lrelu', 0.1, dt, dt)
    ref, pre = R.conv2d_ref(x, wk, scale, shift, 'lrelu', 0.1, dt)
    print('head layer %s: splits %d, worst err / bound %.3f' % (dt, splits_of(L, x, wk), _tol.check_one_rounding(y, ref, pre, dt, 'head layer ' + dt)))
    assert torch.equal(y, conv(L, x, wk, scale, shift, 'lrelu', 0.1, dt, dt))


# ------------------------------------------------------------------------------------------------------------ pool
def pool(L, x, dt, stream=None):
    B, Rr, C, N = x.shape
    xd = torch.from_numpy(x).to(DEV).to(TT[dt])
    y = torch.empty(B, (Rr + 1) // 2, (C + 1) // 2, N, dtype=TT[dt], device=DEV)
    L.call('vv_maxpool2d_same_fwd', L.ptr(xd), L.ptr(y), B, Rr, C, N, DT[dt], _stream_ptr(stream))
    torch.cuda.synchronize()
    return y


@pytest.mark.parametrize('N', [32, 40])
@pytest.mark.parametrize('grid', [(2, 5, 7), (1, 1, 1), (2, 2, 2), (1, 13, 13)], ids=lambda g: 'x'.join(map(str, g)))
@pytest.mark.parametrize('dt', ['f32', 'bf16'])
def test_maxpool_is_exact(L, dt, grid, N):
    rng = np.random.default_rng(sum(grid) + N)
    x = R.round_to(rng.standard_normal(grid + (N,)) - 3.0, dt).astype(np.float32)       # mostly negative: a zero pad would win
    _tol.check_exact(pool(L, x, dt), R.pool_ref(x), 'maxpool %s %s %d' % (dt, grid, N))


# ------------------------------------------------------------------------------------------------------------ contract
RAGGED = [(3, 13, 13, 64, 128, 3), (1, 13, 13, 128, 245, 1), (2, 6, 10, 3, 32, 3)]


@pytest.mark.parametrize('case', RAGGED, ids=lambda c: '-'.join(map(str, c)))
@pytest.mark.parametrize('dt', ['f32', 'bf16'])
def test_same_bits_twice_side_stream_and_larger_workspace(L, dt, case):
    x, wk, scale, shift = random_case(case)
    a = conv(L, x, wk, scale, shift, 'elu', 0.0, dt)
    assert torch.equal(a, conv(L, x, wk, scale, shift, 'elu', 0.0, dt))
    assert torch.equal(a, conv(L, x, wk, scale, shift, 'elu', 0.0, dt, stream=torch.cuda.Stream(DEV)))
    assert torch.equal(a, conv(L, x, wk, scale, shift, 'elu', 0.0, dt, extra_ws=4096))


def test_workspace_below_minimum_is_refused(L):
    case = (3, 13, 13, 64, 128, 3)
    x, wk, _, _ = random_case(case)
    need = L.load().vv_conv2d_workspace_bytes(3, 13, 13, 3, 64, 128, 0)
    assert need > 0 and splits_of(L, x, wk) > 1
    xd, packed = device_input(x, 'f32'), pack(L, wk, 'f32')
    y = torch.full((3, 13, 13, 128), 7.0, device=DEV)
    ws = torch.empty(need, dtype=torch.uint8, device=DEV)
    st = L.load().vv_conv2d_fwd(L.ptr(xd), L.ptr(packed), None, None, L.ptr(y), 3, 13, 13, 64, 128, 3, 0, 0.0, 0, 0, L.ptr(ws), need - 1, _stream_ptr())
    torch.cuda.synchronize()
    assert st == G.VV_ERR_WORKSPACE and bool((y == 7.0).all())


@pytest.mark.parametrize('fill', [0x00, 0xFF])
@pytest.mark.parametrize('case', RAGGED, ids=lambda c: '-'.join(map(str, c)))
@pytest.mark.parametrize('dt', ['f32', 'bf16'])
def test_guard_banded_conv(L, dt, case, fill):
    """Inputs and weights between 0xFF guards (a NaN in f32 and bf16), output and workspace between sentinels; the workspace itself
    pre-filled with zeros or NaNs: nothing outside the payloads changes, no NaN arrives, both fills give the plain run's bits."""
    B, Rr, C, cin, cout, k = case
    x, wk, scale, shift = random_case(case)
    plain = conv(L, x, wk, scale, shift, 'lrelu', 0.1, dt)
    lib = L.load()
    arena = G.Arena(DEV)
    w_in = arena.input(torch.from_numpy(wk).to(DEV), 'w_keras')
    packed = arena.output((lib.vv_conv2d_packed_bytes(k, cin, cout, DT[dt]),), torch.uint8, 'packed')
    x_in = arena.input(device_input(x, dt), 'x')
    sc = arena.input(torch.from_numpy(scale).to(DEV), 'scale')
    sh = arena.input(torch.from_numpy(shift).to(DEV), 'shift')
    y = arena.output((B, Rr, C, cout), TT[dt], 'y')
    need = lib.vv_conv2d_workspace_bytes(B, Rr, C, k, cin, cout, DT[dt])
    ws = arena.workspace(max(need, 16), fill)
    arena.commit()
    st = lib.vv_pack_conv2d(w_in.ptr, packed.ptr, k, cin, cout, DT[dt], _stream_ptr())
    assert st == 0
    st = lib.vv_conv2d_fwd(x_in.ptr, packed.ptr, sc.ptr, sh.ptr, y.ptr, B, Rr, C, cin, cout, k, 3, 0.1, DT[dt], DT[dt], ws.ptr, need, _stream_ptr())
    torch.cuda.synchronize()
    assert st == 0
    arena.check()
    assert not bool(torch.isnan(y.tensor.float()).any())
    assert torch.equal(y.tensor, plain)


@pytest.mark.parametrize('grid', [(2, 5, 7, 40), (1, 13, 13, 32)], ids=lambda g: 'x'.join(map(str, g)))
@pytest.mark.parametrize('dt', ['f32', 'bf16'])
def test_guard_banded_pool(L, dt, grid):
    B, Rr, C, N = grid
    x = R.round_to(np.random.default_rng(1).standard_normal(grid) - 3.0, dt).astype(np.float32)
    arena = G.Arena(DEV)
    x_in = arena.input(torch.from_numpy(x).to(DEV).to(TT[dt]), 'x')
    y = arena.output((B, (Rr + 1) // 2, (C + 1) // 2, N), TT[dt], 'y')
    arena.commit()
    st = L.load().vv_maxpool2d_same_fwd(x_in.ptr, y.ptr, B, Rr, C, N, DT[dt], _stream_ptr())
    torch.cuda.synchronize()
    assert st == 0
    arena.check()
    _tol.check_exact(y.tensor, R.pool_ref(x), 'guarded maxpool')
