"""GPU tests of the layers Darknet53 / Darknet53Tiny add to the 2D engine (csrc/conv2d.hip `vv_conv2d_ex_fwd`, `vv_maxpool2d_s1_same_fwd`;
DESIGN 4k) against the float64 statement of tests/_darknet53_ref.py: the stride-2 convolution, the residual add in the epilogue of both
forms (one launch, split-K), and the stride-1 pool.  Selector cases are exact, random cases meet tests/_tol.check_one_rounding on every
element (pre_act = the pre-activation and the residual together), stride 1 without a residual is vv_conv2d_fwd bit for bit."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import _conv2d_ref as R
import _darknet53_ref as R53
import _guarded as G
import _tol
from test_gpu_conv2d import ACT, DEV, DT, RAGGED, TT, conv, device_input, pack, random_case, small_ints

pytestmark = pytest.mark.gpu


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


def conv_ex(L, x, wk, scale=None, shift=None, res=None, act=None, alpha=0.0, stride=1, dt='f32', odt=None, stream=None, extra_ws=0):
    odt = odt or dt
    B, Rr, C, cin = x.shape
    k, cout = wk.shape[0], wk.shape[3]
    Ro, Co = R53.out_grid(Rr, C, stride)
    xd, packed = device_input(x, dt), pack(L, wk, dt)
    sc = None if scale is None else torch.from_numpy(np.asarray(scale, dtype=np.float32)).to(DEV)
    sh = None if shift is None else torch.from_numpy(np.asarray(shift, dtype=np.float32)).to(DEV)
    rd = None if res is None else torch.from_numpy(np.ascontiguousarray(res, dtype=np.float32)).to(DEV).to(TT[dt])
    need = L.load().vv_conv2d_ex_workspace_bytes(B, Rr, C, k, stride, cin, cout, DT[dt])
    ws = torch.full((need + extra_ws + 16,), 0xA5, dtype=torch.uint8, device=DEV)
    y = torch.empty(B, Ro, Co, cout, dtype=TT[odt], device=DEV)
    torch.cuda.synchronize()
    st = stream if stream is not None else torch.cuda.current_stream(DEV)
    with torch.cuda.stream(st):
        L.call('vv_conv2d_ex_fwd', L.ptr(xd), L.ptr(packed), L.ptr(sc), L.ptr(sh), L.ptr(rd), L.ptr(y), B, Rr, C, cin, cout, k, stride, ACT[act],
               float(alpha), DT[dt], DT[odt], L.ptr(ws), need + extra_ws, _stream_ptr(st))
    st.synchronize()
    return y


def splits_ex(L, x, wk, stride):
    B, Rr, C, cin = x.shape
    return L.load().vv_conv2d_ex_splits(B, Rr, C, wk.shape[0], stride, cin, wk.shape[3])


# ------------------------------------------------------------------------------------------------------------ exact selector cases
@pytest.mark.parametrize('force', [None, 1], ids=['default', 'direct'])
@pytest.mark.parametrize('grid', [(1, 2, 2), (2, 5, 7), (1, 3, 9), (2, 13, 13)], ids=lambda g: 'x'.join(map(str, g)))
@pytest.mark.parametrize('cin', [32, 64])
@pytest.mark.parametrize('dt', ['f32', 'bf16'])
def test_stride2_selector_kernels_are_exact(L, dt, cin, grid, force, monkeypatch):
    """One 1 in the kernel, all 9 taps: every output is one input value, or a zero where the tap has index -1.  Row -1 of image 1 is the
    ADDRESS of image 0's last row, so a kernel that decides validity by address fails on the batched grids.  With an integer-valued
    residual the sum is still exact."""
    if force is not None:
        monkeypatch.setenv('VV_C2_SPLITS', str(force))
    rng = np.random.default_rng(cin + sum(grid))
    B, Rr, C = grid
    x = small_ints(rng, (B, Rr, C, cin)) + 5.0          # no zero in the input: a zero in the output is a padded tap
    res = small_ints(rng, (B, Rr // 2, C // 2, 32))
    for tr in range(3):
        for tc in range(3):
            ci, co = int(rng.integers(cin)), int(rng.integers(32))
            wk = R.selector_kernel(3, cin, 32, tr, tc, ci, co)
            want = np.zeros((B, Rr // 2, C // 2, 32))
            want[..., co] = R53.shifted_s2(x, tr, tc, ci)
            what = 'stride-2 selector %s cin%d tap (%d,%d) %s' % (dt, cin, tr, tc, grid)
            _tol.check_exact(conv_ex(L, x, wk, stride=2, dt=dt), want, what)
            _tol.check_exact(conv_ex(L, x, wk, res=res, stride=2, dt=dt), want + res, what + ' + residual')
    if force == 1:
        assert splits_ex(L, x, wk, 2) == 1


# ------------------------------------------------------------------------------------------------------------ one rounding
GRID, CIN = (3, 13, 13), 64          # stride 1: 507 rows (8 tiles, the last ragged); stride 2: 3 x 6 x 6 = 108 rows (2 tiles, the last ragged)
COUTS = [40, 64, 96]                 # a masked tile, one full tile, two tiles
ACTS = [(None, 0.0), ('elu', 0.0), ('lrelu', 0.1)]


@functools.lru_cache(maxsize=None)
def ex_case(stride, cout):
    """Operands and the residual of one (stride, cout), made once and never changed."""
    rng = np.random.default_rng(100 * stride + cout)
    x = rng.standard_normal(GRID + (CIN,)).astype(np.float32)
    wk = (rng.standard_normal((3, 3, CIN, cout)) / np.sqrt(9 * CIN)).astype(np.float32)
    scale = rng.uniform(0.5, 2.0, cout).astype(np.float32) * rng.choice([-1.0, 1.0], cout).astype(np.float32)
    shift = rng.uniform(-1, 1, cout).astype(np.float32)
    Ro, Co = R53.out_grid(GRID[1], GRID[2], stride)
    res = (2.0 * rng.standard_normal((GRID[0], Ro, Co, cout))).astype(np.float32)
    return x, wk, scale, shift, res


@functools.lru_cache(maxsize=None)
def ex_ref(stride, cout, with_res, act, alpha, dt):
    x, wk, scale, shift, res = ex_case(stride, cout)
    return R53.conv_ex_ref(x, wk, scale, shift, res if with_res else None, act, alpha, stride, dt)


@pytest.mark.parametrize('force', [None, 1, 3], ids=['default', 'direct', 'split3'])
@pytest.mark.parametrize('stride', [1, 2])
@pytest.mark.parametrize('dt,odt', [('f32', 'f32'), ('bf16', 'bf16'), ('bf16', 'f32')])
def test_one_rounding_with_stride_and_residual(L, dt, odt, stride, force, monkeypatch):
    if force is not None:
        monkeypatch.setenv('VV_C2_SPLITS', str(force))
    worst_all = 0.0
    for cout in COUTS:
        x, wk, scale, shift, res = ex_case(stride, cout)
        if force is not None:
            assert splits_ex(L, x, wk, stride) == force
        for with_res in (False, True):
            for act, alpha in ACTS:
                y = conv_ex(L, x, wk, scale, shift, res if with_res else None, act, alpha, stride, dt, odt)
                ref, pre = ex_ref(stride, cout, with_res, act, alpha, dt)
                what = 'conv2d_ex stride %d cout %d res %s %s %s->%s' % (stride, cout, with_res, act, dt, odt)
                worst = _tol.check_one_rounding(y, ref, pre, odt, what)
                worst_all = max(worst_all, worst)
                print('%s splits %d: worst err / bound %.3f' % (what, splits_ex(L, x, wk, stride), worst))
    print('stride %d %s->%s force %s: worst err / bound over the cases %.3f' % (stride, dt, odt, force, worst_all))


@pytest.mark.parametrize('dt', ['f32', 'bf16'])
def test_real_strided_layer_runs_split_k_with_its_residual_shape(L, dt):
    """Darknet53's last strided layer on one 416 x 416 frame: 26 x 26 x 512 -> 13 x 13 x 1024, 169 rows against K = 4608: split-K by itself."""
    rng = np.random.default_rng(3)
    x = rng.standard_normal((1, 26, 26, 512)).astype(np.float32)
    wk = (rng.standard_normal((3, 3, 512, 1024)) / np.sqrt(9 * 512)).astype(np.float32)
    scale, shift = rng.uniform(0.5, 2.0, 1024).astype(np.float32), rng.uniform(-1, 1, 1024).astype(np.float32)
    res = rng.standard_normal((1, 13, 13, 1024)).astype(np.float32)
    s = splits_ex(L, x, wk, 2)
    assert s > 1 and L.load().vv_conv2d_ex_workspace_bytes(1, 26, 26, 3, 2, 512, 1024, DT[dt]) == s * 169 * 1024 * 4
    y = conv_ex(L, x, wk, scale, shift, res, 'lrelu', 0.1, 2, dt)
    xr, wr = R.round_to(x, dt), R.round_to(wk, dt)
    conv64 = torch.nn.functional.conv2d(torch.nn.functional.pad(torch.from_numpy(xr).permute(0, 3, 1, 2), (1, 0, 1, 0)),
                                        torch.from_numpy(wr).permute(3, 2, 0, 1), stride=2).permute(0, 2, 3, 1).numpy()   # (the statement is checked against this on the CPU)
    pre = conv64 * scale.astype(np.float64) + shift.astype(np.float64)
    rr = R.round_to(res, dt)
    print('strided split-K layer %s: splits %d, worst err / bound %.3f' % (
        dt, s, _tol.check_one_rounding(y, R.act_ref(pre, 'lrelu', 0.1) + rr, np.stack([pre, rr]), dt, 'strided split-K layer ' + dt)))


# ------------------------------------------------------------------------------------------------------------ identity with vv_conv2d_fwd
@pytest.mark.parametrize('force', [None, 1, 3], ids=['default', 'direct', 'split3'])
@pytest.mark.parametrize('case', RAGGED, ids=lambda c: '-'.join(map(str, c)))
@pytest.mark.parametrize('dt,odt', [('f32', 'f32'), ('bf16', 'bf16'), ('bf16', 'f32')])
def test_stride1_without_residual_is_vv_conv2d_fwd(L, dt, odt, case, force, monkeypatch):
    if force is not None:
        monkeypatch.setenv('VV_C2_SPLITS', str(force))
    x, wk, scale, shift = random_case(case)
    for act, alpha in [(None, 0.0), ('elu', 0.0), ('lrelu', 0.1)]:
        old = conv(L, x, wk, scale, shift, act, alpha, dt, odt)
        new = conv_ex(L, x, wk, scale, shift, None, act, alpha, 1, dt, odt)
        assert torch.equal(old.view(torch.uint8), new.view(torch.uint8)), (case, dt, odt, act)


# ------------------------------------------------------------------------------------------------------------ stride-1 pool
def pool1(L, x, dt):
    xd = torch.from_numpy(x).to(DEV).to(TT[dt])
    y = torch.empty_like(xd)
    B, Rr, C, N = x.shape
    L.call('vv_maxpool2d_s1_same_fwd', L.ptr(xd), L.ptr(y), B, Rr, C, N, DT[dt], _stream_ptr())
    torch.cuda.synchronize()
    return y


@pytest.mark.parametrize('N', [32, 40])
@pytest.mark.parametrize('grid', [(2, 5, 7), (1, 1, 1), (1, 1, 9), (1, 13, 13)], ids=lambda g: 'x'.join(map(str, g)))
@pytest.mark.parametrize('dt', ['f32', 'bf16'])
def test_stride1_pool_is_exact(L, dt, grid, N):
    rng = np.random.default_rng(sum(grid) + N)
    x = R.round_to(rng.standard_normal(grid + (N,)) - 3.0, dt).astype(np.float32)       # mostly negative: a zero pad would win
    _tol.check_exact(pool1(L, x, dt), R53.pool1_ref(x), 'stride-1 pool %s %s %d' % (dt, grid, N))


# ------------------------------------------------------------------------------------------------------------ contract
CONTRACT = [(2, 40), (2, 96), (1, 96)]          # (stride, cout) of ex_case: 108 / 507 rows, ragged tiles; all take the split-K form by default


@pytest.mark.parametrize('stride,cout', CONTRACT)
@pytest.mark.parametrize('dt', ['f32', 'bf16'])
def test_same_bits_twice_side_stream_and_larger_workspace(L, dt, stride, cout):
    x, wk, scale, shift, res = ex_case(stride, cout)
    a = conv_ex(L, x, wk, scale, shift, res, 'elu', 0.0, stride, dt)
    assert torch.equal(a, conv_ex(L, x, wk, scale, shift, res, 'elu', 0.0, stride, dt))
    assert torch.equal(a, conv_ex(L, x, wk, scale, shift, res, 'elu', 0.0, stride, dt, stream=torch.cuda.Stream(DEV)))
    assert torch.equal(a, conv_ex(L, x, wk, scale, shift, res, 'elu', 0.0, stride, dt, extra_ws=4096))


def test_workspace_below_minimum_is_refused(L):
    x, wk, _, _, res = ex_case(2, 96)
    B, Rr, C = GRID
    need = L.load().vv_conv2d_ex_workspace_bytes(B, Rr, C, 3, 2, CIN, 96, 0)
    assert need > 0 and splits_ex(L, x, wk, 2) > 1
    xd, packed, rd = device_input(x, 'f32'), pack(L, wk, 'f32'), torch.from_numpy(res).to(DEV)
    y = torch.full((B, Rr // 2, C // 2, 96), 7.0, device=DEV)
    ws = torch.empty(need, dtype=torch.uint8, device=DEV)
    st = L.load().vv_conv2d_ex_fwd(L.ptr(xd), L.ptr(packed), None, None, L.ptr(rd), L.ptr(y), B, Rr, C, CIN, 96, 3, 2, 0, 0.0, 0, 0, L.ptr(ws), need - 1,
                                   _stream_ptr())
    torch.cuda.synchronize()
    assert st == G.VV_ERR_WORKSPACE and bool((y == 7.0).all())


@pytest.mark.parametrize('fill', [0x00, 0xFF])
@pytest.mark.parametrize('force', [None, 1], ids=['default', 'direct'])
@pytest.mark.parametrize('stride,cout', CONTRACT)
@pytest.mark.parametrize('dt', ['f32', 'bf16'])
def test_guard_banded_conv_ex(L, dt, stride, cout, force, fill, monkeypatch):
    """x, w, scale, shift and the residual between 0xFF guards (a NaN in f32 and bf16), output and workspace between sentinels, the
    workspace pre-filled with zeros or NaNs: nothing outside the payloads changes, no NaN arrives, both fills give the plain run's bits."""
    if force is not None:
        monkeypatch.setenv('VV_C2_SPLITS', str(force))
    B, Rr, C = GRID
    Ro, Co = R53.out_grid(Rr, C, stride)
    x, wk, scale, shift, res = ex_case(stride, cout)
    plain = conv_ex(L, x, wk, scale, shift, res, 'lrelu', 0.1, stride, dt)
    lib = L.load()
    arena = G.Arena(DEV)
    w_in = arena.input(torch.from_numpy(wk).to(DEV), 'w_keras')
    packed = arena.output((lib.vv_conv2d_packed_bytes(3, CIN, cout, DT[dt]),), torch.uint8, 'packed')
    x_in = arena.input(device_input(x, dt), 'x')
    sc = arena.input(torch.from_numpy(scale).to(DEV), 'scale')
    sh = arena.input(torch.from_numpy(shift).to(DEV), 'shift')
    rs = arena.input(torch.from_numpy(res).to(DEV).to(TT[dt]), 'residual')
    y = arena.output((B, Ro, Co, cout), TT[dt], 'y')
    need = lib.vv_conv2d_ex_workspace_bytes(B, Rr, C, 3, stride, CIN, cout, DT[dt])
    assert (need > 0) == (force is None)
    ws = arena.workspace(max(need, 16), fill)
    arena.commit()
    assert lib.vv_pack_conv2d(w_in.ptr, packed.ptr, 3, CIN, cout, DT[dt], _stream_ptr()) == 0
    st = lib.vv_conv2d_ex_fwd(x_in.ptr, packed.ptr, sc.ptr, sh.ptr, rs.ptr, y.ptr, B, Rr, C, CIN, cout, 3, stride, 3, 0.1, DT[dt], DT[dt], ws.ptr, need,
                              _stream_ptr())
    torch.cuda.synchronize()
    assert st == 0
    arena.check()
    assert not bool(torch.isnan(y.tensor.float()).any())
    assert torch.equal(y.tensor, plain)


@pytest.mark.parametrize('grid', [(2, 5, 7, 40), (1, 13, 13, 32)], ids=lambda g: 'x'.join(map(str, g)))
@pytest.mark.parametrize('dt', ['f32', 'bf16'])
def test_guard_banded_stride1_pool(L, dt, grid):
    x = R.round_to(np.random.default_rng(1).standard_normal(grid) - 3.0, dt).astype(np.float32)
    arena = G.Arena(DEV)
    x_in = arena.input(torch.from_numpy(x).to(DEV).to(TT[dt]), 'x')
    y = arena.output(grid, TT[dt], 'y')
    arena.commit()
    st = L.load().vv_maxpool2d_s1_same_fwd(x_in.ptr, y.ptr, grid[0], grid[1], grid[2], grid[3], DT[dt], _stream_ptr())
    torch.cuda.synchronize()
    assert st == 0
    arena.check()
    _tol.check_exact(y.tensor, R53.pool1_ref(x), 'guarded stride-1 pool')
