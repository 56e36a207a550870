"""Exact GPU tests of the weight-gradient entries vv_wgrad_dense and vv_wgrad_conv_k4s2 (csrc/wgrad.hip, csrc/wgrad_phase.hip).

Operands are non-zero integers of magnitude 1..4 (tests/_wgrad_inputs.py): exact in float32 and bf16, integer products, every partial
sum below 2^24.  The float32 accumulators of both MFMA paths, the per-split slabs and either reduce kernel then give ONE answer in any
summation order, and it must EQUAL the float64 definition on every element (tests/_tol.check_exact); outputs are pre-filled with NaN,
so an unwritten element fails too.  Every case of the tables is the smallest shape that reaches one branch of the dispatch; the
branch is named beside the case in tests/_wgrad_inputs.py.  tests/test_tol_host.py proves on the CPU that the inputs are what they
claim, and that this check rejects a reference that is off by one product where the max-norm bound 2e-5 max|ref| + 1e-5 accepts it."""
import pytest
import torch

import _layer_calls as LC
import _tol as T
import _wgrad_inputs as WI

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
TDT = {'f32': torch.float32, 'bf16': torch.bfloat16}
_st, _dev = LC.st, LC.dev


@pytest.fixture(scope='module')
def L():
    from voxvae import lib
    lib.load()
    assert torch.cuda.is_available()
    return lib


def _nan(shape):
    return torch.full(tuple(shape), float('nan'), dtype=torch.float32, device=DEV)


@pytest.mark.parametrize('rows,m,n,lda,adt,gdt', WI.DENSE_CASES)
def test_wgrad_dense_exact(L, rows, m, n, lda, adt, gdt):
    case = (rows, m, n, lda, adt, gdt)
    a, g = WI.dense_inputs(case)
    ad, gd = _dev(a, TDT[adt]), _dev(g, TDT[gdt])
    out = _nan((m, n))
    ws = torch.empty(L.load().vv_wgrad_workspace_bytes(rows, m, n), dtype=torch.uint8, device=DEV)
    L.call('vv_wgrad_dense', L.ptr(ad), L.ptr(gd), L.ptr(out), rows, m, n, lda, L.DTYPES[adt], L.DTYPES[gdt], L.ptr(ws), ws.numel(), _st())
    torch.cuda.synchronize()
    T.check_exact(out, WI.dense_ref(case), 'wgrad_dense %s' % (case,))


@pytest.mark.parametrize('B,side,cin,cout,sdt,gdt', WI.CONV_CASES)
def test_wgrad_conv_exact(L, B, side, cin, cout, sdt, gdt):
    case = (B, side, cin, cout, sdt, gdt)
    src, g = WI.conv_inputs(case[:4])
    sd, gd = _dev(src, TDT[sdt]), _dev(g, TDT[gdt])
    out = _nan((4, 4, 4, cin, cout))
    ws = torch.empty(L.load().vv_wgrad_workspace_bytes(WI.conv_rows(case), 64 * cin, cout), dtype=torch.uint8, device=DEV)
    L.call('vv_wgrad_conv_k4s2', L.ptr(sd), L.ptr(gd), L.ptr(out), B, side, cin, cout, L.DTYPES[sdt], L.DTYPES[gdt], L.ptr(ws), ws.numel(), _st())
    torch.cuda.synchronize()
    T.check_exact(out, WI.conv_ref(case[:4]), 'wgrad_conv %s' % (case,))


@pytest.mark.parametrize('B,side,cin,cout', WI.PHASE_CASES)
def test_wgrad_conv_phase_exact(L, B, side, cin, cout, monkeypatch):
    """bf16 operands three ways: the phase form, the reduction-GEMM bf16 kernel (VV_NO_WGRAD_PHASE) and the widening float32 kernel
    (VV_WGRAD_F32).  All three equal the float64 definition, hence one another bit for bit."""
    case = (B, side, cin, cout)
    src, g = WI.conv_inputs(case)
    ref = WI.conv_ref(case)
    sd, gd = _dev(src, torch.bfloat16), _dev(g, torch.bfloat16)
    ws = torch.empty(L.load().vv_wgrad_workspace_bytes(WI.conv_rows(case), 64 * cin, cout), dtype=torch.uint8, device=DEV)
    for env in WI.PHASE_ENVS:
        for v in ('VV_NO_WGRAD_PHASE', 'VV_WGRAD_F32'):
            monkeypatch.delenv(v, raising=False)
        for v, x in env.items():
            monkeypatch.setenv(v, x)
        out = _nan((4, 4, 4, cin, cout))
        L.call('vv_wgrad_conv_k4s2', L.ptr(sd), L.ptr(gd), L.ptr(out), B, side, cin, cout, L.VV_BF16, L.VV_BF16, L.ptr(ws), ws.numel(), _st())
        torch.cuda.synchronize()
        T.check_exact(out, ref, 'wgrad_conv %s under %s' % (case, env or 'no override'))
