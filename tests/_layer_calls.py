"""The ctypes launch sequences of the forward layer entries (pack the weights, size the workspace, call), once, for
tests/test_gpu_ops.py and tests/test_gpu_exact.py.  Every function takes the voxvae.lib module first and device tensors, allocates
what the call needs, launches on the current stream, synchronises and returns the output tensor.  Outputs are pre-filled with NaN
so that an element the kernel leaves unwritten fails every comparison.  Kernel forms are chosen by the caller (monkeypatch.setenv)."""
import ctypes

import numpy as np
import torch

DEV = 'cuda:0'
F8 = getattr(torch, 'float8_e4m3fn', None)
TDT = {'f32': torch.float32, 'bf16': torch.bfloat16, 'fp8': F8}


def st():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def dev(a, dt=torch.float32):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(DEV).to(dt).contiguous()


def nan_out(shape, tdt):
    return torch.full(tuple(shape), float('nan'), dtype=torch.float32, device=DEV).to(tdt)


def _ws(nbytes):
    return torch.empty(max(nbytes, 16), dtype=torch.uint8, device=DEV)


# ------------------------------------------------------------------------------------------------------------ weight images
def pack_conv_k4(L, wd, cin, cout, dtname):
    wp = torch.empty(cout, 64 * cin, dtype=TDT[dtname], device=DEV)
    L.call('vv_pack_conv_k4', L.ptr(wd), L.ptr(wp), cin, cout, L.DTYPES[dtname], st())
    return wp


def pack_convT_k4s2(L, wd, cin, cout, dtname):
    wp = torch.empty(8, cout, 8 * cin, dtype=TDT[dtname], device=DEV)
    L.call('vv_pack_convT_k4s2', L.ptr(wd), L.ptr(wp), cin, cout, L.DTYPES[dtname], st())
    return wp


def _pack_bf16_image(L, name, wd, cin, cout):
    wp = torch.empty(64 * cin * cout, dtype=torch.bfloat16, device=DEV)
    L.call(name, L.ptr(wd), L.ptr(wp), cin, cout, st())
    return wp


def pack_conv_k4_skip(L, wd, cin, cout):
    return _pack_bf16_image(L, 'vv_pack_conv_k4_skip', wd, cin, cout)


def pack_convT_k4s2_skip(L, wd, cin, cout):
    return _pack_bf16_image(L, 'vv_pack_convT_k4s2_skip', wd, cin, cout)


def pack_convT_k4s2_frag(L, wd, cin, cout):
    return _pack_bf16_image(L, 'vv_pack_convT_k4s2_frag', wd, cin, cout)


def pack_convT_k4s2_frag_fp8(L, wd, cin, cout):
    wf = torch.empty(64 * cin * cout, dtype=torch.uint8, device=DEV)
    L.call('vv_pack_convT_k4s2_frag_fp8', L.ptr(wd), L.ptr(wf), cin, cout, st())
    return wf


def pack_dense(L, wd, K, N, dtname):
    wp = torch.empty(N, K, dtype=TDT[dtname], device=DEV)
    L.call('vv_pack_dense', L.ptr(wd), L.ptr(wp), K, N, L.DTYPES[dtname], st())
    return wp


# ------------------------------------------------------------------------------------------------------------ implicit GEMM
def conv3d_k4s2(L, xd, wp, scd, shd, B, side, cin, cout, act, dtname, odt=None):
    """vv_conv3d_k4s2_fwd (output in the operand type), or vv_conv3d_k4s2_fwd_io when an output type `odt` is named."""
    ws = _ws(L.load().vv_conv3d_k4s2_workspace_bytes(B, side, cin, cout, L.DTYPES[dtname]))
    so = side // 2
    y = nan_out((B, so, so, so, cout), TDT[odt or dtname])
    if odt is None:
        L.call('vv_conv3d_k4s2_fwd', L.ptr(xd), L.ptr(wp), L.ptr(scd), L.ptr(shd), L.ptr(y), B, side, cin, cout, act, L.DTYPES[dtname],
               L.ptr(ws), ws.numel(), st())
    else:
        L.call('vv_conv3d_k4s2_fwd_io', L.ptr(xd), L.ptr(wp), L.ptr(scd), L.ptr(shd), L.ptr(y), B, side, cin, cout, act, L.DTYPES[dtname],
               L.DTYPES[odt], L.ptr(ws), ws.numel(), st())
    torch.cuda.synchronize()
    return y


def convT3d_k4s2(L, xd, wp, scd, shd, B, side, cin, cout, act, dtname, odt=None):
    ws = _ws(L.load().vv_convT3d_k4s2_workspace_bytes(B, side, cin, cout, L.DTYPES[dtname]))
    y = nan_out((B, 2 * side, 2 * side, 2 * side, cout), TDT[odt or dtname])
    if odt is None:
        L.call('vv_convT3d_k4s2_fwd', L.ptr(xd), L.ptr(wp), L.ptr(scd), L.ptr(shd), L.ptr(y), B, side, cin, cout, act, L.DTYPES[dtname],
               L.ptr(ws), ws.numel(), st())
    else:
        L.call('vv_convT3d_k4s2_fwd_io', L.ptr(xd), L.ptr(wp), L.ptr(scd), L.ptr(shd), L.ptr(y), B, side, cin, cout, act, L.DTYPES[dtname],
               L.DTYPES[odt], L.ptr(ws), ws.numel(), st())
    torch.cuda.synchronize()
    return y


# ------------------------------------------------------------------------------- skip / position-major / whole-sample (bf16)
def conv3d_k4s2_skip(L, xd, wp, scd, shd, B, cin, cout, act):
    y = nan_out((B, 4, 4, 4, cout), torch.bfloat16)
    L.call('vv_conv3d_k4s2_skip_fwd', L.ptr(xd), L.ptr(wp), L.ptr(scd), L.ptr(shd), L.ptr(y), B, 8, cin, cout, act, L.VV_BF16, st())
    torch.cuda.synchronize()
    return y


def convT3d_k4s2_skip(L, xd, wp, scd, shd, B, cin, cout, act):
    y = nan_out((B, 8, 8, 8, cout), torch.bfloat16)
    L.call('vv_convT3d_k4s2_skip_fwd', L.ptr(xd), L.ptr(wp), L.ptr(scd), L.ptr(shd), L.ptr(y), B, 4, cin, cout, act, L.VV_BF16, st())
    torch.cuda.synchronize()
    return y


def convT3d_k4s2_whole(L, xd, wp, scd, shd, B, act, cin=128, cout=64):
    y = nan_out((B, 16, 16, 16, cout), torch.bfloat16)
    L.call('vv_convT3d_k4s2_whole_fwd', L.ptr(xd), L.ptr(wp), L.ptr(scd), L.ptr(shd), L.ptr(y), B, 8, cin, cout, act, L.VV_BF16, st())
    torch.cuda.synchronize()
    return y


def conv3d_k4s2_pos(L, xd, wp, scd, shd, B, cin, cout, act):
    ws = _ws(L.load().vv_conv3d_k4s2_pos_workspace_bytes(B, cin, cout))
    y = nan_out((B, 2, 2, 2, cout), torch.bfloat16)
    L.call('vv_conv3d_k4s2_pos_fwd', L.ptr(xd), L.ptr(wp), L.ptr(scd), L.ptr(shd), L.ptr(y), B, 4, cin, cout, act, L.VV_BF16,
           L.ptr(ws), ws.numel(), st())
    torch.cuda.synchronize()
    return y


def convT3d_k4s2_pos(L, xd, wp, scd, shd, B, cin, cout, act):
    ws = _ws(L.load().vv_convT3d_k4s2_pos_workspace_bytes(B, cin, cout))
    y = nan_out((B, 4, 4, 4, cout), torch.bfloat16)
    L.call('vv_convT3d_k4s2_pos_fwd', L.ptr(xd), L.ptr(wp), L.ptr(scd), L.ptr(shd), L.ptr(y), B, 2, cin, cout, act, L.VV_BF16,
           L.ptr(ws), ws.numel(), st())
    torch.cuda.synchronize()
    return y


# ------------------------------------------------------------------------------------------ direct E2 / D4 kernels and twins
def conv3d_k4s2_direct(L, xd, wp, scd, shd, B, side, act, odt='bf16', cin=64, cout=128):
    so = side // 2
    y = nan_out((B, so, so, so, cout), TDT[odt])
    if odt == 'bf16':
        L.call('vv_conv3d_k4s2_direct_fwd', L.ptr(xd), L.ptr(wp), L.ptr(scd), L.ptr(shd), L.ptr(y), B, side, cin, cout, act, L.VV_BF16, st())
    else:
        L.call('vv_conv3d_k4s2_direct_fwd_io', L.ptr(xd), L.ptr(wp), L.ptr(scd), L.ptr(shd), L.ptr(y), B, side, cin, cout, act, L.VV_BF16,
               L.DTYPES[odt], st())
    torch.cuda.synchronize()
    return y


def convT3d_k4s2_direct(L, xd, wf, scd, shd, B, side, act, cin=128, cout=64):
    y = nan_out((B, 2 * side, 2 * side, 2 * side, cout), torch.bfloat16)
    L.call('vv_convT3d_k4s2_direct_fwd', L.ptr(xd), L.ptr(wf), L.ptr(scd), L.ptr(shd), L.ptr(y), B, side, cin, cout, act, L.VV_BF16, st())
    torch.cuda.synchronize()
    return y


def conv3d_k4s2_direct_fp8(L, xd, wp, scd, shd, B, side, act, odt, cin=64, cout=128):
    so = side // 2
    y = nan_out((B, so, so, so, cout), TDT[odt])
    L.call('vv_conv3d_k4s2_direct_fp8_fwd', L.ptr(xd), L.ptr(wp), L.ptr(scd), L.ptr(shd), L.ptr(y), B, side, cin, cout, act, L.DTYPES[odt], st())
    torch.cuda.synchronize()
    return y


def convT3d_k4s2_direct_fp8(L, xd, wf, scd, shd, B, side, act, odt, cin=128, cout=64):
    y = nan_out((B, 2 * side, 2 * side, 2 * side, cout), TDT[odt])
    L.call('vv_convT3d_k4s2_direct_fp8_fwd', L.ptr(xd), L.ptr(wf), L.ptr(scd), L.ptr(shd), L.ptr(y), B, side, cin, cout, act, L.DTYPES[odt], st())
    torch.cuda.synchronize()
    return y


# ------------------------------------------------------------------------------------------------ first / last layer, dense
def conv3d_first(L, xd, wp, scd, shd, B, D, act, dtname, odt=None):
    y = nan_out((B, D // 2, D // 2, D // 2, 64), TDT[odt or dtname])
    if odt is None:
        L.call('vv_conv3d_first_fwd', L.ptr(xd), L.ptr(wp), L.ptr(scd), L.ptr(shd), L.ptr(y), B, D, 64, act, L.DTYPES[dtname], st())
    else:
        L.call('vv_conv3d_first_fwd_io', L.ptr(xd), L.ptr(wp), L.ptr(scd), L.ptr(shd), L.ptr(y), B, D, 64, act, L.DTYPES[dtname], L.DTYPES[odt], st())
    torch.cuda.synchronize()
    return y


def convT3d_final_bce(L, xd, wd, yd, B, side, dtname):
    """-> (probs, logits, stats, workspace): the caller may launch the metrics form into the same workspace."""
    D = 2 * side
    ws = _ws(L.load().vv_convT3d_final_bce_workspace_bytes(B, side))
    probs = nan_out((B, D, D, D, 1), torch.float32)
    logits = nan_out((B, D, D, D, 1), torch.float32)
    stats = nan_out((B, 4), torch.float32)
    L.call('vv_convT3d_final_bce_fwd', L.ptr(xd), L.ptr(wd), L.ptr(yd), L.ptr(probs), L.ptr(logits), L.ptr(stats), B, side, 64, 0.6, 1e-7,
           L.DTYPES[dtname], L.ptr(ws), ws.numel(), st())
    torch.cuda.synchronize()
    return probs, logits, stats, ws


def dense(L, xd, wp, scd, shd, M, N, K, act, dtname, odt='f32'):
    ws = _ws(L.load().vv_dense_workspace_bytes(M, N, K, L.DTYPES[dtname]))
    y = nan_out((M, N), TDT[odt])
    L.call('vv_dense_fwd', L.ptr(xd), L.ptr(wp), L.ptr(scd), L.ptr(shd), L.ptr(y), M, N, K, act, L.DTYPES[dtname], L.DTYPES[odt],
           L.ptr(ws), ws.numel(), st())
    torch.cuda.synchronize()
    return y
