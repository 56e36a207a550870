"""Exactly summable operands, float64 references and the case tables of the weight-gradient tests (tests/test_gpu_wgrad_exact.py; host
self-test: tests/test_tol_host.py).  No GPU, no torch.

Both operands of dW = A^T G are non-zero integers of magnitude 1..4: exact in float32 and in bf16, every product an integer of
magnitude <= 16, every partial sum of at most `rows` of them below 2^24 (16 * rows <= 16 * 4096 at the shapes here).  The float32
accumulators of both MFMA paths, the per-split slabs and either reduce kernel then hold integers that float32 represents, whatever
the summation order: the stored result must EQUAL the float64 definition.  There is no zero among the values, so a dropped,
doubled or misplaced product always changes the sum.

The split arithmetic and the routes of csrc/wgrad_plan.h are restated below (wgrad_plan, wgrad_plan_bf16, wg_phase_plan and the
choice of reduce kernel) for ONE purpose: tests/test_gpu_wgrad_exact.py asserts with it that the tables still hold a case without a
reduce pass, one of the plain reduce, one of the sliced reduce and a phase plan of several splits.  Nothing is computed from it.
tests/test_wgrad_plan_host.py holds it against the header itself, case by case."""
import functools

import numpy as np


def nonzero_ints(rng, shape):
    """Integers of {-4..-1, 1..4} as float32 (tests/test_gpu_conv2d.py small_ints without the zero)."""
    return (rng.integers(1, 5, shape) * rng.choice([-1, 1], shape)).astype(np.float32)


def wgrad_conv_ref(src, g):
    """dW[t][ci][co] = sum over (b, o) of src[b, 2o-1+t, ci] * g[b, o, co] (zero padding), float64."""
    B, S, _, _, cin = src.shape
    o, cout = S // 2, g.shape[-1]
    p = np.zeros((B, S + 2, S + 2, S + 2, cin))
    p[:, 1:-1, 1:-1, 1:-1] = src
    dw = np.zeros((4, 4, 4, cin, cout))
    for td in range(4):
        for th in range(4):
            for tw in range(4):
                win = p[:, td:td + 2 * o:2, th:th + 2 * o:2, tw:tw + 2 * o:2]          # [B,o,o,o,cin]
                dw[td, th, tw] = np.einsum('bdhwi,bdhwo->io', win, g)
    return dw


# ------------------------------------------------------------------------------------------------------------------ case tables
# Each case is the smallest shape that reaches its branch; the comment names the branch and the condition it was read from.
# vv_wgrad_dense: (rows, m, n, lda, a dtype, g dtype)
DENSE_CASES = [
    (300, 160, 96, 160, 'f32', 'f32'),      # wgrad_kernel<0, 64> (n % 128 != 0): ragged M tile (160 = 2 * 64 + 32), ragged N tile (96 = 64 + 32), r < r_end inside a 32-row chunk
    (64, 128, 4096, 128, 'f32', 'f32'),     # wgrad_kernel<0, 128>: wgrad_plan's bn = 128 (n % 128 == 0)
    (1000, 32, 32, 32, 'f32', 'f32'),       # 32 splits, m * n = 1024: wgrad_reduce_sliced's `splits >= 16 && n <= 65536` -> wgrad_reduce_sliced_kernel
    (300, 160, 96, 192, 'f32', 'f32'),      # lda != m: `r * a.lda + m` of wgrad_kernel<0>; the 32 floats behind every row hold 3
    (300, 160, 96, 192, 'bf16', 'bf16'),    # lda != m: `(r * a.lda + mcol + pch * 8) * 2` of wgrad_bf16_kernel<0>, a_bytes = rows * lda * 2
    (37, 160, 96, 160, 'bf16', 'bf16'),     # one 64-row chunk: wgrad_plan_bf16 splits == 1, launch_wgrad_bf16 `a.slabs = out` (no reduce pass)
    (1000, 160, 96, 160, 'bf16', 'bf16'),   # wgrad_bf16_kernel<0>: 16 splits, M = 160 and N = 96 ragged against the 128 x 128 tile
    (300, 36, 20, 36, 'bf16', 'bf16'),      # wgrad_dense_route `m % 32 == 0 && n % 32 == 0` fails: bf16 operands widened by wgrad_kernel<0, 64> (ld4_rt)
    (300, 160, 96, 160, 'bf16', 'f32'),     # wgrad_dense_route `a_dtype == WG_DT_BF16 && g_dtype == WG_DT_BF16` fails: a_bf16 = 1, g_bf16 = 0
    (300, 160, 96, 160, 'f32', 'bf16'),     # the other order: a_bf16 = 0, g_bf16 = 1
]
# vv_wgrad_conv_k4s2, reduction-GEMM forms: (B, side, cin, cout, src dtype, g dtype)
CONV_CASES = [
    (3, 8, 64, 128, 'f32', 'f32'),          # cin = 64: a 128-column tile spans two taps (`t = mcol / a.cin`); 192 rows < 128 * 8, so wgrad_conv_route leaves the phase form out
    (3, 8, 64, 128, 'bf16', 'bf16'),        # wgrad_bf16_kernel<1>
    (3, 8, 64, 128, 'bf16', 'f32'),         # mixed: wgrad_kernel<1, 128> with a_bf16 = 1
    (5, 8, 64, 32, 'f32', 'f32'),           # cout % 128 != 0: wgrad_kernel<1, 64>, `nn < a.N`
    (5, 8, 64, 32, 'bf16', 'bf16'),         # wgrad_bf16_kernel<1>: `ncol < a.N` leaves three of four column blocks of G empty
    (2, 4, 128, 64, 'f32', 'f32'),          # cin = 128: a 64-column tile is half a tap
    (2, 4, 128, 64, 'bf16', 'bf16'),        # cin = 128: a 128-column tile is exactly one tap
    (5, 2, 64, 64, 'f32', 'f32'),           # side == 2: din_log2 == 1, lo == 0, omsk == 0, r == b; per axis taps 0 and 3 are padding
    (5, 2, 64, 64, 'bf16', 'bf16'),         # side == 2 on wgrad_bf16_kernel<1>; 5 rows: splits == 1, written without a reduce pass
    (3, 16, 1, 64, 'f32', 'f32'),           # one source channel: wgrad_kernel<2, 64>; 24 splits, 4096 outputs: the sliced reduce
    (3, 16, 1, 64, 'f32', 'bf16'),          # `cin == 1 && side >= 4` with bf16 g (WG_BF16_GRID): launch_wgrad_bf16<2>, wgrad_grid_one_tile -> wgrad_bf16_kernel<2, true>
    (2, 8, 1, 128, 'f32', 'bf16'),          # cout > 64: wgrad_bf16_kernel<2, false>, column blocks 2, 3 of A zeroed once
    (2, 2, 1, 32, 'f32', 'f32'),            # side == 2 with one channel: wgrad_kernel<2, 64>
    (2, 2, 1, 32, 'f32', 'bf16'),           # `side >= 4` fails: bf16 g stays on wgrad_kernel<2, 64> (g_bf16 = 1)
]
# phase form (wgrad_phase.hip; bf16 / bf16, cin % 64 == 0, cout % 128 == 0, at least 1024 output rows): (B, side, cin, cout)
PHASE_CASES = [
    (16, 8, 64, 128),                       # output side 4 (WgGeo<2>): NS = 2 samples per box, 8 boxes, 8 splits
    (17, 8, 128, 256),                      # odd batch: `b0 + sample < a.batch` and rleft = 64 empty the second half of the last box; two cin and two cout blocks
    (2, 16, 64, 128),                       # output side 8 (WgGeo<3>): a box is two depth planes
    (3, 16, 64, 128),                       # 12 boxes over 8 splits of 2: splits becomes 6
    (1, 32, 64, 128),                       # output side 16 (WgGeo<4>): a box is half a depth plane
]
PHASE_ENVS = [{}, {'VV_NO_WGRAD_PHASE': '1'}, {'VV_WGRAD_F32': '1'}]   # phase form, wgrad_bf16_kernel<1>, wgrad_kernel<1> on the same bf16 operands
PITCH_FILL = 3.0                            # what the gap behind every row of a pitched A holds: a kernel that reads it shows it


def dense_rows(case):
    return case[0]


def conv_rows(case):
    return case[0] * (case[1] // 2) ** 3


def _seed(case):
    return sum((i + 1) * 7919 * (v if isinstance(v, int) else len(v)) for i, v in enumerate(case)) % (2 ** 31)


@functools.lru_cache(maxsize=None)
def dense_inputs(case):
    """-> (a [rows, lda] with the pitch gap filled, g [rows, n]) float32, read-only."""
    rows, m, n, lda, _, _ = case
    rng = np.random.default_rng(_seed(case))
    a = np.full((rows, lda), PITCH_FILL, np.float32)
    a[:, :m] = nonzero_ints(rng, (rows, m))
    g = nonzero_ints(rng, (rows, n))
    a.setflags(write=False), g.setflags(write=False)
    return a, g


@functools.lru_cache(maxsize=None)
def dense_ref(case):
    a, g = dense_inputs(case)
    ref = a[:, :case[1]].astype(np.float64).T @ g.astype(np.float64)
    ref.setflags(write=False)
    return ref


@functools.lru_cache(maxsize=None)
def conv_inputs(case):
    """-> (src [B, side, side, side, cin], g [B, o, o, o, cout]) float32, read-only; case = its first four numbers."""
    B, side, cin, cout = case[:4]
    rng = np.random.default_rng(_seed(case[:4]))
    o = side // 2
    src, g = nonzero_ints(rng, (B, side, side, side, cin)), nonzero_ints(rng, (B, o, o, o, cout))
    src.setflags(write=False), g.setflags(write=False)
    return src, g


@functools.lru_cache(maxsize=None)
def conv_ref(case):
    src, g = conv_inputs(case[:4])
    ref = wgrad_conv_ref(src.astype(np.float64), g.astype(np.float64))
    ref.setflags(write=False)
    return ref


# ------------------------------------------------------------------------------------- the split arithmetic, restated (see the top)
def _cdiv(a, b):
    return (a + b - 1) // b


def wgrad_plan(R, M, N):
    """wgrad_plan.h wgrad_plan -> (bn, splits): 64 x bn tiles, 32-row chunks."""
    bn = 128 if N % 128 == 0 else 64
    tiles, chunks, splits = _cdiv(M, 64) * _cdiv(N, bn), _cdiv(R, 32), 1
    while tiles * splits < 1024 and splits * 2 <= chunks and splits < 256:
        splits *= 2
    return bn, _cdiv(R, _cdiv(chunks, splits) * 32)


def wgrad_plan_bf16(R, M, N):
    """wgrad_plan.h wgrad_plan_bf16 -> splits: 128 x 128 tiles, 64-row chunks."""
    tiles, chunks, splits = _cdiv(M, 128) * _cdiv(N, 128), _cdiv(R, 64), 1
    want = 1024 if tiles <= 2 else 512
    while tiles * splits < want and splits * 2 <= chunks and splits < want:
        splits *= 2
    return _cdiv(R, _cdiv(chunks, splits) * 64)


def wg_phase_plan(rows, cin, cout):
    """wgrad_plan.h wg_phase_plan -> splits: boxes of 128 rows."""
    nboxes, kinds, splits = _cdiv(rows, 128), 8 * (cin // 64) * (cout // 128), 1
    while kinds * splits * 2 <= 256 and splits * 2 <= nboxes:
        splits *= 2
    return _cdiv(nboxes, _cdiv(nboxes, splits))


def reduce_kind(splits, n, bf16_kernel):
    """wgrad_reduce_kind's choice; the bf16 kernel alone writes dw itself when there is one split (launch_wgrad_bf16)."""
    if bf16_kernel and splits == 1:
        return 'none'
    return 'sliced' if splits >= 16 and n <= 65536 else 'plain'


def _span_ok(elems):
    """A bf16 operand of `elems` elements ends below the 32-bit buffer offset the bf16 kernels keep for "out of range"."""
    return elems * 2 < 0xFFFFFFF0


def dense_route(case, env=()):
    """-> (kernel, splits, reduce) of vv_wgrad_dense under the overrides `env` (aligned operands)."""
    rows, m, n, lda, adt, gdt = case
    if (adt == gdt == 'bf16' and 'VV_WGRAD_F32' not in env and m % 32 == 0 and n % 32 == 0 and lda % 8 == 0
            and _span_ok(rows * lda) and _span_ok(rows * n)):
        s = wgrad_plan_bf16(rows, m, n)
        return 'bf16', s, reduce_kind(s, m * n, True)
    s = wgrad_plan(rows, m, n)[1]
    return 'f32', s, reduce_kind(s, m * n, False)


def conv_route(case, env=()):
    """-> (kernel, splits, reduce) of vv_wgrad_conv_k4s2 under the overrides `env` (aligned operands)."""
    B, side, cin, cout, sdt, gdt = case
    rows, m = conv_rows(case), 64 * cin
    f32_only = 'VV_WGRAD_F32' in env
    g_fits = _span_ok(rows * cout)
    if cin != 1 and sdt == gdt == 'bf16' and not f32_only and g_fits and _span_ok(B * side ** 3 * cin):
        if 'VV_NO_WGRAD_PHASE' not in env and side // 2 in (4, 8, 16) and cout % 128 == 0 and rows >= 1024:
            s = wg_phase_plan(rows, cin, cout)
            return 'phase', s, reduce_kind(s, m * cout, False)
        if cout % 32 == 0:
            s = wgrad_plan_bf16(rows, m, cout)
            return 'bf16', s, reduce_kind(s, m * cout, True)
    if cin == 1 and side >= 4 and gdt == 'bf16' and cout % 32 == 0 and not f32_only and g_fits:
        s = wgrad_plan_bf16(rows, 64, cout)
        return 'bf16 one channel, %s' % ('one tile' if cout <= 64 else 'full tile'), s, reduce_kind(s, 64 * cout, True)
    s = wgrad_plan(rows, m, cout)[1]
    return 'f32', s, reduce_kind(s, m * cout, False)
