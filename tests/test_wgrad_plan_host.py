"""csrc/wgrad_plan.h against its restatement in tests/_wgrad_inputs.py (no GPU): tests/wgrad_plan_main.cpp, a stand-alone program over
the header alone, is built under the host sanitizers, self-checks its plans against vv_wgrad_workspace_bytes' maximum, and then prints
form, splits and reduce kind for every case handed to it.  The GPU tests choose their cases with the Python restatement; if the C++
drifts from it, this fails instead of the exact tests silently reaching fewer forms than their tables name."""
import itertools
import subprocess

import pytest
import torch

import _wgrad_inputs as WI
from _common import build_and_run_sanitized

DT = {'f32': 0, 'bf16': 1}
ENVS = [(), ('VV_WGRAD_F32',), ('VV_NO_WGRAD_PHASE',)]
DENSE_FORM = {'bf16': 'BF16_DENSE', 'f32': 'F32'}
CONV_FORM = {'phase': 'PHASE', 'bf16': 'BF16_TAPS', 'bf16 one channel, one tile': 'BF16_GRID_ONE', 'bf16 one channel, full tile': 'BF16_GRID',
             'f32': 'F32'}


def dense_line(case, env=(), a_aligned=1, g_aligned=1):
    rows, m, n, lda, adt, gdt = case
    return 'd %d %d %d %d %d %d %d %d %d' % (rows, m, n, lda, DT[adt], DT[gdt], a_aligned, g_aligned, 'VV_WGRAD_F32' in env)


def conv_line(case, env=(), src_aligned=1, g_aligned=1):
    B, side, cin, cout, sdt, gdt = case
    return 'c %d %d %d %d %d %d %d %d %d %d' % (B, side, cin, cout, DT[sdt], DT[gdt], src_aligned, g_aligned, 'VV_WGRAD_F32' in env,
                                                 'VV_NO_WGRAD_PHASE' in env)


def dense_expected(case, env=()):
    k, s, red = WI.dense_route(case, env)
    return '%s %d %s' % (DENSE_FORM[k], s, red)


def conv_expected(case, env=()):
    if case[2] == 1 and case[4] != 'f32':
        return 'refused'                       # vv_wgrad_conv_k4s2: single-channel sources are float32 grids (VV_ERR_DTYPE), before any route
    k, s, red = WI.conv_route(case, env)
    return '%s %d %s' % (CONV_FORM[k], s, red)


def rows_sweep():
    """1 .. 2^20 at the powers of two and their two neighbours."""
    return sorted({r for p in range(21) for r in (2 ** p - 1, 2 ** p, 2 ** p + 1) if r >= 1})


def sweep():
    """-> [(line, expected)]: the tables of the GPU tests under every override, then shapes across every threshold of the plans."""
    out = []
    for c in WI.DENSE_CASES:
        out.append((dense_line(c), dense_expected(c)))
    for c in WI.CONV_CASES:
        out.append((conv_line(c), conv_expected(c)))
    for c in WI.PHASE_CASES:
        for env in WI.PHASE_ENVS:
            out.append((conv_line(c + ('bf16', 'bf16'), tuple(env)), conv_expected(c + ('bf16', 'bf16'), tuple(env))))
    pairs = list(itertools.product(('f32', 'bf16'), repeat=2))
    # dense: m over ragged, whole-tile and panel sizes; a pitch equal to m, one that keeps 16-byte rows for bf16 and one that does not
    for rows, m, n, pad, (adt, gdt), env in itertools.product(rows_sweep(), (36, 64, 160, 4096, 16384), (4, 32, 64, 96, 128, 512), (0, 4, 8), pairs, ENVS):
        c = (rows, m, n, m + pad, adt, gdt)
        out.append((dense_line(c, env), dense_expected(c, env)))
    # stride-2 layers: every batch that brings the row count B (side / 2)^3 next to a value of the row sweep
    for side in (2, 4, 8, 16, 32, 64):
        o3 = (side // 2) ** 3
        batches = sorted({b for r in rows_sweep() for b in (r // o3, -(-r // o3)) if b >= 1})
        for B, cin, cout, (sdt, gdt), env in itertools.product(batches, (1, 64, 128, 192, 256), (4, 32, 64, 96, 128, 512), pairs, ENVS):
            c = (B, side, cin, cout, sdt, gdt)
            out.append((conv_line(c, env), conv_expected(c, env)))
    return out


# What the restatement does not model, with the form read from the conditions the entries had before the routes were one function
# (`vv_aligned16(A) && vv_aligned16(G)` of the bf16 forms -- `vv_aligned16(g)` alone on one channel, whose source is read by plain
# loads -- and `elems * 2 >= 0xFFFFFFF0` against rows * lda, rows * n, B side^3 cin and rows * cout): 0xFFFFFFF0 / 2 = 2147483640.
NAMED = [
    # unaligned operands
    (dense_line((300, 160, 96, 160, 'bf16', 'bf16')), 'BF16_DENSE'),
    (dense_line((300, 160, 96, 160, 'bf16', 'bf16'), a_aligned=0), 'F32'),
    (dense_line((300, 160, 96, 160, 'bf16', 'bf16'), g_aligned=0), 'F32'),
    (conv_line((16, 8, 64, 128, 'bf16', 'bf16'), src_aligned=0), 'F32'),            # neither the phase form nor the tap form
    (conv_line((16, 8, 64, 128, 'bf16', 'bf16'), g_aligned=0), 'F32'),
    (conv_line((3, 8, 64, 128, 'bf16', 'bf16'), src_aligned=0), 'F32'),
    (conv_line((3, 16, 1, 64, 'f32', 'bf16'), src_aligned=0), 'BF16_GRID_ONE'),     # the float32 grid is not a DMA operand
    (conv_line((3, 16, 1, 64, 'f32', 'bf16'), g_aligned=0), 'F32'),
    # dense, A: rows * lda = 17895696 * 120 = 2147483520 fits, 17895697 * 120 = 2147483640 does not
    (dense_line((17895696, 32, 32, 120, 'bf16', 'bf16')), 'BF16_DENSE'),
    (dense_line((17895697, 32, 32, 120, 'bf16', 'bf16')), 'F32'),
    # dense, G: rows * n = (2^25 - 1) * 64 fits, 2^25 * 64 = 2^31 does not (A is half of it)
    (dense_line((2 ** 25 - 1, 32, 64, 32, 'bf16', 'bf16')), 'BF16_DENSE'),
    (dense_line((2 ** 25, 32, 64, 32, 'bf16', 'bf16')), 'F32'),
    # tap form, source: B * 2^3 * 64 = (2^22 - 1) * 512 fits, 2^22 * 512 = 2^31 does not (output side 1: no phase form)
    (conv_line((2 ** 22 - 1, 2, 64, 32, 'bf16', 'bf16')), 'BF16_TAPS'),
    (conv_line((2 ** 22, 2, 64, 32, 'bf16', 'bf16')), 'F32'),
    # tap form, g: rows * cout = (2^21 - 1) * 1024 fits, 2^21 * 1024 does not (the source is half of it)
    (conv_line((2 ** 21 - 1, 2, 64, 1024, 'bf16', 'bf16')), 'BF16_TAPS'),
    (conv_line((2 ** 21, 2, 64, 1024, 'bf16', 'bf16')), 'F32'),
    # phase form, source: B * 8^3 * 64 = 65535 * 32768 fits, 65536 * 32768 = 2^31 does not (and the tap form has the same limit)
    (conv_line((65535, 8, 64, 128, 'bf16', 'bf16')), 'PHASE'),
    (conv_line((65536, 8, 64, 128, 'bf16', 'bf16')), 'F32'),
    # phase form, g: B * 4^3 * 1024 = 32767 * 65536 fits, 32768 * 65536 = 2^31 does not (the source is half of it)
    (conv_line((32767, 8, 64, 1024, 'bf16', 'bf16')), 'PHASE'),
    (conv_line((32768, 8, 64, 1024, 'bf16', 'bf16')), 'F32'),
    # one channel, g: B * 2^3 * 64 = (2^22 - 1) * 512 fits, 2^22 * 512 does not; the float32 source has no such limit
    (conv_line((2 ** 22 - 1, 4, 1, 64, 'f32', 'bf16')), 'BF16_GRID_ONE'),
    (conv_line((2 ** 22, 4, 1, 64, 'f32', 'bf16')), 'F32'),
]


@pytest.mark.skipif(torch.cuda.is_available(), reason='sanitizer programs run on CPU-only machines')
def test_wgrad_plan_header_agrees_with_the_restatement(tmp_path):
    build_and_run_sanitized('wgrad_plan_main.cpp', tmp_path, 'wgrad_plan_main')        # bare: the self-check, ends with OK
    cases = sweep()
    assert len(cases) > 100000
    lines = [c[0] for c in cases] + [c[0] for c in NAMED]
    (tmp_path / 'cases.txt').write_text('\n'.join(lines) + '\n')
    r = subprocess.run([str(tmp_path / 'wgrad_plan_main'), str(tmp_path / 'cases.txt')], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and 'runtime error' not in r.stderr and 'AddressSanitizer' not in r.stderr, r.stdout[-2000:] + r.stderr[-4000:]
    got = r.stdout.split('\n')[:-1]
    assert len(got) == len(lines)
    bad = [(ln, g, want) for (ln, want), g in zip(cases, got) if g != want]
    assert not bad, '%d of %d routes differ, the first: %s' % (len(bad), len(cases), bad[:10])
    named = [(ln, g.split()[0], want) for (ln, want), g in zip(NAMED, got[len(cases):])]
    assert all(g == want for _, g, want in named), [x for x in named if x[1] != x[2]]
    # the sweep reached every form and every reduce kind, so equality above is not equality of one branch
    assert {g.split()[0] for g in got} == set(DENSE_FORM.values()) | set(CONV_FORM.values()) | {'refused'}
    assert {g.split()[2] for g in got if g != 'refused'} == {'none', 'plain', 'sliced'}
