"""CPU tests of the memory-discipline checker (tests/_guarded.py): it reports every kind of corruption it claims to, with the buffer's
name and the byte offsets, its guard byte poisons float32 / bfloat16 / e4m3fn reductions, and the table of tests/test_gpu_guards.py
names every launching entry of include/voxvae.h and only cases an oracle-parity test holds."""
import importlib
import re

import pytest
import torch

import _guarded as G

F8 = getattr(torch, 'float8_e4m3fn', None)


def _arena(device='cpu'):
    a = G.Arena(device)
    x = a.input(torch.arange(3 * 700, dtype=torch.float32).view(3, 700), 'x')                   # sample 2800 B -> guard 4096
    big = a.input(torch.ones(2, 5000, dtype=torch.bfloat16), 'big')                              # sample 10000 B -> guard 10240
    idx = a.input(torch.arange(7, dtype=torch.int32), 'idx')
    io = a.input(torch.zeros(9), 'param', inout=True)
    y = a.output((3, 8, 5), torch.float32, 'y')
    ws = a.workspace(1000, 0x00, 'ws', extra=1016)
    a.commit()
    return a, x, big, idx, io, y, ws


def test_layout():
    a, x, big, idx, io, y, ws = _arena()
    assert (x.guard, big.guard, idx.guard, y.guard, ws.guard) == (4096, 10240, 4096, 4096, 4096)
    for b in a.buffers:
        assert b.address % 512 == 0 and b.trail >= b.guard
    assert torch.equal(x.tensor, torch.arange(3 * 700, dtype=torch.float32).view(3, 700))
    assert bool((a.base[x.off - 4096:x.off] == 0xFF).all()) and bool((a.base[idx.off - 4096:idx.off] == G.SENTINEL).all())   # int operand: sentinel
    assert bool((G.as_bytes(y.tensor) == 0xFF).all()) and bool(torch.isnan(y.tensor).all())
    assert bool((a.base[y.off + y.nbytes:y.off + y.nbytes + y.trail] == G.SENTINEL).all())
    assert ws.nbytes == 2016 and bool((ws.payload[:1000] == 0).all()) and bool((ws.payload[1000:] == 0xFF).all())
    assert int(a.base[ws.off + ws.nbytes]) == G.SENTINEL                                        # the guard starts right behind the workspace


def test_untouched_arena_passes():
    a = _arena()[0]
    a.check()
    a.check()


def _flip(a, offset):
    a.base[offset] ^= 1


@pytest.mark.parametrize('which,where,side,first', [
    ('x', lambda b: b.off - 1, 'leading guard', -1),
    ('x', lambda b: b.off - b.guard, 'leading guard', -4096),
    ('y', lambda b: b.off + b.nbytes, 'trailing guard', 480),
    ('big', lambda b: b.off + b.nbytes + 17, 'trailing guard', 20017),
    ('x', lambda b: b.off + 5, 'input payload', 5),
    ('idx', lambda b: b.off + b.nbytes - 1, 'input payload', 27),
    ('ws', lambda b: b.off + b.nbytes + b.trail - 1, 'trailing guard', None),                  # the very last guard byte of the arena
])
def test_one_flipped_byte_is_reported_with_buffer_side_and_offset(which, where, side, first):
    a = _arena()[0]
    b = {q.name: q for q in a.buffers}[which]
    if first is None:
        first = b.nbytes + b.trail - 1
        assert where(b) == a.base.numel() - 1
    _flip(a, where(b))
    with pytest.raises(AssertionError) as e:
        a.check()
    msg = str(e.value)
    assert "buffer '%s'" % which in msg and side in msg, msg
    assert re.search(r': 1 byte\(s\), first at payload offset %d, last at payload offset %d$' % (first, first), msg), msg


def test_a_run_of_corrupted_bytes_reports_first_last_and_count():
    a, x, *_ = _arena()
    a.base[x.off + x.nbytes + 8:x.off + x.nbytes + 24:2] = 0                                    # 8 bytes, every other one
    with pytest.raises(AssertionError, match=r"buffer 'x' .*trailing guard changed: 8 byte\(s\), first at payload offset 8408, last at payload offset 8422"):
        a.check()


def test_inout_payload_may_change_its_guards_may_not():
    a, x, big, idx, io, y, ws = _arena()
    io.tensor.add_(1.0)
    y.tensor.zero_()
    ws.payload.fill_(3)
    a.check()
    _flip(a, io.off + io.nbytes)
    with pytest.raises(AssertionError, match="buffer 'param' .*trailing guard"):
        a.check()


@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16] + ([F8] if F8 is not None else []))
def test_one_element_past_an_input_poisons_a_reduction(dtype):
    """Why the guard byte of a float input is 0xFF: it is a NaN in all three operand types."""
    a = G.Arena('cpu')
    b = a.input(torch.ones(4, 33).to(dtype), 'x')
    a.commit()
    assert float(b.raw().float().sum()) == 4 * 33
    assert torch.isnan(b.raw(elements_past_end=1).float().sum())
    assert torch.isnan(b.raw(elements_past_end=1).float()[-1])


# ---------------------------------------------------------------------------------------------------- the header and the table
def test_roles_come_from_the_header():
    p = G.header_protos()
    assert p['vv_conv3d_k4s2_fwd'].params[0] == ('x', True, True) and p['vv_conv3d_k4s2_fwd'].params[4] == ('y', True, False)
    assert ('workspace', True, False) in p['vv_dense_fwd'].params and ('workspace_bytes', False, False) in p['vv_dense_fwd'].params
    launching = G.launching_entries(p)
    assert 'vv_adam_step' in launching and 'vv_pack_bits' in launching and len(launching) >= 70
    for name in ('vv_abi_version', 'vv_dense_workspace_bytes', 'vv_conv3d_k4s2_skip_supported', 'vv_object_pose_host', 'vv_convT3d_k4s2_whole_stats_blocks'):
        assert name not in launching
    for name, (query, _) in G.WORKSPACE_QUERY.items():
        assert name in launching and p[query].ret == 'size_t'
    for name, names in G.INOUT.items():
        assert set(names) <= {q[0] for q in p[name].params if q[1] and not q[2]}
    # every entry that takes a workspace it writes has its size query here (a const workspace is an input: vv_voxel_points_emit)
    takes = {n for n in launching if ('workspace', True, False) in p[n].params}
    assert takes - set(G.WORKSPACE_QUERY) <= {'vv_pr_curve_accumulate', 'vv_voxel_points_count', 'vv_object_pose'}


def test_every_launching_entry_has_a_row_or_an_exemption():
    T = importlib.import_module('test_gpu_guards')
    launching = set(G.launching_entries())
    covered = set().union(*(r.entries for r in T.ROWS))
    assert covered <= launching, covered - launching
    assert set(T.LEFT_OUT) <= launching, set(T.LEFT_OUT) - launching
    assert not covered & set(T.LEFT_OUT), covered & set(T.LEFT_OUT)
    missing = launching - covered - set(T.LEFT_OUT)
    assert not missing, 'entries of include/voxvae.h without a row in tests/test_gpu_guards.py or a reason in LEFT_OUT: %s' % sorted(missing)
    assert all(len(why) > 20 for why in T.LEFT_OUT.values())


def test_every_row_is_a_case_of_an_oracle_parity_test():
    T = importlib.import_module('test_gpu_guards')
    ids = [r.id for r in T.ROWS]
    assert len(ids) == len(set(ids))
    for r in T.ROWS:
        assert callable(r.test) and r.test.__name__.startswith('test_') and r.test.__module__.startswith('test_gpu_'), r.id
        named = set()
        for mark in getattr(r.test, 'pytestmark', []):          # the parity test's own parameter lists: the row must be one of its cases
            if mark.name != 'parametrize':
                continue
            names = [n.strip() for n in mark.args[0].split(',')] if isinstance(mark.args[0], str) else list(mark.args[0])
            assert set(names) <= set(r.case), '%s: no value for %s' % (r.id, names)
            case = tuple(r.case[n] for n in names)
            cases = [c if isinstance(c, tuple) else (c,) for c in mark.args[1]]
            assert case in cases, '%s: %s = %r is not a case of %s' % (r.id, names, case, r.test.__name__)
            named |= set(names)
        assert set(r.case) == named, '%s: %s are not parameters of %s' % (r.id, set(r.case) - named, r.test.__name__)
        assert r.tail.strip(), r.id                                 # every row says what makes it a tail (or that it is the B = 1 case)


def test_the_wgrad_forms_only_the_exact_tests_reach_have_rows():
    """A pitched A (lda != m) on the float32 and on the bf16 kernel, the single-channel bf16 kernel at its full tile (cout > 64) and
    source side 2 are launched by tests/test_gpu_wgrad_exact.py alone; each has a row, and each row is a case of that file's tables."""
    T = importlib.import_module('test_gpu_guards')
    WI = importlib.import_module('_wgrad_inputs')
    dense = [tuple(r.case.values()) for r in T.ROWS if r.test.__name__ == 'test_wgrad_dense_exact']
    conv = [tuple(r.case.values()) for r in T.ROWS if r.test.__name__ == 'test_wgrad_conv_exact']
    assert set(dense) <= set(WI.DENSE_CASES) and set(conv) <= set(WI.CONV_CASES)
    assert {WI.dense_route(c)[0] for c in dense if c[3] != c[1]} == {'f32', 'bf16'}
    assert any(WI.conv_route(c)[0] == 'bf16 one channel, full tile' for c in conv)
    assert {WI.conv_route(c)[0] for c in conv if c[1] == 2} == {'f32', 'bf16'}


# ------------------------------------------------------------ the recorder and the replayer, on a stand-in library of numpy "kernels"
class _FakeLib:
    """voxvae.lib's surface (ptr, call, load, HOOK_VARS) over two entries of the real header computed by numpy through raw host pointers;
    `bug` plants the faults the replayer must catch."""
    HOOK_VARS = ('VV_FAKE_FORM',)

    def __init__(self, bug=None):
        self.bug = bug

    @staticmethod
    def ptr(t):
        import ctypes
        return None if t is None else ctypes.c_void_p(t.data_ptr())

    def load(self):
        return self

    def call(self, name, *args):
        status = getattr(self, name)(*args)
        assert status == 0, (name, status)

    @staticmethod
    def _f32(p, n):
        import ctypes
        import numpy as np
        return np.ctypeslib.as_array(ctypes.cast(p, ctypes.POINTER(ctypes.c_float)), shape=(n,))

    def vv_transpose_f32(self, src, dst, rows, cols, stream):
        a, o = self._f32(src, rows * cols), self._f32(dst, rows * cols + 1)
        o[:rows * cols] = a.reshape(rows, cols).T.reshape(-1)
        if self.bug == 'store one past':
            o[rows * cols] = 1.0
        if self.bug == 'scribble on the input':
            a[3] = 0.0
        return 0

    def vv_wgrad_workspace_bytes(self, rows, m, n):
        return 4 * m * n

    def vv_wgrad_dense(self, a, g, dw, rows, m, n, lda, a_dtype, g_dtype, workspace, workspace_bytes, stream):
        if workspace_bytes < 4 * m * n:
            return G.VV_ERR_WORKSPACE
        A, Gm, ws = self._f32(a, rows * m).reshape(rows, m), self._f32(g, rows * n + 1), self._f32(workspace, workspace_bytes // 4 + 1)
        if self.bug == 'read the workspace first':
            ws[:m * n] += (A.T @ Gm[:rows * n].reshape(rows, n)).reshape(-1)
        elif self.bug == 'read one past':
            ws[:m * n] = (A.T @ Gm[:rows * n].reshape(rows, n)).reshape(-1) + Gm[rows * n]
        else:
            ws[:m * n] = (A.T @ Gm[:rows * n].reshape(rows, n)).reshape(-1)
        if self.bug == 'use what was announced':
            ws[m * n:workspace_bytes // 4] = 0
            ws[0] += ws[workspace_bytes // 4 - 1] * 0 + (workspace_bytes // 4 - m * n)
        self._f32(dw, m * n)[:] = ws[:m * n]
        return 0


def _record(bug, monkeypatch):
    L = _FakeLib()
    rec = G.Recorder(L).install(monkeypatch)
    x = torch.arange(15, dtype=torch.float32).view(3, 5)
    y = torch.full((5, 3), float('nan'))
    L.call('vv_transpose_f32', L.ptr(x), L.ptr(y), 3, 5, None)
    assert torch.equal(y, x.T)
    a, g, dw = torch.randn(6, 4), torch.randn(6, 2), torch.empty(4, 2)
    ws = torch.empty(64, dtype=torch.uint8)
    L.call('vv_wgrad_dense', L.ptr(a), L.ptr(g), L.ptr(dw), 6, 4, 2, 4, 0, 0, L.ptr(ws), ws.numel(), None)
    assert [c.name for c in rec.calls] == ['vv_transpose_f32', 'vv_wgrad_dense']
    L.bug = bug
    return L, rec.units()


def test_replay_of_a_sound_library_passes(monkeypatch):
    L, units = _record(None, monkeypatch)
    for u in units:
        G.guard_unit(L, u, 'cpu')


@pytest.mark.parametrize('bug,unit,message', [
    ('store one past', 0, r"buffer 'vv_transpose_f32.out' \(output, 60 bytes\): trailing guard changed: 4 byte\(s\), first at payload offset 60, last at payload offset 63"),
    ('scribble on the input', 0, r"buffer 'vv_transpose_f32.in' \(input, 60 bytes\): input payload changed: 2 byte\(s\), first at payload offset 14, last at payload offset 15"),     # 3.0f -> 0.0f: its two high bytes
    ('read one past', 1, r'vv_wgrad_dense.dw: guarded run against the plain run: 8 element\(s\) differ'),
    ('read the workspace first', 1, r'vv_wgrad_dense.dw: workspace pre-filled with 0xFF against the plain run'),
    ('use what was announced', 1, r'vv_wgrad_dense.dw: workspace announced as twice its size'),
])
def test_replay_catches_each_planted_fault(bug, unit, message, monkeypatch):
    L, units = _record(bug, monkeypatch)
    with pytest.raises(AssertionError, match=message):
        G.guard_unit(L, units[unit], 'cpu')
