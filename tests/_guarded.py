"""Memory-discipline test infrastructure (torch only): guard-banded buffers and a replayer that puts ANY recorded C-ABI call onto them.

Arena      buffers laid out [guard | payload | guard] inside ONE torch.uint8 allocation, so a near overrun stays inside memory the
           test owns.  A guard is max(4096, bytes of one sample of the buffer) rounded up to 512 bytes (a sample = index 0 of the
           tensor: a batch element of an activation, a row of a 2-D operand), so a tail tile that handles sample B or row M lands
           entirely in the guard; the payload start keeps the 512-byte alignment every production buffer has.
             input(t)              payload = a copy of t.  Guards 0xFF: a NaN in float32, bfloat16 and e4m3fn alike, so a guard byte
                                   that reaches an accumulator poisons the result.  Integer buffers (int32 / int64 indices, packed
                                   bits) have no NaN: their guards hold the sentinel.
             input(t, inout=True)  the same, exempt from the payload check (Adam's param / m / v, in-place sigmoid, moving statistics).
             output(shape, dtype)  payload 0xFF (an unwritten float element is a NaN), guards the sentinel 0xA5.
             workspace(n, fill)    payload `fill`, then `extra` bytes of 0xFF that still belong to the payload, guards the sentinel;
                                   the trailing guard starts right behind the last payload byte.
           check(): every guard byte-identical to what it was, every input payload byte-identical to what was copied in; an
           AssertionError names the buffer, the side, the first and last corrupted byte offset relative to the payload, and the count.
Recorder   wraps voxvae.lib's ptr() / call() while an existing oracle-parity test runs: every launching call is kept with its
           tensors, their bytes before the call, the bytes the call left in its outputs, and the VV_* overrides it ran under.
guard_unit replays a recorded call on an Arena and asserts the memory-discipline contract of include/voxvae.h.
Which argument is read, written or scratch comes from the header itself (const-ness, the name `workspace`)."""
import ctypes
import os
import re

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, 'include', 'voxvae.h')
POISON, SENTINEL = 0xFF, 0xA5
ALIGN, MIN_GUARD = 512, 4096
VV_ERR_WORKSPACE = -5
_FLOATS = {torch.float32, torch.bfloat16, torch.float16, torch.float64} | ({torch.float8_e4m3fn} if hasattr(torch, 'float8_e4m3fn') else set())


def _up(n, a=ALIGN):
    return (n + a - 1) // a * a


def guard_bytes(sample_bytes):
    return _up(max(MIN_GUARD, sample_bytes))


def sample_bytes(t):
    n = t.numel() * t.element_size()
    return n // t.shape[0] if t.dim() >= 1 and t.shape[0] > 0 else n


def as_bytes(t):
    """Flat uint8 view of a contiguous tensor's elements."""
    return t.reshape(-1).view(torch.uint8)


class Buffer:
    def __init__(self, arena, name, kind, nbytes, guard, guard_fill, dtype=torch.uint8, shape=None, source=None, fill=POISON, extra=0):
        self.arena, self.name, self.kind, self.nbytes, self.guard, self.guard_fill = arena, name, kind, nbytes, guard, guard_fill
        self.dtype, self.shape, self.source, self.fill, self.extra = dtype, shape, source, fill, extra
        self.off = self.trail = None                  # payload offset / trailing guard length, set by commit()
        self.pristine = None

    @property
    def payload(self):
        """The payload as flat bytes (a view into the arena)."""
        return self.arena.base[self.off:self.off + self.nbytes]

    @property
    def tensor(self):
        """The payload as the tensor the entry sees."""
        t = self.payload.view(self.dtype)
        return t if self.shape is None else t.view(self.shape)

    @property
    def address(self):
        return self.arena.base.data_ptr() + self.off

    @property
    def ptr(self):
        return ctypes.c_void_p(self.address)

    def raw(self, elements_past_end=0):
        """Payload plus `elements_past_end` elements of the trailing guard, in the buffer's type: what an overreading kernel consumes."""
        n = self.nbytes + elements_past_end * torch.empty(0, dtype=self.dtype).element_size()
        assert n <= self.nbytes + self.trail
        return self.arena.base[self.off:self.off + n].view(self.dtype)


class Arena:
    def __init__(self, device):
        self.device, self.buffers, self.base = torch.device(device), [], None

    def _add(self, b):
        assert self.base is None, 'declare every buffer before commit()'
        self.buffers.append(b)
        return b

    def input(self, t, name, inout=False):
        assert t.is_contiguous(), name
        fill = POISON if t.dtype in _FLOATS else SENTINEL          # integer operands: no NaN to poison with, the sentinel instead
        return self._add(Buffer(self, name, 'inout' if inout else 'input', t.numel() * t.element_size(), guard_bytes(sample_bytes(t)), fill,
                                t.dtype, tuple(t.shape), source=t))

    def output(self, shape, dtype, name):
        shape = tuple(shape)
        t = torch.empty(shape, dtype=dtype, device='meta')
        return self._add(Buffer(self, name, 'output', t.numel() * t.element_size(), guard_bytes(sample_bytes(t)), SENTINEL, dtype, shape))

    def workspace(self, nbytes, fill, name='workspace', extra=0):
        return self._add(Buffer(self, name, 'workspace', nbytes + extra, guard_bytes(0), SENTINEL, fill=fill, extra=extra))

    def commit(self):
        off = 0
        for b in self.buffers:
            b.off = off + b.guard
            end = b.off + b.nbytes + b.guard
            b.trail = _up(end) - (b.off + b.nbytes)                   # the trailing guard runs up to the next 512-byte boundary
            off = _up(end)
        raw = torch.empty(off + ALIGN, dtype=torch.uint8, device=self.device)
        shift = (-raw.data_ptr()) % ALIGN
        self.base = raw[shift:shift + off]
        assert self.base.data_ptr() % ALIGN == 0
        for b in self.buffers:
            self.base[b.off - b.guard:b.off] = b.guard_fill
            self.base[b.off + b.nbytes:b.off + b.nbytes + b.trail] = b.guard_fill
            if b.source is not None:
                b.pristine = as_bytes(b.source).to(self.device).clone()
                b.payload.copy_(b.pristine)
            else:
                b.payload.fill_(b.fill)
                if b.extra:
                    b.payload[b.nbytes - b.extra:] = POISON
        return self

    @staticmethod
    def _report(b, side, bad, origin):
        idx = bad.nonzero().reshape(-1)
        if idx.numel():
            first, last = int(idx[0]) + origin, int(idx[-1]) + origin
            raise AssertionError("buffer '%s' (%s, %d bytes): %s changed: %d byte(s), first at payload offset %d, last at payload offset %d"
                                 % (b.name, b.kind, b.nbytes, side, idx.numel(), first, last))

    def check(self):
        """Call after the device is synchronised."""
        for b in self.buffers:
            self._report(b, 'leading guard', self.base[b.off - b.guard:b.off] != b.guard_fill, -b.guard)
            self._report(b, 'trailing guard', self.base[b.off + b.nbytes:b.off + b.nbytes + b.trail] != b.guard_fill, b.nbytes)
            if b.kind == 'input':
                self._report(b, 'input payload', b.payload != b.pristine, 0)


# ------------------------------------------------------------------------------------------------------- the header's view of a call
class Proto:
    def __init__(self, name, ret, params):
        self.name, self.ret, self.params = name, ret, params     # params: (name, is_pointer, is_const)

    def index(self, pname):
        return [p[0] for p in self.params].index(pname)


def header_protos(path=HEADER):
    src = re.sub(r'/\*.*?\*/', '', open(path).read(), flags=re.S)
    out = {}
    for m in re.finditer(r'\b(int|size_t|const char \*)\s*(vv_\w+)\s*\(([^;]*?)\)\s*;', src, flags=re.S):
        params = []
        for a in m.group(3).split(','):
            a = ' '.join(a.split())
            if a and a != 'void':
                params.append((re.findall(r'\w+', a)[-1], '*' in a, a.startswith('const')))
        out[m.group(2)] = Proto(m.group(2), m.group(1), params)
    return out


def launching_entries(protos=None):
    """The entries of the header that put a kernel on a stream."""
    protos = protos or header_protos()
    return sorted(n for n, p in protos.items() if p.ret == 'int' and any(q[0] == 'stream' for q in p.params))


# pointers an entry both reads and writes (everything else non-const is a pure output); an argument passed twice, once const, is found
# at run time (in-place vv_sigmoid_f32)
INOUT = {'vv_adam_step': ('param', 'm', 'v'), 'vv_bn_train_stats': ('moving_mean', 'moving_var'),
         'vv_bn_finalize_stats': ('moving_mean', 'moving_var')}
# the one entry that runs behind another on the SAME workspace (the entry on the right writes it first): replayed alone, where its
# workspace must be write-before-read like any other, and as that pair, with the fills applied to the pair
WORKSPACE_FROM = {'vv_convT3d_final_bce_metrics_fwd': 'vv_convT3d_final_bce_fwd'}


def _rows(a):
    return a['batch'] * (a['side'] // 2) ** 3


# entry -> (size query, its arguments from the call's own)
WORKSPACE_QUERY = {
    'vv_conv3d_k4s2_fwd': ('vv_conv3d_k4s2_workspace_bytes', lambda a: (a['batch'], a['side'], a['cin'], a['cout'], a['dtype'])),
    'vv_conv3d_k4s2_fwd_io': ('vv_conv3d_k4s2_workspace_bytes', lambda a: (a['batch'], a['side'], a['cin'], a['cout'], a['dtype'])),
    'vv_convT3d_k4s2_fwd': ('vv_convT3d_k4s2_workspace_bytes', lambda a: (a['batch'], a['side'], a['cin'], a['cout'], a['dtype'])),
    'vv_convT3d_k4s2_fwd_io': ('vv_convT3d_k4s2_workspace_bytes', lambda a: (a['batch'], a['side'], a['cin'], a['cout'], a['dtype'])),
    'vv_conv3d_k4s2_pos_fwd': ('vv_conv3d_k4s2_pos_workspace_bytes', lambda a: (a['batch'], a['cin'], a['cout'])),
    'vv_convT3d_k4s2_pos_fwd': ('vv_convT3d_k4s2_pos_workspace_bytes', lambda a: (a['batch'], a['cin'], a['cout'])),
    'vv_dense_fwd': ('vv_dense_workspace_bytes', lambda a: (a['m'], a['n'], a['k'], a['dtype'])),
    'vv_latent_tail_fwd': ('vv_latent_tail_workspace_bytes', lambda a: (a['batch'], a['K5'], a['E'], a['n1'])),
    'vv_conv_pos_latent_tail_fwd': ('vv_conv_pos_latent_tail_workspace_bytes', lambda a: (a['batch'], a['cin4'], a['cout4'], a['E'])),
    'vv_convT3d_final_bce_fwd': ('vv_convT3d_final_bce_workspace_bytes', lambda a: (a['batch'], a['side'])),
    'vv_convT3d_final_bce_metrics_fwd': ('vv_convT3d_final_bce_workspace_bytes', lambda a: (a['batch'], a['side'])),
    'vv_convT3d_final_mean_fwd': ('vv_convT3d_final_mean_workspace_bytes', lambda a: (a['objects'], a['samples'], a['side'])),
    'vv_bn_train_stats': ('vv_bn_workspace_bytes', lambda a: (a['rows'], a['channels'])),
    'vv_bn_act_bwd': ('vv_bn_workspace_bytes', lambda a: (a['rows'], a['channels'])),
    'vv_wgrad_dense': ('vv_wgrad_workspace_bytes', lambda a: (a['rows'], a['m'], a['n'])),
    'vv_wgrad_conv_k4s2': ('vv_wgrad_workspace_bytes', lambda a: (_rows(a), 64 * a['cin'], a['cout'])),
}


# ------------------------------------------------------------------------------------------------------------------- recording
class TensorArg:
    def __init__(self, pname, const, tensor):
        self.pname, self.const, self.tensor, self.key = pname, const, tensor, tensor.data_ptr()
        self.before = self.after = None


class Call:
    def __init__(self, name, proto, args, env):
        self.name, self.proto, self.args, self.env = name, proto, args, env

    def tensor_args(self):
        return [a for a in self.args if isinstance(a, TensorArg)]

    def scalars(self):
        return {p[0]: (a.value if hasattr(a, 'value') else a) for p, a in zip(self.proto.params, self.args) if not p[1]}


class Recorder:
    """Stands in for voxvae.lib's ptr() and call().  Every tensor whose pointer was taken is kept alive, so an address names one tensor."""

    def __init__(self, L, protos=None):
        self.L, self.protos, self.tensors, self.calls = L, protos or header_protos(), {}, []
        self._ptr, self._call = L.ptr, L.call
        self.launching = set(launching_entries(self.protos))

    def install(self, monkeypatch):
        monkeypatch.setattr(self.L, 'ptr', self.ptr)
        monkeypatch.setattr(self.L, 'call', self.call)
        return self

    def ptr(self, t):
        if t is not None:
            self.tensors[t.data_ptr()] = t
        return self._ptr(t)

    def call(self, name, *args):
        if name not in self.launching:
            return self._call(name, *args)
        proto, rec = self.protos[name], []
        for (pname, is_ptr, const), a in zip(proto.params, args):
            t = self.tensors.get(a.value) if is_ptr and isinstance(a, ctypes.c_void_p) else None
            if t is not None and t.is_contiguous() and pname != 'stream':
                ta = TensorArg(pname, const, t)
                if pname != 'workspace':
                    ta.before = as_bytes(t).clone()
                rec.append(ta)
            else:
                rec.append(a)
        self._call(name, *args)
        for ta in rec:
            if isinstance(ta, TensorArg) and not ta.const and ta.pname != 'workspace':
                ta.after = as_bytes(ta.tensor).clone()
        call = Call(name, proto, rec, {v: os.environ[v] for v in self.L.HOOK_VARS if v in os.environ})
        # a device pointer that did not come from ptr() (the engine's own buffers, a pointer moved by hand) cannot be re-homed
        call.resolved = all(isinstance(a, TensorArg) or getattr(a, 'value', None) is None
                            for (pname, is_ptr, _), a in zip(proto.params, rec) if is_ptr and pname != 'stream')
        self.calls.append(call)

    def units(self, skip=()):
        """Recorded calls as replay units: one call each; an entry that follows WORKSPACE_FROM's producer on the same workspace is replayed
        behind it as a pair as well (one guarded workspace, the fills applied to the pair).  Calls with a pointer of unknown extent are
        left out."""
        out = []
        for i, c in enumerate(self.calls):
            if c.name in skip or not c.resolved:
                continue
            out.append([c])
            src = WORKSPACE_FROM.get(c.name)
            if src:
                ws = [a.key for a in c.tensor_args() if a.pname == 'workspace']
                prev = [d for d in self.calls[:i] if d.resolved and d.name == src and [a.key for a in d.tensor_args() if a.pname == 'workspace'] == ws]
                if prev:
                    out.append([prev[-1], c])
        return out


# --------------------------------------------------------------------------------------------------------------------- replay
class _Env:
    def __init__(self, L, env):
        self.L, self.env = L, env

    def __enter__(self):
        self.saved = {v: os.environ.get(v) for v in self.L.HOOK_VARS}
        for v in self.L.HOOK_VARS:
            os.environ.pop(v, None)
        os.environ.update(self.env)

    def __exit__(self, *exc):
        for v, x in self.saved.items():
            os.environ.pop(v, None)
            if x is not None:
                os.environ[v] = x


def workspace_need(L, call):
    q = WORKSPACE_QUERY.get(call.name)
    assert q is not None, 'no workspace size query known for %s' % call.name
    with _Env(L, call.env):
        return int(getattr(L.load(), q[0])(*q[1](call.scalars())))


def replay(L, unit, device, ws_fill=0x00, ws_mode='exact'):
    """Run the unit's calls on one fresh Arena.  ws_mode: 'exact' = a workspace of exactly the queried size; 'double' = the same buffer
    announced as twice that plus 16 bytes, the excess 0xFF; 'short' = announced one byte short.  -> (arena, {address: Buffer}, status)."""
    arena, bufs, announced = Arena(device), {}, {}
    for call in unit:
        inout = INOUT.get(call.name, ())
        const_keys = {a.key for a in call.tensor_args() if a.const}
        inout_keys = {a.key for a in call.tensor_args() if a.pname in inout or (not a.const and a.pname != 'workspace' and a.key in const_keys)}
        for a in call.tensor_args():
            if a.key in bufs:
                continue
            name = '%s.%s' % (call.name, a.pname)
            if a.pname == 'workspace':
                need = workspace_need(L, call)
                extra = need + 16 if ws_mode == 'double' else 0
                bufs[a.key] = arena.workspace(need, ws_fill, name, extra)
                announced[a.key] = need + extra - (1 if ws_mode == 'short' else 0)
            elif a.key in inout_keys:
                bufs[a.key] = arena.input(a.before.view(a.tensor.dtype).view(a.tensor.shape), name, inout=True)
            elif a.const:
                bufs[a.key] = arena.input(a.before.view(a.tensor.dtype).view(a.tensor.shape), name)
            else:
                bufs[a.key] = arena.output(a.tensor.shape, a.tensor.dtype, name)
    arena.commit()
    status = 0
    for call in unit:
        args = []
        for (pname, _, _), a in zip(call.proto.params, call.args):
            if isinstance(a, TensorArg):
                args.append(bufs[a.key].ptr)
            elif pname == 'workspace_bytes' and any(t.pname == 'workspace' for t in call.tensor_args()):
                args.append(announced[[t.key for t in call.tensor_args() if t.pname == 'workspace'][0]])
            else:
                args.append(a)
        with _Env(L, call.env):
            status = getattr(L.load(), call.name)(*args)
        if status != 0:
            break
    if arena.device.type == 'cuda':
        torch.cuda.synchronize()
    return arena, bufs, status


def expected_outputs(unit):
    """{address: (name, dtype, bytes the plain run left)} for everything the unit writes."""
    out = {}
    for call in unit:
        for a in call.tensor_args():
            if a.after is not None:
                out[a.key] = ('%s.%s' % (call.name, a.pname), a.tensor.dtype, a.after)
    return out


def assert_same_bits(name, dtype, got, want, what):
    """Raw bytes equal.  Where they differ the element must be unwritten on both sides: 0xFF.. in the guarded run and a NaN the plain
    run's own pre-fill left."""
    if torch.equal(got, want):
        return
    size = torch.empty(0, dtype=dtype).element_size()
    diff = (got != want).view(-1, size).any(1)
    untouched = (got.view(-1, size) == POISON).all(1)
    plain_nan = torch.isnan(want.view(dtype).float()) if dtype in _FLOATS else torch.zeros_like(diff)
    bad = (diff & ~(untouched & plain_nan)).nonzero().reshape(-1)
    assert bad.numel() == 0, '%s: %s: %d element(s) differ bit for bit, first at element %d, last at element %d' % (
        name, what, bad.numel(), int(bad[0]), int(bad[-1]))


def written(bufs, unit):
    return {k: bufs[k].payload.clone() for k in expected_outputs(unit)}


def guard_unit(L, unit, device='cuda:0'):
    """The memory-discipline contract for one recorded call (see include/voxvae.h), against the plain run the parity test checked:
    guards and inputs untouched, outputs bit-identical, a second run bit-identical, and for a workspace entry: the result independent of
    what the workspace held (0x00 / 0xFF) and of an announced size beyond the minimum, one byte short refused before any launch."""
    want = expected_outputs(unit)
    what = unit[-1].name
    has_ws = any(a.pname == 'workspace' for c in unit for a in c.tensor_args())

    def run(fill, mode, label):
        arena, bufs, status = replay(L, unit, device, fill, mode)
        assert status == 0, '%s: %s returned %d' % (what, label, status)
        arena.check()
        got = written(bufs, unit)
        for k, (name, dtype, exp) in want.items():
            assert_same_bits(name, dtype, got[k], exp, label + ' against the plain run')
        return got

    first = run(0x00, 'exact', 'guarded run')
    second = run(0x00, 'exact', 'second guarded run')
    for k, (name, dtype, _) in want.items():
        assert torch.equal(first[k], second[k]), '%s: two guarded runs differ' % name
    if not has_ws:
        return
    run(POISON, 'exact', 'workspace pre-filled with 0xFF')
    run(0x00, 'double', 'workspace announced as twice its size + 16, excess 0xFF')
    if workspace_need(L, unit[0]) > 0:
        arena, bufs, status = replay(L, unit, device, 0x00, 'short')
        assert status == VV_ERR_WORKSPACE, '%s: a workspace one byte short returned %d, not VV_ERR_WORKSPACE' % (what, status)
        arena.check()
        for k, b in bufs.items():
            if b.kind == 'output':
                assert bool((b.payload == POISON).all()), '%s: refused for its workspace, yet %s was written' % (what, b.name)
