"""The image encoder on the HIP 2D convolution (csrc/conv2d.hip; include/voxvae.h `vv_conv2d_fwd`, `vv_maxpool2d_same_fwd`).

`Conv2dChain(module)` runs the inference form of a `src.net_core.darknet` module -- Darknet19, head2D, Darknet53 or Darknet53Tiny -- as
a walk over its layer plan: Conv2D 'same' -> folded BatchNormalization -> activation per layer, MaxPool2D(2, 2, 'same') between the
stages; for the Darknet53 family also the stride-2 convolution, the residual add in the convolution's epilogue (vv_conv2d_ex_fwd),
MaxPool2D(2, 1, 'same') (vv_maxpool2d_s1_same_fwd) and the tuple of outputs.  The torch module
stays the owner of the parameters (training, `.losses`, `save_weights` / `load_weights` are its own); the chain packs the weights FROM
it (torch OIHW -> the ABI's [k,k,cin,cout] -> vv_pack_conv2d), folds the BN with vv_fold_bn (Keras epsilon 1e-3, the module's), and
packs again whenever a parameter or a BN buffer has changed since (the sum of the tensors' `_version` counters: an optimizer step,
load_weights and a training-mode forward all bump one).

Operand type: `voxvae.default_dtype()` when the chain is built -- 'f32' (v_mfma_f32_32x32x2_f32) or 'bf16' (bf16 operands and
activations, f32 accumulation, one rounding per layer).  'fp8' runs THIS stage in bf16: there are no fp8 2D kernels.  The last layer of a
chain always stores float32, which is what the next consumer takes (the head, voxvae.detect, the model classes).

The engine is opt-in: `voxvae.set_image_engine('hip')`, VOXVAE_IMAGE_ENGINE=hip, or `engine='hip'` at the builders.  There is no
fallback: without a GPU a 'hip' chain is a VoxVaeError.
"""
import ctypes

import numpy as np
import torch

import voxvae

from . import lib as L

BN_EPS = 1e-3


def _require_gpu():
    if not torch.cuda.is_available():
        raise L.VoxVaeError("no HIP device visible: the image engine 'hip' runs on MI355X only (no CPU fallback; engine='torch' is the stock path)")


def operand_dtype(name=None):
    """The operand type of the 2D stage for a package dtype name: 'fp8' -> bf16."""
    name = voxvae.default_dtype() if name is None else name
    return L.VV_F32 if name in ('f32', 'fp32', 'float32') else L.VV_BF16


def keras_kernel(weight):
    """torch Conv2d weight [cout, cin, k, k] -> the ABI's Keras layout [k, k, cin, cout], contiguous float32."""
    return weight.detach().permute(2, 3, 1, 0).contiguous().float()


def version_key(tensors):
    """Changes whenever one of `tensors` is written in place (optimizer step, load_state_dict's copy_, BN's running statistics)."""
    return sum(int(t._version) for t in tensors)


def module_plan(module):
    """The layer plan of a darknet module in execution order.  Darknet19 / head2D: ('conv', conv, bn or None, act name, alpha) and
    ('pool',).  Darknet53 / Darknet53Tiny add ('conv', conv, bn, act, alpha, stride, res) -- stride 2 and / or `res`, the index of the
    step whose output is added behind the activation -- and ('pool1',) = MaxPool2D(2, 1, 'same'); `plan_taps` names their extra outputs."""
    import torch.nn as nn
    from src.net_core import darknet as D
    plan = []

    def act_of(m):
        a = m.act
        if isinstance(a, nn.LeakyReLU):
            return 'lrelu', float(a.negative_slope)
        if isinstance(a, nn.ELU):
            return 'elu', 0.0
        if isinstance(a, nn.ReLU):
            return 'relu', 0.0
        return None, 0.0

    res = getattr(module, '_res', {})
    for i, m in enumerate(module.layers):
        if isinstance(m, nn.MaxPool2d):
            plan.append(('pool',))
        elif isinstance(m, D._Pool1Same):
            plan.append(('pool1',))
        elif isinstance(m, D._ConvBNAct):
            step = ('conv', m.conv, m.bn) + act_of(m)
            if m.stride != 1 or i in res:
                step += (m.stride, res.get(i))
            plan.append(step)
        else:
            raise L.VoxVaeError('Conv2dChain: no HIP form of %r' % type(m).__name__)
    last = getattr(module, 'last', None)
    if last is not None:
        plan.append(('conv', last, None, None, 0.0))
    return plan


def plan_taps(module):
    """Steps of module_plan(module) whose outputs leave the module in front of the last one's; None for a module with ONE output."""
    taps = getattr(module, '_taps', None)
    return None if taps is None else list(taps)


def step_stride_res(step):
    return (step[5], step[6]) if len(step) > 5 else (1, None)


def out_grid(kind, rows, cols, stride=1):
    """The output grid of a step on a rows x cols input: ceil for the stride-2 pool, floor for the stride-2 convolution."""
    if kind == 'pool':
        return (rows + 1) // 2, (cols + 1) // 2
    if kind == 'conv' and stride == 2:
        return rows // 2, cols // 2
    return rows, cols


def plan_shapes(plan, rows, cols):
    """[(kind, rows, cols, cin, cout, k)] with the INPUT grid of each step; the last entry's output grid follows from its kind (and, for a
    convolution, its stride: `out_grid`)."""
    out = []
    for step in plan:
        if step[0] in ('pool', 'pool1'):
            out.append((step[0], rows, cols, out[-1][4], out[-1][4], 2))
            rows, cols = out_grid(step[0], rows, cols)
        else:
            conv = step[1]
            out.append(('conv', rows, cols, conv.in_channels, conv.out_channels, conv.kernel_size[0]))
            rows, cols = out_grid('conv', rows, cols, step_stride_res(step)[0])
    return out


def _up32(n):
    return (n + 31) // 32 * 32


class _Layer:
    __slots__ = ('k', 'cin', 'cout', 'act', 'alpha', 'packed', 'scale', 'shift', 'stride', 'res')


class Conv2dChain:
    def __init__(self, module, dtype=None):
        _require_gpu()
        self.module = module
        self.dt = operand_dtype(dtype)
        self.tdt = torch.float32 if self.dt == L.VV_F32 else torch.bfloat16
        self.plan = module_plan(module)
        self.taps = plan_taps(module)
        self.device = next(module.parameters()).device
        if self.device.type != 'cuda':
            raise L.VoxVaeError("the image engine 'hip' needs the module on the GPU, not on %s" % self.device)
        # The channels each step RUNS with.  A width that is no multiple of 32 and feeds another layer (Darknet53Tiny's first, 16) is
        # padded to one: kernel, scale and shift are zero there, so the extra channels are exactly 0 behind every activation, and the
        # next kernel's input channels are zero-padded to match.
        lib, self.widths, ch = L.load(), [], None
        for i, step in enumerate(self.plan):
            if step[0] == 'conv':
                c = step[1]
                cin = c.in_channels if ch is None else ch
                ch = c.out_channels if i == len(self.plan) - 1 else _up32(c.out_channels)
                stride = step_stride_res(step)[0]
                if cin < c.in_channels or not lib.vv_conv2d_ex_supported(c.kernel_size[0], stride, cin, ch, self.dt, self.dt):
                    raise L.VoxVaeError('vv_conv2d_ex_fwd takes no k=%d stride %d %d -> %d layer' % (c.kernel_size[0], stride, c.in_channels, c.out_channels))
                self.widths.append((cin, ch))
            else:
                self.widths.append((ch, ch))
        self._tensors = [t for t in list(module.parameters()) + list(module.buffers())]
        self._key = None
        self.layers = None
        self._bufs = {}

    # ------------------------------------------------------------------------------------------------------------ weights
    def stale(self):
        return self._key != version_key(self._tensors)

    def _stream(self):
        return ctypes.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    def pack(self):
        key, st, layers = version_key(self._tensors), self._stream(), []
        for step, (cin, cout) in zip(self.plan, self.widths):
            if step[0] != 'conv':
                layers.append(None)
                continue
            _, conv, bn, act, alpha = step[:5]
            l = _Layer()
            l.k, l.cin, l.cout, l.act, l.alpha = conv.kernel_size[0], cin, cout, L.ACT[act], alpha
            l.stride, l.res = step_stride_res(step)
            wk = keras_kernel(conv.weight)
            pad = (0, cout - conv.out_channels, 0, cin - conv.in_channels)
            if any(pad):
                wk = torch.nn.functional.pad(wk, pad).contiguous()
            l.packed = torch.empty(L.load().vv_conv2d_packed_bytes(l.k, l.cin, l.cout, self.dt), dtype=torch.uint8, device=self.device)
            L.call('vv_pack_conv2d', L.ptr(wk), L.ptr(l.packed), l.k, l.cin, l.cout, self.dt, st)
            if bn is None:
                l.scale = l.shift = None
            else:
                n = conv.out_channels
                l.scale = torch.zeros(l.cout, dtype=torch.float32, device=self.device)
                l.shift = torch.zeros_like(l.scale)
                g, b, mu, var = (t.detach().float().contiguous() for t in (bn.weight, bn.bias, bn.running_mean, bn.running_var))
                L.call('vv_fold_bn', L.ptr(g), L.ptr(b), L.ptr(mu), L.ptr(var), None, float(bn.eps), L.ptr(l.scale), L.ptr(l.shift), n, 1, st)
            layers.append(l)
        self.layers, self._key = layers, key

    # ------------------------------------------------------------------------------------------------------------ forward
    def _steps(self, rows, cols):
        """plan_shapes with the channels the chain runs with: [(kind, rows, cols, cin, cout, k)], input grids."""
        return [(kind, r, c) + w + (k,) for (kind, r, c, _, _, k), w in zip(plan_shapes(self.plan, rows, cols), self.widths)]

    def _buffers(self, shape):
        """Activation and workspace buffers of one input shape, made once."""
        if shape in self._bufs:
            return self._bufs[shape]
        B, rows, cols, _ = shape
        lib, acts, need = L.load(), [], 0
        steps = self._steps(rows, cols)
        for i, ((kind, r, c, cin, cout, k), step) in enumerate(zip(steps, self.plan)):
            last = i == len(steps) - 1
            stride = step_stride_res(step)[0] if kind == 'conv' else 1
            if kind == 'conv':
                need = max(need, lib.vv_conv2d_ex_workspace_bytes(B, r, c, k, stride, cin, cout, self.dt))
            r, c = out_grid(kind, r, c, stride)
            acts.append(torch.empty(B, r, c, cout, dtype=torch.float32 if last else self.tdt, device=self.device))
        ws = torch.empty(max(need, 16), dtype=torch.uint8, device=self.device)
        self._bufs[shape] = (steps, acts, ws, need)
        return self._bufs[shape]

    def max_batch(self, rows, cols):
        """The largest batch whose every tensor stays within 2^31 - 1 elements (vv_conv2d_fwd's limit)."""
        widest = 1
        for kind, r, c, cin, cout, k in self._steps(rows, cols):
            widest = max(widest, r * c * max(cin, cout))
        return max(1, (2 ** 31 - 1) // widest)

    def __call__(self, x, layer_outputs=None):
        """x [B,R,C,Cin] on the device: float32 for an image (Cin = 3), else float32 or the chain's operand type.  -> float32 [B,R',C',Cout],
        or for a module with taps (Darknet53, Darknet53Tiny) the tuple of float32 tensors its forward returns: the taps are exact
        conversions of the operand-type activations.  `layer_outputs`: a list that receives every step's output tensor (tests); a padded
        layer's tensor comes with its padding."""
        if self.stale():
            self.pack()
        B = int(x.shape[0])
        cap = self.max_batch(int(x.shape[1]), int(x.shape[2]))
        if B > cap:
            parts = [self(x[i:i + cap]) for i in range(0, B, cap)]
            return torch.cat(parts, 0) if self.taps is None else tuple(torch.cat(p, 0) for p in zip(*parts))
        first = next(l for l in self.layers if l is not None)
        h = x.contiguous()
        h = h.float() if first.cin == 3 else h.to(self.tdt)
        steps, acts, ws, need = self._buffers(tuple(h.shape))
        st = self._stream()
        for i, ((kind, r, c, cin, cout, k), l, y) in enumerate(zip(steps, self.layers, acts)):
            if kind == 'pool':
                L.call('vv_maxpool2d_same_fwd', L.ptr(h), L.ptr(y), B, r, c, cin, self.dt, st)
            elif kind == 'pool1':
                L.call('vv_maxpool2d_s1_same_fwd', L.ptr(h), L.ptr(y), B, r, c, cin, self.dt, st)
            else:
                odt = L.VV_F32 if y.dtype == torch.float32 else L.VV_BF16
                if l.stride == 1 and l.res is None:
                    L.call('vv_conv2d_fwd', L.ptr(h), L.ptr(l.packed), L.ptr(l.scale), L.ptr(l.shift), L.ptr(y), B, r, c, cin, cout, k, l.act,
                           float(l.alpha), self.dt, odt, L.ptr(ws) if need else None, need, st)
                else:
                    res = None if l.res is None else acts[l.res]          # every step keeps its own buffer: still what that step wrote
                    L.call('vv_conv2d_ex_fwd', L.ptr(h), L.ptr(l.packed), L.ptr(l.scale), L.ptr(l.shift), L.ptr(res), L.ptr(y), B, r, c, cin, cout, k,
                           l.stride, l.act, float(l.alpha), self.dt, odt, L.ptr(ws) if need else None, need, st)
            if layer_outputs is not None:
                layer_outputs.append(y)
            h = y
        if self.taps is None:
            return h.clone()          # the cached buffer is reused by the next call
        # copies, like the clone: the cached buffers are reused by the next call.  bf16 -> float32 is exact
        taps = tuple(acts[t][..., :self.plan[t][1].out_channels].to(torch.float32, copy=True).contiguous() for t in self.taps)
        return taps + (h.clone(),)


def max_over_positions(x):
    """head2D last_pooling='max' on the float32 head output [B,R,C,N] -> [B,N] (vv_max_over_positions)."""
    B, R, C, N = (int(v) for v in x.shape)
    out = torch.empty(B, N, dtype=torch.float32, device=x.device)
    L.call('vv_max_over_positions', L.ptr(x), L.ptr(out), B, R * C, N, ctypes.c_void_p(torch.cuda.current_stream(x.device).cuda_stream))
    return out
