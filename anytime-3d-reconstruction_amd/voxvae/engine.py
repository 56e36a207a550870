"""Device-side engines for the two sub-models of the hot path.

`EncoderEngine` / `DecoderEngine` own the float32 master weights (Keras layouts, torch CUDA
tensors), the packed MFMA panels derived from them and the layer chain, and drive the C ABI
(voxvae.lib).  torch is used for device memory and the current HIP stream only; every
arithmetic step is a libvoxvae kernel.  Reference: src/net_core/autoencoder3D.py:72-139.
"""
import collections
import contextlib
import ctypes
import functools

import numpy as np
import torch

from . import lib as L
from . import routes as R

BN_EPS = 1e-3  # Keras BatchNormalization default (autoencoder3D.py:31)

# Diagnostic only (profiles/microbench/fp8_schemes.py): callable(layer name, activation tensor) -> tensor applied to the input of
# every stride-2 layer, so that a quantisation scheme can be evaluated on the real kernels before a kernel is written for it.
LAYER_INPUT_HOOK = None


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _tdtype(dt):
    return torch.bfloat16 if dt == L.VV_BF16 else torch.float32


def _require_gpu():
    if not torch.cuda.is_available():
        raise L.VoxVaeError('no HIP device visible: the voxel VAE path runs on MI355X only (no CPU fallback)')


class LayerTimer:
    """Optional per-layer HIP-event timing on the launch stream (bench.py's roofline leg).  `only` restricts the
    events to one layer name so the timed region carries two events per step, not two per layer."""

    def __init__(self, only=None):
        self.only = only
        self.events = {}

    def begin(self, name):
        if self.only is not None and name != self.only:
            return None
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        return name, e0, e1

    def end(self, tok):
        if tok is not None:
            tok[2].record()
            self.events.setdefault(tok[0], []).append((tok[1], tok[2]))

    def summary_ms(self):
        """name -> (launches, mean ms); call after torch.cuda.synchronize()."""
        return {k: (len(v), sum(a.elapsed_time(b) for a, b in v) / len(v)) for k, v in self.events.items()}


class _Workspace:
    """Grow-only scratch buffers shared by the layers of one engine (split-K slabs, loss partials), ONE PER HIP STREAM: the
    same engine can then run independent batches on several streams at once (the chunked host-array path of getEval,
    voxvae/hostio.py) without a second in-flight step overwriting the first one's slabs."""

    def __init__(self, device):
        self.device = device
        self.bufs = {}

    def get(self, nbytes):
        nbytes = max(int(nbytes), 16)
        key = torch.cuda.current_stream(self.device).cuda_stream
        buf = self.bufs.get(key)
        if buf is None or buf.numel() < nbytes:
            buf = self.bufs[key] = torch.empty(nbytes, dtype=torch.uint8, device=self.device)
        return buf


def round_e4m3(x):
    """float tensor -> nearest OCP e4m3fn value (round half to even, saturating at 448), in float32 arithmetic; bit-for-bit what a
    cast to torch.float8_e4m3fn gives for |x| <= 448 (tests/test_host_logic.py), without depending on that dtype's kernels."""
    x = x.float()
    ax = x.abs().clamp(max=448.0)
    _, e = torch.frexp(ax)                    # ax = m 2^e with m in [0.5, 1)
    e = (e - 1).clamp(min=-6)                 # the binade's exponent; the subnormals share 2^-6
    step = torch.exp2((e - 3).float())
    q = (torch.round(ax / step) * step).clamp(max=448.0)
    return torch.where(x < 0, -q, q)


# The taps ONE output element sums: all 64 of a stride-2 / stride-1 convolution kernel [kd,kh,kw,Cin,Cout]; for the stride-2 transposed
# convolution [kd,kh,kw,Cout,Cin] the 8 taps of an output-parity class (tap parity = 1 - output parity per axis).
CONV_TAP_GROUPS = (tuple(range(64)),)
CONVT_TAP_GROUPS = tuple(tuple((kd * 4 + kh) * 4 + kw for kd in range(4) for kh in range(4) for kw in range(4)
                               if (kd % 2, kh % 2, kw % 2) == (pd, ph, pw)) for pd in range(2) for ph in range(2) for pw in range(2))


def quant_fp8(w, cout_axis, tap_groups=None):
    """Per-output-channel scaling ahead of the fp8 pack: returns (q, s) with q = the e4m3fn image of w / s as float32 values and
    s = max|w| / 256 per channel (e4m3fn holds +-448; its relative precision does not depend on the scale, its range and subnormal
    floor do).  The caller folds s into the per-channel scale vector the epilogue applies; the pack kernels convert q exactly.

    tap_groups (round 4): ERROR DIFFUSION over the taps of one (cin, cout) pair.  Rounded independently, the 64 (or 8) tap weights
    a pair contributes to one output carry ~sqrt(n)/sqrt(12) ulps of summed error, and that sum is multiplied by whatever part of
    the activation is common to the taps -- which, for the locally constant feature maps of occupancy grids, is most of it.  With
    the running rounding error of a group carried into the next tap, the errors of a group sum to <= half an ulp whatever n is
    (partial sums over a raster range of the group likewise, which is what a SAME-padding border sees); the price is ~sqrt(2) more
    error per single weight.  Measured at the trained operating points (profiles/microbench/fp8_schemes.py, 256 samples): the IoU
    cost of the WEIGHT rounding of policy 'wide' goes from 3.2e-4 (32^3) / 2.9e-4 (64^3) to < 5e-5 -- it disappears in the noise."""
    red = [d for d in range(w.dim()) if d != cout_axis]
    s = w.abs().amax(dim=red).clamp_min(1e-20) / 256.0
    shape = [1] * w.dim()
    shape[cout_axis] = -1
    ws = w / s.view(shape)
    if tap_groups is None or not R.switches().fp8_shaped:
        return round_e4m3(ws).contiguous(), s.contiguous()
    if w.dim() != 5 or w.shape[0] * w.shape[1] * w.shape[2] != 64:
        raise ValueError('tap groups are defined for [4,4,4,a,b] kernels, got %s' % (tuple(w.shape),))
    flat = ws.reshape(64, w.shape[3], w.shape[4])
    q = torch.empty_like(flat)
    for g in tap_groups:
        carry = torch.zeros_like(flat[0])
        for t in g:
            v = flat[t] + carry
            q[t] = round_e4m3(v)
            carry = v - q[t]
    return q.reshape(w.shape).contiguous(), s.contiguous()


# One stride-2 layer of an engine's plan (built by _pack, walked by forward, latent_tail and the trainer): the kernel form (a route of
# voxvae/routes.py), the element types the kernel reads and writes, the weight image it reads (None in a training pack: the trainer's) and every
# image the engine keeps for the layer, by kind.
_Layer = collections.namedtuple('_Layer', 'name route idt odt w images')


class _EngineBase:
    def __init__(self, structure, dtype, device):
        _require_gpu()
        L.load()
        self.structure = structure
        self.dt = L.DTYPES[dtype] if isinstance(dtype, str) else int(dtype)
        # 'fp8': inference mode in which the MFMA layers whose Cin is a multiple of 128 run on e4m3fn operands (weights
        # quantised per output channel, the scale folded into the BatchNorm scale; activations stored as fp8 between
        # consecutive fp8 layers); every other layer, the latent algebra and the losses are the bf16 path.
        self.fp8 = self.dt == L.VV_FP8
        if self.fp8:
            self.dt = L.VV_BF16
            from . import fp8_policy
            self.fp8_policy = fp8_policy()        # 'wide': only the layers with a direct fp8 kernel; 'mid' / 'most' / 'all': voxvae.set_fp8_policy
        self.tdt = _tdtype(self.dt)
        self.device = torch.device(device)
        self.params = {}          # name -> float32 CUDA tensor, Keras layout (the trainable/master copy)
        self.packed = {}          # the other layers' images and every layer's folded vectors, by name
        self.plan = []            # the stride-2 layers (_Layer), rebuilt by _pack
        self.switches = R.switches()    # re-read by every _pack
        self.ws = _Workspace(self.device)
        self._dirty = True
        self._folded, self._want_fold = False, True
        self.act = L.ACT[structure['activation']]
        self.timer = None         # LayerTimer or None
        self.tag = ''
        # vv_schedule of the 4^3 <-> 2^3 layers: latency for a caller that runs one batch at a time; the evaluators that keep several
        # batches in flight on their own streams (voxvae/streams.py) switch to throughput around each submit (`scheduled`)
        self.schedule = L.VV_SCHED_LATENCY

    def _call(self, layer, fn, *args):
        t = self.timer
        tok = t.begin(self.tag + layer) if t is not None else None
        L.call(fn, *args)
        if tok is not None:
            t.end(tok)

    # ---- weights
    def set_params(self, params):
        for k, v in params.items():
            t = torch.as_tensor(np.ascontiguousarray(v) if isinstance(v, np.ndarray) else v, dtype=torch.float32)
            if k in self.params and tuple(self.params[k].shape) != tuple(t.shape):
                raise ValueError('%s: shape %s != %s' % (k, tuple(t.shape), tuple(self.params[k].shape)))
            self.params[k] = t.to(self.device).contiguous()
        self.weights_changed()

    def get_params(self):
        return {k: v.detach().cpu().numpy() for k, v in self.params.items()}

    def _fold(self, prefix, channels, repeat=1, bias=None):
        if not self._want_fold:
            return None, None
        p = self.params
        scale = torch.empty(channels * repeat, dtype=torch.float32, device=self.device)
        shift = torch.empty_like(scale)
        L.call('vv_fold_bn', L.ptr(p[prefix + '/gamma']), L.ptr(p[prefix + '/beta']), L.ptr(p[prefix + '/moving_mean']),
               L.ptr(p[prefix + '/moving_variance']), L.ptr(bias), BN_EPS, L.ptr(scale), L.ptr(shift), channels, repeat,
               _stream())
        return scale, shift

    def _empty(self, *shape, dtype=None):
        return torch.empty(shape, dtype=dtype or self.tdt, device=self.device)

    def _plan_layers(self, direction, sw):
        """-> (route of every stride-2 layer, the layers the fp8 policy keeps on bf16); self.switches = sw from now on."""
        self.switches = sw
        f, n, enc = self.filters, len(self.filters), direction == R.CONV
        off = R.fp8_layers_off(self.fp8_policy, enc, n, sw) if self.fp8 else ()
        wide = self.fp8 and self.fp8_policy == 'wide'
        routes = []
        for i in range(1, n - 1):
            want = self.fp8 and ('%s%d' % ('E' if enc else 'D', i + 1)) not in off
            if enc:
                routes.append(R.conv_route(self.D >> i, f[i - 1], f[i], self.dt, want, wide, False, sw))
            else:
                routes.append(R.convT_route(self.S << (i - 1), f[i - 1], f[i], self.dt, want, wide, sw))
        return routes, off

    def _pack_layer(self, direction, i, route, st):
        """Weight images (routes.ENGINE_IMAGES) and folded BatchNorm vectors of stride-2 layer i -> {kind: image}."""
        wname, bn, cout_axis, taps = ('conv%d/kernel', 'bn%d', 4, CONV_TAP_GROUPS) if direction == R.CONV else ('convT%d/kernel', 'bnT%d', 3, CONVT_TAP_GROUPS)
        cin, cout, pk = self.filters[i - 1], self.filters[i], self.packed
        q = route.endswith('_fp8')
        wk = self.params[wname % i]
        if q:
            wk, qs = quant_fp8(wk, cout_axis, taps)
        kinds = R.ENGINE_IMAGES[direction][route][0 if self._want_fold else 1]
        images = {k: R.pack_image(direction, k, wk, cin, cout, L.VV_FP8 if q else self.dt, st) for k in kinds[:1]}
        pk['scale%d' % i], pk['shift%d' % i] = self._fold(bn % i, cout)
        for k in kinds[1:]:
            images[k] = R.pack_image(direction, k, self.params[wname % i], cin, cout, self.dt, st)
        if q:
            pk['q%d' % i] = True
            if pk['scale%d' % i] is not None:
                pk['scale%d' % i].mul_(qs)
        return images

    def _as_fp8(self, h, label):
        """bf16 activation -> fp8 copy (the hand-over from a bf16-only layer into an fp8 stretch)."""
        o = torch.empty(h.shape, dtype=torch.uint8, device=self.device)
        self._call(label, 'vv_convert', L.ptr(h), L.ptr(o), h.numel(), L.VV_BF16, L.VV_FP8, _stream())
        return o

    def needs_pack(self, fold=True):
        """True when the next ensure_packed(fold) will repack: the weights changed, or the folded vectors are wanted and stale."""
        return self._dirty or (fold and not self._folded)

    def weights_changed(self):
        self._dirty = True

    def statistics_moved(self):
        """A training-mode forward updated the moving statistics in place: the folded inference scale / shift vectors are stale (the
        weight images are not)."""
        self._folded = False

    def ensure_packed(self, fold=True):
        """Refresh the packed weight images after a weight change.  fold=False (the training step, which uses batch
        statistics) skips the folded moving-statistics scale/shift vectors; the next inference call packs them."""
        if self.needs_pack(fold):
            self._want_fold = fold
            self._pack()
            self._dirty = False
            self._folded = fold


def _check_cubic_pow2(shape):
    d = int(shape[0])
    if len(shape) != 4 or shape[1] != d or shape[2] != d or d & (d - 1):
        raise ValueError('voxel grid must be cubic with a power-of-two side, got %s' % (shape,))
    return d


class EncoderEngine(_EngineBase):
    """encoder3D (autoencoder3D.py:72-102): [B,D,D,D,1] -> [B,E] float32."""

    def __init__(self, structure, dtype='bf16', device='cuda:0'):
        super().__init__(structure, dtype, device)
        s = structure
        self.D = _check_cubic_pow2(s['input_shape'])
        self.filters = [int(c) for c in s['filter_num_list']]
        n = len(self.filters)
        if s['input_shape'][-1] != 1:
            raise NotImplementedError('encoder input must have 1 channel (occupancy grid)')
        if any(int(k) != 4 for k in s['filter_size_list']) or [int(v) for v in s['strides_list']] != [2] * (n - 1) + [1]:
            raise NotImplementedError('encoder3D kernels cover filter size 4 with strides [2]*(n-1)+[1] '
                                      '(every config of the reference)')
        if s['final_pool'] not in ('average', 'max', 'None', None):
            raise NotImplementedError("final_pool=%r: 'average' (every reference config), 'max' or 'None' (autoencoder3D.py:90-95)" % s['final_pool'])
        self.pool_max = s['final_pool'] == 'max'
        self.pool_none = s['final_pool'] in ('None', None)      # no pooling: the model returns the last conv's [B,S,S,S,E] map
        self.final_sigmoid = s['final_activation'] == 'sigmoid'  # tf.nn.sigmoid on the output (autoencoder3D.py:97-99)
        if not self.final_sigmoid and s['final_activation'] not in (None, 'None', 'linear'):
            raise NotImplementedError('encoder final_activation %r' % s['final_activation'])
        if self.D >> (n - 1) < 1:
            raise ValueError('grid too small for %d stride-2 layers' % (n - 1))
        self.S = self.D >> (n - 1)      # side of the last feature map
        self.E = self.filters[-1]
        if (self.pool_max or self.pool_none) and (self.S ** 3 * self.E) * (self.S ** 3 * self.filters[-2]) > (1 << 28):
            # the max pool is not linear, so the last conv runs position by position as one dense panel [S^3 E][S^3 Cin]; that is 4 M
            # elements at the 32^3 geometry (S = 2) and 268 M at 64^3 (S = 4): no reference config asks for it there
            raise NotImplementedError("final_pool=%r with a %d^3 last feature map" % (s['final_pool'], self.S))

    def param_shapes(self):
        shp, cin = {}, 1
        for i, c in enumerate(self.filters):
            shp['conv%d/kernel' % i] = (4, 4, 4, cin, c)
            if i < len(self.filters) - 1:
                for nme in ('gamma', 'beta', 'moving_mean', 'moving_variance'):
                    shp['bn%d/%s' % (i, nme)] = (c,)
            cin = c
        return shp

    def _pack(self):
        p, f, st, pk = self.params, self.filters, _stream(), {}
        routes, off = self._plan_layers(R.CONV, R.switches())
        n, self.packed, self.plan = len(f), pk, []
        pk['scale0'], pk['shift0'] = self._fold('bn0', f[0])
        pk['w0'] = R.pack_image(R.CONV, 'igemm', p['conv0/kernel'], 1, f[0], self.dt, st)
        pooled = not (self.pool_max or self.pool_none)
        tail_fp8 = pooled and self.fp8 and self.fp8_policy != 'wide' and (self.S ** 3 * f[n - 2]) % 128 == 0 and ('E%d' % n) not in off
        fp8, self._tail_fp8 = [r.endswith('_fp8') for r in routes] + [tail_fp8], tail_fp8
        # element type of the first layer's output: the engine's dtype, or fp8 when the second layer is fp8 and the first layer's
        # plane-form kernel applies (it stores e4m3fn itself)
        self._h0_dt = L.VV_FP8 if (fp8[0] and self.D >= 32 and f[0] == 64 and self.dt == L.VV_BF16) else self.dt
        for i, route in enumerate(routes, 1):
            q, nq = fp8[i - 1], fp8[i]
            images = self._pack_layer(R.CONV, i, route, st)
            if nq and route in ('pos', 'skip'):     # these forms store the engine's dtype only; an fp8 next layer wants e4m3fn
                route = R.conv_route(self.D >> i, f[i - 1], f[i], self.dt, False, False, False, self.switches._replace(no_skip=True))
            self.plan.append(_Layer('E%d' % (i + 1), route, L.VV_FP8 if q else self.dt, L.VV_FP8 if nq else self.dt,
                                    images.get(R.ROUTE_IMAGE[R.CONV][route]), images))
        i = n - 1
        if not pooled:
            # tf.reduce_max over the positions (autoencoder3D.py:92-93) / no pooling: the conv output itself is needed -> full panel [S^3 E][S^3 Cin]
            w = self._empty(self.S ** 3 * f[i], self.S ** 3 * f[i - 1])
            L.call('vv_pack_conv_k4s1_full', L.ptr(p['conv%d/kernel' % i]), L.ptr(w), self.S, f[i - 1], f[i], self.dt, st)
            pk['w%d' % i] = w
            return
        wk = p['conv%d/kernel' % i]
        if tail_fp8:
            wk, qs = quant_fp8(wk, 4, CONV_TAP_GROUPS)
            pk['q%d' % i], pk['scale%d' % i] = True, qs
        w = self._empty(f[i], self.S ** 3 * f[i - 1], dtype=torch.uint8 if tail_fp8 else None)
        L.call('vv_pack_conv_k4s1_meanpool', L.ptr(wk), L.ptr(w), self.S, f[i - 1], f[i], L.VV_FP8 if tail_fp8 else self.dt, st)
        pk['w%d' % i] = w

    def forward(self, x, stop_before_tail=False, stop_before_pos=False):
        """x: float32 CUDA tensor [B,D,D,D,1] (contiguous) -> enc_out float32 [B,E].
        stop_before_tail: return the last stride-2 activation [B,S,S,S,C] instead (the fused latent tail consumes it).
        stop_before_pos (with stop_before_tail): when the last stride-2 layer is the position-major 4^3 -> 2^3 form, stop in FRONT of it and
        return its input [B,4,4,4,C]: latent_tail(..., pos_layer=True) runs that layer and the tail as one fused call (its split-K
        partial sums are summed by the tail's first kernel)."""
        self.ensure_packed()
        B, D, f, pk, st = x.shape[0], self.D, self.filters, self.packed, _stream()
        if tuple(x.shape[1:]) != (D, D, D, 1) or x.dtype != torch.float32 or not x.is_contiguous():
            raise ValueError('encoder input must be contiguous float32 [B,%d,%d,%d,1], got %s %s' % (D, D, D, tuple(x.shape), x.dtype))
        side = D // 2
        hdt = self._h0_dt             # element type of h: the engine's dtype, or fp8 inside an fp8 stretch
        h = self._empty(B, side, side, side, f[0], dtype=torch.uint8 if hdt == L.VV_FP8 else None)
        self._call('E1', 'vv_conv3d_first_fwd_io', L.ptr(x), L.ptr(pk['w0']), L.ptr(pk['scale0']), L.ptr(pk['shift0']),
               L.ptr(h), B, D, f[0], self.act, self.dt, hdt, st)
        for i, ly in enumerate(self.plan, 1):
            if LAYER_INPUT_HOOK is not None:
                h = LAYER_INPUT_HOOK(ly.name, h)
            if ly.idt == L.VV_FP8 and hdt != L.VV_FP8:
                h = self._as_fp8(h, ly.name + 'c')
            if stop_before_pos and stop_before_tail and ly.route == 'pos' and i == len(f) - 2:
                return h
            o = self._empty(B, side // 2, side // 2, side // 2, f[i], dtype=torch.uint8 if ly.odt == L.VV_FP8 else None)
            R.launch_conv(functools.partial(self._call, ly.name), ly.route, self.ws, h, ly.w, pk['scale%d' % i], pk['shift%d' % i], o,
                          B, side, f[i - 1], f[i], self.act, self.dt, ly.odt, st, schedule=self.schedule)
            h, side, hdt = o, side // 2, ly.odt
        i = len(f) - 1
        K = side ** 3 * f[i - 1]
        q = self._tail_fp8
        if self.pool_max or self.pool_none:
            if stop_before_tail:
                raise L.VoxVaeError("stop_before_tail: the fused latent tail folds the MEAN pool into its weights")
            if hdt != self.dt:
                raise L.VoxVaeError("final_pool='max' takes a %s activation" % self.tdt)
            P = side ** 3
            ws = self.ws.get(L.load().vv_dense_workspace_bytes(B, P * f[i], K, self.dt))
            full = self._empty(B, P, f[i], dtype=torch.float32)
            self._call('E%d' % (i + 1), 'vv_dense_fwd', L.ptr(h), L.ptr(pk['w%d' % i]), None, None, L.ptr(full), B, P * f[i], K, 0,
                       self.dt, L.VV_F32, L.ptr(ws), ws.numel(), st)
            if self.pool_none:
                out = full.view(B, side, side, side, f[i])
            else:
                out = self._empty(B, f[i], dtype=torch.float32)
                self._call('E%dp' % (i + 1), 'vv_max_over_positions', L.ptr(full), L.ptr(out), B, P, f[i], st)
            if self.final_sigmoid:
                self._call('E%ds' % (i + 1), 'vv_sigmoid_f32', L.ptr(out), L.ptr(out), out.numel(), st)
            return out
        if stop_before_tail:
            if q or hdt != self.dt:
                raise L.VoxVaeError('stop_before_tail: the fused latent tail takes a %s activation' % self.tdt)
            if self.final_sigmoid:
                raise L.VoxVaeError("stop_before_tail: the fused latent tail has no sigmoid on the encoder output")
            return h
        if q and hdt != L.VV_FP8:
            h = self._as_fp8(h, 'E%dc' % (i + 1))
        ddt = L.VV_FP8 if q else self.dt
        ws = self.ws.get(L.load().vv_dense_workspace_bytes(B, f[i], K, ddt))
        out = self._empty(B, f[i], dtype=torch.float32)
        self._call('E%d' % (i + 1), 'vv_dense_fwd', L.ptr(h), L.ptr(pk['w%d' % i]), L.ptr(pk.get('scale%d' % i)), None, L.ptr(out), B, f[i], K, 0,
                   ddt, L.VV_F32, L.ptr(ws), ws.numel(), st)
        if self.final_sigmoid:
            self._call('E%ds' % (i + 1), 'vv_sigmoid_f32', L.ptr(out), L.ptr(out), out.numel(), st)
        return out


class DecoderEngine(_EngineBase):
    """decoder3D (autoencoder3D.py:104-139): z [B,L] -> logits/probabilities [B,D,D,D,1] float32,
    with the BCE / TP / FP / FN reductions of function.py:73-115 fused into the last layer."""

    def __init__(self, structure, dtype='bf16', device='cuda:0'):
        super().__init__(structure, dtype, device)
        s = structure
        self.D = _check_cubic_pow2(s['output_shape'])
        self.filters = [int(c) for c in s['filter_num_list']]
        n = len(self.filters)
        if any(int(k) != 4 for k in s['filter_size_list']) or [int(v) for v in s['strides_list']] != [1] + [2] * (n - 1):
            raise NotImplementedError('decoder3D kernels cover filter size 4 with strides [1]+[2]*(n-1) '
                                      '(every config of the reference)')
        if self.filters[-1] != 1 or s['output_shape'][-1] != 1:
            raise NotImplementedError('decoder must end in 1 channel')
        self.L = int(s['input_dim'])
        self.S = self.D >> (n - 1)                      # autoencoder3D.py:115
        self.ch = max(self.filters[0] // 64, 8)         # autoencoder3D.py:116-118
        self.final_sigmoid = s['final_activation'] == 'sigmoid'
        if not self.final_sigmoid and s['final_activation'] not in (None, 'None', 'linear'):
            raise NotImplementedError('decoder final_activation %r' % s['final_activation'])

    def param_shapes(self):
        lin = self.S ** 3 * self.ch
        shp = {'dense/kernel': (self.L, lin), 'dense/bias': (lin,)}
        for nme in ('gamma', 'beta', 'moving_mean', 'moving_variance'):
            shp['bn_dense/' + nme] = (lin,)
        cin = self.ch
        for i, c in enumerate(self.filters):
            shp['convT%d/kernel' % i] = (4, 4, 4, c, cin)
            if i < len(self.filters) - 1:
                for nme in ('gamma', 'beta', 'moving_mean', 'moving_variance'):
                    shp['bnT%d/%s' % (i, nme)] = (c,)
            cin = c
        return shp

    def _pack(self):
        p, f, st, S3 = self.params, self.filters, _stream(), self.S ** 3
        lin = S3 * self.ch
        pk = self.packed = {}
        pk['wd'] = self._empty(lin, self.L)
        L.call('vv_pack_dense', L.ptr(p['dense/kernel']), L.ptr(pk['wd']), self.L, lin, self.dt, st)
        pk['scaled'], pk['shiftd'] = self._fold('bn_dense', lin, 1, p['dense/bias'])
        pk['w0'] = self._empty(S3 * f[0], lin)
        L.call('vv_pack_convT_k4s1_dense', L.ptr(p['convT0/kernel']), L.ptr(pk['w0']), self.S, self.ch, f[0], self.dt, st)
        pk['scale0'], pk['shift0'] = self._fold('bnT0', f[0], S3)
        routes, _ = self._plan_layers(R.CONVT, R.switches())
        fp8 = [r.endswith('_fp8') for r in routes] + [False]
        self._h1_dt = L.VV_FP8 if fp8[0] else self.dt            # D1 hands fp8 to an fp8 D2
        self.plan = []
        for i, route in enumerate(routes, 1):
            images = self._pack_layer(R.CONVT, i, route, st)
            # the implicit GEMM stores what the next layer reads; every other form stores the engine's dtype (an fp8 next layer converts
            # it itself: cheaper than the implicit GEMM), the fp8 direct kernel optionally e4m3fn (forward: routes.final_takes_fp8)
            odt = L.VV_FP8 if fp8[i] and route in ('igemm', 'igemm_fp8') else self.dt
            self.plan.append(_Layer('D%d' % (i + 1), route, L.VV_FP8 if fp8[i - 1] else self.dt, odt,
                                    images.get(R.ROUTE_IMAGE[R.CONVT][route]), images))

    def _hidden(self, z_act, h1, final_fp8):
        """The layers in front of the last one (D0 ... D(n-1)), shared by forward and forward_mean -> (h [B,side^3,C], its element type,
        side, B).  final_fp8: the last hidden layer may be stored as e4m3fn for the fp8 form of the last layer (routes.final_takes_fp8)."""
        self.ensure_packed()
        f, pk, st, S, D = self.filters, self.packed, _stream(), self.S, self.D
        lin = S ** 3 * self.ch
        n0 = S ** 3 * f[0]
        if h1 is not None:
            B = h1.shape[0]
            if h1.dtype != self.tdt or h1.numel() != B * n0 or not h1.is_contiguous():
                raise ValueError('h1 must be contiguous %s [B,%d,%d,%d,%d]' % (self.tdt, S, S, S, f[0]))
            h, hdt = h1, self.dt
        else:
            B = z_act.shape[0]
            if z_act.dtype != self.tdt or tuple(z_act.shape) != (B, self.L) or not z_act.is_contiguous():
                raise ValueError('decoder input must be contiguous %s [B,%d]' % (self.tdt, self.L))
            ws = self.ws.get(L.load().vv_dense_workspace_bytes(B, lin, self.L, self.dt))
            t = self._empty(B, lin)
            self._call('D0', 'vv_dense_fwd', L.ptr(z_act), L.ptr(pk['wd']), L.ptr(pk['scaled']), L.ptr(pk['shiftd']), L.ptr(t), B, lin,
                   self.L, self.act, self.dt, self.dt, L.ptr(ws), ws.numel(), st)
            ws = self.ws.get(L.load().vv_dense_workspace_bytes(B, n0, lin, self.dt))
            hdt = self._h1_dt
            h = self._empty(B, S, S, S, f[0], dtype=torch.uint8 if hdt == L.VV_FP8 else None)
            self._call('D1', 'vv_dense_fwd', L.ptr(t), L.ptr(pk['w0']), L.ptr(pk['scale0']), L.ptr(pk['shift0']), L.ptr(h), B, n0, lin,
                   self.act, self.dt, hdt, L.ptr(ws), ws.numel(), st)
        side = S
        for i, ly in enumerate(self.plan, 1):
            if LAYER_INPUT_HOOK is not None:
                h = LAYER_INPUT_HOOK(ly.name, h)
            if ly.idt == L.VV_FP8 and hdt != L.VV_FP8:
                h = self._as_fp8(h, ly.name + 'c')
            odt = ly.odt
            if final_fp8 and ly.route == 'direct_fp8' and i == len(f) - 2 and R.final_takes_fp8(2 * side, B, self.switches):
                odt = L.VV_FP8
            o = self._empty(B, 2 * side, 2 * side, 2 * side, f[i], dtype=torch.uint8 if odt == L.VV_FP8 else None)
            R.launch_convT(functools.partial(self._call, ly.name), ly.route, self.ws, h, ly.w, pk['scale%d' % i], pk['shift%d' % i], o,
                           B, side, f[i - 1], f[i], self.act, self.dt, odt, st, schedule=self.schedule)
            h, side, hdt = o, 2 * side, odt
        return h, hdt, side, B

    def forward(self, z_act, target=None, want_logits=False, gamma=0.6, epsilon=1e-7, want_metrics=False, h1=None):
        """z_act: [B,L] in the activation dtype.  target: float32 [B,D,D,D,1] or None.
        Returns (out, logits, stats): out = probabilities (final_activation 'sigmoid') or logits;
        stats float32 [B,4] = per-sample (bce, TP, FP, FN) against target (zeros if None).
        want_metrics: also return float32 [4] = (mean bce, precision, recall, IoU) -- nolbo.py:1498-1501 -- from the same
        reduction launch as `stats` (a fourth return value).
        h1: the output of the first (stride-1) decoder layer [B,S,S,S,C0] when the fused latent tail has produced it already
        (z_act is then not read)."""
        f, st, D = self.filters, _stream(), self.D
        h, hdt, side, B = self._hidden(z_act, h1, True)
        if target is None:
            target = torch.zeros(B, D, D, D, 1, dtype=torch.float32, device=self.device)
        elif target.dtype != torch.float32 or target.numel() != B * D ** 3 or not target.is_contiguous():
            raise ValueError('target must be contiguous float32 [B,%d,%d,%d,1]' % (D, D, D))
        probs = self._empty(B, D, D, D, 1, dtype=torch.float32) if self.final_sigmoid else None
        logits = self._empty(B, D, D, D, 1, dtype=torch.float32) if (want_logits or not self.final_sigmoid) else None
        stats = self._empty(B, 4, dtype=torch.float32)
        ws = self.ws.get(L.load().vv_convT3d_final_bce_workspace_bytes(B, side))
        if want_metrics:
            metrics = self._empty(4, dtype=torch.float32)
            self._call('D%d' % len(f), 'vv_convT3d_final_bce_metrics_fwd', L.ptr(h), L.ptr(self.params['convT%d/kernel' % (len(f) - 1)]),
                       L.ptr(target), L.ptr(probs), L.ptr(logits), L.ptr(stats), L.ptr(metrics), B, side, f[-2], gamma, epsilon, hdt,
                       L.ptr(ws), ws.numel(), st)
            return (probs if self.final_sigmoid else logits), logits, stats, metrics
        self._call('D%d' % len(f), 'vv_convT3d_final_bce_fwd', L.ptr(h), L.ptr(self.params['convT%d/kernel' % (len(f) - 1)]), L.ptr(target),
               L.ptr(probs), L.ptr(logits), L.ptr(stats), B, side, f[-2], gamma, epsilon, hdt, L.ptr(ws), ws.numel(), st)
        return (probs if self.final_sigmoid else logits), logits, stats

    def forward_mean(self, z_act, samples, target=None, h1=None, gamma=0.6, epsilon=1e-7, want_metrics=True):
        """Sampled-mean reconstruction (nolbo_test.py:174-177): z_act [B*K,L] holds K = `samples` latents per object, sample k of object b
        in row b*K + k (sample_latents).  D0 ... D(n-1) run as in forward at batch B*K; the last layer averages the K occupancy
        probabilities of an object inside the kernel (vv_convT3d_final_mean_fwd) and scores the average.
        Returns (mean_probs float32 [B,D,D,D,1], stats [B,4] = (bce, TP, FP, FN) of the averaged prediction or None, metrics float32 [4] =
        (mean bce, precision, recall, IoU) or None); stats and metrics need a target [B,D,D,D,1]; want_metrics=False skips the metrics
        launch (a caller that scores several passes together)."""
        if not self.final_sigmoid:
            raise NotImplementedError("forward_mean averages probabilities: final_activation must be 'sigmoid' (an average of logits is "
                                      "not the reference's quantity)")
        K = int(samples)
        if K < 1:
            raise ValueError('samples must be >= 1, got %r' % (samples,))
        f, st, D = self.filters, _stream(), self.D
        h, hdt, side, BK = self._hidden(z_act, h1, False)       # the last hidden layer in the engine's dtype: the kernel takes bf16 / f32
        if BK % K:
            raise ValueError('%d latents do not divide into objects of %d samples' % (BK, K))
        B = BK // K
        if target is not None and (target.dtype != torch.float32 or target.numel() != B * D ** 3 or not target.is_contiguous()):
            raise ValueError('target must be contiguous float32 [B,%d,%d,%d,1]' % (D, D, D))
        mean_probs = self._empty(B, D, D, D, 1, dtype=torch.float32)
        stats = self._empty(B, 4, dtype=torch.float32) if target is not None else None
        ws = self.ws.get(L.load().vv_convT3d_final_mean_workspace_bytes(B, K, side))
        self._call('D%dm' % len(f), 'vv_convT3d_final_mean_fwd', L.ptr(h), L.ptr(self.params['convT%d/kernel' % (len(f) - 1)]), L.ptr(target),
                   L.ptr(mean_probs), L.ptr(stats), B, K, side, f[-2], gamma, epsilon, hdt, L.ptr(ws), ws.numel(), st)
        return mean_probs, stats, (shape_metrics(stats) if (stats is not None and want_metrics) else None)


def sample_latents(mean, logvar, eps, act_dtype):
    """K draws per object (nolbo_test.py:169-173; function.py:35-38): mean / logvar float32 [B,L], eps [B,K,L] ->
    (z float32 [B*K,L], z_act = the same values in act_dtype), row b*K + k = mean[b] + sqrt(exp(logvar[b])) * eps[b,k]."""
    B, K, Lz = eps.shape
    if tuple(mean.shape) != (B, Lz) or tuple(logvar.shape) != (B, Lz):
        raise ValueError('mean / logvar must be [%d,%d] for eps %s' % (B, Lz, tuple(eps.shape)))
    for t in (mean, logvar, eps):
        if t.dtype != torch.float32 or not t.is_contiguous():
            raise ValueError('sample_latents takes contiguous float32 tensors')
    z = torch.empty(B * K, Lz, dtype=torch.float32, device=eps.device)
    z_act = z if act_dtype == L.VV_F32 else torch.empty(B * K, Lz, dtype=torch.bfloat16, device=eps.device)
    L.call('vv_sample_latents', L.ptr(mean), L.ptr(logvar), L.ptr(eps), L.ptr(z), L.ptr(z_act) if act_dtype != L.VV_F32 else None,
           act_dtype, B, K, Lz, _stream())
    return z, z_act


def reparam_kl(enc_out, eps, latent, act_dtype, drop_mask=None, drop_scale=1.0, want_stats=False):
    """Fused slice|clip|sampling|dropout|KL (nolbo.py:1417-1431; function.py:35-38, 84-98)."""
    B = enc_out.shape[0]
    dev = enc_out.device
    z = torch.empty(B, latent, dtype=torch.float32, device=dev)
    z_act = z if act_dtype == L.VV_F32 else torch.empty(B, latent, dtype=torch.bfloat16, device=dev)
    kl = torch.empty(B, dtype=torch.float32, device=dev)
    mean = torch.empty_like(z) if want_stats else None
    logvar = torch.empty_like(z) if want_stats else None
    L.call('vv_reparam_kl_fwd', L.ptr(enc_out), L.ptr(eps), L.ptr(drop_mask), float(drop_scale), L.ptr(z),
           L.ptr(z_act) if act_dtype != L.VV_F32 else None, act_dtype, L.ptr(kl), L.ptr(mean), L.ptr(logvar), B, latent,
           _stream())
    return z, z_act, kl, mean, logvar


@contextlib.contextmanager
def scheduled(engines, schedule):
    """The engines issue their 4^3 <-> 2^3 layers with `schedule` (vv_schedule) inside the block.  The results are the same bits; what
    changes is how many workgroups a launch takes (include/voxvae.h)."""
    old = [e.schedule for e in engines]
    for e in engines:
        e.schedule = schedule
    try:
        yield
    finally:
        for e, s in zip(engines, old):
            e.schedule = s


def latent_tail_supported(enc, dec, variational):
    """True when encoder tail -> reparam/KL -> Dense -> first decoder layer can run as the two fused launches of latent_tail.hip."""
    if getattr(enc, 'pool_max', False) or getattr(enc, 'pool_none', False) or getattr(enc, 'final_sigmoid', False):
        return False
    if enc.dt != L.VV_BF16 or enc.fp8 or dec.fp8 or dec.dt != L.VV_BF16 or enc.act != dec.act:
        return False
    return R.fused_tail(enc.S ** 3 * enc.filters[-2], enc.E, dec.L, dec.S ** 3 * dec.ch, dec.S ** 3 * dec.filters[0], int(variational), enc.switches)


def pos_latent_tail_supported(enc, dec, variational, batch=1):
    """True when the last stride-2 encoder layer (4^3 -> 2^3, position-major form) and the latent tail can run as ONE fused call
    (vv_conv_pos_latent_tail_fwd: the layer's split-K partial sums are summed inside the tail; one launch, so the batch's layer
    input has to fit 32-bit buffer offsets)."""
    if not latent_tail_supported(enc, dec, variational) or enc.switches.no_pos_tail or enc.S != 2 or len(enc.filters) < 3:
        return False
    if batch * 64 * enc.filters[-3] * 2 > 0x7FFFFFFF:
        return False
    enc.ensure_packed()
    if enc.plan[-1].route != 'pos':
        return False
    return R.fused_pos_tail(enc.filters[-3], enc.filters[-2], enc.E, dec.L, dec.S ** 3 * dec.ch, dec.S ** 3 * dec.filters[0], int(variational))


def latent_tail(enc, dec, h, eps, variational, want_enc_out=False, pos_layer=False):
    """Fused latent tail (vv_latent_tail_fwd): h = EncoderEngine.forward(x, stop_before_tail=True).
    pos_layer: h = EncoderEngine.forward(x, stop_before_tail=True, stop_before_pos=True), the INPUT of the last stride-2 layer
    (pos_latent_tail_supported): that layer runs inside the call (vv_conv_pos_latent_tail_fwd).
    Returns (z float32 [B,L], z_act bf16, kl [B] or None, enc_out or None, h1 = the decoder's first-layer output)."""
    enc.ensure_packed()
    dec.ensure_packed()
    B, dev = h.shape[0], h.device
    Lz, E = dec.L, enc.E
    K5 = enc.S ** 3 * enc.filters[-2]
    lin, n1 = dec.S ** 3 * dec.ch, dec.S ** 3 * dec.filters[0]
    ne = len(enc.filters) - 1
    if pos_layer and tuple(h.shape[1:]) != (4, 4, 4, enc.filters[-3]):
        raise L.VoxVaeError('latent_tail(pos_layer=True) takes the [B,4,4,4,%d] input of the last stride-2 layer, got %s' % (enc.filters[-3], tuple(h.shape)))
    z = torch.empty(B, Lz, dtype=torch.float32, device=dev)
    z_act = torch.empty(B, Lz, dtype=torch.bfloat16, device=dev)
    kl = torch.empty(B, dtype=torch.float32, device=dev) if variational else None
    enc_out = torch.empty(B, E, dtype=torch.float32, device=dev) if want_enc_out else None
    h1 = torch.empty(B, dec.S, dec.S, dec.S, dec.filters[0], dtype=torch.bfloat16, device=dev)
    pe, pd = enc.packed, dec.packed
    tail = (L.ptr(pe['w%d' % ne]), L.ptr(pe.get('scale%d' % ne)), L.ptr(eps), L.ptr(pd['wd']), L.ptr(pd['scaled']), L.ptr(pd['shiftd']),
            L.ptr(pd['w0']), L.ptr(pd['scale0']), L.ptr(pd['shift0']), L.ptr(enc_out), L.ptr(z), L.ptr(z_act), L.ptr(kl), L.ptr(h1), B)
    if pos_layer:
        c3, c4, i4 = enc.filters[-3], enc.filters[-2], ne - 1
        ws = enc.ws.get(L.load().vv_conv_pos_latent_tail_workspace_bytes(B, c3, c4, E))
        head = (L.ptr(h), L.ptr(enc.plan[-1].w), L.ptr(pe['scale%d' % i4]), L.ptr(pe['shift%d' % i4]), c3, c4, *tail, E, Lz, lin, n1, int(variational), dec.act)
        if enc.schedule == L.VV_SCHED_LATENCY:
            enc._call('E%dLT' % ne, 'vv_conv_pos_latent_tail_fwd', *head, L.VV_BF16, L.ptr(ws), ws.numel(), _stream())
        else:
            enc._call('E%dLT' % ne, 'vv_conv_pos_latent_tail_fwd_ex', *head, enc.schedule, L.ptr(ws), ws.numel(), _stream())
    else:
        ws = enc.ws.get(L.load().vv_latent_tail_workspace_bytes(B, K5, E, n1))
        enc._call('LT', 'vv_latent_tail_fwd', L.ptr(h), *tail, K5, E, Lz, lin, n1, int(variational), dec.act, L.VV_BF16, L.ptr(ws), ws.numel(),
                  _stream())
    return z, z_act, kl, enc_out, h1


def shape_metrics(stats):
    """[B,4] (bce,TP,FP,FN) -> float32 [4] = (mean bce, precision, recall, IoU) -- nolbo.py:1498-1501."""
    out = torch.empty(4, dtype=torch.float32, device=stats.device)
    L.call('vv_shape_metrics', L.ptr(stats), L.ptr(out), stats.shape[0], _stream())
    return out
