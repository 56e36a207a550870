"""Which kernel form a stride-2 layer runs on: the one place that decides it.

A stride-2 convolution / transposed convolution has up to six forms in libvoxvae --

    'pos'         position-major split-K GEMM (4^3 -> 2^3 / 2^3 -> 4^3)                  *_pos_fwd
    'skip'        whole samples resident in LDS, padded taps skipped (8^3 -> 4^3 / 4^3 -> 8^3)  *_skip_fwd
    'whole'       the whole-sample transposed kernel (8^3 x 128 -> 16^3 x 64)            vv_convT3d_k4s2_whole_fwd
    'direct'      the direct kernels of the widest layers                                *_direct_fwd
    'direct_fp8'  their e4m3fn twins                                                     *_direct_fp8_fwd
    'igemm', 'igemm_fp8'   the implicit GEMM (every shape, every dtype)                  *_fwd_io / *_fwd

-- and this module holds the policy (conv_route / convT_route), the weight image each form reads (IMAGES, ROUTE_IMAGE), what an
engine packs for a layer (ENGINE_IMAGES) and the argument list of every entry point (launch_conv / launch_convT).  The engines
(voxvae/engine.py) call the route functions once per layer when they pack and keep the answers in their plan; the trainer
(voxvae/train.py) calls them per launch with the switches it read at the start of the step.
"""
import collections
import functools
import os

import torch

from . import lib as L

Switches = collections.namedtuple('Switches', 'no_skip no_direct no_whole no_latent_tail no_pos_tail no_prepack no_stats_fusion '
                                              'fp8_e2 fp8_last fp8_d5 fp8_off fp8_shaped')


def switches():
    """The Python-side diagnostic switches, read from the environment NOW.  An engine reads them when it builds its plan (the pack after
    construction or a weight change), the trainer once per step: set them before the model is built."""
    env = os.environ.get
    return Switches(
        no_skip=bool(env('VV_NO_SKIP')),                    # no 'pos' / 'skip' forms
        no_direct=bool(env('VV_NO_DIRECT')),                # no 'direct' / 'direct_fp8' / 'whole' forms
        no_whole=bool(env('VV_NO_WHOLE')),                  # 'direct' instead of 'whole'
        no_latent_tail=bool(env('VV_NO_LATENT_TAIL')),      # the five calls instead of the fused latent tail
        no_pos_tail=bool(env('VV_NO_POS_TAIL')),            # the last stride-2 encoder layer outside the fused tail
        no_prepack=bool(env('VV_NO_PREPACK')),              # training: weight images packed per use, not batched
        no_stats_fusion=bool(env('VV_NO_STATS_FUSION')),    # training: 'whole' + a statistics sweep instead of the fused kernel
        fp8_e2=env('VV_FP8_E2', '1'),                       # the Cin 64 encoder layer in fp8 mode: '1' direct fp8 kernel, 'igemm', '0' bf16
        fp8_last=env('VV_FP8_LAST', 'direct'),              # the 128 -> 64 decoder layer in fp8 mode: 'direct', 'igemm', '0' bf16
        fp8_d5=env('VV_FP8_D5', '0') == '1',                # that layer hands e4m3fn to the final layer
        fp8_off=frozenset(n for n in env('VV_FP8_OFF', '').replace(' ', '').split(',') if n),   # layers kept on bf16: 'E5,D2'
        fp8_shaped=env('VV_FP8_SHAPED', '1') != '0')        # error diffusion over the taps in quant_fp8


def fp8_layers_off(policy, encoder, nlayers, sw):
    """Layers kept on bf16 operands in 'fp8' mode: VV_FP8_OFF plus what the policy excludes.  'mid' and 'most' are policy 'all' minus a
    set: 'mid' keeps fp8 on the two widest stride-2 layers of each side (E2, E3 / D3, D4 of the five-layer models), 'most' only takes
    the encoder tail back (the layer whose error moves the whole latent).  'wide' is a rule of the route functions."""
    off = set(sw.fp8_off)
    if policy in ('mid', 'most') and encoder:
        off.add('E%d' % nlayers)
    if policy == 'mid':
        off |= set('E%d' % (i + 1) for i in range(3, nlayers - 1)) if encoder else set('D%d' % (i + 1) for i in range(1, nlayers - 3))
    return off


def conv_route(side, cin, cout, dt, want_fp8, wide, training, sw):
    """Form of a stride-2 convolution [side^3 x cin] -> [(side/2)^3 x cout] on operands of dtype dt.  want_fp8: the engine is in fp8
    mode and neither the policy nor VV_FP8_OFF excludes the layer; wide: policy 'wide' (fp8 only where a direct fp8 kernel exists)."""
    lib = L.load()
    # Cin 64 (the second layer) has an fp8 form too (tap-pair rows); VV_FP8_E2=0 keeps it on the bf16 direct kernel
    if want_fp8 and (cin % 128 == 0 or (cin == 64 and sw.fp8_e2 != '0')):
        if sw.fp8_e2 != 'igemm' and lib.vv_conv3d_k4s2_direct_fp8_supported(side, cin, cout):
            # the widest encoder layer: fp8 twin of its direct kernel, same packed weights as the implicit GEMM
            return 'igemm_fp8' if sw.no_direct else 'direct_fp8'
        if not wide:
            return 'igemm_fp8'
    if not sw.no_skip:
        if lib.vv_conv3d_k4s2_pos_supported(side, cin, cout, dt):
            return 'pos'
        if lib.vv_conv3d_k4s2_skip_supported(side, cin, cout, dt):
            return 'skip'
    # (the training step has always taken the direct kernel whatever VV_NO_DIRECT says)
    if (training or not sw.no_direct) and lib.vv_conv3d_k4s2_direct_supported(side, cin, cout, dt):
        return 'direct'
    return 'igemm'


def convT_route(side, cin, cout, dt, want_fp8, wide, sw):
    """Form of a stride-2 transposed convolution [side^3 x cin] -> [(2 side)^3 x cout]; arguments as conv_route.  fp8 mode: the
    layers with Cin % 128 == 0 run on fp8 operands -- the 128 -> 64 layer on the fp8 twin of its direct kernel (VV_FP8_LAST=igemm: fp8
    implicit GEMM, VV_FP8_LAST=0: bf16 direct kernel), the others on the implicit GEMM."""
    lib = L.load()
    direct = not sw.no_direct and bool(lib.vv_convT3d_k4s2_direct_supported(side, cin, cout, dt))
    if want_fp8 and cin % 128 == 0:
        if direct and sw.fp8_last not in ('0', 'igemm') and lib.vv_convT3d_k4s2_direct_fp8_supported(side, cin, cout):
            return 'direct_fp8'
        if not wide and not (direct and sw.fp8_last == '0'):
            return 'igemm_fp8'
    if direct:
        # the 8^3 x 128 -> 16^3 x 64 layer of the 32^3 model: one whole sample resident in LDS per workgroup
        return 'whole' if not sw.no_whole and lib.vv_convT3d_k4s2_whole_supported(side, cin, cout, dt) else 'direct'
    if not sw.no_skip:
        if lib.vv_convT3d_k4s2_pos_supported(side, cin, cout, dt):
            return 'pos'
        if lib.vv_convT3d_k4s2_skip_supported(side, cin, cout, dt):
            return 'skip'
    return 'igemm'


def igemm_admits(cin, cout, dt):
    """The channel rule of the implicit GEMM's stride-2 forms (run_igemm, igemm.hip): input channels a power-of-two multiple of the K
    block (64 bf16 elements, 32 float32), output channels whole 16-byte stores (8 bf16, 4 float32).  The form every route function
    falls back to, so a layer it does not admit has no kernel."""
    bk, vec = (64, 8) if dt == L.VV_BF16 else (32, 4)
    q = cin // bk
    return cin > 0 and cin % bk == 0 and q & (q - 1) == 0 and cout > 0 and cout % vec == 0


@functools.lru_cache(maxsize=None)
def fused_tail(K5, E, Lz, lin, n1, variational, sw):
    """True when encoder tail -> reparam / KL -> Dense -> first decoder layer run as the fused launches of latent_tail.hip (bf16).  A pure
    function of the shapes and the switches, asked on every forward: cached."""
    # Measured: at the 32^3 model (K5 = n1 = 4096) the two fused launches take 0.028 ms against 0.045 ms for the five calls;
    # at the 64^3 model (K5 = n1 = 32768: 128 K slices of float32 slabs to sum, 8x the seed columns) 0.197 ms against 0.06 ms.
    if sw.no_latent_tail or K5 > 8192 or n1 > 8192:
        return False
    return bool(L.load().vv_latent_tail_supported(K5, E, Lz, lin, n1, variational, L.VV_BF16))


@functools.lru_cache(maxsize=None)
def fused_pos_tail(cin4, cout4, E, Lz, lin, n1, variational):
    """True when a 'pos' last stride-2 encoder layer cin4 -> cout4 and the fused tail behind it run as ONE call (the caller asks
    the no_pos_tail switch first: it decides before the encoder has to be packed)."""
    return bool(L.load().vv_conv_pos_latent_tail_supported(cin4, cout4, E, Lz, lin, n1, variational, L.VV_BF16))


def final_takes_fp8(side, batch, sw):
    """VV_FP8_D5=1: the fp8 direct kernel in front of the final layer hands it e4m3fn [side^3] maps (the final layer's sweep form, large
    batches).  Off by default: it is 5 % faster at 32^3 and not at all at 64^3, and takes the IoU delta at 64^3 from 6e-5 to 4e-4
    (gate 1e-3)."""
    return sw.fp8_d5 and side >= 8 and batch * (side // 8) ** 2 >= 128


_TORCH_DTYPE = {L.VV_F32: torch.float32, L.VV_BF16: torch.bfloat16, L.VV_FP8: torch.uint8}

# ---- weight images.  (direction, kind) -> (pack entry point, shape of the image, the entry point takes the element type)
CONV, CONVT = 0, 1            # also the `kind` codes of vv_pack_skip_images
IMAGES = {
    (CONV, 'igemm'): ('vv_pack_conv_k4', lambda cin, cout: (cout, 64 * cin), True),
    (CONV, 'skip'): ('vv_pack_conv_k4_skip', lambda cin, cout: (64 * cin * cout,), False),          # [tap][Cin/64][Cout][64]
    (CONVT, 'igemm'): ('vv_pack_convT_k4s2', lambda cin, cout: (8, cout, 8 * cin), True),
    (CONVT, 'skip'): ('vv_pack_convT_k4s2_skip', lambda cin, cout: (64 * cin * cout,), False),
    (CONVT, 'frag'): ('vv_pack_convT_k4s2_frag', lambda cin, cout: (64 * cin * cout,), False),
    (CONVT, 'frag_fp8'): ('vv_pack_convT_k4s2_frag_fp8', lambda cin, cout: (64 * cin * cout,), False),
}
# the image a form reads
ROUTE_IMAGE = {
    CONV: {'pos': 'skip', 'skip': 'skip', 'direct': 'igemm', 'direct_fp8': 'igemm', 'igemm': 'igemm', 'igemm_fp8': 'igemm'},
    CONVT: {'pos': 'skip', 'skip': 'skip', 'whole': 'skip', 'direct': 'frag', 'direct_fp8': 'frag_fp8', 'igemm': 'igemm', 'igemm_fp8': 'igemm'},
}
# What an engine packs for a layer: (before an evaluation, before a training step), the first image ahead of the folded BatchNorm
# vectors and the others behind them.  Evaluation keeps the implicit-GEMM image beside the form's own (and the fragment image
# beside the whole-sample one).  Training leaves the 'pos' / 'skip' images to the trainer, which batches them with the images of the
# data gradients (Trainer._prepack), and keeps the implicit-GEMM panel beside the fragment image.
ENGINE_IMAGES = {
    CONV: {'pos': (('igemm', 'skip'), ()), 'skip': (('igemm', 'skip'), ()), 'direct': (('igemm',), ('igemm',)),
           'direct_fp8': (('igemm',), ('igemm',)), 'igemm': (('igemm',), ('igemm',)), 'igemm_fp8': (('igemm',), ('igemm',))},
    CONVT: {'pos': (('igemm', 'skip'), ()), 'skip': (('igemm', 'skip'), ()), 'whole': (('igemm', 'frag', 'skip'), ('skip',)),
            'direct': (('igemm', 'frag'), ('igemm', 'frag')), 'direct_fp8': (('frag_fp8',), ('frag_fp8',)),
            'igemm': (('igemm',), ('igemm',)), 'igemm_fp8': (('igemm',), ('igemm',))},
}


def pack_image(direction, kind, w_keras, cin, cout, dt, st):
    """One weight image with elements of type dt, from a Keras kernel array (float32; for dt = VV_FP8 the e4m3fn-valued array
    engine.quant_fp8 returns)."""
    fn, shape, typed = IMAGES[direction, kind]
    out = torch.empty(shape(cin, cout), dtype=_TORCH_DTYPE[dt], device=w_keras.device)
    L.call(fn, L.ptr(w_keras), L.ptr(out), cin, cout, *((dt, st) if typed else (st,)))
    return out


# ---- launches.  call(fn, *args) issues one library call (the engines wrap it in their layer timer); wsp is a _Workspace.
# odt: element type of y for the engines' entry points; None = the training step's entry points (raw output in dt, which the
# trainer calls with scale = shift = None and act = 0: BatchNorm follows with batch statistics).
# schedule: vv_schedule of the 'pos' form (the other forms have only one); the workspace query serves either.
def _launch(fn, call, route, wsp, x, w, scale, shift, y, B, side, cin, cout, act, dt, odt, st, schedule=L.VV_SCHED_LATENCY):
    head = (L.ptr(x), L.ptr(w), L.ptr(scale), L.ptr(shift), L.ptr(y), B, side, cin, cout, act)
    if route == 'pos':
        ws = wsp.get(getattr(L.load(), fn + '_pos_workspace_bytes')(B, cin, cout))
        if schedule == L.VV_SCHED_LATENCY:
            call(fn + '_pos_fwd', *head, dt, L.ptr(ws), ws.numel(), st)
        else:
            call(fn + '_pos_fwd_ex', *head, schedule, L.ptr(ws), ws.numel(), st)
    elif route == 'direct_fp8':
        call(fn + '_direct_fp8_fwd', *head, odt, st)
    elif route == 'direct' and odt is not None and fn == 'vv_conv3d_k4s2':
        call(fn + '_direct_fwd_io', *head, dt, odt, st)          # (the transposed direct kernel stores dt only: no _io form)
    elif route in ('skip', 'whole', 'direct'):
        call('%s_%s_fwd' % (fn, route), *head, dt, st)
    else:
        idt = L.VV_FP8 if route == 'igemm_fp8' else dt
        ws = wsp.get(getattr(L.load(), fn + '_workspace_bytes')(B, side, cin, cout, idt))
        if odt is None:
            call(fn + '_fwd', *head, idt, L.ptr(ws), ws.numel(), st)
        else:
            call(fn + '_fwd_io', *head, idt, odt, L.ptr(ws), ws.numel(), st)


launch_conv = functools.partial(_launch, 'vv_conv3d_k4s2')
launch_convT = functools.partial(_launch, 'vv_convT3d_k4s2')
