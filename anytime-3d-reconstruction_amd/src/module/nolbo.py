"""Drop-in for the ModelNet model classes of the reference's src/module/nolbo.py:

    nolboSingleObject_modelnet_category_AE    (reference nolbo.py:1206-1385)
    nolboSingleObject_modelnet_category_VAE   (reference nolbo.py:1387-1592)

Same constructor arguments, methods, argument meaning and return tuples; the arithmetic is the MI355X HIP
library.  Host inputs are numpy float32 NDHWC arrays exactly as the reference's data loader produces
(src/dataset_loader/modelnet_dataset.py:83); device-resident torch tensors / DeviceArrays are accepted too and
skip the host->device copy.

The reference draws three random tensors inside these methods (the sampling epsilon, nolbo.py:1470; the
np.random mask, :1475; the prior epsilon, :1508) and the dropout rate/mask (:1423-1425).  They are drawn here
the same way by default (mask through np.random.choice with the same arguments, so seeding np.random
reproduces the reference's mask stream); the keyword-only `_eps`, `_mask`, `_eps2` arguments (an extension)
inject them, which is what makes bit-level parity tests possible.  With voxvae.set_mask_source('device') the uninjected keep
masks (dropout, missing latents) are drawn on the device instead, by the model's voxvae.masks.KeepMasks: no upload, and a
host twin that reproduces any step's mask; the default is the host draw.
"""
import ctypes
import os

import numpy as np
import torch

import src.net_core.autoencoder3D as ae3D
import src.net_core.darknet as darknet
import src.net_core.priornet as priornet
from voxvae import engine as _E
from voxvae import lib as _L
from voxvae.tensor import DeviceArray, as_device_f32


def _st():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _sample_kl_torch(mean, lv, mean_p, lv_p, eps, eps_p, take_z):
    """Sampling | prior / posterior choice | KL(q || prior) (function.py:35-38, 84-98) as torch autograd code: the comparison leg
    (latent='torch') of the HIP latent stages.  take_z: None (z itself) or bool [B, L], False where z_prior stands in -> z_in [B, L], kl [B]."""
    z = mean + torch.sqrt(torch.exp(lv)) * eps
    z_prior = mean_p + torch.sqrt(torch.exp(lv_p)) * eps_p
    z_in = z if take_z is None else torch.where(take_z, z, z_prior)
    return z_in, (0.5 * (lv_p - lv) + (torch.exp(lv) + (mean - mean_p) ** 2) / (2.0 * torch.exp(lv_p)) - 0.5).sum(-1)


def _pair_reg_torch(mean_p, lv_p, dist, cls=None):
    """The pairwise regulariser of a prior's outputs (function.py:40-71) -> [B]; cls [B, C]: only pairs of one class count."""
    d = (torch.abs(mean_p[:, None, :] - mean_p[None, :, :]) / torch.exp(0.5 * lv_p)[:, None, :]).sum(-1) - dist
    v = torch.where(d > 0, torch.zeros_like(d), d * d)
    if cls is not None:
        v = v * (torch.abs(cls[:, None, :] - cls[None, :, :]).sum(-1) <= 0).to(v.dtype)
    return v.sum(-1)


def _one_prior_latent_torch(e, pri, eps, eps_p, keep, dist):
    """The latent algebra of the models with ONE learned prior: what vv_prior_latent_train_fwd / _bwd compute.  e [B, 2L] = (mean | logVar),
    pri = the prior's (mean, logVar), keep None or [B, L] (1: the element is z's, else z_prior's) -> z_in [B, L], kl [B], reg [B]."""
    Lz = e.shape[1] // 2
    z_in, kl = _sample_kl_torch(e[:, :Lz], torch.clamp(e[:, Lz:], -10.0, 10.0), *pri, eps, eps_p, None if keep is None else keep == 1.)
    return z_in, kl, _pair_reg_torch(*pri, dist)


def _prior_checkpoints(cls):
    """Class decorator: the reference's savePrior<X> / loadPrior<X> for every (network attribute, structure attribute, X) of cls._priors;
    _ModelnetBase.saveModel / loadModel call them."""
    def add(net, structure, suffix):
        def save(self, save_path):
            getattr(self, net).save_weights(os.path.join(save_path, getattr(self, structure)['name']))

        def load(self, load_path, file_name=None):
            getattr(self, net).load_weights(os.path.join(load_path, file_name or getattr(self, structure)['name']))

        setattr(cls, 'savePrior' + suffix, save)
        setattr(cls, 'loadPrior' + suffix, load)

    for entry in cls._priors:
        add(*entry)
    return cls


class _ModelnetBase(object):
    _variational = True
    _keep_masks = None      # voxvae.mask_source() == 'device' when the model was built: its voxvae.masks.KeepMasks stream
    _priors = ()            # the learned prior networks: ((network attribute, structure attribute, X of savePrior<X>), ...)

    @property
    def _latent_dim(self):
        return self._enc_backbone_str['z_category_dim']

    def _buildModel(self):
        print('build Models...')
        self._encoder = ae3D.encoder3D(structure=self._enc_str)
        # ==============set decoder3D
        self._decoder = ae3D.decoder3D(structure=self._dec_str)
        self._enc_eng, self._dec_eng = self._encoder._engine, self._decoder._engine
        self._device = self._enc_eng.device
        self._act_dt = self._dec_eng.dt
        self._init_masks()
        print('done')

    def _init_masks(self):
        """Where the uninjected keep masks come from, read as the model is built (voxvae.set_mask_source): None = np.random on the
        host, the reference's calls; 'device' = a KeepMasks stream of this model's own (no upload, voxvae/masks.py)."""
        import voxvae
        from voxvae import masks as _M
        self._keep_masks = _M.KeepMasks(self._device) if voxvae.mask_source() == 'device' else None

    def _draw_keep(self, B, Lz, rate):
        """The device source's dropout mask [B, L] for this step, or None where the host draws it."""
        return None if self._keep_masks is None else self._keep_masks.dropout(B, Lz, rate)

    def _draw_dropout(self, B, Lz, rate=None, keep=None):
        """One step's inverted dropout on the latent (reference nolbo.py:586-588, 1423-1425) -> (keep [B, L] on the device, 1 / (1 - rate)):
        the rate ~ U[0,1) from np.random unless injected; the keep injected, else the model's KeepMasks stream when the masks are drawn on
        the device, else torch.rand(...) >= rate."""
        rate = float(np.random.rand()) if rate is None else float(rate)
        keep = self._draw_keep(B, Lz, rate) if keep is None else self._dev(keep)
        keep = (torch.rand(B, Lz, device=self._device) >= rate).float() if keep is None else keep
        return keep, 1.0 / (1.0 - rate)

    def _draw_mix(self, B, Lz, r, a=(True, False), missing_pr=0.3):
        """A training step's draw of what the decoder sees (nolbo.py:1042-1047, 1642-1647; :119-122 with a = (False, True) and 0.5):
        `rand > 0.5` -> None (z itself), else a [B, L] selector drawn per element from `a` with probabilities (1 - missing_pr, missing_pr)
        -- the category-only models' keep, 0 where z_prior stands in (the same RNG calls); `r['mix']` (bool) and `r['noise']` [B, L]
        inject them."""
        mix = bool(r['mix']) if 'mix' in r else not (np.random.rand() > 0.5)
        if not mix:
            return None
        return self._dev(r['noise'] if 'noise' in r else
                         np.random.choice(a=list(a), size=(B, Lz), p=[1. - missing_pr, missing_pr]).astype('float32')).contiguous()

    @staticmethod
    def _check_width(enc_out, width, layout):
        if enc_out.dim() != 2 or enc_out.shape[1] != width:
            raise ValueError('the encoder must emit [B, %d] (%s), got %s' % (width, layout, tuple(enc_out.shape)))

    # ---------------------------------------------------------------- device-side building blocks
    def _dev(self, a):
        return as_device_f32(a, self._device)

    def _dev_pair(self, a, b):
        """(input, target) on the device; an autoencoder's caller usually passes the SAME host array twice (the reference's
        scripts feed `output_images = input_images`): it is uploaded once (33.6 MB at 32^3, batch 256)."""
        x = self._dev(a)
        return x, (x if b is a else self._dev(b))

    def _draw_eps(self, B, eps=None):
        """A sampling / prior epsilon [B,L]: torch.randn for the reference's tf.random.normal (nolbo.py:1470, 1508) unless injected."""
        return torch.randn(B, self._latent_dim, dtype=torch.float32, device=self._device) if eps is None else self._dev(eps)

    def _draw_mask(self, B, missing_prob, mask=None, Lz=None):
        """The missing-latent mask [B,L] (1 = kept): reference nolbo.py:1475-1476, same RNG call, unless injected or the model draws
        its masks on the device."""
        if mask is None:
            Lz = self._latent_dim if Lz is None else Lz
            if self._keep_masks is not None:
                return self._keep_masks.missing(B, Lz, missing_prob)
            mask = np.reshape(np.random.choice(2, B * Lz, p=[missing_prob, 1. - missing_prob]), [B, Lz]).astype('float32')
        return self._dev(mask)

    def _enc_out(self, x, training=False):
        """What the latent is formed from: the voxel encoder's output (the image -> 3D model: its 2D encoder's)."""
        return self._enc_eng.forward(x)

    def _reparam(self, enc_out, eps=None, act_dt=None, want_stats=False):
        """(mean | logVar) [B,2L] -> slice | clip | sampling | KL (nolbo.py:1417-1420, 1464-1470) through vv_reparam_kl_fwd.
        Returns (z, z_act, kl, mean, clipped logVar), the last two None without want_stats."""
        Lz = self._latent_dim
        self._check_width(enc_out, 2 * Lz, 'mean | logVar')
        return _E.reparam_kl(enc_out, self._draw_eps(enc_out.shape[0], eps), Lz, self._act_dt if act_dt is None else act_dt,
                             want_stats=want_stats)

    def _encode_latent(self, x, eps=None):
        """encoder -> (slice | clip | sampling) for the VAE, identity for the AE.  Returns (z, z_act, kl)."""
        enc_out = self._enc_out(x)
        if not self._variational:
            return enc_out, (enc_out if self._act_dt == _L.VV_F32 else enc_out.to(torch.bfloat16)), None
        return self._reparam(enc_out, eps)[:3]

    def _decode_metrics(self, z_act, target, h1=None):
        out, _, stats, m = self._dec_eng.forward(z_act, target, want_metrics=True, h1=h1)
        return out, stats, m

    def _encode_decode_seed(self, x, eps=None):
        """encoder -> latent -> first decoder layer for the paths that decode the latent unchanged (getEval with
        missing_prob = 0, eval_forward_device): the fused latent tail when it applies, else the split calls.
        Returns (z, z_act, kl, h1 or None)."""
        if self._enc_eng is not None and _E.latent_tail_supported(self._enc_eng, self._dec_eng, self._variational):
            pos = _E.pos_latent_tail_supported(self._enc_eng, self._dec_eng, self._variational, x.shape[0])
            h = self._enc_eng.forward(x, stop_before_tail=True, stop_before_pos=pos)
            pos = pos and h.shape[1] == 4          # the layer in front of the tail was left to the fused call
            eps = self._draw_eps(x.shape[0], eps) if self._variational else None
            z, z_act, kl, _, h1 = _E.latent_tail(self._enc_eng, self._dec_eng, h, eps, self._variational, pos_layer=pos)
            return z, z_act, kl, h1
        return self._encode_latent(x, eps) + (None,)

    def _latent_training_mode(self, x, eps=None):
        """_encode_decode_seed's counterpart for training=True: the trainer's encoder forward (batch statistics)."""
        return self._train_helper().latent_training_mode(x, None if eps is None else self._dev(eps)) + (None,)

    def _eval_hooks(self, training, seed=False):
        """What differs between the forms of getEval: how the latent is obtained and how a latent is decoded.
            latent(x, eps) -> (z, z_act, kl, h1 or None)        decode(z_act, y, h1) -> (prediction, stats [B,4], metrics [4])
        Evaluation: the engines (seed: with the fused latent tail when it applies).  training=True (reference nolbo.py:1449, 1463,
        1496: `self._encoder(x, training=training)`): the trainer's forward halves -- BatchNorm normalises with batch statistics and
        moves the moving ones (momentum 0.99), no optimisation step.  In that mode the callers hand the decoder entry a FLOAT32 latent,
        which it casts (one more vv_convert in bf16), even where an activation-dtype copy exists (the trainer's z_act, _zero_masked's twin),
        and the latent ops write float32 only (`twin=False`): the launches of the copies this replaced, kept for identical results and
        traces -- inherited, not something the algorithm needs."""
        if training:
            return self._latent_training_mode, lambda z_act, y, h1: self._train_helper().decoder_training_mode(z_act, y)
        return (self._encode_decode_seed if seed else lambda x, eps: self._encode_latent(x, eps) + (None,)), self._decode_metrics

    def _out_pair(self, z, twin):
        """Buffers of a latent op's result: float32, the activation-dtype twin (the same tensor in f32 mode or without `twin`), its dtype code."""
        act_dt = self._act_dt if twin else _L.VV_F32
        o = torch.empty_like(z)
        return o, (o if act_dt == _L.VV_F32 else torch.empty(z.shape, dtype=torch.bfloat16, device=self._device)), act_dt

    def _mask_fill(self, z, mask, cats, twin=True):
        """z * mask with the zeros replaced by the prototypes' column means (nolbo.py:1477-1482) -> (float32, activation dtype)."""
        zf, zf_act, act_dt = self._out_pair(z, twin)
        _L.call('vv_latent_mask_fill', _L.ptr(z), _L.ptr(mask), _L.ptr(cats), cats.shape[0], _L.ptr(zf),
                None if zf_act is zf else _L.ptr(zf_act), act_dt, z.shape[0], z.shape[1], _st())
        return zf, zf_act

    def _latent_correct(self, z, mask, cats, idx, eps2, twin=True):
        """The prior sample cats[idx] + eps2 wherever mask == 0, z elsewhere (nolbo.py:1507-1510) -> (float32, activation dtype)."""
        zc, zc_act, act_dt = self._out_pair(z, twin)
        _L.call('vv_latent_correct', _L.ptr(z), _L.ptr(mask), _L.ptr(cats), _L.ptr(idx), _L.ptr(eps2), _L.ptr(zc),
                None if zc_act is zc else _L.ptr(zc_act), act_dt, z.shape[0], z.shape[1], _st())
        return zc, zc_act

    def _zero_masked(self, z, mask):
        """where(mask == 0, 0, z) (legacy body nolbo.py:1544-1548): the latent_correct kernel with a zero prototype table and
        zero epsilon.  Returns (float32, activation-dtype) copies."""
        B, Lz = z.shape
        zeros = lambda *shape, dtype=torch.float32: torch.zeros(shape, dtype=dtype, device=self._device)
        return self._latent_correct(z, mask, zeros(1, Lz), zeros(B, dtype=torch.int32), zeros(B, Lz))

    def _category_acc(self, z, cats, onehot, mask=None):
        B, Lz, C = z.shape[0], z.shape[1], cats.shape[0]
        idx = torch.empty(B, dtype=torch.int32, device=self._device)
        _L.call('vv_nearest_category', _L.ptr(z), _L.ptr(mask), _L.ptr(cats), C, _L.ptr(idx), B, Lz, _st())
        acc = None
        if onehot is not None:
            acc = torch.empty(1, dtype=torch.float32, device=self._device)
            _L.call('vv_category_accuracy', _L.ptr(idx), _L.ptr(onehot), C, _L.ptr(acc), B, _st())
        return idx, acc

    def _fit(self, inputs, eps, drop_mask, drop_rate):
        """One optimisation step (GradientTape + Adam.apply_gradients of the reference) through voxvae.train.Trainer."""
        x, y = self._dev_pair(*inputs)
        mask, scale = None, 1.0
        if self._dropout:      # reference nolbo.py:1423-1425: rate ~ U[0,1) per step, inverted dropout on z
            rate = float(np.random.rand()) if drop_rate is None else float(drop_rate)
            if drop_mask is None:
                drop_mask = self._draw_keep(x.shape[0], self._latent_dim, rate)
            if drop_mask is None:
                drop_mask = (np.random.rand(x.shape[0], self._latent_dim) >= rate).astype('float32')
            mask, scale = self._dev(drop_mask), 1.0 / (1.0 - rate)
        kl, stats, m = self._train_helper().step(x, y, None if eps is None else self._dev(eps), mask, scale)
        return kl, m

    # ---------------------------------------------------------------- public API (reference signatures)
    def getEval(self, inputs, category_vectors=None, training=False, missing_prob=0.0, *, _eps=None, _mask=None, _eps2=None):
        """reference nolbo.py:1449-1528 (VAE) / :1260-1332 (AE): returns the 10-tuple
        (pred, loss_shape, pr, rc, acc_cat, pred_corrected, loss_corrected, pr_corrected, rc_corrected, acc_cat_corrected),
        the last five being 0 when missing_prob == 0.
        Legacy form still used by the reference's train scripts (train_modelnet_category_VAE.py:83-84, body kept as
        the commented block nolbo.py:1530-1555): inputs=(x, y) without category_vectors -> (pred, loss_shape, pr, rc)."""
        if len(inputs) == 2 or category_vectors is None:
            return self._getEval_legacy(inputs, training, missing_prob, _eps, _mask)
        input_images, output_images, category_list = inputs
        from voxvae.hostio import PackedVoxels as _PV
        if not training and missing_prob == 0.0 and isinstance(input_images, (np.ndarray, _PV)) and isinstance(output_images, (np.ndarray, _PV)):
            out = self._getEval_host_chunked(input_images, output_images, category_list, category_vectors, _eps,
                                             lazy=getattr(self, '_lazy_host', False))
            if out is not None:
                return out
        x, y = self._dev_pair(input_images, output_images)
        onehot, cats = self._dev(category_list), self._dev(category_vectors)
        latent, decode = self._eval_hooks(training, seed=not missing_prob > 0)
        twin = not training
        z, z_act, _, h1 = latent(x, _eps)
        z_act = z_act if twin else z                                                  # training: float32 to the decoder entry (_eval_hooks)
        mask = None
        if missing_prob > 0:
            mask = self._draw_mask(z.shape[0], missing_prob, _mask)                   # :1475-1476
            z, z_act = self._mask_fill(z, mask, cats, twin)                           # :1477-1482
        _, acc = self._category_acc(z, cats, onehot)                                  # :1489-1494
        pred, _, m = decode(z_act, y, h1)                                             # :1496-1501
        self._z_category = DeviceArray(z)
        res = self._scored(pred, m, acc)
        if missing_prob == 0.0:
            return res + (0, 0, 0, 0, 0)
        idx, _ = self._category_acc(z, cats, None, mask)                              # :1505-1506
        zc, zc_act = self._latent_correct(z, mask, cats, idx, self._draw_eps(z.shape[0], _eps2), twin)   # :1507-1510
        _, acc_c = self._category_acc(zc, cats, onehot)                               # :1512-1518
        pred_c, _, mc = decode(zc_act, y, None)                                       # :1520-1527
        self._z_category_corrected = DeviceArray(zc)
        return res + self._scored(pred_c, mc, acc_c)

    @staticmethod
    def _scored(pred, m, acc=None):
        """(prediction, loss_shape, precision, recall[, category accuracy]) as the public methods return them."""
        out = (DeviceArray(pred), DeviceArray(m[0]), DeviceArray(m[1]), DeviceArray(m[2]))
        return out if acc is None else out + (DeviceArray(acc[0]),)

    def _getEval_legacy(self, inputs, training, missing_prob, _eps, _mask):
        """The 2-input form (commented body nolbo.py:1530-1555) -> (pred, loss_shape, pr, rc): the same two hooks, and with
        missing_prob > 0 the masked latent entries become 0 (:1544-1548)."""
        if training and self._enc_eng is None:
            raise ValueError('nolboSingleObject_VAE.getEval takes (images, voxels, one-hot) and category_vectors')
        x, y = self._dev_pair(inputs[0], inputs[1])
        latent, decode = self._eval_hooks(training)
        z, z_act, _, h1 = latent(x, _eps)
        if missing_prob > 0:
            zc, zc_act = self._zero_masked(z, self._draw_mask(z.shape[0], missing_prob, _mask))
            z_act = zc if training else zc_act                                            # training: as in getEval (_eval_hooks)
        pred, _, m = decode(z_act, y, h1)
        return self._scored(pred, m)

    def _getEval_host_chunked(self, input_images, output_images, category_list, category_vectors, _eps, lazy=False):
        """getEval(missing_prob=0) on HOST arrays (the reference's calling convention, test_modelnet_VAE.py:114-130) as a
        pipeline over sample ranges: the upload of chunk k+1 runs under the kernels of chunk k, the download of chunk k's
        prediction (into a recycled pinned block) under the kernels of chunk k+1 -- two streams, this model's one pair of
        engines (per-stream workspaces).  Every kernel of the path treats samples independently with a batch-size-independent
        summation order, so the result is the whole-batch result bit for bit (tests/test_gpu_api.py).  Returns None when the
        batch is too small to split or no pinned block is available (the caller then takes the plain path).
        lazy (voxvae.streams.HostPipeline): nothing here waits for the device -- the prediction's download is enqueued behind the
        kernels and the returned HostPrediction waits for it on first access; ONE pass over the whole batch by default (the overlap
        comes from the NEXT batch, issued by the pipeline on another stream, and whole-batch kernels fill the chip)."""
        from voxvae import hostio as _H
        if self._enc_eng is None or input_images.ndim != 5:
            return None                                  # the image -> 3D model: its inputs are images / head outputs, not voxel grids
        B = int(input_images.shape[0])
        # Two chunks pay when the download is the long pole (float32 probabilities: 33.6 MB at the PCIe rate = 0.60 ms beside 0.49 ms of
        # kernels); with the uint8 occupancy return (0.16 ms) one whole-batch pass is faster than two half-batch ones, whose
        # one-workgroup-per-sample kernels fill half the chip each (profiles/r04_host_chunks.json: 0.94 against 1.05 ms per call)
        nchunk = int(os.environ.get('VV_HOST_CHUNKS', '1' if lazy else ('2' if _H.prediction_host_dtype() == 'float32' else '1')))

        def usable(a):      # a float32 C-contiguous array, or a bit-packed host batch (voxvae/hostio.py: 1 bit per voxel over PCIe)
            return isinstance(a, _H.PackedVoxels) or (a.dtype == np.float32 and a.flags['C_CONTIGUOUS'])

        def upload(a, lo, hi):
            return a.to_device(dev, lo, hi) if isinstance(a, _H.PackedVoxels) else torch.from_numpy(a[lo:hi]).to(dev)

        if (nchunk < 2 and not lazy) or nchunk < 1 or B < 64 * nchunk or not usable(input_images):
            return None
        same = output_images is input_images
        if not same and (not usable(output_images) or tuple(output_images.shape) != tuple(input_images.shape)):
            return None
        pd = _H.prediction_host_dtype()
        host, hview = _H.pinned_array(tuple(input_images.shape), pd)
        if host is None:
            return None
        dev = self._device
        main = torch.cuda.current_stream(dev)
        if lazy and nchunk == 1:
            io_streams = [main]                     # the pipeline gives every batch in flight its own stream: no fork needed
        else:
            if getattr(self, '_io_streams', None) is None or len(self._io_streams) != nchunk:
                self._io_streams = [torch.cuda.Stream(device=dev) for _ in range(nchunk)]
            io_streams = self._io_streams
        eps = self._draw_eps(B, _eps) if self._variational else None
        onehot, cats = self._dev(category_list), self._dev(category_vectors)
        self._enc_eng.ensure_packed()               # weight packing (first call / after a weight change) stays on the caller's stream
        self._dec_eng.ensure_packed()
        bounds = [B * k // nchunk // 4 * 4 for k in range(nchunk)] + [B]
        zs, stats, preds = [], [], []
        for k, s in enumerate(io_streams):
            lo, hi = bounds[k], bounds[k + 1]
            if s is not main:
                s.wait_stream(main)
            with torch.cuda.stream(s):
                # pageable source, synchronous copy at the PCIe rate.  (Staging the chunk through a pinned block to make the upload
                # asynchronous was measured and is NOT used: an async host -> device copy issued beside running kernels took 10-50x
                # longer on this platform -- profiles/microbench/mb_pin.py: 78 ms against 14 ms for two matmuls with and without it.)
                x = upload(input_images, lo, hi)
                y = x if same else upload(output_images, lo, hi)
                z, z_act, _, h1 = self._encode_decode_seed(x, None if eps is None else eps[lo:hi])
                pred, _, st_ = self._dec_eng.forward(z_act, y, h1=h1)
                hview[lo:hi].copy_(_H.device_prediction_as(pred), non_blocking=True)
            for t in (z, st_, pred):
                t.record_stream(main)
            zs.append(z); stats.append(st_); preds.append(pred)
        for s in io_streams:
            if s is not main:
                main.wait_stream(s)
        z = torch.cat(zs, dim=0)
        m = _E.shape_metrics(torch.cat(stats, dim=0))
        _, acc = self._category_acc(z, cats, onehot)
        self._z_category = DeviceArray(z)
        ready = None
        if lazy:                                    # the caller's stream has joined every chunk stream above: one event covers the downloads
            ready = [torch.cuda.Event()]
            ready[0].record(main)
        else:
            for s in io_streams:                    # the host array is handed out: its downloads must have landed
                s.synchronize()
        return (_H.HostPrediction(host, preds, ready), DeviceArray(m[0]), DeviceArray(m[1]), DeviceArray(m[2]), DeviceArray(acc[0]), 0, 0, 0, 0, 0)

    def _train_helper(self):
        from voxvae import train as _T
        if getattr(self, '_trainer', None) is None:
            import torch.distributed as dist
            world = dist.get_world_size() if (dist.is_available() and dist.is_initialized()) else 1
            self._trainer = _T.Trainer(self._enc_eng, self._dec_eng, self._variational, self._learning_rate, world_size=world)
        return self._trainer

    def getLatent(self, inputs, *, _eps=None):
        """reference nolbo.py:1557-1566 (VAE: a SAMPLED z) / :1355-1358 (AE: the encoder output) -> numpy [B,L]."""
        z, _, _ = self._encode_latent(self._dev(inputs), _eps)
        return np.array(DeviceArray(z))

    # ---------------------------------------------------------------- sampled-mean reconstruction (an extension)
    def _posterior(self, x):
        """encoder -> (mean, clipped logVar) [B,L] through the class's own latent op (vv_reparam_kl_fwd's outputs; nolbo.py:1417-1420);
        classes without a posterior (the autoencoder) raise ValueError."""
        if not self._variational:
            raise ValueError('%s has no posterior to sample from (an autoencoder): getSampledEval needs a variational class' % type(self).__name__)
        enc_out = self._enc_out(x)
        zero = torch.zeros(enc_out.shape[0], self._latent_dim, dtype=torch.float32, device=self._device)
        return self._reparam(enc_out, zero, want_stats=True)[3:]

    def getSampledShape(self, mean, logvar, sampling_num=32, target=None, *, _eps=None, max_decode_batch=256):
        """The "anytime" reconstruction of the reference's nolbo_test.py:169-177 at latent level: `sampling_num` latents
        mean + sqrt(exp(logvar)) * eps per object, every one decoded, the occupancy probabilities averaged -- the average formed
        inside the last decoder layer's kernel.  mean / logvar: [B,L], host or device; `_eps` [B,K,L] injects the draw (torch.randn
        otherwise).  max(1, max_decode_batch // sampling_num) objects go through the decoder per pass, so the activation memory is
        that of max_decode_batch samples; an object's result does not depend on the pass it lands in.
        Returns DeviceArray pred_mean [B,D,D,D,1], or (pred_mean, loss_shape, pr, rc) of the AVERAGED prediction when `target`
        [B,D,D,D,1] is given (means over all B objects, nolbo.py:1498-1501)."""
        K = int(sampling_num)
        if K < 1:
            raise ValueError('sampling_num must be >= 1, got %r' % (sampling_num,))
        mean, logvar = self._dev(mean), self._dev(logvar)
        B, Lz = mean.shape
        if tuple(logvar.shape) != (B, Lz) or Lz != self._dec_eng.L:
            raise ValueError('mean / logvar must both be [B,%d], got %s and %s' % (self._dec_eng.L, tuple(mean.shape), tuple(logvar.shape)))
        eps = torch.randn(B, K, Lz, dtype=torch.float32, device=self._device) if _eps is None else self._dev(_eps)
        if tuple(eps.shape) != (B, K, Lz):
            raise ValueError('_eps must be [%d,%d,%d], got %s' % (B, K, Lz, tuple(eps.shape)))
        y = None if target is None else self._dev(target)
        per = max(1, int(max_decode_batch) // K)
        preds, stats = [], []
        for b0 in range(0, B, per):
            b1 = min(B, b0 + per)
            _, z_act = _E.sample_latents(mean[b0:b1], logvar[b0:b1], eps[b0:b1], self._act_dt)
            p, s, _ = self._dec_eng.forward_mean(z_act, K, None if y is None else y[b0:b1], want_metrics=False)   # metrics: over all B, below
            preds.append(p)
            stats.append(s)
        pred = preds[0] if len(preds) == 1 else torch.cat(preds)
        if y is None:
            return DeviceArray(pred)
        m = _E.shape_metrics(stats[0] if len(stats) == 1 else torch.cat(stats))
        return self._scored(pred, m)

    def getSampledEval(self, inputs, sampling_num=32, *, _eps=None):
        """inputs = (x, y): the encoder runs once per object, `sampling_num` latents are drawn from its posterior (mean and the clipped
        logVar of this class's latent op) and getSampledShape scores their averaged reconstruction against y
        -> (pred_mean, loss_shape, pr, rc).  Classes without a posterior (the autoencoder) raise ValueError."""
        if not self._variational:       # before anything is uploaded
            return self._posterior(None)
        x, y = self._dev_pair(inputs[0], inputs[1])
        mean, logvar = self._posterior(x)
        return self.getSampledShape(mean, logvar, sampling_num, y, _eps=_eps)

    def getSampledPoints(self, mean, logvar, dims, pose=None, sampling_num=32, prob=0.5, surface_only=False, *, _eps=None):
        """getSampledShape followed by voxvae.points.voxel_points on the averaged prediction: the reference's nolbo_test.getPred ->
        visualizer.getObjectInRealWorld (objRescaleTransform, visualizer.py:171-188) at latent level, without the probabilities
        leaving the device.  dims [B,3] = (h, w, l) per object, pose None / [4,4] / [B,4,4].  Returns a voxvae.points.PointCloud
        (`.split()` is the reference's list of [n_b,3] arrays); the count's 8-byte total is the one thing read back."""
        from voxvae.points import voxel_points
        pred = self.getSampledShape(mean, logvar, sampling_num, _eps=_eps)
        return voxel_points(pred, dims, pose, prob=prob, surface_only=surface_only)

    def getSampledObjects(self, mean, logvar, bbox2D, bbox3D, sin, cos, image_size, sampling_num=32, proj_mat=None, proj_mat_inv=None,
                          prob=0.5, surface_only=False, *, _eps=None):
        """Detections in, posed point clouds out: getSampledShape for every detection's latent, voxvae.pose.object_poses for the
        detections' boxes and angles, then ObjectPoses.points on the kept ones -- what a caller of the reference's
        nolbo_test.getPred(...) followed by visualizer.getObjectInRealWorld(...) gets, without a grid or a pose leaving the device.
        mean / logvar [n,L]; bbox2D [n,5] normalised, bbox3D [n,3] = (w, h, l), sin / cos [n,3]; image_size = (cols, rows); proj_mat
        None: the KITTI matrix.  Returns (ObjectPoses, PointCloud or None when nothing is kept); the 4-byte count of kept detections
        and the cloud's 8-byte total are what is read back."""
        from voxvae.pose import KITTI_PROJ_MAT, object_poses
        pred = self.getSampledShape(mean, logvar, sampling_num, _eps=_eps)
        poses = object_poses(self._dev(bbox2D), self._dev(bbox3D), self._dev(sin), self._dev(cos), image_size,
                             KITTI_PROJ_MAT if proj_mat is None else proj_mat, proj_mat_inv)
        return poses, poses.points(pred, prob=prob, surface_only=surface_only)

    # ---------------------------------------------------------------- precision / recall curves (an extension)
    def getPRCurve(self, inputs, curve, category_vectors=None, missing_prob=0.0, sampling_num=0, corrected=None, *, group=None,
                   training=False, _eps=None, _mask=None, _eps2=None):
        """getEval (or, with sampling_num > 0, getSampledEval over that many latents per object) followed by one more launch that
        adds this batch's (target, prediction) to `curve`, a voxvae.prcurve.PRCurve -- the threshold sweep the reference runs on the
        host over the saved `_gt.npy` / `_pred.npy` (modelnetAE3.ipynb cell 2) without the probabilities leaving the device.  With
        missing_prob > 0 the corrected prediction is added to `corrected`, a second PRCurve, when one is given.  group: the curves'
        per-sample group (int [B] or one-hot [B, G], e.g. the batch's class list for per-category curves).  The target is uploaded
        once and shared with the evaluation.  Returns what the underlying call returns; nothing here synchronises."""
        y = self._dev(inputs[1])
        inputs = ((y if inputs[0] is inputs[1] else inputs[0]), y) + tuple(inputs[2:])
        if sampling_num > 0:
            if missing_prob or training or _mask is not None or _eps2 is not None:
                raise ValueError('the sampled-mean reconstruction takes neither missing_prob nor training / _mask / _eps2')
            out = self.getSampledEval((inputs[0], y), sampling_num, _eps=_eps)
        else:
            # positional: the second argument is `category_indices` in the class with a learned prior
            out = self.getEval(inputs, *(() if category_vectors is None else (category_vectors,)), training=training,
                               missing_prob=missing_prob, _eps=_eps, _mask=_mask, _eps2=_eps2)
        curve.update(y, out[0], group=group)
        if corrected is not None and missing_prob > 0 and len(out) == 10:
            corrected.update(y, out[5], group=group)
        return out

    def eval_forward_device(self, x, y, eps=None):
        """Device-resident core of getEval(missing_prob=0) (reference nolbo.py:1463-1501): what bench.py times.
        x, y: float32 CUDA tensors [B,D,D,D,1]; returns (pred, stats [B,4], metrics [4], kl [B] or None), all on device."""
        z, z_act, kl, h1 = self._encode_decode_seed(x, eps)
        pred, stats, m = self._decode_metrics(z_act, y, h1)
        return pred, stats, m, kl

    # ---------------------------------------------------------------- checkpoints (reference nolbo.py:1568-1592)
    def saveEncoder(self, save_path):
        file_name = self._enc_str['name']
        self._encoder.save_weights(os.path.join(save_path, file_name))

    def saveDecoder(self, save_path):
        file_name = self._dec_str['name']
        self._decoder.save_weights(os.path.join(save_path, file_name))

    def saveModel(self, save_path):
        self.saveEncoder(save_path=save_path)
        self.saveDecoder(save_path=save_path)
        for p in self._priors:
            getattr(self, 'savePrior' + p[2])(save_path=save_path)

    def loadEncoder(self, load_path, file_name=None):
        if file_name == None:
            file_name = self._enc_str['name']
        self._encoder.load_weights(os.path.join(load_path, file_name))

    def loadDecoder(self, load_path, file_name=None):
        if file_name == None:
            file_name = self._dec_str['name']
        self._decoder.load_weights(os.path.join(load_path, file_name))

    def loadModel(self, load_path):
        self.loadEncoder(load_path=load_path)
        self.loadDecoder(load_path=load_path)
        for p in self._priors:
            getattr(self, 'loadPrior' + p[2])(load_path=load_path)


class nolboSingleObject_modelnet_category_AE(_ModelnetBase):
    """reference nolbo.py:1206-1385."""
    _variational = False

    def __init__(self, nolbo_structure,
                 learning_rate=1e-4,
                 dropout=False):
        self._enc_backbone_str = nolbo_structure
        self._enc_str = nolbo_structure['encoder']
        self._dec_str = nolbo_structure['decoder']
        self._dropout = dropout
        self._learning_rate = learning_rate
        self._buildModel()

    def fit(self, inputs, *, _mask=None, _rate=None):
        """reference nolbo.py:1230-1258 -> (loss_shape, pr, rc)."""
        _, m = self._fit(inputs, None, _mask, _rate)
        return DeviceArray(m[0]), DeviceArray(m[1]), DeviceArray(m[2])


class nolboSingleObject_modelnet_category_VAE(_ModelnetBase):
    """reference nolbo.py:1387-1592."""
    _variational = True

    def __init__(self, nolbo_structure,
                 dropout=False,
                 learning_rate=1e-4):
        self._enc_backbone_str = nolbo_structure
        self._enc_str = nolbo_structure['encoder']
        self._dec_str = nolbo_structure['decoder']
        self._dropout = dropout
        self._learning_rate = learning_rate
        self._buildModel()

    def fit(self, inputs, *, _eps=None, _mask=None, _rate=None):
        """reference nolbo.py:1411-1447 -> (loss_kl, loss_shape, pr, rc)."""
        kl, m = self._fit(inputs, _eps, _mask, _rate)
        return DeviceArray(kl.mean()), DeviceArray(m[0]), DeviceArray(m[1]), DeviceArray(m[2])


class nolboSingleObject_VAE(_ModelnetBase):
    """The reference's image -> 3D model, nolbo.py:750-982 (BASELINE.json configs[2], test_pascal_VAE_dr.py): decoder3D +
    losses + latent masking / prior correction + modality dropout run on the HIP path exactly as in the modelnet classes
    (the reference's getEval bodies are line-for-line the same algorithm, nolbo.py:856-928 vs 1449-1528).

    The 2D image encoder is outside the voxel hot path and runs on stock PyTorch ops:
    `backbone_style=darknet.Darknet19` builds the backbone and, as the reference does (nolbo.py:775-783), a `head2D` on
    top of it from `nolbo_structure['encoder_head']`; any other callable images -> features works as `encoder_backbone`.
    With neither, `input_images` are taken to BE head outputs [B, 2*z_dim] (synthetic head features, SURVEY §8d
    config 3).  fit() (nolbo.py:786-833) trains all three: the decoder step runs on the HIP path and hands back
    d loss / d head-output, which continues through the 2D encoder by torch autograd (f32 models only)."""
    _variational = True

    def __init__(self, nolbo_structure,
                 backbone_style=None, encoder_backbone=None,
                 dropout=False,
                 learning_rate=1e-4):
        self._enc_backbone_str = nolbo_structure['encoder_backbone']
        self._enc_head_str = nolbo_structure.get('encoder_head')
        self._dec_str = nolbo_structure['decoder']
        self._backbone_style = backbone_style
        self._encoder_backbone = encoder_backbone
        self._dropout = dropout
        self._learning_rate = learning_rate
        self._buildModel()

    @property
    def _latent_dim(self):
        return self._enc_backbone_str['z_dim']

    def _buildModel(self):
        print('build Models...')
        # ==============set decoder3D
        self._decoder = ae3D.decoder3D(structure=self._dec_str)
        self._enc_eng, self._dec_eng = None, self._decoder._engine      # no voxel encoder: the latent comes from the 2D encoder
        self._device = self._dec_eng.device
        self._act_dt = self._dec_eng.dt
        if self._encoder_backbone is None and self._backbone_style is not None:
            self._encoder_backbone = self._backbone_style(name=self._enc_backbone_str['name'], device=self._device)
        # ==============set encoder head (nolbo.py:775-783)
        self._encoder_head = None
        if self._encoder_backbone is not None and self._enc_head_str is not None and hasattr(self._encoder_backbone, 'output_shape'):
            self._encoder_head = darknet.head2D(name=self._enc_head_str['name'],
                                                input_shape=self._encoder_backbone.output_shape[1:],
                                                output_dim=self._enc_head_str['output_dim'],
                                                filter_num_list=self._enc_head_str['filter_num_list'],
                                                filter_size_list=self._enc_head_str['filter_size_list'],
                                                last_pooling='max', activation=self._enc_head_str['activation'],
                                                device=self._device)
        self._trainer2d = None
        self._init_masks()
        print('done')

    def _encoder_2d(self, x, training=False):
        if self._encoder_backbone is None:
            return x
        f = self._encoder_backbone(x, training=training) if self._encoder_head is not None else self._encoder_backbone(x)
        f = darknet.last_output(f)                           # Darknet53 / Darknet53Tiny give tuples: the head takes the last map
        return self._encoder_head(f, training=training) if self._encoder_head is not None else f

    def _enc_out(self, x, training=False):
        return self._dev(self._encoder_2d(x, training=training)).contiguous()

    def _latent_training_mode(self, x, eps=None):
        """Reference nolbo.py:856-928 passes `training` to the backbone and the head (torch modules) as well as to the decoder."""
        with torch.no_grad():
            enc_out = self._enc_out(x, training=True)
        return self._reparam(enc_out, eps, _L.VV_F32)[:3] + (None,)

    def _train_helper(self):
        """Training-mode forwards need the decoder's half only: a trainer without gradient / optimiser state."""
        from voxvae import train as _T
        if getattr(self, '_fwd_dec', None) is None:
            self._fwd_dec = _T.Trainer.forward_only(dec=self._dec_eng)
        return self._fwd_dec

    def _dev(self, a):
        if callable(getattr(a, 'numpy', None)) and not isinstance(a, (torch.Tensor, DeviceArray)):
            a = a.numpy()
        return as_device_f32(a, self._device)

    # ---------------------------------------------------------------- what the fits of the image family share
    def _image_trainer(self, variational=False):
        """(the decoder's Trainer, torch Adam over whichever of backbone, head and prior networks are torch modules -- None without
        parameters), built by the first fit."""
        if self._trainer2d is None:
            from voxvae import train as _T
            self._trainer2d = _T.Trainer(None, self._dec_eng, variational=variational, learning_rate=self._learning_rate)
            mods = [self._encoder_backbone, self._encoder_head] + [getattr(self, p[0]) for p in self._priors]
            params = [p for m in mods if isinstance(m, torch.nn.Module) for p in m.parameters()]
            self._opt2d = torch.optim.Adam(params, lr=self._learning_rate, eps=1e-7) if params else None   # Keras epsilon
        return self._trainer2d, self._opt2d

    def _l2_terms(self):
        """The l2 terms of head, backbone and prior networks as a list of their one sum, [] without any (the decoder's: the trainer's l2=)."""
        l2 = [l for m in [self._encoder_head, self._encoder_backbone] + [getattr(self, p[0]) for p in self._priors] if hasattr(m, 'losses')
              for l in m.losses]
        return [torch.stack(l2).sum()] if l2 else []

    def _head_output_training(self, input_images):
        """The 2D encoder's output in training mode; one without a graph (no parameters, or head outputs fed in) is moved to the device."""
        enc_out = self._encoder_2d(input_images, training=True)
        return enc_out if torch.is_tensor(enc_out) and enc_out.requires_grad else self._dev(enc_out)

    def fit(self, inputs, _eps=None, _dropout=None):
        """nolbo.py:786-833: (input_images, output_images) -> (loss_kl, loss_shape, pr, rc).  total = KL + shape + the l2
        terms of the 2D head; Adam(learning_rate) on backbone + head (torch) and decoder (HIP)."""
        input_images, output_images = inputs
        y = self._dev(output_images)
        trainer, opt = self._image_trainer(variational=True)
        enc_out = self._encoder_2d(input_images, training=True) if opt is not None else self._dev(self._encoder_2d(input_images))
        B = enc_out.shape[0]
        eps = self._draw_eps(B, _eps)
        drop_mask, drop_scale = self._draw_dropout(B, self._latent_dim, *(_dropout or ())) if self._dropout else (None, 1.0)
        kl, stats, metrics, de = trainer.step_from_latent(enc_out.detach().contiguous(), y, eps, drop_mask, drop_scale,
                                                          l2=ae3D.L2_REG)               # + decoder.losses, nolbo.py:819-823
        if opt is not None:
            opt.zero_grad(set_to_none=True)
            reg = self._l2_terms()
            enc_out.backward(de, retain_graph=bool(reg))
            for t in reg:
                t.backward()
            opt.step()
        m = metrics.cpu().numpy()
        return float(kl.mean().item()), float(m[0]), float(m[1]), float(m[2])

    def saveEncoderBackbone(self, save_path):
        if hasattr(self._encoder_backbone, 'save_weights'):
            self._encoder_backbone.save_weights(os.path.join(save_path, self._enc_backbone_str['name']))

    def saveEncoderHead(self, save_path):
        if self._encoder_head is not None:
            self._encoder_head.save_weights(os.path.join(save_path, self._enc_head_str['name']))

    def saveEncoder(self, save_path):
        self.saveEncoderBackbone(save_path)
        self.saveEncoderHead(save_path)

    def loadEncoderBackbone(self, load_path, file_name=None):
        if hasattr(self._encoder_backbone, 'load_weights'):
            self._encoder_backbone.load_weights(os.path.join(load_path, file_name or self._enc_backbone_str['name']))

    def loadEncoderHead(self, load_path, file_name=None):
        if self._encoder_head is not None:
            self._encoder_head.load_weights(os.path.join(load_path, file_name or self._enc_head_str['name']))

    def loadEncoder(self, load_path, file_name=None):
        self.loadEncoderBackbone(load_path)
        self.loadEncoderHead(load_path)


@_prior_checkpoints
class nolboSingleObject_modelnet_category_only(_ModelnetBase):
    """reference nolbo.py:1594-1787: the VAE with a learned class-conditional prior.  Encoder, decoder, losses and the
    missing-latent correction run on the HIP path as in nolboSingleObject_modelnet_category_VAE -- getEval is that class's
    getEval with the prototype table replaced by the prior network's means over `category_indices` (nolbo.py:1685-1688).
    The prior network (a 40 -> ... -> L MLP, src/net_core/priornet.py) and the [B, L] latent algebra of fit() -- KL to the
    learned prior, prior / posterior mixing, the pairwise regulariser -- are outside the voxel path (SURVEY §8(f)
    rank 2) and run by default as torch autograd code between the HIP encoder and decoder (voxvae.train.Trainer.step_custom_latent);
    fit(latent='hip') puts the two launches of csrc/prior_latent.hip in the closure's place."""
    _variational = True
    _priors = (('_priornet_class', '_prior_class_str', 'Category'),)

    def __init__(self, nolbo_structure,
                 learning_rate=1e-4):
        self._enc_backbone_str = nolbo_structure
        self._enc_str = nolbo_structure['encoder']
        self._dec_str = nolbo_structure['decoder']
        self._prior_class_str = nolbo_structure['prior_class']
        self._dropout = False
        self._learning_rate = learning_rate
        self._buildModel()
        # ==============set prior network
        self._priornet_class = priornet.priornet(structure=self._prior_class_str, device=self._device)
        self._trainer_c = None

    def fit(self, inputs, dropout=False, *, latent='torch', _rand=None):
        """nolbo.py:1620-1676: (x, y, onehot) -> (loss_kl, loss_shape, loss_reg, pr, rc); total = KL(q || prior) + shape +
        0.01 reg.  `_rand` (tests) = dict(eps, eps_prior, mix (bool), noise [B,L], drop_rate, drop_keep [B,L]).
        latent='torch' (the default): the latent algebra is the autograd closure below; latent='hip': ONE vv_prior_latent_train_fwd
        and ONE vv_prior_latent_train_bwd stand in its place (voxvae.prior_latent.latent_stage), the dropout through vv_mask_scale
        forward and on dz."""
        from voxvae import train as _T
        if latent not in ('hip', 'torch'):
            raise ValueError("latent must be 'hip' or 'torch', got %r" % (latent,))
        input_images, output_images, category_list = inputs
        x, y = self._dev_pair(input_images, output_images)
        onehot = self._dev(category_list)
        B, Lz = x.shape[0], self._latent_dim
        if self._trainer_c is None:
            self._trainer_c = _T.Trainer(self._enc_eng, self._dec_eng, variational=False, learning_rate=self._learning_rate)
            self._opt_prior = torch.optim.Adam(self._priornet_class.parameters(), lr=self._learning_rate, eps=1e-7)
        r = _rand or {}
        eps, eps_p = self._draw_eps(B, r.get('eps')).contiguous(), self._draw_eps(B, r.get('eps_prior')).contiguous()
        noise = self._draw_mix(B, Lz, r)                                       # :1642: z itself with probability 1/2
        drop = self._draw_dropout(B, Lz, r.get('drop_rate'), r.get('drop_keep')) if dropout else None
        dist = 2.0 * Lz

        def latent_torch(enc_out):
            z_in, kl, reg = _one_prior_latent_torch(enc_out, self._priornet_class(onehot, training=True), eps, eps_p, noise, dist)
            if drop is not None:
                z_in = z_in * drop[0] * drop[1]
            kl, reg = kl.mean(), reg.mean()                                           # function.py:84-98; :40-71, no class input (:1663)
            return z_in, kl + 0.01 * reg, (kl.detach(), reg.detach())

        def latent_hip(enc_out):
            from voxvae import prior_latent as _PL
            mean_p, lv_p = self._priornet_class(onehot, training=True)
            z_in, extra, kl, reg, _ = _PL.latent_stage(enc_out, mean_p, lv_p, eps, eps_p, noise, dist, 0.01)
            if drop is not None:
                z_in = _PL.mask_scale(z_in, drop[0].contiguous(), drop[1])
            return z_in, extra, (kl.mean(), reg.mean())

        self._opt_prior.zero_grad(set_to_none=True)
        stats, m, (kl, reg) = self._trainer_c.step_custom_latent(x, y, latent_hip if latent == 'hip' else latent_torch)
        self._opt_prior.step()
        return DeviceArray(kl), DeviceArray(m[0]), DeviceArray(reg), DeviceArray(m[1]), DeviceArray(m[2])

    def getEval(self, inputs, category_indices=np.identity(40), training=False, missing_prob=0.0, *, _eps=None, _mask=None, _eps2=None):
        """nolbo.py:1678-1754 -> the 10-tuple of the VAE class, classified / corrected against the prior means."""
        # reference :1686, :1691, :1724: `training` goes to the prior network, the encoder and the decoder alike
        mean_prior, _ = self._priornet_class(np.asarray(category_indices, dtype='float32'), training=bool(training))
        return _ModelnetBase.getEval(self, inputs, category_vectors=mean_prior.detach().contiguous(), training=training,
                                     missing_prob=missing_prob, _eps=_eps, _mask=_mask, _eps2=_eps2)


class _PriorImageModel(nolboSingleObject_VAE):
    """The image models with learned prior networks: the image encoder and the decoder are nolboSingleObject_VAE's, and fit's span between
    the head output and the decoder step (voxvae.train.Trainer.step_decoder) is a latent stage with ONE forward and ONE backward launch
    (latent='hip') or the same algebra as torch autograd code (latent='torch'); its gradients continue through the 2D encoder and the prior
    networks by torch autograd.  The training step is written once, here; a subclass names its prior networks (_priors, the structure
    attribute being '_<structure key>_str') and the reference's constants, and supplies what differs:
        _enc_layout() -> (width of the head output, its layout in words)
        _prior_outputs(onehots) -> the prior networks in training mode on the step's one-hots: the tuple of their (mean, logVar) tensors
        _decoder_input_draw(B, r) -> the step's draw of what the decoder sees: None = z, or a [B, L] selector between z and z_prior
        _latent_stage(latent, e, pri, eps, eps_p, draw, onehots) -> (z_in [B, L], extra = the latent terms of the total loss, kl [B],
            reg [B], bfloat16 twin of z_in or None) on either leg;    _debug_extra(draw) -> the class's own keys of the _debug capture"""
    _reg_weight = 1.0        # the regulariser's weight in the total loss
    _network_l2 = True       # whether the sub-models' l2 terms are part of the total loss

    def __init__(self, nolbo_structure, backbone_style=None, encoder_backbone=None, learning_rate=1e-4):
        for _, structure, _ in self._priors:
            setattr(self, structure, nolbo_structure[structure[1:-4]])
        self._debug = None         # set to a dict to capture the latent stage's inputs and gradients of the next fit (tests)
        nolboSingleObject_VAE.__init__(self, nolbo_structure, backbone_style=backbone_style, encoder_backbone=encoder_backbone,
                                       dropout=False, learning_rate=learning_rate)

    def _buildModel(self):
        nolboSingleObject_VAE._buildModel(self)
        # ==============set prior network, under the reference's names (nolbo.py:85-87)
        for net, structure, _ in self._priors:
            setattr(self, net, priornet.priornet(structure=getattr(self, structure), device=self._device))

    def _debug_extra(self, draw):
        return {}

    def fit(self, inputs, *, latent='hip', _rand=None):
        """(input_images, output_images, one one-hot list per prior network) -> (loss_kl, loss_shape, loss_reg, pr, rc);
        total = mean KL(q || priors) + shape + _reg_weight mean reg (+ the l2 terms of every sub-model with _network_l2); Adam on the 2D
        encoder, the prior networks (torch) and the decoder (HIP).  `_rand` (tests) = dict(eps, eps_prior [B, L]) and the class's draw."""
        input_images, output_images, *onehots = inputs
        if latent not in ('hip', 'torch'):
            raise ValueError("latent must be 'hip' or 'torch', got %r" % (latent,))
        if len(onehots) != len(self._priors):
            raise ValueError('inputs must be (input_images, output_images) and %d one-hot list(s), got %d values' % (len(self._priors), len(inputs)))
        y, onehots = self._dev(output_images), [self._dev(o).contiguous() for o in onehots]
        trainer, opt = self._image_trainer()
        opt.zero_grad(set_to_none=True)
        pri = self._prior_outputs(onehots)                    # in front of the 2D encoder: their dropout draws first (nolbo.py:95-100)
        enc_out = self._head_output_training(input_images)
        self._check_width(enc_out, *self._enc_layout())
        B = enc_out.shape[0]
        r = _rand or {}
        eps, eps_p = self._draw_eps(B, r.get('eps')).contiguous(), self._draw_eps(B, r.get('eps_prior')).contiguous()
        draw = self._decoder_input_draw(B, r)
        l2 = self._l2_terms() if self._network_l2 else []     # nolbo.py:142-144; the decoder's: step_decoder(l2=)
        e = enc_out.detach().float().contiguous().requires_grad_(True)
        with torch.enable_grad():
            z_in, extra, kl, reg, twin = self._latent_stage(latent, e, pri, eps, eps_p, draw, onehots)
        if self._debug is not None:
            for t in pri:
                if t.requires_grad:
                    t.retain_grad()
        _, m, dz = trainer.step_decoder(z_in.detach().contiguous(), y, z_act=twin, l2=ae3D.L2_REG if self._network_l2 else 0.0)
        torch.autograd.backward([z_in, extra] + l2, [dz.contiguous(), torch.ones_like(extra)] + [torch.ones_like(t) for t in l2])
        if enc_out.requires_grad:
            enc_out.backward(e.grad)
        opt.step()
        if self._debug is not None:                           # a constant log-variance has no gradient: None
            self._debug.update({'enc_out': e.detach(), 'pri': [t.detach() for t in pri], 'z_in': z_in.detach(), 'dz_in': dz, 'd_enc_out': e.grad,
                                'd_pri': [t.grad if t.requires_grad else None for t in pri]}, **self._debug_extra(draw))
        return DeviceArray(kl.detach().mean()), DeviceArray(m[0]), DeviceArray(reg.detach().mean()), DeviceArray(m[1]), DeviceArray(m[2])


@_prior_checkpoints
class nolboSingleObject(_PriorImageModel):
    """The reference's multi-modal model, nolbo.py:49-324: an image encoder that emits a category latent and an instance latent
    ([mean_c | logVar_c | mean_i | logVar_i]), a learned prior network for each, and missing-modality correction of the category
    half against the category prior.  Structure keys as the reference's: encoder_backbone (z_category_dim, z_inst_dim), encoder_head,
    decoder, prior_class, prior_inst.  The image encoder and the decoder are nolboSingleObject_VAE's (either image engine, the HIP
    decoder engine); everything between the head output and the decoder input is ONE vv_mm_latent_eval (csrc/mm_latent.hip, through
    voxvae.mm_latent.eval).

    fit (nolbo.py:90-159): inputs = (input_images, output_images, category_list, inst_list); total = mean KL(q || priors) + shape +
    mean reg + the l2 terms of all five sub-models.  Its latent stage is ONE vv_mm_latent_train_fwd and, with the decoder's
    d shape / d z_in, ONE vv_mm_latent_train_bwd (voxvae.mm_latent.latent_stage); latent='torch' runs the same algebra as an autograd
    closure.  `_rand` (tests) = dict(eps, eps_prior [B, Lc+Li], mix (bool), noise [B, Lc+Li])."""
    _priors = (('_priornet_class', '_prior_class_str', 'Category'), ('_priornet_inst', '_prior_inst_str', 'Inst'))

    @property
    def _latent_dim(self):
        """The decoder's input: the concatenated latent (what getSampledShape and its kin sample)."""
        return self._enc_backbone_str['z_category_dim'] + self._enc_backbone_str['z_inst_dim']

    def _latent_torch(self, e, pri, eps, eps_p, noise, cat_oh):
        """fit's latent algebra (nolbo.py:101-140, function.py:40-98) as torch autograd code: what vv_mm_latent_train_fwd / _bwd compute,
        kept as the comparison leg (latent='torch').  -> z_in [B, Lc+Li], kl [B], reg [B]."""
        Lc, Li = self._enc_backbone_str['z_category_dim'], self._enc_backbone_str['z_inst_dim']
        mean_cp, lv_cp, mean_ip, lv_ip = pri
        mean = torch.cat([e[:, :Lc], e[:, 2 * Lc:2 * Lc + Li]], dim=1)
        lv = torch.clamp(torch.cat([e[:, Lc:2 * Lc], e[:, 2 * Lc + Li:]], dim=1), -10.0, 10.0)
        mean_p, lv_p = torch.cat([mean_cp, mean_ip], dim=1), torch.cat([lv_cp, lv_ip], dim=1)
        z_in, kl = _sample_kl_torch(mean, lv, mean_p, lv_p, eps, eps_p, None if noise is None else noise == 0)   # :122-123
        return z_in, kl, _pair_reg_torch(mean_cp, lv_cp, 3.0 * Lc) + _pair_reg_torch(mean_ip, lv_ip, 3.0 * Li, cat_oh)

    def _enc_layout(self):
        return 2 * self._latent_dim, 'mean_c | logVar_c | mean_i | logVar_i'

    def _prior_outputs(self, onehots):                                                # :95-97
        return self._priornet_class(onehots[0], training=True) + self._priornet_inst(torch.cat(onehots, dim=-1), training=True)

    def _decoder_input_draw(self, B, r):
        """:119-122: z itself with probability 1/2, else noise ~ Bernoulli(1/2) per element, 1 where z_prior stands in."""
        return self._draw_mix(B, self._latent_dim, r, a=(False, True), missing_pr=0.5)

    def _latent_stage(self, latent, e, pri, eps, eps_p, noise, onehots):
        if latent == 'torch':
            z_in, kl, reg = self._latent_torch(e, pri, eps, eps_p, noise, onehots[0])
            return z_in, kl.mean() + reg.mean(), kl, reg, None
        from voxvae import mm_latent as _ML
        return _ML.latent_stage(e, *pri, eps, eps_p, noise, onehots[0], bf16=self._act_dt != _L.VV_F32)

    def _prior_means(self, category_list, category_indices, inst_indices, training):
        """prior_cat [C, Lc] and the instance prior's means of each sample [B, I, Li] (nolbo.py:166-181)."""
        if torch.is_tensor(category_list):                                 # a device loader's one-hots: one [B, C] copy to build the table's rows
            category_list = category_list.detach().cpu().numpy()
        cat_l = np.asarray(np.array(category_list), dtype=np.float32)
        inst_ind = np.asarray(inst_indices, dtype=np.float32)
        B, I = cat_l.shape[0], inst_ind.shape[0]
        inst_in = np.concatenate([np.repeat(cat_l, I, axis=0), np.tile(inst_ind, (B, 1))], axis=-1)
        prior_cat, _ = self._priornet_class(np.asarray(category_indices, dtype=np.float32), training=training)
        prior_inst, _ = self._priornet_inst(inst_in, training=training)
        return prior_cat.detach().float().contiguous(), prior_inst.detach().float().reshape(B, I, -1).contiguous()

    def getEval(self, inputs, category_indices=np.identity(12), inst_indices=np.identity(10), training=False, missing_prob=0.0, *,
                _eps=None, _mask=None, _eps2=None):
        """reference nolbo.py:161-259 -> (pred, loss_shape, pr, rc, acc_cat, acc_inst) at missing_prob == 0, else these and
        (pred_corrected, loss_shape_corrected, pr_corrected, rc_corrected, acc_cat_corrected).  `_eps` [B, Lc+Li] (the category
        draw, then the instance draw), `_mask` [B, Lc] and `_eps2` [B, Lc] inject the draws."""
        from voxvae import mm_latent as _ML
        input_images, output_images, category_list, inst_list = inputs
        Lc = self._enc_backbone_str['z_category_dim']
        prior_cat, prior_inst = self._prior_means(category_list, category_indices, inst_indices, training)
        enc_out = self._enc_out(input_images, training=training)
        self._check_width(enc_out, *self._enc_layout())
        B = enc_out.shape[0]
        y, cat_oh, inst_oh = self._dev(output_images), self._dev(category_list).contiguous(), self._dev(inst_list).contiguous()
        eps = self._draw_eps(B, _eps).contiguous()
        mask = eps2 = None
        if missing_prob > 0:
            mask = self._draw_mask(B, missing_prob, _mask, Lc).contiguous()             # :202-203, the same RNG call
            eps2 = (torch.randn(B, Lc, dtype=torch.float32, device=self._device) if _eps2 is None else self._dev(_eps2)).contiguous()
        act_dt = _L.VV_F32 if training else self._act_dt                               # training: float32 to the decoder entry (_eval_hooks)
        z, zc, z_act, zc_act, idx, acc = _ML.eval(enc_out, eps, mask, eps2, prior_cat, prior_inst, cat_oh, inst_oh, act_dt)
        twin = z_act is not None
        decode = self._eval_hooks(training)[1]
        pred, _, m = decode(z_act if twin else z, y, None)                             # :229-235
        self._z, self._nearest = DeviceArray(z), DeviceArray(idx)
        res = self._scored(pred, m) + (DeviceArray(acc[0]), DeviceArray(acc[1]))
        if missing_prob == 0.0:
            return res
        pred_c, _, mc = decode(zc_act if twin else zc, y, None)                        # :252-258
        self._z_corrected = DeviceArray(zc)
        return res + self._scored(pred_c, mc) + (DeviceArray(acc[2]),)


class nolboSingleObject_AE(nolboSingleObject_VAE):
    """The reference's image -> 3D autoencoder, nolbo.py:541-748 (the AE baseline of test_pascal_3D.py): nolboSingleObject_VAE without
    the sampling -- the head output [B, z_dim] IS the latent.  getEval (the 10-tuple, :632-698) and getLatent are _ModelnetBase's
    non-variational forms; fit (:580-610) trains the 2D encoder by torch autograd and the decoder through the HIP trainer's
    decoder-only step; save / load are nolboSingleObject_VAE's."""
    _variational = False

    def _latent_training_mode(self, x, eps=None):
        with torch.no_grad():
            z = self._enc_out(x, training=True)
        return z, z, None, None

    def fit(self, inputs, *, _dropout=None):
        """nolbo.py:580-610: (input_images, output_images) -> (loss_shape, pr, rc); total = shape + the l2 terms of head, backbone
        and decoder.  dropout=True: inverted dropout on z at a rate ~ U[0,1) per step (:586-588); `_dropout` = (rate, keep [B, L])
        injects it."""
        input_images, output_images = inputs
        y = self._dev(output_images)
        trainer, opt = self._image_trainer()
        z = self._head_output_training(input_images)
        z_in, keep = z.detach().float().contiguous(), None
        if self._dropout:
            keep, scale = self._draw_dropout(z_in.shape[0], z_in.shape[1], *(_dropout or ()))
            keep = keep * scale
            z_in = z_in * keep
        _, m, dz = trainer.step_decoder(z_in, y, l2=ae3D.L2_REG)                       # + decoder.losses, :595-596
        if opt is not None and z.requires_grad:
            opt.zero_grad(set_to_none=True)
            reg = self._l2_terms()
            torch.autograd.backward([z] + reg, [dz if keep is None else dz * keep] + [torch.ones_like(t) for t in reg])
            opt.step()
        return DeviceArray(m[0]), DeviceArray(m[1]), DeviceArray(m[2])


class _OnePriorImageModel(_PriorImageModel):
    """What nolboSingleObject_instOnly and nolboSingleObject_category_only share: an image encoder that emits ONE latent group
    ([mean | logVar]), ONE learned prior network over the sample's one-hot, and as latent stage ONE vv_prior_latent_train_fwd and ONE
    vv_prior_latent_train_bwd (csrc/prior_latent.hip, through voxvae.prior_latent.latent_stage).  A subclass names its structure keys and
    the reference's constants."""
    _z_key = None            # the latent's width in nolbo_structure['encoder_backbone']
    _dist_per_dim = None     # dist_in_z_space = _dist_per_dim * L

    @property
    def _latent_dim(self):
        return self._enc_backbone_str[self._z_key]

    @property
    def _priornet(self):
        return getattr(self, self._priors[0][0])

    def _enc_layout(self):
        return 2 * self._latent_dim, 'mean | logVar'

    def _prior_outputs(self, onehots):
        return self._priornet(onehots[0], training=True)

    def _latent_stage(self, latent, e, pri, eps, eps_p, keep, onehots):
        dist = float(self._dist_per_dim) * self._latent_dim
        if latent == 'torch':
            z_in, kl, reg = _one_prior_latent_torch(e, pri, eps, eps_p, keep, dist)
            return z_in, kl.mean() + self._reg_weight * reg.mean(), kl, reg, None
        from voxvae import prior_latent as _PL
        return _PL.latent_stage(e, pri[0], pri[1], eps, eps_p, keep, dist, self._reg_weight, bf16=self._act_dt != _L.VV_F32)

    def _debug_extra(self, keep):
        return {'keep': keep, 'dist': float(self._dist_per_dim) * self._latent_dim, 'reg_weight': self._reg_weight}


@_prior_checkpoints
class nolboSingleObject_instOnly(_OnePriorImageModel):
    """The reference's instance-only image model, nolbo.py:326-540 (train_kitti.py): one instance latent, a learned prior network over
    the instance one-hot.  Structure keys as the reference's: encoder_backbone (z_inst_dim), encoder_head, decoder, prior_inst.
    fit (:365-415): inputs = (input_images, output_images, inst_list); total = mean KL(q || prior) + shape + mean reg (dist 10 L) + the
    l2 terms of all four sub-models; the decoder sees z or, with probability 1/2 (`_rand['from_prior']`), z_prior for the whole batch.
    getEval (:417-485): ONE vv_inst_latent_eval between the head output and the two decoder passes."""
    _z_key, _priors = 'z_inst_dim', (('_priornet_inst', '_prior_inst_str', 'Inst'),)
    _dist_per_dim, _reg_weight, _network_l2 = 10.0, 1.0, True

    def _decoder_input_draw(self, B, r):
        """:383-386: `rand < 0.5` -> decoder(z), else decoder(z_prior): an all-zero keep; `_rand['from_prior']` (bool) injects the choice."""
        from_prior = bool(r['from_prior']) if 'from_prior' in r else not (np.random.rand() < 0.5)
        return torch.zeros(B, self._latent_dim, dtype=torch.float32, device=self._device) if from_prior else None

    def getEval(self, input_images, output_images, inst_list=np.identity(10), missing_prob=0.1, training=True, *, _eps=None, _mask=None,
                _fill=None):
        """reference nolbo.py:417-485 -> (pred, loss_shape, pr, rc, pred_corrected, loss_shape_corrected, pr_corrected, rc_corrected):
        the decoder on z (masked elements replaced by an N(0,1) draw) and on the nearest instance prior's mean.  inst_list [I, I']: the
        one-hots the prior table is made of.  `training` defaults to True as in the reference.  `_eps`, `_mask`, `_fill` [B, L] inject
        the draws."""
        from voxvae import prior_latent as _PL
        prior, _ = self._priornet(np.asarray(inst_list, dtype=np.float32), training=bool(training))
        prior = prior.detach().float().contiguous()
        with torch.no_grad():
            enc_out = self._enc_out(input_images, training=training).detach()
        B, Lz = enc_out.shape[0], self._latent_dim
        self._check_width(enc_out, *self._enc_layout())
        y = self._dev(output_images)
        eps = self._draw_eps(B, _eps).contiguous()
        mask = fill = None
        if missing_prob > 0:
            mask = self._draw_mask(B, missing_prob, _mask, Lz).contiguous()             # :433-434, the same RNG call
            fill = self._draw_eps(B, _fill).contiguous()                                # :438
        twin = not training and self._act_dt != _L.VV_F32                              # training: float32 to the decoder entry (_eval_hooks)
        z, zc, zb, zcb, idx = _PL.inst_eval(enc_out, eps, mask, fill, prior, bf16=twin)
        decode = self._eval_hooks(training)[1]
        pred, _, m = decode(zb if twin else z, y, None)                                # :443-449
        pred_c, _, mc = decode(zcb if twin else zc, y, None)                           # :477-483
        self._z, self._z_corrected, self._nearest = DeviceArray(z), DeviceArray(zc), DeviceArray(idx)
        return self._scored(pred, m) + self._scored(pred_c, mc)


@_prior_checkpoints
class nolboSingleObject_category_only(_OnePriorImageModel):
    """The reference's category-only image model, nolbo.py:984-1204 (train_pascal_category.py, test_pascal_category.py): one category
    latent, a learned prior network over the category one-hot.  Structure keys as the reference's: encoder_backbone (z_category_dim),
    encoder_head, decoder, prior_class.  fit (:1023-1075): inputs = (input_images, output_images, category_list); total = mean KL(q ||
    prior) + shape + 0.01 mean reg (dist 3 L), no network l2 terms; the decoder sees z or, with probability 1/2 (`_rand['mix']`), z with
    30 % of its elements (`_rand['noise']` [B, L], 0 there) replaced by z_prior's.  getEval (:1077-1149) is
    nolboSingleObject_VAE's with the prototype table replaced by the prior network's means over `category_indices`."""
    _z_key, _priors = 'z_category_dim', (('_priornet_class', '_prior_class_str', 'Category'),)
    _dist_per_dim, _reg_weight, _network_l2 = 3.0, 0.01, False

    def _decoder_input_draw(self, B, r):
        return self._draw_mix(B, self._latent_dim, r)                                  # :1042-1047

    def getEval(self, inputs, category_indices=np.identity(12), training=False, missing_prob=0.0, *, _eps=None, _mask=None, _eps2=None):
        """nolbo.py:1077-1149 -> the 10-tuple of the VAE class, classified / corrected against the prior means."""
        mean_prior, _ = self._priornet(np.asarray(category_indices, dtype='float32'), training=bool(training))
        return _ModelnetBase.getEval(self, inputs, category_vectors=mean_prior.detach().contiguous(), training=training,
                                     missing_prob=missing_prob, _eps=_eps, _mask=_mask, _eps2=_eps2)
