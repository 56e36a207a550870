"""Bernoulli keep masks over a [B, L] latent drawn on the device (csrc/keep_mask.hip): the dropout mask of fit and the missing-latent
mask of getEval(missing_prob > 0), keep = u >= p in both.

A mask is a pure function of (seed, offset, element): Philox4x32-10 keyed by the 64-bit seed, with the 64-bit offset

    offset = kind << 56 | rank << 40 | step        kind: 0 dropout, 1 missing;  rank: the torch.distributed rank (0 without one);
                                                    step: how many masks of that kind this KeepMasks has drawn before

so no two ranks, kinds or steps share a counter, and `KeepMasks.host` (vv_keep_mask_host: the same header in a loop on the CPU, no GPU
needed) reproduces any step's mask bit for bit.

The seed is `voxvae.manual_seed(seed)`.  If none was set when the first mask is drawn, it is taken ONCE per process from np.random (one
host draw, in device mode only), so a single np.random.seed at the top of a script still fixes the run.  The dropout RATE stays the
reference's host scalar np.random.rand() in both modes: it is a kernel argument, not a transfer.
"""
import ctypes

import numpy as np
import torch

from . import lib as L

KINDS = {'dropout': 0, 'missing': 1}
KIND_SHIFT, RANK_SHIFT = 56, 40
_SEED = {'value': None}


def manual_seed(seed):
    """The 64-bit seed of every KeepMasks built without one of its own (None: back to 'take it from np.random at the first draw')."""
    _SEED['value'] = None if seed is None else int(seed) & 0xFFFFFFFFFFFFFFFF


def seed():
    """The process seed; unset, it is drawn here from np.random (one host draw) and kept."""
    if _SEED['value'] is None:
        _SEED['value'] = int(np.random.randint(0, 2 ** 63 - 1, dtype=np.int64))
    return _SEED['value']


def pack_offset(kind, rank, step):
    """kind << 56 | rank << 40 | step; kind by name or number (8 bits), rank 16 bits, step 40 bits."""
    kind = KINDS[kind] if isinstance(kind, str) else int(kind)
    rank, step = int(rank), int(step)
    if not (0 <= kind < 1 << 8 and 0 <= rank < 1 << (KIND_SHIFT - RANK_SHIFT) and 0 <= step < 1 << RANK_SHIFT):
        raise ValueError('mask counter out of range: kind %d, rank %d, step %d' % (kind, rank, step))
    return kind << KIND_SHIFT | rank << RANK_SHIFT | step


def _rank():
    import torch.distributed as dist
    return dist.get_rank() if dist.is_available() and dist.is_initialized() else 0


class KeepMasks(object):
    """The mask stream of one model.  seed None: the process seed (manual_seed), resolved at the first draw; rank None: the
    torch.distributed rank at the first draw."""

    def __init__(self, device, seed=None, rank=None):
        self.device = torch.device(device)
        self._seed = None if seed is None else int(seed) & 0xFFFFFFFFFFFFFFFF
        self._rank = None if rank is None else int(rank)
        self.steps = {k: 0 for k in KINDS}

    @property
    def seed(self):
        if self._seed is None:
            self._seed = seed()
        return self._seed

    @property
    def rank(self):
        if self._rank is None:
            self._rank = _rank()
        return self._rank

    def offset(self, kind, step):
        return pack_offset(kind, self.rank, step)

    def _draw(self, kind, B, Lz, p):
        keep = torch.empty(int(B), int(Lz), dtype=torch.float32, device=self.device)
        off = self.offset(kind, self.steps[kind])
        with torch.cuda.device(self.device):
            st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
        L.call('vv_keep_mask', L.ptr(keep), int(B), int(Lz), float(p), self.seed, off, st)
        self.steps[kind] += 1
        return keep

    def dropout(self, B, Lz, rate):
        """The next dropout mask [B, L] (float32 on the device, 1 = kept): keeps where u >= rate."""
        return self._draw('dropout', B, Lz, rate)

    def missing(self, B, Lz, missing_prob):
        """The next missing-latent mask [B, L]: an entry is missing (0) with probability missing_prob."""
        return self._draw('missing', B, Lz, missing_prob)

    def host(self, kind, B, Lz, p, step):
        """The mask `step` of `kind` as a numpy float32 [B, L]: what the device drew, or will draw, at that step."""
        keep = np.empty((int(B), int(Lz)), dtype=np.float32)
        L.call('vv_keep_mask_host', keep.ctypes.data_as(ctypes.c_void_p), int(B), int(Lz), float(p), self.seed, self.offset(kind, step))
        return keep
