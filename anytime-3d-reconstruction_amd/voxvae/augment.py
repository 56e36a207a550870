"""Pascal3D image batches built on the device (csrc/augment.hip, arithmetic in csrc/augment.h): the reference's per-object chain -- crop
with a random border, flip, Invert / Add, warpAffine, cubic resize, / 255 -- as two launches over a batch.

    arena  = ImageArena.from_arrays([uint8 HWC arrays])                  the photos, once, in device memory
    params = draw_params(arena, image_index, boxes, augmentation, step)  int32 [B, 16]: the random half (vv_augment_draw)
    images = augment_images(arena, params, (rows, cols))                 float32 [B, rows, cols, 3] (vv_augment_images)

A params row is a pure function of (seed, offset, sample): Philox4x32-10 keyed by voxvae.manual_seed's seed, offset = KIND << 56 |
rank << 40 | step exactly as voxvae.masks.KeepMasks packs it (kind 2: no counter is shared with a keep mask).  `host=True` runs the same
header in a loop on the CPU (no GPU needed) and gives the same bits.  Injected params always win: augment_images applies whatever rows
it is handed.

By default Invert and Add are the colour operations, as before.  The reference's other two, GaussianBlur and AddToHueAndSaturation, are
opt-in through a second table, colour int32 [B, 4] (flags, sigma bits, hue, sat: csrc/augment.h):

    params, colour = draw_params(..., colour=True)                       vv_augment_draw_ex: both tables in one launch
    images = augment_images(arena, params, (rows, cols), colour=colour)  vv_augment_images_ex: colour pre-pass, then the warp

and then the four apply in the reference's order blur -> invert -> add -> hue/saturation.  What the header does not model (scipy's
summation order, cv2's fixed-point paths, the unmeasured agreement of its 8-bit HSV chain with cv2) is stated there.
"""
import ctypes

import numpy as np
import torch

from . import lib as L
from . import masks

KIND = 2                 # beside masks.KINDS' 0 (dropout) and 1 (missing)
WORDS = 16
COLOUR_WORDS = 4
C_FLAGS, C_SIGMA, C_HUE, C_SAT = 0, 1, 2, 3
FLAG_BLUR, FLAG_HUE_SAT = 1, 2
P_IMAGE, P_ROW0, P_COL0, P_ROWS, P_COLS, P_FLIP, P_SCALE, P_DROW, P_DCOL, P_INVERT, P_ADD, P_ROWPAD, P_COLPAD = 0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 13, 14


def _hp(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def _stream(device):
    with torch.cuda.device(device):
        return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def scale_bits(s):
    """The int32 word 6 of a params row for the scale s (float32 bits)."""
    return int(np.float32(s).view(np.int32))


def make_params(image=0, row0=0, col0=0, rows=1, cols=1, flip=0, scale=1.0, d_row=0, d_col=0, invert=0, add=(0, 0, 0), row_pad=0, col_pad=0):
    """One params row (numpy int32 [16]) from named fields."""
    return np.array([image, row0, col0, rows, cols, flip, scale_bits(scale), d_row, d_col, invert, add[0], add[1], add[2], row_pad, col_pad, 0],
                    dtype=np.int32)


def make_colour(sigma=0.0, hue=0, sat=0, blur=False, hue_sat=False):
    """One colour row (numpy int32 [4]) from named fields: sigma of the blur, hue add in H units (-179 .. 179), saturation add."""
    return np.array([(FLAG_BLUR if blur else 0) | (FLAG_HUE_SAT if hue_sat else 0), scale_bits(sigma), hue, sat], dtype=np.int32)


class ImageArena(object):
    """uint8 HWC 3-channel images of differing sizes back to back in one buffer, with the int64 table (byte offset, rows, cols); a host
    copy is kept for host=True.  device None: host only (no GPU is touched)."""

    def __init__(self, data, meta, device):
        self.host_data, self.host_meta = data, meta
        self.device = None if device is None else torch.device(device)
        self.data = self.meta = None
        self._colour_ws = None           # the colour pre-pass's slabs, kept between calls (augment_images)
        if self.device is not None:
            self.data = torch.from_numpy(data).to(self.device)
            self.meta = torch.from_numpy(meta).to(self.device)

    @classmethod
    def from_arrays(cls, images, device='default'):
        if device == 'default':
            import voxvae
            device = voxvae.default_device() if torch.cuda.is_available() else None
        images = [np.ascontiguousarray(im, dtype=np.uint8) for im in images]
        if not images:
            raise ValueError('no images')
        meta, off = np.empty((len(images), 3), dtype=np.int64), 0
        for i, im in enumerate(images):
            if im.ndim != 3 or im.shape[2] != 3 or min(im.shape[:2]) < 1 or max(im.shape[:2]) > 16383:
                raise ValueError('image %d: expected uint8 [rows, cols, 3] with extents in 1 .. 16383, got %s' % (i, im.shape))
            meta[i] = (off, im.shape[0], im.shape[1])
            off += im.size
        return cls(np.concatenate([im.reshape(-1) for im in images]), meta, device)

    def __len__(self):
        return self.host_meta.shape[0]


def offset(step, rank=None):
    return masks.pack_offset(KIND, masks._rank() if rank is None else rank, step)


def _host_rows(x, dtype, cols):
    a = np.ascontiguousarray(x.detach().cpu().numpy() if torch.is_tensor(x) else x, dtype=dtype)
    return a.reshape(-1, cols) if cols else a.reshape(-1)


def draw_params(arena, image_index, boxes, augmentation, step, host=False, seed=None, rank=None, colour=False):
    """int32 [B, 16] for objects (image_index [B], boxes [B, 4] = colMin, rowMin, colMax, rowMax) at draw `step`: a device tensor, or with
    host=True a CPU tensor with the same bits.  On the device nothing is read back: a sample whose index or box is inadmissible gets the
    refused row (word 0 = -1), which augment_images leaves unwritten; host=True raises for it.  colour=True returns (params, colour)
    with the int32 [B, 4] colour table drawn beside the same params rows."""
    sd = masks.seed() if seed is None else int(seed) & 0xFFFFFFFFFFFFFFFF
    off = offset(step, rank)
    if host:
        idx, bx = _host_rows(image_index, np.int32, 0), _host_rows(boxes, np.float32, 4)
        if bx.shape[0] != idx.shape[0]:
            raise ValueError('boxes %s against %d indices' % (bx.shape, idx.shape[0]))
        params = np.zeros((idx.shape[0], WORDS), dtype=np.int32)
        if colour:
            col = np.zeros((idx.shape[0], COLOUR_WORDS), dtype=np.int32)
            L.call('vv_augment_draw_ex_host', _hp(arena.host_meta), len(arena), _hp(idx), _hp(bx), idx.shape[0], int(bool(augmentation)), sd, off,
                   _hp(params), _hp(col))
            return torch.from_numpy(params), torch.from_numpy(col)
        L.call('vv_augment_draw_host', _hp(arena.host_meta), len(arena), _hp(idx), _hp(bx), idx.shape[0], int(bool(augmentation)), sd, off, _hp(params))
        return torch.from_numpy(params)
    dev = arena.device
    idx = torch.as_tensor(image_index).to(device=dev, dtype=torch.int32).contiguous().view(-1)
    bx = torch.as_tensor(boxes).to(device=dev, dtype=torch.float32).contiguous().view(-1, 4)
    if bx.shape[0] != idx.shape[0]:
        raise ValueError('boxes %s against %d indices' % (tuple(bx.shape), idx.shape[0]))
    params = torch.empty(idx.shape[0], WORDS, dtype=torch.int32, device=dev)
    if colour:
        col = torch.empty(idx.shape[0], COLOUR_WORDS, dtype=torch.int32, device=dev)
        L.call('vv_augment_draw_ex', L.ptr(arena.meta), len(arena), L.ptr(idx), L.ptr(bx), idx.shape[0], int(bool(augmentation)), sd, off,
               L.ptr(params), L.ptr(col), _stream(dev))
        return params, col
    L.call('vv_augment_draw', L.ptr(arena.meta), len(arena), L.ptr(idx), L.ptr(bx), idx.shape[0], int(bool(augmentation)), sd, off, L.ptr(params),
           _stream(dev))
    return params


def check_params(arena, params):
    """Raises VoxVaeError when a host-side params row is inadmissible for the arena."""
    p = _host_rows(params, np.int32, WORDS)
    L.call('vv_augment_check_host', _hp(arena.host_meta), len(arena), _hp(p), p.shape[0])


def _slab_extents(arena, params_host):
    """(max_rows, max_cols) of the colour slabs: from the rows when they are on the host, otherwise the arena's largest image (a drawn
    crop lies inside its image).  Only the product counts: a flagged row is refused by the launch when its h * w exceeds
    max_rows * max_cols, whatever its shape -- an injected padded crop of more pixels than the largest image, for rows that stay on
    the device."""
    if params_host is not None and params_host.shape[0]:
        return max(1, int(params_host[:, P_ROWS].max())), max(1, int(params_host[:, P_COLS].max()))
    return int(arena.host_meta[:, 1].max()), int(arena.host_meta[:, 2].max())


def augment_images(arena, params, out_size, colour=None, host=False, out=None, workspace=None):
    """float32 [B, rows, cols, 3] in 0 .. 1 for params [B, 16] and out_size = (rows, cols).  Params handed over on the host (numpy or a CPU
    tensor) are checked here and raise; params that are already on the device are applied without a read-back.  colour [B, 4] (None:
    Invert and Add only) selects blur and hue/saturation per sample; its launch needs a workspace (a uint8 device tensor), which is
    allocated, kept on the arena and grown as needed when none is given."""
    rows, cols = int(out_size[0]), int(out_size[1])
    if host:
        p = _host_rows(params, np.int32, WORDS)
        res = np.empty((p.shape[0], rows, cols, 3), dtype=np.float32)
        if colour is not None:
            c = _host_rows(colour, np.int32, COLOUR_WORDS)
            if c.shape[0] != p.shape[0]:
                raise ValueError('colour %s against %d params rows' % (c.shape, p.shape[0]))
            mr, mc = _slab_extents(arena, p)
            need = L.load().vv_augment_colour_workspace_bytes(mr, mc, p.shape[0])
            ws = np.empty(max(need, 4), dtype=np.uint8)
            L.call('vv_augment_images_ex_host', _hp(arena.host_data), _hp(arena.host_meta), len(arena), _hp(p), p.shape[0], rows, cols, _hp(res),
                   _hp(c), _hp(ws), need, mr, mc)
            return torch.from_numpy(res)
        L.call('vv_augment_images_host', _hp(arena.host_data), _hp(arena.host_meta), len(arena), _hp(p), p.shape[0], rows, cols, _hp(res))
        return torch.from_numpy(res)
    dev = arena.device
    p_host = None
    if not (torch.is_tensor(params) and params.is_cuda):
        check_params(arena, params)
        p_host = _host_rows(params, np.int32, WORDS)
        params = torch.from_numpy(p_host)
    p = params.to(device=dev, dtype=torch.int32).contiguous().view(-1, WORDS)
    if out is None:
        out = torch.empty(p.shape[0], rows, cols, 3, dtype=torch.float32, device=dev)
    if colour is not None:
        c = (colour if torch.is_tensor(colour) else torch.from_numpy(_host_rows(colour, np.int32, COLOUR_WORDS)))
        c = c.to(device=dev, dtype=torch.int32).contiguous().view(-1, COLOUR_WORDS)
        if c.shape[0] != p.shape[0]:
            raise ValueError('colour %s against %d params rows' % (tuple(c.shape), p.shape[0]))
        mr, mc = _slab_extents(arena, p_host)
        need = L.load().vv_augment_colour_workspace_bytes(mr, mc, p.shape[0])
        if workspace is None:
            if arena._colour_ws is None or arena._colour_ws.numel() < need:
                arena._colour_ws = torch.empty(need, dtype=torch.uint8, device=dev)
            workspace = arena._colour_ws
        L.call('vv_augment_images_ex', L.ptr(arena.data), L.ptr(arena.meta), len(arena), L.ptr(p), p.shape[0], rows, cols, L.ptr(out), L.ptr(c),
               L.ptr(workspace), workspace.numel() * workspace.element_size(), mr, mc, _stream(dev))
        return out
    L.call('vv_augment_images', L.ptr(arena.data), L.ptr(arena.meta), len(arena), L.ptr(p), p.shape[0], rows, cols, L.ptr(out), _stream(dev))
    return out
