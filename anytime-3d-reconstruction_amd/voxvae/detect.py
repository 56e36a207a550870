"""The detector head's output -> the selected detections on the device (csrc/detect_decode.hip and csrc/detect_decode.h behind
vv_detect_decode / vv_detect_decode_host).

The reference decodes a frame on the host (src/module/nolbo_test.py:81-153: activations, a Python loop over the grid cells, the greedy
numpy NMS of src/module/function.py:117-150).  Here that is one launch for all frames of a batch, and the selected rows stay on the
device for voxvae.pose.object_poses and the sampled-mean decoder:

    det = decode_detections(head_out)                         # [B, R, C, P * (17 + 2 Z)]
    b2, b3, sn, cs, rad, mean, logvar = det.frame(0)          # device slices of frame 0's kept rows; det.counts() is THE read-back
    bbox2D, bbox3D, sin, cos, rad_log_var, inst_mean, inst_log_var = det.numpy(0)      # the reference's arrays

All arithmetic is float32 with the reference's roundings; the order of the rows is the NMS's pick order; ties and thresholds are
decided as DESIGN 4h states.
"""
import ctypes

import numpy as np
import torch

NHWC, NCHW = 0, 1
MAX_PREDICTORS, MAX_Z, MAX_SLOTS = 16, 64, 4096


def channel_width(z_inst_dim):
    """Channels of one predictor: objectness 1, bbox2D 4, bbox3D 3, two latents of z_inst_dim, sin 3, cos 3, rad_log_var 3."""
    return 1 + 4 + 3 + 2 * int(z_inst_dim) + 9


def partition(predictor_num, z_inst_dim):
    """-> {field: [(start, end) per predictor]}: the channel ranges _encOutPartitioning (nolbo_test.py:214-246) cuts the head output into."""
    out = dict((k, []) for k in ('objness', 'bbox2D', 'bbox3D', 'inst_mean', 'inst_log_var', 'sin', 'cos', 'rad_log_var'))
    at = 0
    for _ in range(int(predictor_num)):
        for name, w in (('objness', 1), ('bbox2D', 4), ('bbox3D', 3), ('inst_mean', int(z_inst_dim)), ('inst_log_var', int(z_inst_dim)),
                        ('sin', 3), ('cos', 3), ('rad_log_var', 3)):
            out[name].append((at, at + w))
            at += w
    return out


class Detections(object):
    """The result of decode_detections for B frames of N candidate slots each, as tensors on the device (on the CPU for host=True).

    count int32 [B];  index int32 [B,N] (cell * predictor_num + predictor);  bbox2d float32 [B,N,5] = (col_min, row_min, col_max,
    row_max, objectness);  bbox3d [B,N,3];  inst_mean, inst_log_var [B,N,Z];  sin, cos, rad_log_var [B,N,3].  Frame b's rows are in
    pick order; only rows below count[b] hold values."""
    __slots__ = ('count', 'index', 'bbox2d', 'bbox3d', 'inst_mean', 'inst_log_var', 'sin', 'cos', 'rad_log_var', 'grid', '_counts')

    def __init__(self, count, index, bbox2d, bbox3d, inst_mean, inst_log_var, sin, cos, rad_log_var, grid):
        self.count, self.index, self.bbox2d, self.bbox3d = count, index, bbox2d, bbox3d
        self.inst_mean, self.inst_log_var, self.sin, self.cos, self.rad_log_var = inst_mean, inst_log_var, sin, cos, rad_log_var
        self.grid = grid                      # (grid_row, grid_col, predictor_num)
        self._counts = None

    def __len__(self):
        return int(self.count.shape[0])

    def counts(self):
        """Kept detections per frame (reads 4 B bytes, once: THE synchronisation)."""
        if self._counts is None:
            self._counts = [int(v) for v in self.count.cpu().tolist()]
        return self._counts

    def frame(self, f=0):
        """-> (bbox2d [M,5], bbox3d [M,3], sin [M,3], cos [M,3], rad_log_var [M,3], inst_mean [M,Z], inst_log_var [M,Z]): the kept
        rows of frame f where they are, in the reference's order of return values."""
        M = self.counts()[f]
        return tuple(t[f, :M] for t in (self.bbox2d, self.bbox3d, self.sin, self.cos, self.rad_log_var, self.inst_mean, self.inst_log_var))

    def numpy(self, frame=0):
        """-> the reference's (bbox2D_selected, bbox3D_selected, sin_mean_selected, cos_mean_selected, rad_log_var_selected,
        inst_mean_selected, inst_log_var_selected) of one frame as numpy arrays."""
        return tuple(t.cpu().numpy() for t in self.frame(frame))


def _as_head(head_out, device, channels):
    """-> (tensor whose storage the kernel reads, layout).  An NHWC-contiguous tensor or the permuted view of an NCHW-contiguous one
    passes as it is; anything else is copied to NHWC."""
    from .tensor import DeviceArray
    if isinstance(head_out, DeviceArray):
        head_out = head_out.t
    t = head_out if isinstance(head_out, torch.Tensor) else torch.from_numpy(np.asarray(head_out, dtype=np.float32))
    if t.dim() == 3:
        t = t.unsqueeze(0)
    if t.dim() != 4 or t.shape[-1] != channels:
        raise ValueError('head output must be [B, grid_row, grid_col, %d], got %s' % (channels, tuple(t.shape)))
    t = t.detach()
    if t.dtype != torch.float32 or t.device != device:
        t = t.to(device=device, dtype=torch.float32)
    if t.is_contiguous():
        return t, NHWC
    if t.permute(0, 3, 1, 2).is_contiguous():
        return t, NCHW
    return t.contiguous(), NHWC


def decode_detections(head_out, predictor_num=5, z_inst_dim=16, obj_thresh=0.5, IOU_thresh=0.5, top_1_pred=True, host=False):
    """Head output -> Detections.

    head_out [B, grid_row, grid_col, predictor_num * (17 + 2 z_inst_dim)] (or one frame without B): a torch tensor on any device, a
    numpy array or a DeviceArray.  The thresholds are rounded to float32, as numpy rounds them beside the reference's float32 values.
    host=False  runs on the current stream of the device the input lives on (voxvae's default device for host input); without a GPU
                that is an error, not a fallback.
    host=True   the same code compiled for the CPU (vv_detect_decode_host), bit for bit the device's result."""
    import voxvae
    from . import lib as L
    from .tensor import DeviceArray
    P, Z = int(predictor_num), int(z_inst_dim)
    channels = P * channel_width(Z)
    if host:
        device = torch.device('cpu')
    else:
        held = head_out.t if isinstance(head_out, DeviceArray) else head_out
        device = held.device if isinstance(held, torch.Tensor) and held.is_cuda else torch.device(voxvae.default_device())
        if device.type != 'cuda' or not torch.cuda.is_available():
            raise L.VoxVaeError('decode_detections runs on the GPU (default device %s, CUDA available: %s); there is no silent CPU '
                                'fallback: pass host=True for the host entry' % (device, torch.cuda.is_available()))
    t, layout = _as_head(head_out, device, channels)
    B, R, C = int(t.shape[0]), int(t.shape[1]), int(t.shape[2])
    N = R * C * (1 if top_1_pred else P)
    if not (1 <= P <= MAX_PREDICTORS and 1 <= Z <= MAX_Z and B >= 1 and 1 <= N <= MAX_SLOTS):
        raise ValueError('decode_detections: predictor_num 1..%d, z_inst_dim 1..%d, at least one frame and at most %d candidate slots per '
                         'frame; got P %d, Z %d, B %d, %d slots' % (MAX_PREDICTORS, MAX_Z, MAX_SLOTS, P, Z, B, N))
    new = lambda shape, dt: torch.empty(shape, dtype=dt, device=device)
    f32 = torch.float32
    out = Detections(new((B,), torch.int32), new((B, N), torch.int32), new((B, N, 5), f32), new((B, N, 3), f32), new((B, N, Z), f32),
                     new((B, N, Z), f32), new((B, N, 3), f32), new((B, N, 3), f32), new((B, N, 3), f32), (R, C, P))
    args = (L.ptr(t), layout, B, R, C, P, Z, channels, float(obj_thresh), float(IOU_thresh), 1 if top_1_pred else 0, L.ptr(out.count),
            L.ptr(out.index), L.ptr(out.bbox2d), L.ptr(out.bbox3d), L.ptr(out.inst_mean), L.ptr(out.inst_log_var), L.ptr(out.sin),
            L.ptr(out.cos), L.ptr(out.rad_log_var))
    if host:
        L.call('vv_detect_decode_host', *args)
    else:
        with torch.cuda.device(device):
            L.call('vv_detect_decode', *args, ctypes.c_void_p(torch.cuda.current_stream(device).cuda_stream))
    return out


def activation_host(x, which):
    """The kernel's own exp / sigmoid / tanh (which = 'exp', 'sigmoid', 'tanh') of a float32 array, on the host."""
    from . import lib as L
    x = np.ascontiguousarray(np.asarray(x, dtype=np.float32))
    y = np.empty_like(x)
    L.call('vv_detect_activation_host', x.ctypes.data_as(ctypes.c_void_p), y.ctypes.data_as(ctypes.c_void_p), x.size,
           {'exp': 0, 'sigmoid': 1, 'tanh': 2}[which])
    return y
