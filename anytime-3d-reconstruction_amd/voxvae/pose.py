"""Detections -> posed objects on the device (csrc/object_pose.hip and csrc/pose_solve.h behind vv_object_pose / vv_object_pose_host).

The reference poses every detection of a frame on the host (src/visualizer/visualizer.py:237-308, getObjectInRealWorld: pre-filter,
angles -> rotation, ray correction, the translation fit of getTranslation -- 128 candidates with a 4x4 SVD each --, the 4x4 pose, the
projected corners, post-filter).  Here that is two launches for all detections, and the kept objects' poses stay on the device for
voxvae.points.voxel_points:

    poses = object_poses(bbox2D, bbox3D, sin, cos, (image_col, image_row))      # [n,5], [n,3], [n,3], [n,3]
    cloud = poses.points(shapes)                                                # shapes [n,D,D,D,1] on the device -> PointCloud
    objsPose, objsBbox3DSize, objsBbox2D, objsBbox3DProj = poses.numpy()        # the reference's arrays

All arithmetic is float64 inside and float32 / int32 at the interface; candidate order, acceptance tests, the unclamped IoU and the
lowest-k tie rule are the reference's.  One camera and one image size per call.
"""
import ctypes

import numpy as np
import torch

# The reference's kitti_proj_mat (visualizer.py:5-10): a setting, kept as data.
KITTI_PROJ_MAT = np.array([[7.21537720e+02, 0.00000000e+00, 6.09559326e+02, 4.48572807e+01],
                           [0.00000000e+00, 7.21537720e+02, 1.72854004e+02, 2.16379106e-01],
                           [0.00000000e+00, 0.00000000e+00, 1.00000000e+00, 2.74588400e-03],
                           [0.00000000e+00, 0.00000000e+00, 0.00000000e+00, 1.00000000e+00]])
MAX_DETECTIONS = 65536


class ObjectPoses(object):
    """The result of object_poses for n detections, as tensors on the device (on the CPU for host=True).

    per detection i    keep int32 [n];  candidate int32 [n] (the winning k; -1 no candidate accepted; -2 pre-filtered or NaN input);
                       iou float32 [n]
    compacted          count int32 [1];  index int32 [n] (source row of each kept detection, input order);  pose float32 [n,16];
                       size float32 [n,3] = (h, l, w);  box2d int32 [n,4];  box3d_proj float32 [n,16].  Only rows below count hold values."""
    __slots__ = ('keep', 'candidate', 'iou', 'count_', 'index', 'pose', 'size', 'box2d', 'box3d_proj', '_count')

    def __init__(self, keep, candidate, iou, count, index, pose, size, box2d, box3d_proj):
        self.keep, self.candidate, self.iou, self.count_, self.index = keep, candidate, iou, count, index
        self.pose, self.size, self.box2d, self.box3d_proj = pose, size, box2d, box3d_proj
        self._count = None

    def __len__(self):
        return int(self.keep.shape[0])

    def count(self):
        """Kept detections (reads 4 bytes, once: THE synchronisation)."""
        if self._count is None:
            self._count = int(self.count_.item()) if len(self) else 0
        return self._count

    def numpy(self):
        """-> the reference's (objsPose [M,4,4], objsBbox3DSize [M,3], objsBbox2D [M,4] int, objsBbox3DProj [M,2,2,2,2])."""
        M = self.count()
        return (self.pose[:M].cpu().numpy().reshape(M, 4, 4), self.size[:M].cpu().numpy(), self.box2d[:M].cpu().numpy(),
                self.box3d_proj[:M].cpu().numpy().reshape(M, 2, 2, 2, 2))

    def points(self, shapes, prob=0.5, surface_only=False):
        """shapes [n, D^3 values] (one grid per DETECTION, e.g. getSampledShape's result) -> the PointCloud of the kept objects:
        shapes[index[:M]] gathered on the device, then voxel_points with `size` and `pose`.  None when nothing is kept."""
        from .hostio import HostPrediction
        from .points import voxel_points
        from .tensor import DeviceArray, as_device_f32
        M = self.count()
        if M == 0:
            return None
        if isinstance(shapes, (DeviceArray, HostPrediction)):
            shapes = shapes.t
        device = self.pose.device if self.pose.is_cuda else (shapes.device if isinstance(shapes, torch.Tensor) and shapes.is_cuda else None)
        if device is None:
            import voxvae
            device = torch.device(voxvae.default_device())
        if device.type != 'cuda':
            from .lib import VoxVaeError
            raise VoxVaeError('ObjectPoses.points runs on the GPU only (device %s); there is no CPU fallback' % device)
        t = as_device_f32(shapes, device)
        if t.shape[0] != len(self):
            raise ValueError('shapes holds %d grids for %d detections' % (t.shape[0], len(self)))
        picked = t.index_select(0, self.index[:M].to(device=device, dtype=torch.int64))
        # `size` is (h, l, w) where voxel_points documents (h, w, l): it uses max(h, w, l) only, so the order is harmless
        return voxel_points(picked, self.size[:M].to(device), self.pose[:M].to(device).reshape(M, 4, 4), prob=prob, surface_only=surface_only)


def _rows(x, device, width, what):
    from .tensor import DeviceArray
    if isinstance(x, DeviceArray):
        x = x.t
    t = x if isinstance(x, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(np.asarray(x, dtype=np.float32).reshape(-1, width)))
    t = t.to(device=device, dtype=torch.float32).reshape(-1, width).contiguous()
    return t


def object_poses(bbox2D, bbox3D, sin, cos, image_size, proj_mat=KITTI_PROJ_MAT, proj_mat_inv=None, host=False):
    """Detections -> ObjectPoses.

    bbox2D [n,5] = (x1, y1, x2, y2, objectness) normalised to the image, bbox3D [n,3] = (w, h, l), sin / cos [n,3] of (azimuth,
    elevation, in-plane): numpy arrays, torch tensors or DeviceArrays.  image_size = (image_col, image_row).  proj_mat 4x4;
    proj_mat_inv None: inverted in float64 on the host.  Both travel to the kernel as arguments: no allocation, no copy.
    host=False  runs on the current stream of the device the inputs live on (voxvae's default device for host input); without a GPU
                that is an error, not a fallback.
    host=True   the same arithmetic compiled for the CPU (vv_object_pose_host): a handful of objects without a GPU.
    n == 0 returns an empty result without a call."""
    import voxvae
    from . import lib as L
    from .tensor import DeviceArray
    if host:
        device = torch.device('cpu')
    else:
        held = [v.t if isinstance(v, DeviceArray) else v for v in (bbox2D, bbox3D, sin, cos)]
        on = [v.device for v in held if isinstance(v, torch.Tensor) and v.is_cuda]
        device = on[0] if on else torch.device(voxvae.default_device())
        if device.type != 'cuda' or not torch.cuda.is_available():
            raise L.VoxVaeError('object_poses runs on the GPU (default device %s, CUDA available: %s); there is no silent CPU fallback: '
                                'pass host=True for the host entry' % (device, torch.cuda.is_available()))
    b2, b3, sn, cs = _rows(bbox2D, device, 5, 'bbox2D'), _rows(bbox3D, device, 3, 'bbox3D'), _rows(sin, device, 3, 'sin'), _rows(cos, device, 3, 'cos')
    n = int(b2.shape[0])
    if not (b3.shape[0] == sn.shape[0] == cs.shape[0] == n):
        raise ValueError('bbox2D, bbox3D, sin, cos must describe the same detections, got %d / %d / %d / %d rows'
                         % (n, b3.shape[0], sn.shape[0], cs.shape[0]))
    if n > MAX_DETECTIONS:
        raise ValueError('at most %d detections per call, got %d' % (MAX_DETECTIONS, n))
    col, row = float(image_size[0]), float(image_size[1])
    P = np.ascontiguousarray(np.asarray(proj_mat, dtype=np.float64).reshape(4, 4))
    Pinv = np.ascontiguousarray(np.linalg.inv(P) if proj_mat_inv is None else np.asarray(proj_mat_inv, dtype=np.float64).reshape(4, 4))
    new = lambda shape, dt: torch.empty(shape, dtype=dt, device=device)
    out = ObjectPoses(new((n,), torch.int32), new((n,), torch.int32), new((n,), torch.float32), new((1,), torch.int32), new((n,), torch.int32),
                      new((n, 16), torch.float32), new((n, 3), torch.float32), new((n, 4), torch.int32), new((n, 16), torch.float32))
    if n == 0:
        return out
    head = (L.ptr(b2), L.ptr(b3), L.ptr(sn), L.ptr(cs), n, col, row, P.ctypes.data_as(ctypes.c_void_p), Pinv.ctypes.data_as(ctypes.c_void_p),
            L.ptr(out.keep), L.ptr(out.candidate), L.ptr(out.iou), L.ptr(out.count_), L.ptr(out.index), L.ptr(out.pose), L.ptr(out.size),
            L.ptr(out.box2d), L.ptr(out.box3d_proj))
    if host:
        L.call('vv_object_pose_host', *head, None, 0)
        return out
    lib = L.load()
    need = lib.vv_object_pose_workspace_bytes(n)
    ws = torch.empty(need, dtype=torch.uint8, device=device)
    L.call('vv_object_pose', *head, L.ptr(ws), need, ctypes.c_void_p(torch.cuda.current_stream(device).cuda_stream))
    return out
