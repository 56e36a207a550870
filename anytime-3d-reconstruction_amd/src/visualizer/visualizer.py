"""Drop-in for the reference's src/visualizer/visualizer.py without its drawing functions: detections -> posed objects -> their
points in the world.  Same names, arguments and return forms; the arithmetic is the HIP library.

    getObjectInRealWorld   all detections of a frame in two launches (voxvae/pose.py, csrc/object_pose.hip), the kept objects' grids
                           posed on the device (voxvae/points.py, csrc/voxel_points.hip); returns the reference's five values
    getTranslation, getRay, getRayRotation, get3DbboxProjection
                           the single-object helpers, numpy in and out, through the host build of the same solver (csrc/pose_solve.h):
                           no GPU needed
    objRescaleTransform    (:171-188) one predicted occupancy grid -> the object's points; the grid may have any side up to 128 (the
                           reference hard-codes 64).  objectsRescaleTransform is the batched form, the grids staying on the device.

Not here: the cv2 drawing functions (draw2Dbbox, draw3Dbbox); cv2 is not a dependency of this package.
"""
import ctypes

import numpy as np
import torch

from voxvae.hostio import HostPrediction
from voxvae.points import voxel_points
from voxvae.pose import KITTI_PROJ_MAT, object_poses
from voxvae.tensor import DeviceArray

kitti_proj_mat = KITTI_PROJ_MAT
kitti_proj_mat_inv = np.linalg.inv(kitti_proj_mat)


def _f64(a, shape):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float64).reshape(shape))


def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def getTranslation(proj_mat, R, bbox2D, bbox3D):
    """(:79-146) proj_mat 4x4, R 3x3, bbox2D = (x_min, y_min, x_max, y_max) in pixels, bbox3D = (w, h, l) -> the translation [3,1]
    of the candidate whose reprojected box has the best IoU with bbox2D (zeros when every candidate is rejected)."""
    from voxvae import lib as L
    X = np.zeros(3)
    L.call('vv_pose_translation_host', _p(_f64(proj_mat, (4, 4))), _p(_f64(R, (3, 3))), _p(_f64(bbox2D, (4,))), _p(_f64(bbox3D, (3,))), _p(X),
           None, None)
    return X.reshape(3, 1)


def getRay(P_inv, pixel):
    """(:148-155) the unit ray through `pixel` = (px, py); the reference's print for a ray pointing backwards is dropped."""
    from voxvae import lib as L
    ray = np.zeros(3)
    L.call('vv_pose_ray_host', _p(_f64(P_inv, (4, 4))), float(pixel[0]), float(pixel[1]), _p(ray))
    return ray


def getRayRotation(ray):
    """(:157-168) the rotation that takes the optical axis onto `ray` (about x, then about y)."""
    from voxvae import lib as L
    R = np.zeros((3, 3))
    L.call('vv_pose_ray_rotation_host', _p(_f64(ray, (3,))), _p(R))
    return R


def get3DbboxProjection(projmat, R, t, w, h, l):
    """(:191-205) the eight corners R (+-w/2, +-l/2, +-h/2) + t projected by projmat -> [2,2,2,2] (i, j, k, xy), index 0 = +."""
    from voxvae import lib as L
    a = np.zeros((2, 2, 2, 2))
    L.call('vv_pose_box_projection_host', _p(_f64(projmat, (4, 4))), _p(_f64(R, (3, 3))), _p(_f64(t, (3,))), float(w), float(h), float(l), _p(a))
    return a


def getObjectInRealWorld(normalized_bbox2D_list, bbox3D_list, sin_list, cos_list, shape_3D_list, image_size,
                         proj_mat=kitti_proj_mat, proj_mat_inv=kitti_proj_mat_inv):
    """(:237-308) per detection: normalised box (x1, y1, x2, y2, objectness), size (w, h, l), sines and cosines of (azimuth, elevation,
    in-plane), its predicted occupancy grid (D^3 values; all grids of one side, <= 128) -> for the detections that pass both filters, in
    input order: (objsPose [M,4,4], objsBbox3DSize [M,3] = (h, l, w), objsPoints, objsBbox2D [M,4] int, objsBbox3DProj [M,2,2,2,2]).
    objsPoints is a LIST of M [n_b,3] arrays (the reference's np.array of ragged arrays is an error on current numpy).  shape_3D_list
    may be a DeviceArray / CUDA tensor [n, ...]: then nothing but the results leaves the device."""
    poses = object_poses(normalized_bbox2D_list, bbox3D_list, sin_list, cos_list, image_size, proj_mat, proj_mat_inv)
    objsPose, objsBbox3DSize, objsBbox2D, objsBbox3DProj = poses.numpy()
    if poses.count() == 0:
        return objsPose, objsBbox3DSize, [], objsBbox2D, objsBbox3DProj
    if isinstance(shape_3D_list, (list, tuple)):
        shape_3D_list = (torch.stack([g.reshape(-1) for g in shape_3D_list]) if isinstance(shape_3D_list[0], torch.Tensor)
                         else np.stack([np.asarray(g, dtype=np.float32).reshape(-1) for g in shape_3D_list]))
    grid, side = _grids(shape_3D_list, True)
    return objsPose, objsBbox3DSize, poses.points(grid).split(), objsBbox2D, objsBbox3DProj


def _grids(objPoints, batched):
    """-> (the occupancy in a form voxel_points takes, shaped [B,D,D,D]; the side).  Host arrays of one object may come flat or as
    [D,D,D(,1)], as the reference's reshape allows."""
    if isinstance(objPoints, (DeviceArray, HostPrediction)):
        objPoints = objPoints.t                             # their device tensor
    elif not isinstance(objPoints, torch.Tensor):
        objPoints = np.asarray(objPoints)
    shape = tuple(objPoints.shape)
    n = int(np.prod(shape[1:] if batched else shape))
    side = int(round(n ** (1.0 / 3.0)))
    if side ** 3 != n:
        raise ValueError('objPoints %s is not %s cubic grid' % (list(shape), 'a batch of' if batched else 'one'))
    return objPoints.reshape(-1, side, side, side), side


def objRescaleTransform(objPoints, h, w, l, R):
    """One object: objPoints = its occupancy probabilities (D^3 values in any shape; numpy, torch CUDA tensor or DeviceArray), (h, w, l)
    its size, R its 4x4 pose (rows 0 .. 2 are used; 3x4 is taken too).  Returns the numpy [n,3] array of the reference: the cells with p > 0.5 in
    row-major order, scaled so that their largest extent is max(h, w, l), centred, posed.  An empty grid returns [0,3] (the reference
    raises); a single occupied cell returns the translation (the reference returns NaN)."""
    grid, side = _grids(objPoints, False)
    return voxel_points(grid, [[h, w, l]], R, side=side).split()[0]


def objectsRescaleTransform(objsPoints, hwl, R=None, prob=0.5, surface_only=False):
    """Batched: objsPoints [B, D^3 values], hwl [B,3] = (h, w, l) per object, R None / one pose / [B,4,4] -> the list of B numpy
    [n_b,3] arrays (`objsPoints` of the reference's getObjectInRealWorld).  surface_only keeps the surface cells only (an extension)."""
    grid, side = _grids(objsPoints, True)
    return voxel_points(grid, hwl, R, prob=prob, surface_only=surface_only, side=side).split()
