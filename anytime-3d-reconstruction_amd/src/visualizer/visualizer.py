"""Drop-in for the point-cloud step of the reference's src/visualizer/visualizer.py (objRescaleTransform, :171-188, called per object
from getObjectInRealWorld): a predicted occupancy grid -> the object's points in the world.  Same name, arguments and return form;
the arithmetic is the HIP library (voxvae/points.py, csrc/voxel_points.hip) and the grid may have any side up to 128 (the reference
hard-codes 64).  objectsRescaleTransform is the batched form: one call for all objects of a frame, the grids staying on the device.

Not here: the rest of the reference module -- the SVD translation fit (getTranslation), the ray / projection helpers and the cv2
drawing functions; cv2 is not a dependency of this package.
"""
import numpy as np
import torch

from voxvae.hostio import HostPrediction
from voxvae.points import voxel_points
from voxvae.tensor import DeviceArray


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
