"""Pascal3D+ single-object loader, mirror of the reference's src/dataset_loader/pascal3D.py:56-283 (interface only).

`dataLoaderSingleObject(trainOrVal, Pascal3DDataPath)` with `getNextBatch(batchSizeof3DShape, imageSize, augmentation)`
returning `(instList, classList, sin, cos, inputImages, outputImages)` and the counters the scripts print (`epoch`,
`dataStart`, `dataLength`).  The dataset itself (images + CAD voxelisations, read with cv2 in the reference) does not
exist here, so `Pascal3DDataPath=None` or `'synthetic:N:D[:I]'` serves seeded stand-ins of the same shapes and dtypes:
12 classes (the Pascal3D+ categories), D^3 occupancy grids (default 64, the reference's CAD grid), and an image whose
three channels are the max-projections of the object along the three axes, resampled to `imageSize` -- so a 2D encoder
has something learnable to look at.  `instances=I` (or the `:I` field) makes instList the one-hot [n, I] of a seeded CAD
instance per sample, what the multi-modal model's instance prior reads (reference train_pascal.py); without it instList stays
the [n, 1] zeros."""
import numpy as np

from voxvae import synthetic as syn

CLASSES = 12


def _kmeans_aei(euler, k, max_iter, **kw):
    """reference pascal3D.py:156-181: the rows (sin a, sin e, sin i, cos a, cos e, cos i) in float64 of every object's Euler angles, in
    storage order, clustered by function.kmeans_cosine(...).kmeansSample() -> (centres [k,6], xtoc [n], distance [n]) as numpy."""
    from src.module.function import kmeans_cosine
    if k is None:
        raise ValueError('getKmeansAEI needs k (the reference calls it with k = 30 * 12)')
    e = np.asarray(euler, dtype=np.float64).reshape(-1, 3)
    AEI = np.concatenate([np.sin(e), np.cos(e)], axis=1)
    return kmeans_cosine(X=AEI, k=k, max_iter=max_iter, **kw).kmeansSample()


class dataLoaderSingleObject(object):
    def __init__(self, trainOrVal='train', Pascal3DDataPath=None, voxel=64, instances=None):
        n = 256 if trainOrVal == 'train' else 96
        if isinstance(Pascal3DDataPath, str) and Pascal3DDataPath.startswith('synthetic:'):
            parts = Pascal3DDataPath.split(':')
            n = int(parts[1])
            voxel = int(parts[2]) if len(parts) > 2 else voxel
            instances = int(parts[3]) if len(parts) > 3 else instances
        elif Pascal3DDataPath is not None:
            raise FileNotFoundError('Pascal3D+ is not available in this build; pass None or synthetic:N:D[:I]')
        seed = 4321 if trainOrVal == 'train' else 8765
        self._rng = np.random.default_rng(seed)
        self._voxels = syn.make_voxels(n, voxel, seed=seed)                  # [n,D,D,D,1] in {0,1}
        self._classes = self._rng.integers(0, CLASSES, n)
        self._euler = self._rng.uniform(-np.pi, np.pi, (n, 3)).astype('float32')
        # drawn from a generator of its own: the streams above do not move when instances are asked for
        self._insts = None if instances is None else np.random.default_rng(seed + 1).integers(0, int(instances), n)
        self._instances = instances
        self._order = np.arange(n)
        self.epoch = 0
        self.dataStart = 0
        self.dataLength = n
        self._shuffle = trainOrVal == 'train'
        if self._shuffle:
            self._rng.shuffle(self._order)

    @staticmethod
    def _project(v, size):
        col, row = size                                                      # the reference passes (image_col, image_row)
        g = v[..., 0]
        chans = []
        for ax in range(3):
            p = g.max(axis=ax)                                               # [D,D]
            ri = (np.arange(row) * p.shape[0] // row).clip(0, p.shape[0] - 1)
            ci = (np.arange(col) * p.shape[1] // col).clip(0, p.shape[1] - 1)
            chans.append(p[ri][:, ci])
        return np.stack(chans, axis=-1).astype('float32')                    # [row, col, 3]

    def getNextBatch(self, batchSizeof3DShape=32, imageSize=None, augmentation=True):
        size = imageSize or (256, 256)
        idx = self._order[self.dataStart:self.dataStart + batchSizeof3DShape]
        self.dataStart += len(idx)
        if self.dataStart >= self.dataLength:
            self.epoch += 1
            self.dataStart = 0
            if self._shuffle:
                self._rng.shuffle(self._order)
        out = self._voxels[idx]
        imgs = np.stack([self._project(v, size) for v in out])
        if augmentation:
            imgs = np.clip(imgs + self._rng.normal(0, 0.05, imgs.shape).astype('float32'), 0, 1)
        cls = np.eye(CLASSES, dtype='float32')[self._classes[idx]]
        inst = np.zeros((len(idx), 1), dtype='float32') if self._insts is None else np.eye(int(self._instances), dtype='float32')[self._insts[idx]]
        e = self._euler[idx]
        return inst, cls, np.sin(e), np.cos(e), imgs.astype('float32'), out.astype('float32')

    def getKmeansAEI(self, k=None, max_iter=1000, **kw):
        """reference :156-181 over the loader's objects in storage order; `device=` / `host=` go to kmeans_cosine."""
        return _kmeans_aei(self._euler, k, max_iter, **kw)


class deviceDataLoaderSingleObject(object):
    """On-device variant of dataLoaderSingleObject: the photos live in device memory as one uint8 arena, the CAD grids as packed bits, and
    getNextBatch builds the batch with the reference's own input chain (pascal3D.py:216-283: crop with a random border, flip, colour
    perturbation, warpAffine, cubic resize, / 255) in launches -- permutation slice, vv_augment_draw, vv_augment_images, the existing
    vv_unpack_bits_gather -- with no host round trip.  Same constructor strings (None, 'synthetic:N:D[:I]'), same six return values in the
    same order, as float32 device tensors.  The azimuth's sign follows the horizontal flip (:247-248).

    The synthetic stand-in serves seeded "photos": uint8 images of differing sizes, one per object, with a box; the object's three
    max-projections are pasted at the box over a seeded textured background, so crop, border and warp all matter.  `from_arrays` takes
    decoded data instead.  The draws are a pure function of (voxvae.manual_seed's seed, rank, step): voxvae/augment.py; `last_params` holds
    the rows of the last batch.  colour_ops='invert_add' (the default) applies Invert and Add, as this loader always did; colour_ops='all'
    applies the reference's four -- GaussianBlur, Invert, Add, AddToHueAndSaturation, in that order -- through the colour table of
    csrc/augment.h (`last_colour` holds its rows; the geometry and the Invert / Add draws are the same under both settings)."""

    COLOUR_OPS = ('invert_add', 'all')

    def __init__(self, trainOrVal='train', Pascal3DDataPath=None, voxel=64, instances=None, device=None, seed=None, colour_ops='invert_add'):
        n = 256 if trainOrVal == 'train' else 96
        if isinstance(Pascal3DDataPath, str) and Pascal3DDataPath.startswith('synthetic:'):
            parts = Pascal3DDataPath.split(':')
            n = int(parts[1])
            voxel = int(parts[2]) if len(parts) > 2 else voxel
            instances = int(parts[3]) if len(parts) > 3 else instances
        elif Pascal3DDataPath is not None:
            raise FileNotFoundError('Pascal3D+ is not available in this build; pass None or synthetic:N:D[:I]')
        data_seed = 4321 if trainOrVal == 'train' else 8765
        rng = np.random.default_rng(data_seed)
        voxels = syn.make_voxels(n, voxel, seed=data_seed)[..., 0]           # [n,D,D,D] in {0,1}
        classes = rng.integers(0, CLASSES, n)
        euler = rng.uniform(-np.pi, np.pi, (n, 3)).astype('float32')
        insts = None if instances is None else np.random.default_rng(data_seed + 1).integers(0, int(instances), n)
        images, boxes = self._photos(voxels, np.random.default_rng(data_seed + 2))
        self._setup(images, boxes, classes, np.arange(n), euler, voxels, insts, instances, None, device,
                    data_seed if seed is None else seed, trainOrVal == 'train', colour_ops)

    @classmethod
    def from_arrays(cls, images, boxes, classes, cad_index, euler, cad_grids, inst_index=None, instances=None, image_index=None, device=None,
                    seed=None, shuffle=True, colour_ops='invert_add'):
        """images: uint8 [rows, cols, 3] arrays; boxes [n, 4] = (colMin, rowMin, colMax, rowMax) in pixels; classes [n] in 0 .. 11;
        cad_index [n] rows of cad_grids [m, D, D, D] (occupancy, binarised at 0.5); euler [n, 3] = (azimuth, elevation, in-plane
        rotation) in radians.  image_index [n] (default: object i is in image i) lets several objects share a photo; instances with
        inst_index (default cad_index) makes instList the one-hot [n, instances], otherwise it is the [n, 1] zeros."""
        self = cls.__new__(cls)
        insts = None if instances is None else np.asarray(cad_index if inst_index is None else inst_index)
        self._setup(images, boxes, classes, cad_index, euler, cad_grids, insts, instances, image_index, device, seed, shuffle, colour_ops)
        return self

    @staticmethod
    def _photos(voxels, rng):
        n, D = voxels.shape[:2]
        images, boxes = [], np.empty((n, 4), dtype='float32')
        for i in range(n):
            rows, cols = int(rng.integers(2 * D, 4 * D)), int(rng.integers(2 * D, 4 * D))
            coarse = rng.integers(0, 256, (rows // 8 + 1, cols // 8 + 1, 3))
            photo = np.repeat(np.repeat(coarse, 8, axis=0), 8, axis=1)[:rows, :cols] // 2 + rng.integers(0, 64, (rows, cols, 3))
            bh, bw = int(rng.integers(rows // 3, (2 * rows) // 3)), int(rng.integers(cols // 3, (2 * cols) // 3))
            r0, c0 = int(rng.integers(0, rows - bh)), int(rng.integers(0, cols - bw))
            proj = np.stack([voxels[i].max(axis=ax) for ax in range(3)], axis=-1)          # [D,D,3]
            ri, ci = np.arange(bh) * D // bh, np.arange(bw) * D // bw
            obj = proj[ri][:, ci]
            region = photo[r0:r0 + bh, c0:c0 + bw]
            region[obj.max(axis=-1) > 0] = (obj * 255)[obj.max(axis=-1) > 0]
            images.append(photo.astype('uint8'))
            f = rng.uniform(0, 1, 4)                                                        # boxes are not on the pixel grid
            boxes[i] = (c0 + f[0], r0 + f[1], c0 + bw - f[2], r0 + bh - f[3])
        return images, boxes

    def _setup(self, images, boxes, classes, cad_index, euler, cad_grids, insts, instances, image_index, device, seed, shuffle,
               colour_ops='invert_add'):
        if colour_ops not in self.COLOUR_OPS:
            raise ValueError('colour_ops must be one of %s, got %r' % (self.COLOUR_OPS, colour_ops))
        self.colour_ops = colour_ops
        import torch
        import voxvae
        from voxvae import augment as _A
        from voxvae import lib as _L
        self._torch, self._A, self._L = torch, _A, _L
        self._device = torch.device(device or voxvae.default_device())
        boxes = np.ascontiguousarray(boxes, dtype='float32').reshape(-1, 4)
        n = boxes.shape[0]
        image_index = np.arange(n) if image_index is None else np.asarray(image_index)
        classes, cad_index, euler = np.asarray(classes), np.asarray(cad_index), np.asarray(euler, dtype='float32').reshape(-1, 3)
        grids = np.asarray(cad_grids)
        grids = grids[..., 0] if grids.ndim == 5 else grids
        if not (len(image_index) == len(classes) == len(cad_index) == len(euler) == n):
            raise ValueError('boxes, classes, cad_index, euler and image_index must name the same %d objects' % n)
        if image_index.min() < 0 or image_index.max() >= len(images) or cad_index.min() < 0 or cad_index.max() >= grids.shape[0]:
            raise ValueError('image_index / cad_index outside the images / CAD grids')
        if not np.isfinite(boxes).all():
            raise ValueError('boxes must be finite')
        # every box at least 2 px in both extents after the reference's truncation at border ratio 0
        ext = np.array([images[i].shape[:2] for i in image_index], dtype='float32')
        c0, c1 = np.maximum(0, boxes[:, 0]).astype(int), np.minimum(ext[:, 1], boxes[:, 2]).astype(int)
        r0, r1 = np.maximum(0, boxes[:, 1]).astype(int), np.minimum(ext[:, 0], boxes[:, 3]).astype(int)
        bad = np.flatnonzero(~((c1 - c0 >= 2) & (r1 - r0 >= 2)))
        if bad.size:
            raise ValueError('boxes under 2 px after truncation to the image: objects %s' % bad[:8].tolist())
        self._sample_shape = tuple(grids.shape[1:]) + (1,)
        self._voxels = int(np.prod(self._sample_shape))
        if self._voxels % 8:
            raise ValueError('voxel count per CAD grid must be a multiple of 8')
        dev = self._device
        self._arena = _A.ImageArena.from_arrays(images, device=dev)
        self._packed = torch.from_numpy(np.ascontiguousarray(np.packbits(grids.reshape(grids.shape[0], -1) > 0.5, axis=1, bitorder='little'))).to(dev)
        self._image_index = torch.from_numpy(image_index.astype('int32')).to(dev)
        self._cad_index = torch.from_numpy(cad_index.astype('int32')).to(dev)
        self._boxes = torch.from_numpy(boxes).to(dev)
        self._cls = torch.from_numpy(np.eye(CLASSES, dtype='float32')[classes]).to(dev)
        self._inst = torch.from_numpy(np.zeros((n, 1), dtype='float32') if insts is None else np.eye(int(instances), dtype='float32')[insts]).to(dev)
        self._sin, self._cos = torch.from_numpy(np.sin(euler)).to(dev), torch.from_numpy(np.cos(euler)).to(dev)
        self._euler = euler                                                  # host copy, storage order: getKmeansAEI
        self._gen = torch.Generator(device=dev)
        if seed is not None:
            self._gen.manual_seed(int(seed))
        self._shuffle = bool(shuffle)
        self._order = torch.arange(n, device=dev)
        if self._shuffle:
            self._order = torch.randperm(n, device=dev, generator=self._gen)
        self.epoch, self.dataStart, self.dataLength = 0, 0, n
        self._step = 0
        self.last_params = self.last_colour = None

    def getNextBatch(self, batchSizeof3DShape=32, imageSize=None, augmentation=True):
        torch, A, L = self._torch, self._A, self._L
        col, row = imageSize or (256, 256)                                   # (image_col, image_row), as dataLoaderSingleObject reads it
        idx = self._order[self.dataStart:self.dataStart + batchSizeof3DShape]
        self.dataStart += int(idx.numel())
        if self.dataStart >= self.dataLength:
            self.epoch += 1
            self.dataStart = 0
            if self._shuffle:
                self._order = torch.randperm(self.dataLength, device=self._device, generator=self._gen)
        colour = None
        if self.colour_ops == 'all':
            params, colour = A.draw_params(self._arena, self._image_index[idx], self._boxes[idx], augmentation, self._step, colour=True)
        else:
            params = A.draw_params(self._arena, self._image_index[idx], self._boxes[idx], augmentation, self._step)
        self._step += 1
        self.last_params, self.last_colour = params, colour
        images = A.augment_images(self._arena, params, (row, col), colour=colour)
        B = int(idx.numel())
        out = torch.empty((B,) + self._sample_shape, dtype=torch.float32, device=self._device)
        with torch.cuda.device(self._device):
            st = L.ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
        L.call('vv_unpack_bits_gather', L.ptr(self._packed), L.ptr(self._cad_index[idx].contiguous()), L.ptr(out), B, self._voxels, st)
        sin = self._sin[idx].clone()
        flipped = (params[:, A.P_FLIP] & 1) != 0
        sin[:, 0] = torch.where(flipped, -sin[:, 0], sin[:, 0])              # azimuth -> -azimuth: the sine changes sign, the cosine does not
        return self._inst[idx], self._cls[idx], sin, self._cos[idx], images, out

    def getKmeansAEI(self, k=None, max_iter=1000, **kw):
        """As dataLoaderSingleObject.getKmeansAEI, on this loader's device unless `device=` / `host=` say otherwise."""
        if 'device' not in kw and 'host' not in kw:
            kw['device'] = self._device
        return _kmeans_aei(self._euler, k, max_iter, **kw)


# what the entry scripts' --loader names
LOADERS = {'host': dataLoaderSingleObject, 'device': deviceDataLoaderSingleObject}


def loader_factory(loader, colour_ops='invert_add'):
    """The class behind --loader, with --colour-ops bound to it: 'all' exists on the device loader only (the host class serves
    projections with noise, no photo chain)."""
    cls = LOADERS[loader]
    if colour_ops == 'invert_add':
        return cls
    if loader != 'device':
        raise ValueError("colour_ops=%r needs the device loader (--loader device)" % (colour_ops,))
    import functools
    return functools.partial(cls, colour_ops=colour_ops)
