"""Mirror of the reference's src/dataset_loader/datasetUtils.py for what its scripts call: `imageRandomAugmentation` (with the `imgAug` it
calls) and `natural_keys`.  `noisy` and `imageAugmentation` are not ported (no script calls them).

imageRandomAugmentation takes one uint8 HWC image and returns the reference's 6-tuple
(image, rowPadding, dRowTrans, colPadding, dColTrans, scaleRatio); the image is uint8 [imageRowFinal, imageColFinal, 3].  It needs no
GPU: the warp and the cubic resize run through the host twin of the device kernel (vv_augment_images_host, csrc/augment.h), whose float32
definition of cv2.warpAffine / cv2.resize(INTER_CUBIC) does not model cv2's fixed-point coefficient tables.  The random draws are the
reference's np.random calls in the reference's order, so np.random.seed fixes them.  Of imgAug's four operations Invert and Add are
applied by default (before the padding, as the reference does), as this function always did; colour_ops='all' routes through `imgAug`,
which applies the four in the reference's Sequential order GaussianBlur -> Invert -> Add -> AddToHueAndSaturation on the host twin
(csrc/augment.h 1a, 1b says what of scipy's and cv2's arithmetic is not modelled).  A translation bound of 0 gives 0 (the
reference's randint(0, 0) raises)."""
import re

import numpy as np


def atoi(text):
    return int(text) if text.isdigit() else text


def natural_keys(text):
    return [atoi(c) for c in re.split(r'(\d+)', text)]


def _invert_add(image, channelInvert, brightness):
    """imgaug Invert(0.05, per_channel=True) then Add((-10, 10), per_channel=0.5) on a uint8 image, in integers."""
    v = image.astype(np.int32)
    if channelInvert:
        inv = np.random.rand(3) < 0.05
        v = np.where(inv[None, None, :], 255 - v, v)
    if brightness:
        per_channel = np.random.rand() < 0.5
        add = np.random.randint(-10, 11, 3) if per_channel else np.repeat(np.random.randint(-10, 11), 3)
        v = np.clip(v + add[None, None, :], 0, 255)
    return v.astype(np.uint8)


def imgAug(inputImage, crop=True, flip=True, gaussianBlur=True, channelInvert=True, brightness=True, hueSat=True, choices=None):
    """The reference's imgAug (datasetUtils.py:64-89) for the way imageRandomAugmentation calls it (crop=False, flip=False): uint8 HWC in,
    uint8 of the same shape out, the chosen stages of GaussianBlur(sigma=(0, 3.0)), Invert(0.05, per_channel=True),
    Add((-10, 10), per_channel=0.5), AddToHueAndSaturation((-20, 20)) in that order on the host twin.  The values are drawn from
    np.random in that order; `choices` injects them instead: a dict with any of sigma, invert (3 bits), add (3 values), value."""
    if crop or flip:
        raise NotImplementedError('imgAug(crop=True) / imgAug(flip=True): no reference script passes them')
    from voxvae import augment as A
    inputImage = np.ascontiguousarray(inputImage, dtype=np.uint8)
    ch = dict(choices or {})
    sigma, invert, add, value = 0.0, 0, (0, 0, 0), 0
    if gaussianBlur:
        sigma = ch['sigma'] if 'sigma' in ch else np.random.uniform(0.0, 3.0)
    if channelInvert:
        invert = ch['invert'] if 'invert' in ch else int(sum(int(b) << c for c, b in enumerate(np.random.rand(3) < 0.05)))
    if brightness:
        if 'add' in ch:
            add = tuple(int(v) for v in ch['add'])
        else:
            per_channel = np.random.rand() < 0.5
            add = tuple(int(v) for v in (np.random.randint(-10, 11, 3) if per_channel else np.repeat(np.random.randint(-10, 11), 3)))
    if hueSat:
        value = int(ch['value']) if 'value' in ch else int(np.random.randint(-20, 21))
    rows, cols = inputImage.shape[:2]
    arena = A.ImageArena.from_arrays([inputImage], device=None)
    params = A.make_params(rows=rows, cols=cols, invert=invert, add=add)
    colour = A.make_colour(sigma=sigma, hue=int(value * 180 / 255.0), sat=value, blur=bool(gaussianBlur), hue_sat=bool(hueSat))
    out = A.augment_images(arena, params[None], (rows, cols), colour=colour[None], host=True).numpy()[0]
    return np.rint(out * np.float32(255.0)).astype(np.uint8)


def imageRandomAugmentation(
        inputImage, imageRowFinal, imageColFinal, padding=True,
        imAug=True, imAugPr=0.5,
        randomTrans=True, randomScale=True, transPr=0.5, scalePr=0.5,
        transRatioMax=0.2, scaleRatioMin=0.8, scaleRatioMax=1.2, colour_ops='invert_add'):
    from voxvae import augment as A
    if colour_ops not in ('invert_add', 'all'):
        raise ValueError("colour_ops must be 'invert_add' or 'all', got %r" % (colour_ops,))
    inputImage = np.ascontiguousarray(inputImage, dtype=np.uint8)
    imageRow, imageCol, _ = inputImage.shape
    if imAug:
        if np.random.rand() < imAugPr:
            gaussian, brightness, hueSat, channelInvert = np.random.choice(a=[False, True], size=4, p=[0.5, 0.5])
            if colour_ops == 'all':
                inputImage = imgAug(inputImage=inputImage, crop=False, flip=False, gaussianBlur=gaussian, channelInvert=channelInvert,
                                    brightness=brightness, hueSat=hueSat)
            else:
                inputImage = _invert_add(inputImage, channelInvert, brightness)

    rowPadding, colPadding = 0, 0
    if padding:
        expectedRow, expectedCol = imageRowFinal, imageColFinal
        if imageRow > expectedRow:
            eRowTemp, eColTemp = expectedRow, expectedCol
            expectedRow = eRowTemp * float(imageRow) / float(eRowTemp)
            expectedCol = eColTemp * float(imageRow) / float(eRowTemp)
        if imageCol > expectedCol:
            eRowTemp, eColTemp = expectedRow, expectedCol
            expectedRow = eRowTemp * float(imageCol) / float(eColTemp)
            expectedCol = eColTemp * float(imageCol) / float(eColTemp)
        rowGap, colGap = expectedRow - imageRow, expectedCol - imageCol
        if rowGap * expectedCol < colGap * expectedRow:
            colPadding = int((colGap - rowGap * float(expectedCol) / float(expectedRow)) / 2)
        elif rowGap * expectedCol > colGap * expectedRow:
            rowPadding = int((rowGap - colGap * float(expectedRow) / float(expectedCol)) / 2)
    imageRow, imageCol = imageRow + 2 * rowPadding, imageCol + 2 * colPadding

    scaleRatio = 1.0
    if randomScale:
        if np.random.rand() < scalePr:
            scaleRatio = np.random.uniform(low=scaleRatioMin, high=scaleRatioMax)
    dRowTrans, dColTrans = 0, 0
    if randomTrans:
        if np.random.rand() < transPr:
            rowTransMax, colTransMax = int(imageRow * transRatioMax), int(imageCol * transRatioMax)
            dRowTrans = int(np.random.randint(-rowTransMax, rowTransMax)) if rowTransMax > 0 else 0
            dColTrans = int(np.random.randint(-colTransMax, colTransMax)) if colTransMax > 0 else 0

    arena = A.ImageArena.from_arrays([inputImage], device=None)
    params = A.make_params(rows=imageRow, cols=imageCol, scale=scaleRatio, d_row=dRowTrans, d_col=dColTrans, row_pad=rowPadding,
                           col_pad=colPadding)
    out = A.augment_images(arena, params[None], (imageRowFinal, imageColFinal), host=True).numpy()[0]
    return np.rint(out * np.float32(255.0)).astype(np.uint8), rowPadding, dRowTrans, colPadding, dColTrans, scaleRatio
