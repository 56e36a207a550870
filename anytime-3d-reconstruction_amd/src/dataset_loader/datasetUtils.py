"""Mirror of the reference's src/dataset_loader/datasetUtils.py for what its scripts call: `imageRandomAugmentation` and `natural_keys`.
`noisy`, `imageAugmentation` and `imgAug` are not ported (no script calls them).

imageRandomAugmentation takes one uint8 HWC image and returns the reference's 6-tuple
(image, rowPadding, dRowTrans, colPadding, dColTrans, scaleRatio); the image is uint8 [imageRowFinal, imageColFinal, 3].  It needs no
GPU: the warp and the cubic resize run through the host twin of the device kernel (vv_augment_images_host, csrc/augment.h), whose float32
definition of cv2.warpAffine / cv2.resize(INTER_CUBIC) does not model cv2's fixed-point coefficient tables.  The random draws are the
reference's np.random calls in the reference's order, so np.random.seed fixes them.  Of imgAug's four operations Invert and Add are
applied (before the padding, as the reference does); GaussianBlur and AddToHueAndSaturation are chosen and NOT applied.  A translation
bound of 0 gives 0 (the reference's randint(0, 0) raises)."""
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


def imageRandomAugmentation(
        inputImage, imageRowFinal, imageColFinal, padding=True,
        imAug=True, imAugPr=0.5,
        randomTrans=True, randomScale=True, transPr=0.5, scalePr=0.5,
        transRatioMax=0.2, scaleRatioMin=0.8, scaleRatioMax=1.2):
    from voxvae import augment as A
    inputImage = np.ascontiguousarray(inputImage, dtype=np.uint8)
    imageRow, imageCol, _ = inputImage.shape
    if imAug:
        if np.random.rand() < imAugPr:
            gaussian, brightness, hueSat, channelInvert = np.random.choice(a=[False, True], size=4, p=[0.5, 0.5])
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
