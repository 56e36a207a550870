"""float64 numpy restatement of the image chain of csrc/augment.h, written from the reference (src/dataset_loader/datasetUtils.py:64-89,
:137-148; pascal3D.py:225-242) and the OpenCV semantics it relies on, not from the header:

  source   crop of the zero-padded image, cv2.flip, imgaug Invert then Add (clipped to 0 .. 255)
  warp     cv2.warpAffine(M, (w, h)): dst(x, y) = src(M^-1 (x, y)), pixel centres at integers, bilinear, constant border 0, uint8 result
           (round half up); M = [[s, 0, (w / 2)(1 - s) + dCol], [0, s, (h / 2)(1 - s) + dRow]]
  resize   cv2.resize(INTER_CUBIC): f = (d + 0.5) * src / dst - 0.5, Keys kernel a = -0.75 over four taps, replicated edge, no
           antialiasing, saturate-cast to uint8 (round half up, clip), then / 255
Everything in float64 on exact inputs (the scale is the float32 value the params row holds)."""
import numpy as np

A = -0.75


def keys(x):
    x = np.abs(x)
    return np.where(x <= 1.0, ((A + 2.0) * x - (A + 3.0)) * x * x + 1.0, np.where(x < 2.0, ((A * x - 5.0 * A) * x + 8.0 * A) * x - 4.0 * A, 0.0))


def source(image, row0, col0, h, w, flip=0, invert=0, add=(0, 0, 0), row_pad=0, col_pad=0):
    """The crop after flips and colour changes: float64 [h, w, 3] of integer levels."""
    padded = np.pad(np.asarray(image, dtype=np.int64), ((row_pad, row_pad), (col_pad, col_pad), (0, 0)))
    crop = padded[row0:row0 + h, col0:col0 + w]
    assert crop.shape[:2] == (h, w)
    if flip & 1:
        crop = crop[:, ::-1]
    if flip & 2:
        crop = crop[::-1]
    crop = crop.copy()
    for c in range(3):
        if (invert >> c) & 1:
            crop[..., c] = 255 - crop[..., c]
        crop[..., c] = np.clip(crop[..., c] + int(add[c]), 0, 255)
    return crop.astype(np.float64)


def warp(src, s, d_row, d_col):
    h, w = src.shape[:2]
    s = float(s)
    tx, ty = (w / 2.0) * (1.0 - s) + d_col, (h / 2.0) * (1.0 - s) + d_row
    sx = (np.arange(w, dtype=np.float64) - tx) / s
    sy = (np.arange(h, dtype=np.float64) - ty) / s
    x0, y0 = np.floor(sx).astype(np.int64), np.floor(sy).astype(np.int64)
    ax, ay = (sx - x0)[None, :, None], (sy - y0)[:, None, None]
    big = np.zeros((h + 2, w + 2, 3))                       # a ring of border zeros: index i + 1 holds pixel i, i = -1 .. extent
    big[1:-1, 1:-1] = src

    def take(yy, xx):
        ok_y, ok_x = (yy >= -1) & (yy <= h), (xx >= -1) & (xx <= w)
        v = big[np.clip(yy, -1, h)[:, None] + 1, np.clip(xx, -1, w)[None, :] + 1]
        return v * (ok_y[:, None] & ok_x[None, :])[..., None]

    v = (1 - ay) * ((1 - ax) * take(y0, x0) + ax * take(y0, x0 + 1)) + ay * ((1 - ax) * take(y0 + 1, x0) + ax * take(y0 + 1, x0 + 1))
    return np.clip(np.floor(v + 0.5), 0, 255)


def resize_cubic(src, out_rows, out_cols):
    h, w = src.shape[:2]

    def axis(n_src, n_dst):
        f = (np.arange(n_dst, dtype=np.float64) + 0.5) * (n_src / n_dst) - 0.5
        i = np.floor(f).astype(np.int64)
        taps = i[:, None] + np.arange(-1, 3)[None, :]
        wts = keys(f[:, None] - taps)
        return np.clip(taps, 0, n_src - 1), wts

    ty, wy = axis(h, out_rows)
    tx, wx = axis(w, out_cols)
    g = src[ty[:, :, None, None], tx[None, None, :, :]]     # [out_rows, 4, out_cols, 4, 3]
    v = np.einsum('rickx,ri,ck->rcx', g, wy, wx)
    return np.clip(np.floor(v + 0.5), 0, 255)


def chain(image, out_rows, out_cols, row0, col0, h, w, flip=0, s=1.0, d_row=0, d_col=0, invert=0, add=(0, 0, 0), row_pad=0, col_pad=0):
    """-> integer levels float64 [out_rows, out_cols, 3] (the output is level / 255)."""
    return resize_cubic(warp(source(image, row0, col0, h, w, flip, invert, add, row_pad, col_pad), np.float32(s), d_row, d_col), out_rows, out_cols)


def chain_of_row(images, p, out_rows, out_cols):
    """chain() for one int32 params row of the documented layout."""
    p = np.asarray(p, dtype=np.int32)
    return chain(images[int(p[0])], out_rows, out_cols, int(p[1]), int(p[2]), int(p[3]), int(p[4]), int(p[5]), p[6:7].view(np.float32)[0], int(p[7]),
                 int(p[8]), int(p[9]), (int(p[10]), int(p[11]), int(p[12])), int(p[13]), int(p[14]))


def random_images(seed, sizes):
    rng = np.random.default_rng(seed)
    return [rng.integers(0, 256, (r, c, 3), dtype=np.uint8) for r, c in sizes]


def compare_levels(got01, want_levels):
    """-> (largest level difference, share of values that differ) between an output in 0 .. 1 and oracle levels."""
    got = np.rint(np.asarray(got01, dtype=np.float64) * 255.0)
    d = np.abs(got - want_levels)
    return float(d.max()), float((d > 0).mean())
