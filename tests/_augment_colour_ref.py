"""numpy restatement of the two opt-in colour stages of csrc/augment.h, written from their definitions (imgaug GaussianBlur through
scipy.ndimage.gaussian_filter(mode='mirror', truncate 4); imgaug AddToHueAndSaturation through OpenCV's 8-bit HSV), not from the header:

  blur       float64, separable, rows then columns: weights exp(-0.5 k^2 / sigma^2), k = -r .. r, r = int(4 sigma + 0.5), over their
             sum; mirror reflection about the edge pixels (period 2(n - 1)); ONE rounding at the end (floor(v + 0.5), clipped)
  hue_sat    forward in int64 with the 12-bit reciprocal tables, inverse in np.float32 operations in the stated order
  hue_sat64  the same adds through a float64 HSV chain with colorsys's arithmetic (no 8-bit quantisation of h, s)
  levels     the four stages composed in any order on a crop of integer levels
"""
import numpy as np

SHIFT = 12


def mirror(i, n):
    i = np.asarray(i, dtype=np.int64)
    if n == 1:
        return np.zeros_like(i)
    period = 2 * (n - 1)
    i = np.mod(i, period)
    return np.where(i < n, i, period - i)


def radius(sigma):
    return int(np.float32(4.0) * np.float32(sigma) + np.float32(0.5))


def weights(sigma):
    r = radius(sigma)
    k = np.arange(-r, r + 1, dtype=np.float64)
    sd = float(np.float32(sigma))
    u = np.exp(-0.5 * k * k / (sd * sd)) if r else np.ones(1)
    return r, u / u.sum()


def blur_real(levels, sigma):
    """float64 [h, w, 3] before the final rounding."""
    p = np.asarray(levels, dtype=np.float64)
    r, w = weights(sigma)
    if r == 0:
        return p
    h, wd = p.shape[:2]
    rows = mirror(np.arange(h)[:, None] + np.arange(-r, r + 1)[None, :], h)          # [h, 2r+1]
    t = np.einsum('ykxc,k->yxc', p[rows], w)
    cols = mirror(np.arange(wd)[:, None] + np.arange(-r, r + 1)[None, :], wd)
    return np.einsum('yxkc,k->yxc', t[:, cols], w)


def blur(levels, sigma):
    return np.clip(np.floor(blur_real(levels, sigma) + 0.5), 0, 255).astype(np.int64)


def invert_add(levels, invert, add):
    v = np.asarray(levels, dtype=np.int64).copy()
    for c in range(3):
        if (invert >> c) & 1:
            v[..., c] = 255 - v[..., c]
        v[..., c] = np.clip(v[..., c] + int(add[c]), 0, 255)
    return v


def _tables():
    i = np.arange(1, 256, dtype=np.float64)
    sdiv, hdiv = np.zeros(256, dtype=np.int64), np.zeros(256, dtype=np.int64)
    sdiv[1:] = np.rint((255 << SHIFT) / i).astype(np.int64)
    hdiv[1:] = np.rint((180 << SHIFT) / (6.0 * i)).astype(np.int64)
    return sdiv, hdiv


SDIV, HDIV = _tables()
SECTOR = np.array([[1, 3, 0], [1, 0, 2], [3, 0, 1], [0, 2, 1], [0, 1, 3], [2, 1, 0]])     # (b, g, r) <- tab


def to_hsv8(levels):
    px = np.asarray(levels, dtype=np.int64)
    r, g, b = px[..., 0], px[..., 1], px[..., 2]
    v = np.maximum(np.maximum(r, g), b)
    diff = v - np.minimum(np.minimum(r, g), b)
    s = (diff * SDIV[v] + (1 << (SHIFT - 1))) >> SHIFT
    h0 = np.where(v == r, g - b, np.where(v == g, b - r + 2 * diff, r - g + 4 * diff))
    h = (h0 * HDIV[diff] + (1 << (SHIFT - 1))) >> SHIFT                                  # numpy's >> on int64 is arithmetic
    h = np.where(h < 0, h + 180, h)
    return h, s, v


def from_hsv8(h, s, v):
    f32 = np.float32
    hf = h.astype(f32) * (f32(6.0) / f32(180.0))
    sf = s.astype(f32) * (f32(1.0) / f32(255.0))
    vf = v.astype(f32) * (f32(1.0) / f32(255.0))
    sector = np.floor(hf)
    f = hf - sector
    wrap = sector >= 6
    sector, f = np.where(wrap, f32(0), sector), np.where(wrap, f32(0), f).astype(f32)
    one = f32(1.0)
    tab = np.stack([vf, vf * (one - sf), vf * (one - sf * f), vf * (one - sf * (one - f))], axis=-1)
    assert tab.dtype == np.float32
    idx = SECTOR[sector.astype(np.int64)]                                                   # [..., 3]
    bgr = np.take_along_axis(tab, idx, axis=-1)
    lev = np.clip(np.rint(bgr * f32(255.0)), 0, 255).astype(np.int64)
    out = lev[..., ::-1]
    grey = (s == 0)[..., None]
    return np.where(grey, v[..., None], out)


def hue_sat(levels, hue, sat):
    h, s, v = to_hsv8(levels)
    h = np.mod(h + int(hue), 180)
    s = np.clip(s + int(sat), 0, 255)
    return from_hsv8(h, s, v)


def hue_sat64(levels, hue, sat):
    """The same hue and saturation adds in a float64 HSV chain (colorsys.rgb_to_hsv / hsv_to_rgb arithmetic, vectorised): h in turns,
    s and v in 0 .. 1; hue is in H units of 2 degrees, sat in 1/255.  Real-valued levels, not rounded."""
    px = np.asarray(levels, dtype=np.float64) / 255.0
    r, g, b = px[..., 0], px[..., 1], px[..., 2]
    maxc, minc = px.max(axis=-1), px.min(axis=-1)
    rng = maxc - minc
    safe = np.where(rng > 0, rng, 1.0)
    s = np.where(maxc > 0, rng / np.where(maxc > 0, maxc, 1.0), 0.0)
    rc, gc, bc = (maxc - r) / safe, (maxc - g) / safe, (maxc - b) / safe
    h = np.where(r == maxc, bc - gc, np.where(g == maxc, 2.0 + rc - bc, 4.0 + gc - rc))
    h = np.where(rng > 0, (h / 6.0) % 1.0, 0.0)
    h = (h + hue / 180.0) % 1.0
    s = np.clip(s + sat / 255.0, 0.0, 1.0)
    v = maxc
    i = np.floor(h * 6.0)
    f = h * 6.0 - i
    p, q, t = v * (1.0 - s), v * (1.0 - s * f), v * (1.0 - s * (1.0 - f))
    i = i.astype(np.int64) % 6
    rr = np.choose(i, [v, q, p, p, t, v])
    gg = np.choose(i, [t, v, v, q, p, p])
    bb = np.choose(i, [p, p, t, v, v, q])
    return np.stack([rr, gg, bb], axis=-1) * 255.0


def levels(crop, order='biah', sigma=0.0, invert=0, add=(0, 0, 0), hue=None, sat=0):
    """The stages named in `order` (b blur, i invert, a add, h hue/saturation) applied to integer levels [h, w, 3] in that order; a
    stage whose parameter is None / 0 flags is still applied when named (hue=None skips h)."""
    v = np.asarray(crop, dtype=np.int64)
    for st in order:
        if st == 'b':
            v = blur(v, sigma)
        elif st == 'i':
            v = invert_add(v, invert, (0, 0, 0))
        elif st == 'a':
            v = invert_add(v, 0, add)
        elif st == 'h' and hue is not None:
            v = hue_sat(v, hue, sat)
    return v
