"""Inputs on which a stride-2 4^3 convolution / transposed convolution has ONE exact answer: every output element receives at most one
non-zero product, so the result does not depend on summation order, MFMA shape or split-K and must equal the float64 oracle exactly
(tests/test_gpu_exact.py; representability of the references is proved on the host in tests/test_tol_host.py).

Values come from a grid that both the operand and the output type hold exactly: sign * 2^e * (1 + m / M) with e in -3..2 and
M = 128 (bf16: 7 stored mantissa bits) or 8 (e4m3: 3).  With scale_c = +-2^k, k in -2..2, a product x * scale stays a normal number
of either type (|x * scale| in [2^-5, 32); e4m3's smallest normal is 2^-6, its largest value 448)."""
import numpy as np

# (d, h, w) positions of the impulses as fractions of the side: the 8 corners, an edge, a face, the interior
_WHERE = [(a, b, c) for a in (0, -1) for b in (0, -1) for c in (0, -1)] + [(0, 0, 'm'), (0, 'm', 'm'), ('m', 'm', 'm')]


def grid_values(rng, shape, fp8=False):
    M = 8 if fp8 else 128
    v = 2.0 ** rng.integers(-3, 3, shape) * (1 + rng.integers(0, M, shape) / M)
    return (v * rng.choice([-1.0, 1.0], shape)).astype(np.float32)


def exact_scale(cout):
    """+-2^k, k cycling over -2..2, sign alternating by channel: neighbouring channels never share a scale."""
    c = np.arange(cout)
    return (2.0 ** ((c % 5) - 2) * np.where(c % 2 == 0, 1.0, -1.0)).astype(np.float32)


def selector_conv_weights(cin, cout, launch=0):
    """w [4,4,4,cin,cout]: output channel co has its one non-zero weight (1) at tap (co + launch * cout) % 64 and an input channel of
    its own.  ceil(64 / cout) launches use all 64 taps."""
    w = np.zeros((64, cin, cout), np.float32)
    co = np.arange(cout)
    w[(co + launch * cout) % 64, (co * 7 + 3) % cin, co] = 1.0
    return w.reshape(4, 4, 4, cin, cout)


def selector_conv_launches(cout):
    return -(-64 // cout)


def selector_convT_weights(cin, cout, launch=0):
    """w [4,4,4,cout,cin]: output o = 2 i + t - 1 per axis, so an output voxel of parity class p (3 bits) is fed by the 8 taps whose
    per-axis parity is the opposite of its own.  Output channel co gets one weight (1) per class -- 8 in all, per axis one of {0, 2}
    and one of {1, 3} -- so every output voxel receives exactly one product (or none, at the border).  ceil(8 / cout) launches use all
    64 taps."""
    w = np.zeros((4, 4, 4, cout, cin), np.float32)
    for co in range(cout):
        for p in range(8):
            j = (co + 3 * p + launch * cout) % 8                       # which of the class's 8 taps
            t = [2 * ((j >> a) & 1) + (1 - ((p >> a) & 1)) for a in range(3)]
            w[t[0], t[1], t[2], co, (co * 5 + 11 * p + 1) % cin] = 1.0
    return w


def selector_convT_launches(cout):
    return -(-8 // cout)


def impulse_launches(B):
    return -(-len(_WHERE) // B)


def impulse_input(B, side, cin, launch=0):
    """x [B,side,side,side,cin]: one voxel and channel per sample equal to 1.  Sample b of launch l takes position (l B + b) of the list
    (wrapping), so impulse_launches(B) launches cover all of it and every launch has its impulse in the last sample too."""
    x = np.zeros((B, side, side, side, cin), np.float32)
    for b in range(B):
        n = launch * B + b
        pos = tuple({0: 0, -1: side - 1, 'm': side // 2}[a] for a in _WHERE[n % len(_WHERE)])
        x[(b,) + pos + ((n * 13 + 5) % cin,)] = 1.0
    return x
