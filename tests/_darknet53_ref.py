"""The float64 definition of the three operations Darknet53 / Darknet53Tiny add to the 2D engine (include/voxvae.h `vv_conv2d_ex_fwd`,
`vv_maxpool2d_s1_same_fwd`), written out tap by tap in numpy from their definitions -- no library convolution, no library pool:

  strided conv   y[b,ro,co,n] = sum_{tr,tc,ci} x[b, s ro + tr - p, s co + tc - p, ci] w[tr,tc,ci,n],  p = k // 2; at s = 2 (k = 3) the output
                 grid is floor(R/2) x floor(C/2), index -1 is zero and the last row / column of an odd size is never read
  residual       y = act(scale * conv + shift) + residual, the add in float64 here (float32 behind the activation in the kernel)
  stride-1 pool  y[r,c] = max x[r .. min(r+1, R-1), c .. min(c+1, C-1)]

As in tests/_conv2d_ref.py the operands (and the residual) are rounded to the kernel's operand type BEFORE the reference is computed.
tests/test_darknet53_host.py checks all three against torch's own ops.
"""
import numpy as np

from _conv2d_ref import act_ref, round_to


def out_grid(R, C, stride):
    return (R // 2, C // 2) if stride == 2 else (R, C)


def conv_ex_direct(x, w, stride=1):
    """x [B,R,C,Cin], w Keras [k,k,Cin,Cout], float64 as given -> [B,Ro,Co,Cout]."""
    x, w = np.asarray(x, dtype=np.float64), np.asarray(w, dtype=np.float64)
    B, R, C, _ = x.shape
    k = w.shape[0]
    p = k // 2
    Ro, Co = out_grid(R, C, stride)
    y = np.zeros((B, Ro, Co, w.shape[3]))
    for tr in range(k):
        for tc in range(k):
            for ro in range(Ro):
                rr = stride * ro + tr - p
                if rr < 0 or rr >= R:
                    continue
                for co in range(Co):
                    cc = stride * co + tc - p
                    if 0 <= cc < C:
                        y[:, ro, co] += x[:, rr, cc] @ w[tr, tc]
    return y


def conv_ex_ref(x, w, scale=None, shift=None, residual=None, act=None, alpha=0.0, stride=1, op_dtype='f32'):
    """-> (y, pre): y = act(scale * conv + shift) + residual; pre = the pre-activation and the residual TOGETHER (stacked on a new
    leading axis), so that max|pre| -- all tests/_tol.check_one_rounding takes from it -- covers both."""
    xr, wr = round_to(x, op_dtype), round_to(w, op_dtype)
    y = conv_ex_direct(xr, wr, stride)
    if scale is not None:
        y = y * np.asarray(scale, dtype=np.float64)
    if shift is not None:
        y = y + np.asarray(shift, dtype=np.float64)
    out = act_ref(y, act, alpha)
    if residual is None:
        return out, y
    res = round_to(residual, op_dtype)
    return out + res, np.stack([y, res])


def pool1_ref(x):
    """MaxPool2D(2, 1, 'same') of [B,R,C,N]."""
    x = np.asarray(x, dtype=np.float64)
    B, R, C, N = x.shape
    y = np.empty_like(x)
    for r in range(R):
        for c in range(C):
            r1, c1 = min(r + 1, R - 1), min(c + 1, C - 1)
            y[:, r, c] = np.maximum(np.maximum(x[:, r, c], x[:, r, c1]), np.maximum(x[:, r1, c], x[:, r1, c1]))
    return y


def shifted_s2(x, tr, tc, ci):
    """What a k3 selector kernel at tap (tr, tc), input channel ci puts into its output channel at stride 2."""
    x = np.asarray(x, dtype=np.float64)
    B, R, C, _ = x.shape
    y = np.zeros((B, R // 2, C // 2))
    for ro in range(R // 2):
        for co in range(C // 2):
            rr, cc = 2 * ro + tr - 1, 2 * co + tc - 1
            if rr >= 0 and cc >= 0:
                y[:, ro, co] = x[:, rr, cc, ci]
    return y
