"""The float64 definition the 2D convolution tests hold csrc/conv2d.hip to (tests/test_gpu_conv2d.py, test_gpu_image_encoder.py,
test_conv2d_host.py): Conv2D k in {1, 3} stride 1 'same' without bias -> y * scale + shift -> activation, MaxPool2D(2, 2, 'same'), the
BatchNormalization fold.  Operands are rounded to the kernel's operand type BEFORE the reference is computed (the rule of tests/_tol.py:
the bound is about what the kernel does with the operands it was given); everything after that is float64.
"""
import numpy as np
import torch
import torch.nn.functional as F


def round_to(a, dtype):
    """float64 array of `a` rounded to 'f32' or 'bf16' (round to nearest even, as the device converts)."""
    t = torch.as_tensor(np.asarray(a, dtype=np.float64)).float()
    if dtype == 'bf16':
        t = t.bfloat16()
    return t.double().numpy()


def act_ref(v, act, alpha=0.0):
    if act == 'elu':
        return np.where(v > 0, v, np.expm1(np.minimum(v, 0)))
    if act == 'relu':
        return np.maximum(v, 0)
    if act == 'lrelu':
        return np.where(v > 0, v, alpha * v)
    return v


def conv2d_ref(x, w, scale=None, shift=None, act=None, alpha=0.0, op_dtype='f32'):
    """x [B,R,C,Cin], w Keras [k,k,Cin,Cout], scale / shift [Cout] (float32 inputs of the kernel: taken as they are) ->
    (y, pre_activation), both float64 [B,R,C,Cout]."""
    xr, wr = round_to(x, op_dtype), round_to(w, op_dtype)
    k = wr.shape[0]
    y = F.conv2d(torch.from_numpy(xr).permute(0, 3, 1, 2), torch.from_numpy(wr).permute(3, 2, 0, 1), padding=k // 2).permute(0, 2, 3, 1).numpy()
    if scale is not None:
        y = y * np.asarray(scale, dtype=np.float64)
    if shift is not None:
        y = y + np.asarray(shift, dtype=np.float64)
    return act_ref(y, act, alpha), y


def conv2d_direct(x, w):
    """The same sum written out tap by tap in numpy (no library convolution): the statement conv2d_ref is checked against."""
    x, w = np.asarray(x, dtype=np.float64), np.asarray(w, dtype=np.float64)
    B, R, C, _ = x.shape
    k, p = w.shape[0], w.shape[0] // 2
    xp = np.zeros((B, R + 2 * p, C + 2 * p, x.shape[3]))
    xp[:, p:p + R, p:p + C] = x
    y = np.zeros((B, R, C, w.shape[3]))
    for tr in range(k):
        for tc in range(k):
            y += xp[:, tr:tr + R, tc:tc + C] @ w[tr, tc]
    return y


def pool_ref(x):
    """MaxPool2D(2, 2, 'same') of [B,R,C,N]: ceil mode, padding (-inf) only at the end."""
    x = np.asarray(x, dtype=np.float64)
    B, R, C, N = x.shape
    xp = np.full((B, R + R % 2, C + C % 2, N), -np.inf)
    xp[:, :R, :C] = x
    return np.maximum(np.maximum(xp[:, 0::2, 0::2], xp[:, 0::2, 1::2]), np.maximum(xp[:, 1::2, 0::2], xp[:, 1::2, 1::2]))


def fold_ref(gamma, beta, mean, var, eps=1e-3):
    """BatchNormalization(training=False) as y * scale + shift, in float64."""
    g, b, m, v = (np.asarray(t, dtype=np.float64) for t in (gamma, beta, mean, var))
    scale = g / np.sqrt(v + eps)
    return scale, b - m * scale


def selector_kernel(k, cin, cout, tr, tc, ci, co):
    w = np.zeros((k, k, cin, cout), dtype=np.float32)
    w[tr, tc, ci, co] = 1.0
    return w


def shifted(x, k, tr, tc, ci):
    """What a selector kernel at tap (tr, tc) and input channel ci puts into its output channel: x[..., ci] shifted, zeros from the padding."""
    x = np.asarray(x, dtype=np.float64)
    B, R, C, _ = x.shape
    p = k // 2
    y = np.zeros((B, R, C))
    for r in range(R):
        for c in range(C):
            rr, cc = r + tr - p, c + tc - p
            if 0 <= rr < R and 0 <= cc < C:
                y[:, r, c] = x[:, rr, cc, ci]
    return y
