"""Shared checkers of the bf16 / fp8 forward kernels against the float64 oracle (host self-test: tests/test_tol_host.py).

The operands of those tests are rounded to the kernel's operand type before the reference is computed, so what is left is float32
accumulation, a float32 epilogue and ONE rounding to the output type.  Two checkers follow from that:

  check_exact          inputs that give every output element at most one non-zero product: no summation, no order, the stored value IS
                       the float64 value.  No tolerance, no element left out.
  check_one_rounding   random inputs, per element:  |got - ref| <= u |ref| + 1.004 f + extra
                         u |ref|   the one rounding to the output type, relative to the element itself (half an ulp at the bottom of a
                                   binade: 2^-8 for bf16's 8 significant bits, 2^-4 for e4m3's 4, 2^-24 for a float32 output)
                         f         = 2e-5 max|pre_act| + 1e-5, what the float32-accumulating MFMA kernels are held to where their output
                                   is float32 (the f32 layer tests, test_wgrad_kernels on bf16 operands); pre_act = conv * scale + shift.
                                   The activations are 1-Lipschitz, so an error before them carries to the output unchanged; the term
                                   also covers the hardware exponential of the ELU
                         1.004     rounding a value that is itself off by f moves the rounding error by u f at most (1 + 2^-8 < 1.004)
                         extra     chained kernels only, see boundary_extra
"""
import numpy as np

U = {'bf16': 2.0 ** -8, 'e4m3': 2.0 ** -4, 'f32': 2.0 ** -24}
SUBNORMAL_HALF = {'bf16': 0.0, 'e4m3': 2.0 ** -10, 'f32': 0.0}      # e4m3: subnormal spacing 2^-9 (what check_fp8_out allows as well)


def _f64(a):
    if hasattr(a, 'detach'):                                          # torch tensor of any float type, any device
        a = a.detach().float().cpu().numpy()
    return np.asarray(a).astype(np.float64)


def f32_term(pre_act):
    return 2e-5 * float(np.abs(pre_act).max()) + 1e-5


def check_exact(got, ref, what):
    """got == ref for every element, numerically (-0 == +0, a NaN equals nothing)."""
    got, ref = _f64(got), np.asarray(ref, dtype=np.float64)
    assert got.shape == ref.shape, '%s: shape %s, expected %s' % (what, got.shape, ref.shape)
    bad = ~(got == ref)
    if bad.any():
        idx = np.argwhere(bad)[:5]
        first = ', '.join('%s: got %r expected %r' % (tuple(int(v) for v in i), got[tuple(i)], ref[tuple(i)]) for i in idx)
        raise AssertionError('%s: %d of %d elements differ; first: %s' % (what, int(bad.sum()), bad.size, first))


def check_one_rounding(got, ref, pre_act, out_dtype, what, extra=None):
    """-> worst err / bound over the elements (<= 1); raises if any element is over its bound."""
    got, ref = _f64(got), np.asarray(ref, dtype=np.float64)
    assert got.shape == ref.shape, '%s: shape %s, expected %s' % (what, got.shape, ref.shape)
    f = f32_term(np.asarray(pre_act, dtype=np.float64))
    bound = U[out_dtype] * np.abs(ref) + 1.004 * f + SUBNORMAL_HALF[out_dtype]
    if extra is not None:
        bound = bound + np.asarray(extra, dtype=np.float64)
    err = np.abs(got - ref)
    bad = ~(err <= bound)                                             # a NaN in got is over the bound
    if bad.any():
        r = np.where(bad, np.nan_to_num(err / bound, nan=np.inf), 0.0)
        i = np.unravel_index(int(np.argmax(r)), r.shape)
        raise AssertionError('%s -> %s: %d of %d elements over the one-rounding bound; worst at %s: got %r ref %r err %.3e bound %.3e '
                             '(f %.3e)' % (what, out_dtype, int(bad.sum()), bad.size, tuple(int(v) for v in i), got[i], ref[i], err[i], bound[i], f))
    return float((err / bound).max())


def f32_share(got, ref, pre_act, out_dtype):
    """How much of the float32 term the worst element needs once its full rounding allowance is spent: max (err - u |ref|) / f, 0 if
    rounding alone explains every element.  A figure to print, not a check."""
    got, ref = _f64(got), np.asarray(ref, dtype=np.float64)
    rest = np.abs(got - ref) - U[out_dtype] * np.abs(ref) - SUBNORMAL_HALF[out_dtype]
    return max(float(rest.max()) / f32_term(np.asarray(pre_act, dtype=np.float64)), 0.0)


def check_one_ulp_apart(a, b, pre_act, what):
    """Two bf16 results of the same operands in different float32 summation orders: per element they are the same bf16 value or
    neighbours, |a - b| <= 2^-7 |a| + 2 f (each is within f of the exact value before its rounding)."""
    a, b = _f64(a), _f64(b)
    f = f32_term(np.asarray(pre_act, dtype=np.float64))
    err, bound = np.abs(a - b), 2.0 ** -7 * np.abs(a) + 2 * f
    bad = ~(err <= bound)
    assert not bad.any(), '%s: %d of %d elements more than one bf16 ulp apart, worst %.3e' % (what, int(bad.sum()), bad.size, float(np.nanmax(err)))
    return float((err / bound).max())


def check_fp8_out(got_f8, ref, what, pre_act=None):
    """An e4m3 output against the float64 result: 3 mantissa bits (half an ulp = 2^-4 relative), subnormal spacing 2^-9.  The bound
    this check always had, and -- given the pre-activation -- the one-rounding bound on top of it (-> its worst err / bound)."""
    got, ref = _f64(got_f8), np.asarray(ref, dtype=np.float64)
    bad = ~(np.abs(got - ref) <= 0.0635 * np.abs(ref) + 2.5e-3)
    assert not bad.any(), '%s: %d of %d beyond fp8 rounding, worst %.3e' % (what, int(bad.sum()), bad.size, float(np.nanmax(np.abs(got - ref))))
    return None if pre_act is None else check_one_rounding(got, ref, pre_act, 'e4m3', what)


def bf16_ulp(t):
    """Spacing of the bf16 values around t (float64 array); the smallest normal binade below 2^-126."""
    e = np.floor(np.log2(np.maximum(np.abs(t), 2.0 ** -126)))
    return 2.0 ** (e - 7)


def bf16_boundary_distance(t):
    """Distance of t to the nearest point where bf16 rounding changes its result (a midpoint between two neighbouring bf16 values)."""
    ulp = bf16_ulp(t)
    q = np.abs(t) / ulp                                               # in units of the spacing: boundaries at n + 1/2
    below = (q - (128.0 - 0.25)) * ulp                                # the last boundary of the binade below (half of ITS spacing under 2^e)
    return np.minimum(np.abs(q - np.floor(q) - 0.5) * ulp, below)


def boundary_extra(t, f_t, w, scale):
    """Allowance of a chained kernel whose bf16 intermediate t [M, J] is not an output.  Where the float64 intermediate lies within
    f_t (its own float32 term) of a rounding boundary, the kernel may hold the neighbouring bf16 value; through the next layer
    (w [N, J], per-output scale [N]) that moves output (m, i) by at most ulp(t_mj) |w_ij| scale_i.  Summed over those j only:
    -> [M, N].  Computed from the reference, nothing measured."""
    t = np.asarray(t, dtype=np.float64)
    near = bf16_boundary_distance(t) <= f_t
    return (np.where(near, bf16_ulp(t), 0.0) @ np.abs(np.asarray(w, dtype=np.float64)).T) * np.abs(np.asarray(scale, dtype=np.float64))
