"""Float64 references shared by the training tests (tests/test_gpu_train_ops.py, tests/test_gpu_train.py): Keras Adam on the
float32-rounded constants the kernels receive, the units its error is measured in, and the per-step batches of the multi-step
tests.  numpy only: no GPU, no library."""
import numpy as np

U24 = 2.0 ** -24                                  # half a float32 ulp, relative
TINY = float(np.finfo(np.float32).tiny)           # smallest normal float32: absolute slack where a product underflows

ADAM_B1, ADAM_B2, ADAM_EPS = 0.9, 0.999, 1e-7
ADAM_CHUNK = 16384
ADAM_UNITS = 8.0     # twice the worst of a float32 emulation of the kernel's expression order (1.95 / 2.82 / 3.79 units): the compiler
                     # may contract multiply-adds, which removes roundings but changes which ones remain


def lr_t_of(t, lr=1e-3):
    return lr * (1.0 - ADAM_B2 ** t) ** 0.5 / (1.0 - ADAM_B1 ** t)


def adam_ref(p, g, m, v, lr_t, b1=ADAM_B1, b2=ADAM_B2, eps=ADAM_EPS):
    """Keras Adam in float64 on the float32-rounded constants the kernel receives: beta and 1 - beta formed in float32 (1 - 0.999f is
    1.3e-5 away from 0.001), epsilon, lr_t.  Returns (p, m, v, step) in float64."""
    b1f, b2f = np.float32(b1), np.float32(b2)
    c1, c2 = float(np.float32(1) - b1f), float(np.float32(1) - b2f)
    b1f, b2f, e, lr = float(b1f), float(b2f), float(np.float32(eps)), float(np.float32(lr_t))
    p, g, m, v = (np.asarray(a, np.float64) for a in (p, g, m, v))
    m2 = b1f * m + c1 * g
    v2 = b2f * v + c2 * g * g
    step = lr * m2 / (np.sqrt(v2) + e)
    return p - step, m2, v2, step


def adam_units(got_p, got_m, got_v, p, g, m, v, lr_t, uncancelled=False):
    """Worst error of each output in the units of the bound: 2^-24 (|b1 m| + |(1-b1) g|) for m, 2^-24 v for v,
    2^-24 (|p| + |step|) for the parameter, each plus one smallest-normal float32.

    uncancelled=True measures the parameter in 2^-24 (|p| + lr_t (|b1 m| + |(1-b1) g|) / (sqrt(v) + eps)): the step's size BEFORE b1 m and
    (1-b1) g cancel.  The two units are the same number wherever the two terms share a sign.  Where they cancel, m's own rounding error (a
    few of ITS units, which do not shrink with the sum) goes through lr_t / (sqrt(v) + eps) into the weight and is no longer small against
    |p| + |step| once the weight is near 0 -- in any float32 evaluation of the rule, not only the kernel's
    (tests/test_oracle.py::test_adam_float32_rounding_and_the_units_it_is_measured_in: 78 - 166 plain units on 2 M weights ~ N(0, 0.05), 3.84 of these)."""
    rp, rm, rv, step = adam_ref(p, g, m, v, lr_t)
    b1f = float(np.float32(ADAM_B1))
    c1 = float(np.float32(1) - np.float32(ADAM_B1))
    spread = np.abs(b1f * m.astype(np.float64)) + np.abs(c1 * g.astype(np.float64))
    um = np.abs(got_m.astype(np.float64) - rm) / (U24 * spread + TINY)
    uv = np.abs(got_v.astype(np.float64) - rv) / (U24 * rv + TINY)
    size = float(np.float32(lr_t)) * spread / (np.sqrt(rv) + float(np.float32(ADAM_EPS))) if uncancelled else np.abs(step)
    up = np.abs(got_p.astype(np.float64) - rp) / (U24 * (np.abs(p.astype(np.float64)) + size) + TINY)
    return float(um.max()), float(uv.max()), float(up.max())


def adam_float32_emulation(p, g, m, v, lr_t, contract):
    """The rule in float32 in the kernels' expression order (train.hip adam_kernel), on the CPU.  contract=True: the two sums as fused
    multiply-adds (products of float32 are exact in float64; the one extra float64 rounding is 2^-29 of a float32 ulp)."""
    f, d = np.float32, np.float64
    b1, b2, eps, lr = f(ADAM_B1), f(ADAM_B2), f(ADAM_EPS), f(lr_t)
    c1, c2 = f(1) - b1, f(1) - b2
    if contract:
        mi = (d(b1) * m.astype(d) + d(1) * (c1 * g).astype(d)).astype(f)
        vi = (d(b2) * v.astype(d) + (c2 * g).astype(f).astype(d) * g.astype(d)).astype(f)
    else:
        mi = b1 * m + c1 * g
        vi = b2 * v + (c2 * g) * g
    return (p - lr * mi / (np.sqrt(vi) + eps)).astype(f), mi.astype(f), vi.astype(f)


# ------------------------------------------------------------------------------------------ batches of the multi-step tests
# (D, latent, variational, batch, latent dropout): the three shapes of the one-step oracle test and one run whose dropout mask and
# rate change every step
TRAJECTORY_CONFIGS = [(32, 64, True, 4, False), (16, 64, True, 6, False), (32, 64, False, 3, False), (16, 64, True, 5, True)]
TRAJECTORY_STEPS = 4


def step_batch(D, Lz, B, k, drop=False):
    """Step k's batch, epsilon and (with latent dropout) mask / rate: different at every step, so that anything kept from the step before
    is wrong for this one."""
    from voxvae import synthetic as syn
    x = syn.make_voxels(B, D, seed=100 + k)
    eps = syn.make_eps(B, Lz, seed=200 + k)
    if not drop:
        return x, eps, None, None
    rate = 0.15 + 0.1 * k
    mask = (np.random.default_rng(300 + k).random((B, Lz)) >= rate).astype(np.float32)
    return x, eps, mask, rate
