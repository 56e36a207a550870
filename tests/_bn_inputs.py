"""Inputs, float64 references and error bounds of the BatchNorm training-op tests (tests/test_gpu_train_ops.py; host self-test:
tests/test_tol_host.py).  No GPU.

Everything the kernels of csrc/bn.hip read is an integer or a power of two here, so that most of what they compute is exact in
float32 and the rest has an error that can be counted operation by operation:

  x       integers -4..4 plus a per-channel integer offset -2..2 (|x| <= 6: exact in bf16), sum x^2 < 2^24 at every shape
  dy      non-zero integers -4..4
  scale   +-2^k, k = -2..2 (+-1 on every fourth channel), shift an integer -3..3: u = x scale + shift is a multiple of 1/4, |u| <= 27,
          exact in float32 with or without a fused multiply-add, and a bf16 value.  On every fourth channel x is set to -shift / scale
          in row 0 and in one row of eight: u == 0 there
  mean    an integer -2..2, rstd = 1/2: xhat = (x - mean) / 2 is a multiple of 1/2, |xhat| <= 4

Error bounds are in units of U = 2^-24, the largest relative error of one float32 operation rounded to nearest."""
import functools

import numpy as np
import torch

U = 2.0 ** -24
LRELU = float(np.float32(0.3))                  # the slope as bn_act_grad / vv_apply_act hold it: the float32 nearest to 0.3
EPS, MOMENTUM = 1e-3, 0.99
V = {'f32': 4, 'bf16': 8}                       # channels per thread (BnVec<T>::V)

# C / V: 96, 65, 86, 255 are in 64..256 and no power of two (bn_shape_ok admits them: `channels / V >= 64`), rows_par = 256 / (C / V) =
# 2, 3, 2, 1 with 64, 61, 84, 1 threads of the workgroup owning no row; 32 is the power of two next to them (rows_par = 8); 24 is below 64
# and no divisor of 256 (192 bf16 / 96 float32 channels: rows_par = 10, 16 threads without a row), a width bn_shape_ok once refused
BN_CV = (96, 65, 86, 255, 32, 24)
BN_BIG = (300000, 64)                           # rows past 1024 * 128 (f32) / 1024 * 256 (bf16) reduction rows: bn_blocks' cap, and past
#                                                 4096 * 32 / 4096 * 64 sweep rows: bn_sweep_blocks' cap -- every block walks more than two trips


def rows_par(cvn):
    return max(256 // cvn, 1)


def bn_rows(cvn):
    rp = rows_par(cvn)                          # 4 rp - 1 / 4 rp + 1: one row short of / past the first four-rows-in-flight trip
    return sorted({1, 2, 3, 5, 4 * rp - 1, 4 * rp + 1, 777})


BN_SHAPES = [(dt, rows, cv * V[dt]) for dt in ('f32', 'bf16') for cv in BN_CV for rows in bn_rows(cv)]
BN_STATS_CASES = BN_SHAPES + [(dt,) + BN_BIG for dt in ('f32', 'bf16')]
BN_ACT_CASES = [s + (act,) for s in BN_SHAPES for act in (0, 1, 2, 3)] + [(dt,) + BN_BIG + (act,) for dt in ('f32', 'bf16') for act in (0, 1, 2, 3)]
COLSUM_ROWS, COLSUM_C = (1, 7, 8, 9, 31, 32, 33, 1000), (1, 31, 32, 33, 40)


def bf16_round(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(torch.bfloat16).to(torch.float32).numpy()


def reduce_chain(rows, C, dtname):
    """Longest chain of float32 additions one partial sum of bn_reduce_kernel passes through, from bn_blocks and the kernel:
    rows_par = 256 / (C / V) rows run in parallel; a block covers rpb = ceil(rows / nb) rows, nb = min(ceil(rows / per), 1024),
    per = 8 rows_par kept in 16..256.  A thread adds one term per row it owns, ceil(rpb / rows_par) additions (the first one onto 0),
    then rows_par partials are added through shared memory; the block partials are summed in double (2^-53: nothing) and rounded to
    float32 once."""
    rp = rows_par(C // V[dtname])
    per = min(max(8 * rp, 16), 256)
    nb = min(max(-(-rows // per), 1), 1024)
    rpb = -(-rows // nb)
    return -(-rpb // rp) + rp + 1


class Inputs:
    pass


@functools.lru_cache(maxsize=3)
def inputs(rows, C):
    """One read-only set per shape, shared by the statistics, forward and backward tests of both element types."""
    rng = np.random.default_rng(rows * 4099 + C)
    d = Inputs()
    d.rows, d.C = rows, C
    d.shift = rng.integers(-3, 4, C).astype(np.float32)
    d.scale = (2.0 ** rng.integers(-2, 3, C) * rng.choice([-1.0, 1.0], C)).astype(np.float32)
    d.scale[::4] = np.sign(d.scale[::4])
    x = rng.integers(-4, 5, (rows, C), dtype=np.int8) + rng.integers(-2, 3, C, dtype=np.int8)
    zero_rows = rng.random(rows) < 0.125
    zero_rows[0] = True
    x[np.ix_(zero_rows, np.arange(0, C, 4))] = (-d.shift[::4] / d.scale[::4]).astype(np.int8)
    d.x = x.astype(np.float32)
    d.dy = (rng.integers(1, 5, (rows, C), dtype=np.int8) * rng.choice(np.array([-1, 1], np.int8), (rows, C))).astype(np.float32)
    d.mean = rng.integers(-2, 3, C).astype(np.float32)
    d.rstd = np.full(C, 0.5, np.float32)
    d.gamma = (rng.uniform(0.5, 1.5, C) * rng.choice([-1.0, 1.0], C)).astype(np.float32)
    d.beta = rng.normal(0, 0.3, C).astype(np.float32)
    d.mm0, d.mv0 = rng.normal(0, 1, C).astype(np.float32), rng.uniform(0.5, 2, C).astype(np.float32)
    for a in vars(d).values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return d


# ---------------------------------------------------------------------------------------------------------------- statistics
def stats_ref(d):
    """float64 values of bn_stats_finalize_kernel's outputs and the bound of each, {name: (ref, bound)}.

    The per-block sums of x and x^2 are exact (integers below 2^24) and the finalise divides in double, so
      mean   = float32(s / R): no tolerance
      var    one float32 spacing around float32(ss / R - m m): the compiler may contract the expression into a fused multiply-add,
             which moves the double result by 2^-53 m^2 and with it, rarely, the rounding to float32
    and the rest is counted in U = 2^-24 from the kernel's own operations, with one unit of room for second-order terms and for
    what double arithmetic adds:
      rstd   = float32(1 / sqrt(v + eps)), square root and division in double, ONE rounding                              -> 2 U |rstd|
      scale  = gamma * rstd: rstd's rounding and the product's                                                           -> 3 U |scale|
      shift  = beta - ((float)m * gamma) * rstd: m's rounding, a product, rstd's rounding, a product on |m gamma rstd|;
               the subtraction on |shift| <= |beta| + |m gamma rstd|                                                    -> 6 U (|beta| + |m gamma rstd|)
      moving = old * momentum + (float)stat * (1 - momentum), 1 - momentum exact (Sterbenz): a product on the first term, the
               statistic's rounding and a product on the second, the addition on at most their sum                       -> 4 U (|old momentum| + |stat (1 - momentum)|)"""
    x = d.x.astype(np.float64)
    R = float(d.rows)
    s, ss = x.sum(0), (x * x).sum(0)
    m = s / R
    v = np.maximum(ss / R - m * m, 0.0)
    r = 1.0 / np.sqrt(v + float(np.float32(EPS)))
    g, b = d.gamma.astype(np.float64), d.beta.astype(np.float64)
    mom = float(np.float32(MOMENTUM))
    v32 = v.astype(np.float32)
    out = {'mean': (m.astype(np.float32).astype(np.float64), np.zeros_like(m)),
           'var': (v32.astype(np.float64), np.where(v == 0, 0.0, np.spacing(v32).astype(np.float64))),
           'rstd': (r, 2 * U * r),
           'scale': (g * r, 3 * U * np.abs(g * r)),
           'shift': (b - m * g * r, 6 * U * (np.abs(b) + np.abs(m * g * r)))}
    for name, old, stat in (('moving_mean', d.mm0, m), ('moving_var', d.mv0, v)):
        p1, p2 = old.astype(np.float64) * mom, stat * (1.0 - mom)
        out[name] = (p1 + p2, 4 * U * (np.abs(p1) + np.abs(p2)))
    return out, s, ss


# ------------------------------------------------------------------------------------------------------- forward and backward
def pre_act(d):
    return d.x.astype(np.float64) * d.scale + d.shift


def act_fwd_ref(d, act, dtname):
    """-> (u, reference).  Codes 0 (identity), 2 (ReLU) and 3 (LeakyReLU) are exact: u and max(u, 0) are values of either element
    type, and 0.3f u is ONE float32 product (rounded to nearest), stored as it is or rounded once more to bf16.  ELU in float64."""
    u = pre_act(d)
    if act == 0:
        return u, u
    if act == 2:
        return u, np.maximum(u, 0.0)
    if act == 3:
        neg = (np.float32(LRELU) * u.astype(np.float32)).astype(np.float32)
        if dtname == 'bf16':
            neg = bf16_round(neg)
        return u, np.where(u > 0, u, neg.astype(np.float64))
    return u, np.where(u > 0, u, np.expm1(np.minimum(u, 0.0)))


ACT_GRAD_AT_0 = {0: 1.0, 1: 1.0, 2: 0.0, 3: LRELU}     # bn_act_grad at u == 0: exp(0); `u > 0 ? 1 : 0`; `u > 0 ? 1 : 0.3` (Keras: x > 0 ? 1 : alpha)


def act_grad(u, act):
    if act == 1:
        return np.exp(np.minimum(u, 0.0))
    if act == 2:
        return (u > 0).astype(np.float64)
    if act == 3:
        return np.where(u > 0, 1.0, LRELU)
    return np.ones_like(u)


def act_bwd_ref(d, act, dtname):
    """float64 du, dbeta = sum du, dgamma = sum du xhat, and the per-channel bound of the two sums.

    Codes 0 and 2: du is an integer and du xhat a multiple of 1/2, the partial sums stay below 2^23 in magnitude: exact, bound 0.
    Codes 3 and 1: bound = U sum_r |term_r| (k + c + e_r)
      k    = reduce_chain(): every float32 addition a partial passes through errs by at most U times the sum of |terms| so far
      c    the operations of one term.  LeakyReLU: dy * 0.3f is one rounding (dbeta: 1), d * xhat one more (dgamma: 2).  ELU: expf is
           within one float32 ulp = 2 U, then the same two products (dbeta: 3, dgamma: 4); bf16 takes e_r in place of the 2
      e_r  bf16 ELU only, the relative error of __expf(u) = exp2(u log2 e): (|u| + 2) U, one ulp of v_exp_f32 and the rounding of
           u log2 e, which the exponential turns into |u| U"""
    u = pre_act(d)
    du = d.dy.astype(np.float64) * act_grad(u, act)
    xh = (d.x.astype(np.float64) - d.mean) * d.rstd
    tg = du * xh
    dbeta, dgamma = du.sum(0), tg.sum(0)
    if act in (0, 2):
        zero = np.zeros(d.C)
        return du, dbeta, dgamma, zero, zero
    k = reduce_chain(d.rows, d.C, dtname)
    if act == 3:
        cb, cg, e = 1, 2, 0.0
    elif dtname == 'f32':
        cb, cg, e = 3, 4, 0.0
    else:
        cb, cg, e = 1, 2, np.abs(np.minimum(u, 0.0)) + 2.0
    return du, dbeta, dgamma, U * (np.abs(du) * (k + cb + e)).sum(0), U * (np.abs(tg) * (k + cg + e)).sum(0)


def dx_ref(d, du, dgamma_dev, dbeta_dev):
    """float64 dx from the DEVICE's dgamma and dbeta (only the sweep is measured), and its three terms:
    dx = scale (du - k1 - (x - mean) k2), k1 = dbeta / R, k2 = dgamma rstd / R  ->  (dx, [scale du, scale k1, scale (x - mean) k2])

    float32 bound, 3 float32 ulps (6 U) of |scale| (|du| + |k1| + |x - mean| |k2|), from bn_act_bwd_kernel's operations: invR = 1 / R is
    rounded on the host (1 U); k1 = dbeta invR and k2 = (dgamma invR) rstd carry 2 U each (rstd = 1/2 is exact); du = dy act' carries
    up to 3 U (ELU: expf one ulp = 2 U, one product); (x - mean) is exact and its product with k2 adds 1 U; the two subtractions add
    1 U each of at most the sum of the three magnitudes; scale is a power of two.  That is 5 U on |du|, 4 U on each of the others."""
    k1 = np.asarray(dbeta_dev, np.float64) / d.rows
    k2 = np.asarray(dgamma_dev, np.float64) * d.rstd / d.rows
    xm = d.x.astype(np.float64) - d.mean
    terms = [d.scale * du, d.scale * k1 * np.ones_like(du), d.scale * xm * k2]
    return terms[0] - terms[1] - terms[2], terms


# --------------------------------------------------------------------------------------------------------------------- colsum
@functools.lru_cache(maxsize=None)
def colsum_inputs(rows, C):
    x = np.random.default_rng(rows * 64 + C).integers(-4, 5, (rows, C)).astype(np.float32)
    x.setflags(write=False)
    return x
