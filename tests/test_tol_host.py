"""Host self-test of tests/_tol.py (no GPU): the per-element bound the bf16 / fp8 forward kernels are held to must pass a correct
kernel and reject a subtly wrong one, and the references of the exact tests must be representable in the output type.

The kernel is modelled on the CPU as the hot path computes: operands rounded to bf16, float32 products and accumulation (tap by tap),
float32 epilogue (scale, shift, ELU through a float32 exponential), one bf16 store.  The reference is the float64 oracle."""
import numpy as np
import pytest
import torch

import _bn_inputs as BI
import _exact_inputs as XI
import _tol as T
import _wgrad_inputs as WI
from oracle import numpy_oracle as no


def _bf16(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(torch.bfloat16).to(torch.float32).numpy()


def _e4m3(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(torch.float8_e4m3fn).to(torch.float32).numpy()


def _elu32(u):
    u = u.astype(np.float32)
    return np.where(u > 0, u, np.exp(np.minimum(u, np.float32(0))) - np.float32(1)).astype(np.float32)


CONV = ('conv', no.conv3d_same)
CONVT = ('convT', no.conv3d_transpose_same)
CASES = [(CONV, 2, 8, 64, 128), (CONV, 5, 2, 256, 512), (CONV, 3, 4, 128, 64), (CONVT, 2, 4, 128, 64)]
IDS = ['%s-%d-%d-%d-%d' % (k[0], B, s, ci, co) for k, B, s, ci, co in CASES]


class Case:
    """Operands, float64 reference and the modelled kernel's float32 sums of one shape (built once per shape, never modified)."""

    def __init__(self, kind, B, side, cin, cout):
        self.kind, self.op = kind
        self.B, self.side, self.cin, self.cout = B, side, cin, cout
        rng = np.random.default_rng(B * 1000 + side)
        self.x = _bf16(rng.standard_normal((B, side, side, side, cin)))
        wshape, fan = ((4, 4, 4, cin, cout), 64 * cin) if self.kind == 'conv' else ((4, 4, 4, cout, cin), 8 * cin)
        self.w = _bf16(rng.standard_normal(wshape) / np.sqrt(fan))
        self.scale = rng.uniform(0.5, 1.5, cout).astype(np.float32)
        self.shift = rng.normal(0, 0.3, cout).astype(np.float32)
        self.pre = self.op(self.x.astype(np.float64), self.w.astype(np.float64), 2) * self.scale + self.shift
        self.ref = no.activation(self.pre, 'elu')
        self.acc = self.sums(self.x, self.w)

    def sums(self, x, w):
        return self.op(x.astype(np.float32), w.astype(np.float32), 2)          # float32 products, float32 accumulation

    def store(self, acc):
        return _bf16(_elu32(acc.astype(np.float32) * self.scale + self.shift))

    def w_ci(self, w):
        """view of w as [4,4,4,cin,cout-ish] with the input channel on axis 3 for either layout"""
        return w if self.kind == 'conv' else w.transpose(0, 1, 2, 4, 3)

    def only_taps(self, sel):
        w = np.zeros_like(self.w)
        w[sel] = self.w[sel]
        return self.sums(self.x, w)


_cache = {}


def _case(i):
    if i not in _cache:
        _cache[i] = Case(*CASES[i])
    return _cache[i]


# ---- the planted errors: each returns the float32 sums of a kernel that is wrong in one way.  Tap (1, 2, 1) reads real data (no
# padding) at every shape above for the conv; the transposed conv's tap (1, 1, 1) feeds the even output voxels.
def _drop_one_product(c):
    w = c.w.copy()
    c.w_ci(w)[1, 2, 1, 5, :] = 0                        # one (tap, cin) product missing everywhere
    return c.sums(c.x, w)


def _swap_two_channels(c):
    w = c.w.copy()
    v = c.w_ci(w)
    v[1, 2, 1, [3, 9], :] = v[1, 2, 1, [9, 3], :]       # two input channels of one tap swapped
    return c.sums(c.x, w)


def _drop_tap_at_corner(c):
    acc = c.acc.copy()
    acc[c.B - 1, 0, 0, 0] -= c.only_taps((1, 1, 1))[c.B - 1, 0, 0, 0]            # one tap at one corner voxel of one sample
    return acc


def _drop_depth_tap_on_plane(c):
    acc = c.acc.copy()
    acc[:, 0] -= c.only_taps((1,))[:, 0]                # depth tap 1 missing on output plane 0
    return acc


def _last_channel_from_sample_0(c):
    acc = c.acc.copy()
    acc[c.B - 1, ..., c.cout - 1] = acc[0, ..., c.cout - 1]
    return acc


def _bf16_split_k(c):
    parts = np.array_split(np.arange(c.cin), 4)         # four K shares, each rounded to bf16 before the sum
    acc = np.zeros_like(c.acc)
    for p in parts:
        w = np.zeros_like(c.w)
        c.w_ci(w)[:, :, :, p, :] = c.w_ci(c.w)[:, :, :, p, :]
        acc += _bf16(c.sums(c.x, w))
    return acc


PLANTED = {'product dropped': _drop_one_product, 'channels swapped': _swap_two_channels, 'tap dropped at a corner': _drop_tap_at_corner,
           'depth tap dropped on a plane': _drop_depth_tap_on_plane, 'last channel from sample 0': _last_channel_from_sample_0,
           'split-K partials rounded to bf16': _bf16_split_k}


def _old_global_bound_passes(got, ref):
    return np.abs(got.astype(np.float64) - ref).max() <= 2e-2 * np.abs(ref).max() + 2e-2


@pytest.mark.parametrize('i', range(len(CASES)), ids=IDS)
def test_correct_model_is_inside_the_bound(i):
    """Worst err / bound of the modelled kernel: 0.95-0.97 at these shapes (an element whose float32 value sits next to a rounding
    boundary takes the whole half ulp).  The old global bound 2e-2 max|ref| + 2e-2 is 0.08-0.15 here, the worst error about 0.008."""
    c = _case(i)
    got = c.store(c.acc)
    r = T.check_one_rounding(got, c.ref, c.pre, 'bf16', IDS[i])
    print('\n[%s] correct model: worst err / bound %.3f, max err %.2e' % (IDS[i], r, np.abs(got - c.ref).max()))
    assert 0.5 < r <= 1.0                               # the bound is not loose either: rounding alone comes close to it


@pytest.mark.parametrize('name', sorted(PLANTED))
@pytest.mark.parametrize('i', range(len(CASES)), ids=IDS)
def test_planted_errors_are_rejected(i, name):
    """Every planted error fails check_one_rounding at every shape.  What the old global bound (2e-2 max|ref| + 2e-2) let through, as
    printed by this test: 'split-K partials rounded to bf16' at all four shapes and 'product dropped' at the three conv shapes (at the
    transposed conv, 8 taps per output instead of 64, one product is a larger share and it caught it).  The whole-tap, whole-channel
    and 'channels swapped' errors it caught at these shapes -- through a few large elements: the per-element bound rejects them on
    hundreds to thousands of elements (the counts are printed)."""
    c = _case(i)
    got = c.store(PLANTED[name](c))
    assert not np.array_equal(got, c.store(c.acc)), 'the planted error changed nothing'
    over = int((np.abs(got - c.ref) > T.U['bf16'] * np.abs(c.ref) + 1.004 * T.f32_term(c.pre)).sum())
    print('\n[%s] %s: %d of %d elements over the per-element bound; old global bound %s' %
          (IDS[i], name, over, got.size, 'PASSED it' if _old_global_bound_passes(got, c.ref) else 'caught it'))
    with pytest.raises(AssertionError):
        T.check_one_rounding(got, c.ref, c.pre, 'bf16', name)


@pytest.mark.parametrize('i', range(len(CASES)), ids=IDS)
def test_two_summation_orders_are_one_ulp_apart(i):
    """check_one_ulp_apart (direct kernel against implicit GEMM): the same operands summed in another float32 order (four K shares,
    not rounded) store the same bf16 value or its neighbour; a kernel that drops one product is further away somewhere."""
    c = _case(i)
    acc = np.zeros_like(c.acc)
    for p in np.array_split(np.arange(c.cin), 4):
        w = np.zeros_like(c.w)
        c.w_ci(w)[:, :, :, p, :] = c.w_ci(c.w)[:, :, :, p, :]
        acc += c.sums(c.x, w)
    assert not np.array_equal(acc, c.acc)
    r = T.check_one_ulp_apart(c.store(c.acc), c.store(acc), c.pre, IDS[i])
    print('\n[%s] two orders: worst |a - b| / bound %.3f' % (IDS[i], r))
    with pytest.raises(AssertionError):
        T.check_one_ulp_apart(c.store(c.acc), c.store(_drop_one_product(c)), c.pre, 'product dropped')


def test_check_exact_and_shapes():
    a = np.array([[0.0, 1.5], [-2.0, 3.0]])
    T.check_exact(torch.tensor(a, dtype=torch.bfloat16), a, 'equal')
    T.check_exact(np.array([-0.0]), np.array([0.0]), 'signed zero')                 # numeric, not bitwise
    with pytest.raises(AssertionError, match='1 of 4 elements differ.*\\(1, 0\\)'):
        T.check_exact(np.array([[0.0, 1.5], [-2.0000001, 3.0]]), a, 'one off')
    with pytest.raises(AssertionError):
        T.check_exact(np.array([[0.0, np.nan], [-2.0, 3.0]]), a, 'unwritten')
    with pytest.raises(AssertionError):
        T.check_exact(a[:1], a, 'shape')
    with pytest.raises(AssertionError):                                             # a NaN is over the bound, not ignored
        T.check_one_rounding(np.array([np.nan, 1.0]), np.array([1.0, 1.0]), np.array([1.0, 1.0]), 'bf16', 'nan')


def test_bf16_boundary_helpers():
    t = np.array([1.0, 1.00390625, 1.0 + 2.0 ** -8 + 1e-6, 0.999, 1.0 - 2.0 ** -10, 3.0])
    assert np.array_equal(T.bf16_ulp(t), [2.0 ** -7, 2.0 ** -7, 2.0 ** -7, 2.0 ** -8, 2.0 ** -8, 2.0 ** -6])
    d = T.bf16_boundary_distance(t)
    assert d[1] == 0.0 and abs(d[2] - 1e-6) < 1e-12                                 # 1 + 2^-8 is the midpoint of 1 and 1 + 2^-7
    assert abs(d[0] - 2.0 ** -9) < 1e-15                                            # 1.0: the nearest boundary is 1 - 2^-9, in the binade below
    assert abs(d[4] - 2.0 ** -10) < 1e-15
    # boundary_extra: only intermediates next to a boundary count, each with its ulp times |w| times scale
    tt = np.array([[1.00390625, 3.0]])
    e = T.boundary_extra(tt, 1e-5, np.array([[0.5, 100.0], [-2.0, 100.0]]), np.array([1.0, 3.0]))
    assert np.allclose(e, [[2.0 ** -7 * 0.5, 2.0 ** -7 * 2.0 * 3.0]])


@pytest.mark.parametrize('fp8', [False, True])
@pytest.mark.parametrize('kind,B,side,cin,cout', [('conv', 3, 4, 64, 64), ('conv', 2, 4, 128, 16), ('convT', 3, 2, 64, 64), ('convT', 2, 4, 64, 1)])
def test_exact_references_are_representable(kind, B, side, cin, cout, fp8):
    """Selector, impulse and zero-input references (float64 oracle, scale +-2^k, no activation / ReLU) are values of the output type,
    every launch; the selector and impulse inputs give every output element at most one non-zero product; the launches together use
    all 64 taps."""
    rnd = _e4m3 if fp8 else _bf16
    rng = np.random.default_rng(cin + cout)
    op = no.conv3d_same if kind == 'conv' else no.conv3d_transpose_same
    sel_w, n_sel = ((XI.selector_conv_weights, XI.selector_conv_launches(cout)) if kind == 'conv'
                    else (XI.selector_convT_weights, XI.selector_convT_launches(cout)))
    wshape = (4, 4, 4, cin, cout) if kind == 'conv' else (4, 4, 4, cout, cin)
    scale = XI.exact_scale(cout)
    x = XI.grid_values(rng, (B, side, side, side, cin), fp8)
    assert np.array_equal(rnd(x), x)
    used = np.zeros((4, 4, 4), bool)
    for l in range(n_sel):
        w = sel_w(cin, cout, l)
        used |= (w != 0).any(axis=(3, 4))
        y = op(x.astype(np.float64), w.astype(np.float64), 2) * scale
        assert np.array_equal(rnd(y).astype(np.float64), y)
        terms = op((x != 0).astype(np.float64), (w != 0).astype(np.float64), 2)
        assert terms.max() == 1                          # one product per output element, none at the padded border of the conv
        assert (np.abs(y[y != 0]) >= 2.0 ** -5).all()    # normal numbers in either output type
    assert used.all()
    w = XI.grid_values(rng, wshape, fp8)
    hit = np.zeros(11, bool)
    for l in range(XI.impulse_launches(B)):
        xi = XI.impulse_input(B, side, cin, l)
        assert (xi.reshape(B, -1) != 0).sum(1).tolist() == [1] * B
        hit[[(l * B + b) % 11 for b in range(B)]] = True
        y = op(xi.astype(np.float64), w.astype(np.float64), 2) * scale
        assert np.array_equal(rnd(y).astype(np.float64), y) and (y != 0).any()
        assert op(xi.astype(np.float64), (w != 0).astype(np.float64), 2).max() == 1
    assert hit.all()
    shift = XI.grid_values(rng, (cout,), fp8)
    y0 = np.maximum(op(np.zeros_like(x, dtype=np.float64), w.astype(np.float64), 2) * scale + shift, 0)
    assert np.array_equal(rnd(y0).astype(np.float64), y0) and np.array_equal(y0[0, 0, 0, 0], np.maximum(shift, 0))


# ------------------------------------------------------------- the exactly summable inputs of the weight-gradient tests (_wgrad_inputs.py)
def _is_f32(a):
    return np.array_equal(a.astype(np.float32).astype(np.float64), a)


def _nonzero_small_ints(a):
    return np.array_equal(a, np.rint(a)) and np.abs(a).min() >= 1 and np.abs(a).max() <= 4


def test_wgrad_case_tables_reach_every_reduce_form():
    """The dispatch as restated in tests/_wgrad_inputs.py: the tables hold a case that writes dw without a reduce pass, one of the plain
    reduce, one of the sliced reduce (on either kernel) and phase plans of several splits, and every kernel form they name.  If the
    split arithmetic of wgrad_plan.h changes under the tables, this says so instead of the GPU tests silently testing less
    (tests/test_wgrad_plan_host.py holds the restatement against the header)."""
    routes = [WI.dense_route(c) for c in WI.DENSE_CASES] + [WI.conv_route(c) for c in WI.CONV_CASES]
    phase = [WI.conv_route(c + ('bf16', 'bf16'), env) for c in WI.PHASE_CASES for env in WI.PHASE_ENVS]
    print('\n' + '\n'.join('%-40s %s' % (c, r) for c, r in zip(WI.DENSE_CASES + WI.CONV_CASES, routes)))
    assert {r[2] for r in routes} == {'none', 'plain', 'sliced'}
    assert {r[0] for r in routes} == {'f32', 'bf16', 'bf16 one channel, one tile', 'bf16 one channel, full tile'}
    assert any(k == 'f32' and red == 'sliced' for k, _, red in routes) and any(k == 'bf16' and red == 'sliced' for k, _, red in routes)
    assert any(k == 'bf16' and s == 1 for k, s, _ in routes) and any(k == 'bf16' and s > 1 for k, s, _ in routes)
    assert [r[0] for r in phase] == ['phase', 'bf16', 'f32'] * len(WI.PHASE_CASES)
    assert all(s > 1 for k, s, _ in phase if k == 'phase') and len({s for k, s, _ in phase if k == 'phase'}) > 1
    assert all(WI.conv_route(c)[0] != 'phase' for c in WI.CONV_CASES)
    # the named branches of the dense table
    assert WI.wgrad_plan(64, 128, 4096)[0] == 128 and WI.wgrad_plan(300, 160, 96)[0] == 64
    assert WI.dense_route((300, 36, 20, 36, 'bf16', 'bf16'))[0] == 'f32' and WI.dense_route((300, 160, 96, 192, 'bf16', 'bf16'))[0] == 'bf16'


@pytest.mark.parametrize('case', WI.DENSE_CASES, ids=str)
def test_wgrad_dense_inputs_are_exactly_summable(case):
    rows, m, n, lda, adt, gdt = case
    a, g = WI.dense_inputs(case)
    assert a.shape == (rows, lda) and _nonzero_small_ints(a[:, :m]) and _nonzero_small_ints(g)
    assert np.array_equal(_bf16(a), a) and np.array_equal(_bf16(g), g)                 # survive either operand type
    assert lda == m or (a[:, m:] == WI.PITCH_FILL).all()                               # the pitch gap is not zero
    assert 16 * rows < 2 ** 24
    ref = WI.dense_ref(case)
    assert _is_f32(ref) and np.array_equal(ref, np.rint(ref)) and np.abs(ref).max() <= 16 * rows


@pytest.mark.parametrize('case', sorted({c[:4] for c in WI.CONV_CASES}) + WI.PHASE_CASES, ids=str)
def test_wgrad_conv_inputs_are_exactly_summable(case):
    """Every product is an integer of magnitude <= 16 and an element sums at most `rows` of them, so the bound 16 rows < 2^24 is the
    proof for every element; the reference itself is looked at as well -- whole where that is cheap, the block of the first 4 x 8
    channels (the same elements, computed from the same operands) at the phase shapes."""
    B, side, cin, cout = case
    src, g = WI.conv_inputs(case)
    assert src.shape == (B, side, side, side, cin) and g.shape == (B,) + (side // 2,) * 3 + (cout,)
    assert _nonzero_small_ints(src) and _nonzero_small_ints(g)
    assert np.array_equal(_bf16(src), src) and np.array_equal(_bf16(g), g)
    rows = WI.conv_rows(case)
    assert 16 * rows <= 16 * 4096 < 2 ** 24
    if case in WI.PHASE_CASES:
        assert rows >= 1024 and cin % 64 == 0 and cout % 128 == 0 and side // 2 in (4, 8, 16)
        ref = WI.wgrad_conv_ref(src[..., :4].astype(np.float64), g[..., :8].astype(np.float64))
    else:
        ref = WI.conv_ref(case)
    assert _is_f32(ref) and np.array_equal(ref, np.rint(ref)) and np.abs(ref).max() <= 16 * rows and (ref != 0).any()


def test_wgrad_conv_ref_against_six_loops():
    """The moved reference against the definition written out: dW[t][ci][co] = sum_{b, o} src[b, 2 o - 1 + t, ci] g[b, o, co]."""
    B, side, cin, cout = 2, 4, 2, 3
    rng = np.random.default_rng(11)
    src, g = rng.standard_normal((B, side, side, side, cin)), rng.standard_normal((B, 2, 2, 2, cout))
    dw = np.zeros((4, 4, 4, cin, cout))
    for b in range(B):
        for od in range(2):
            for oh in range(2):
                for ow in range(2):
                    for td in range(4):
                        for th in range(4):
                            for tw in range(4):
                                i = (2 * od - 1 + td, 2 * oh - 1 + th, 2 * ow - 1 + tw)
                                if min(i) >= 0 and max(i) < side:
                                    dw[td, th, tw] += np.outer(src[(b,) + i], g[b, od, oh, ow])
    np.testing.assert_allclose(WI.wgrad_conv_ref(src, g), dw, rtol=1e-13, atol=1e-13)


def test_exact_check_rejects_one_product_where_the_max_norm_bound_passes():
    """Why the weight gradients are tested on integers.  Against numpy references only: one element of dW counts one row twice (the
    reference is off by ONE product).

    On N(0, 1) operands at rows = 4096, m = 64, n = 128 -- the size of the phase-form cases of tests/test_gpu_ops.py -- the old
    check max|err| <= 2e-5 max|ref| + 1e-5 has a bound of 4.7e-3 (max|ref| 235) and accepts every such error whose product is
    smaller: 2.0% of the 33.5 million (row, element) pairs, the first of them (row 0, element (0, 0)) an error of 6.0e-4; both asserted below.  On the operands
    of tests/_wgrad_inputs.py the smallest possible product is 1: check_exact rejects every one of them, and here even the old bound
    would (it is 0.0154 at the 1000 x 32 x 32 case, max|ref| 771) -- the inputs, not only the checker, are what closes the gap."""
    rows, m, n = 4096, 64, 128
    rng = np.random.default_rng(7)
    a, g = rng.standard_normal((rows, m)).astype(np.float32).astype(np.float64), rng.standard_normal((rows, n)).astype(np.float32).astype(np.float64)
    ref = a.T @ g
    bound = 2e-5 * np.abs(ref).max() + 1e-5
    prod = np.abs(a[:, :, None] * g[:, None, :])
    under = prod <= bound
    r, i, j = (int(v) for v in np.argwhere(under)[0])
    wrong = ref.copy()
    wrong[i, j] += a[r, i] * g[r, j]
    print('\n[N(0,1) %d x %d x %d] max|ref| %.1f, old bound %.2e, one-product errors it accepts: %.2f%%, first: row %d element (%d, %d) error %.2e'
          % (rows, m, n, np.abs(ref).max(), bound, 100 * under.mean(), r, i, j, np.abs(wrong - ref).max()))
    assert 0.015 < under.mean() < 0.025 and 4.5e-3 < bound < 5e-3
    assert 5.5e-4 < np.abs(wrong - ref).max() < 6.5e-4 and np.abs(wrong - ref).max() <= bound     # the old check passes this wrong result ...
    with pytest.raises(AssertionError, match='1 of %d elements differ' % (m * n)):     # ... an exact one does not
        T.check_exact(wrong, ref, 'one row counted twice')
    case = WI.DENSE_CASES[2]
    ai, gi = WI.dense_inputs(case)
    refi = WI.dense_ref(case)
    assert np.abs(ai[:, :, None] * gi[:, None, :]).min() == 1.0                         # every single-product error is at least 1
    wrong = refi.copy()
    wrong[5, 9] += ai[17, 5] * gi[17, 9]
    with pytest.raises(AssertionError, match='1 of 1024 elements differ'):
        T.check_exact(wrong, refi, 'one row counted twice')
    assert 2e-5 * np.abs(refi).max() + 1e-5 < 1.0


# ------------------------------------------------------------------ the inputs of the BatchNorm training-op tests (_bn_inputs.py)
@pytest.mark.parametrize('rows,C', sorted({c[1:3] for c in BI.BN_STATS_CASES}))
def test_bn_inputs_are_what_they_claim(rows, C):
    """Operands survive bf16; sum x, sum x^2 and sum |du xhat| stay where float32 adds them exactly; u is a multiple of 1/4 and a bf16
    value with zeros on every fourth channel; the exact references (statistics' mean, forward codes 0 / 2 / 3, the sums of codes 0 / 2)
    are float32 values."""
    d = BI.inputs(rows, C)
    for a in (d.x, d.dy, d.scale, d.shift, d.mean, d.rstd):
        assert np.array_equal(_bf16(a), a)
    assert np.abs(d.x).max() <= 6 and np.array_equal(d.x, np.rint(d.x)) and np.abs(d.dy).min() >= 1 and np.abs(d.dy).max() <= 4
    assert set(np.abs(d.scale).tolist()) <= {0.25, 0.5, 1.0, 2.0, 4.0} and (np.abs(d.scale[::4]) == 1).all() and (d.rstd == 0.5).all()
    (ref, s, ss) = BI.stats_ref(d)
    assert np.abs(s).max() < 2 ** 24 and ss.max() < 2 ** 24 and 36 * rows < 2 ** 24
    assert _is_f32(ref['mean'][0]) and not ref['mean'][1].any()
    u = BI.pre_act(d)
    assert np.array_equal(u * 4, np.rint(u * 4)) and np.abs(u).max() <= 27 and np.array_equal(_bf16(u).astype(np.float64), u)
    assert (u[0, ::4] == 0).all()
    xh = (d.x.astype(np.float64) - d.mean) * d.rstd
    assert np.abs(xh).max() <= 4 and (np.abs(d.dy) * np.abs(xh)).sum(0).max() < 2 ** 23          # multiples of 1/2: exact below 2^23
    for dt in ('f32', 'bf16'):
        if C % BI.V[dt]:
            continue
        for act in (0, 2, 3):
            y = BI.act_fwd_ref(d, act, dt)[1]
            assert np.array_equal((_bf16(y) if dt == 'bf16' else y.astype(np.float32)).astype(np.float64), y)
        for act in (0, 2):
            du, dbeta, dgamma, bb, bg = BI.act_bwd_ref(d, act, dt)
            assert _is_f32(dbeta) and _is_f32(dgamma) and not bb.any() and not bg.any()
        assert BI.act_bwd_ref(d, 3, dt)[3].min() > 0 and BI.act_bwd_ref(d, 1, dt)[4].min() >= 0
        assert BI.reduce_chain(rows, C, dt) >= 3


def test_bn_case_table_reaches_what_it_names():
    cvs = {(dt, C // BI.V[dt]) for dt, rows, C in BI.BN_SHAPES}
    assert {cv for _, cv in cvs} == set(BI.BN_CV) and {BI.rows_par(cv) for cv in BI.BN_CV} == {1, 2, 3, 8, 10}
    assert any(cv < 64 and 256 % cv for cv in BI.BN_CV)                                      # idle threads below 64 vectors too
    for dt, rows, C in BI.BN_STATS_CASES:                                                    # bn_shape_ok
        cv = C // BI.V[dt]
        assert C % BI.V[dt] == 0 and cv <= 256
    for cv in BI.BN_CV:
        rp = BI.rows_par(cv)
        assert {1, 4 * rp - 1, 4 * rp + 1, 777} <= set(BI.bn_rows(cv)) and (rp == 1 or min(BI.bn_rows(cv)) < rp)     # fewer rows than run in parallel
    rows, C = BI.BN_BIG
    for dt in ('f32', 'bf16'):
        rp = BI.rows_par(C // BI.V[dt])
        assert rows > 1024 * min(max(8 * rp, 16), 256) and rows > 4096 * 2 * rp                # past both block caps
    assert {c[3] for c in BI.BN_ACT_CASES} == {0, 1, 2, 3}


@pytest.mark.parametrize('rows,C', [(r, c) for r in BI.COLSUM_ROWS for c in BI.COLSUM_C])
def test_colsum_inputs_are_exactly_summable(rows, C):
    x = BI.colsum_inputs(rows, C)
    assert np.array_equal(_bf16(x), x) and np.array_equal(x, np.rint(x)) and 4 * rows < 2 ** 24 and _is_f32(x.astype(np.float64).sum(0))
