"""Host self-test of tests/_tol.py (no GPU): the per-element bound the bf16 / fp8 forward kernels are held to must pass a correct
kernel and reject a subtly wrong one, and the references of the exact tests must be representable in the output type.

The kernel is modelled on the CPU as the hot path computes: operands rounded to bf16, float32 products and accumulation (tap by tap),
float32 epilogue (scale, shift, ELU through a float32 exponential), one bf16 store.  The reference is the float64 oracle."""
import numpy as np
import pytest
import torch

import _exact_inputs as XI
import _tol as T
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
