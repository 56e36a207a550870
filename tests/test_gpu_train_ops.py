"""GPU parity tests of the training step's own entry points, per kernel, through the C ABI (voxvae.lib): the optimizer, the
backward of the losses and of the latent step, the two "layer as a dense panel" packings with their adjoints, and the small
helpers around them.  Every reference is a float64 restatement written here or taken from oracle/ -- never another kernel of
the library, except where the equality of two forms is the property under test."""
import ctypes

import numpy as np
import pytest
import torch

from oracle import numpy_oracle as no

import _bn_inputs as BI
import _tol as T
from _train_ref import ADAM_B1, ADAM_B2, ADAM_CHUNK, ADAM_EPS, ADAM_UNITS, adam_units, lr_t_of

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
TINY = float(np.finfo(np.float32).tiny)           # smallest normal float32: absolute slack where a result underflows
SENTINEL = -7.25                                  # canary value behind every buffer
PAD = 64
GRID_CAP = 16384 * 256                            # elements one pass of the capped 1-D grid covers (train.hip grid_1d)


@pytest.fixture(scope='module')
def L():
    from voxvae import lib
    lib.load()
    assert torch.cuda.is_available()
    return lib


def _st():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(DEV).contiguous()


def _guarded(a, lead=0, dtype=torch.float32):
    """Device copy of `a` with `lead` sentinel elements in front (moves the payload off 16-byte alignment) and PAD behind.
    Returns (whole buffer, payload view).  The sentinel is a bf16 value as well."""
    a = np.ascontiguousarray(a, dtype=np.float32).ravel()
    buf = torch.full((lead + a.size + PAD,), SENTINEL, dtype=dtype, device=DEV)
    view = buf[lead:lead + a.size]
    view.copy_(torch.from_numpy(a))
    return buf, view


def _guarded_empty(n, lead=0, dtype=torch.float32):
    buf = torch.full((lead + n + PAD,), SENTINEL, dtype=dtype, device=DEV)
    return buf, buf[lead:lead + n]


def _guarded_nan(n, dtype=torch.float32):
    """An output: the payload pre-filled with NaN, so that an element the kernel leaves out fails every comparison."""
    buf, view = _guarded_empty(n, 0, dtype)
    view.fill_(float('nan'))
    return buf, view


def _canaries_intact(buf, lead, n):
    return bool((buf[:lead] == SENTINEL).all().item() and (buf[lead + n:] == SENTINEL).all().item())


# ------------------------------------------------------------------------------------------------------------ Adam
def adam_inputs(n, seed, layer=False):
    """A consistent optimizer state: per-element gradient scale 10^U(-8, 2), m and v the float64 moving averages of three earlier
    gradients of that scale (so they are non-zero and related as a real run relates them: |m| <= 7.3 sqrt(v), |g| <= 31.7 sqrt(v new)),
    the current gradient of the same scale.  One element in eight is dead: g = m = v = 0 exactly, half of those with a weight of 0.
    Weights are +-10^U(-2, 0).  They stay away from 0 because the parameter's unit 2^-24 (|p| + |step|) knows nothing of a cancellation
    in b1 m + (1-b1) g: there m's error (its own unit) times lr_t / sqrt(v) reaches 2^-24 * 1e-3 * (0.9 * 7.3 + 0.1 * 31.7) * 2, which is
    2 units at |p| = 0.01 and unbounded in them as p -> 0 (tests/test_oracle.py::test_adam_float32_rounding_and_the_units_it_is_measured_in).
    layer=True: weights ~ N(0, 0.05) as a real layer has them, some arbitrarily close to 0 -- to be measured with adam_units(uncancelled=True)."""
    rng = np.random.default_rng(seed)
    scale = 10.0 ** rng.uniform(-8.0, 2.0, n)
    m, v = np.zeros(n), np.zeros(n)
    for _ in range(3):
        h = scale * rng.standard_normal(n)
        m = 0.9 * m + 0.1 * h
        v = 0.999 * v + 0.001 * h * h
    g = scale * rng.standard_normal(n)
    p = 0.05 * rng.standard_normal(n) if layer else 10.0 ** rng.uniform(-2.0, 0.0, n) * rng.choice([-1.0, 1.0], n)
    dead = rng.random(n) < 0.125
    if n > 2:
        dead[n - 1] = True
    g[dead], m[dead], v[dead] = 0.0, 0.0, 0.0
    p[dead & (rng.random(n) < 0.5)] = 0.0
    return tuple(a.astype(np.float32) for a in (p, g, m, v)) + (dead,)


ADAM_SIZES = [1, 255, 256, 257, 16383, 16384, 16385, 3 * 16384 + 5, GRID_CAP + 77]


@pytest.mark.parametrize('layer', [False, True])
@pytest.mark.parametrize('t', [1, 2, 7, 1000])
@pytest.mark.parametrize('n', ADAM_SIZES)
def test_adam_step_against_float64(L, n, t, layer):
    """vv_adam_step on non-zero moments at several bias corrections, every size around the 256-thread workgroup and the 16384-element
    chunk, and one past the cap of the launch grid (the stride loop's second pass).  layer=False: weights away from 0, the parameter in
    units of 2^-24 (|p| + |step|); layer=True: weights of a real layer, the parameter against the step's size before m's two terms cancel."""
    p, g, m, v, dead = adam_inputs(n, seed=n % 9973 + t, layer=layer)
    lr_t = lr_t_of(t)
    bufs = [_guarded(a) for a in (p, g, m, v)]
    (pb, pd), (gb, gd), (mb, md), (vb, vd) = bufs
    L.call('vv_adam_step', L.ptr(pd), L.ptr(gd), L.ptr(md), L.ptr(vd), n, lr_t, ADAM_B1, ADAM_B2, ADAM_EPS, _st())
    torch.cuda.synchronize()
    gp, gg, gm, gv = (d.cpu().numpy() for d in (pd, gd, md, vd))
    for buf, _ in bufs:
        assert _canaries_intact(buf, 0, n)
    assert np.array_equal(gg, g)
    assert np.isfinite(gp).all() and np.isfinite(gm).all() and np.isfinite(gv).all()
    assert np.array_equal(gp[dead], p[dead]) and not gm[dead].any() and not gv[dead].any()     # 0 / (0 + eps): no move, no NaN
    um, uv, up = adam_units(gp, gm, gv, p, g, m, v, lr_t, uncancelled=layer)
    print('\n[adam n=%d t=%d layer=%d] worst error in bound units: m %.2f  v %.2f  param %.2f  (bound %.0f)' % (n, t, layer, um, uv, up, ADAM_UNITS))
    assert um <= ADAM_UNITS and uv <= ADAM_UNITS and up <= ADAM_UNITS, (um, uv, up)


def _chunk_table(ptrs_and_sizes):
    """The table of Trainer._apply: every variable cut into records of at most ADAM_CHUNK elements, pointers already offset."""
    recs = []
    for pp, gp, mp, vp, n in ptrs_and_sizes:
        for off in range(0, n, ADAM_CHUNK):
            recs.append((pp + 4 * off, gp + 4 * off, mp + 4 * off, vp + 4 * off, min(ADAM_CHUNK, n - off)))
    return torch.from_numpy(np.asarray(recs, dtype=np.int64)).to(DEV)


ADAM_MULTI_VARS = [1, 255, 64, ADAM_CHUNK, ADAM_CHUNK + 1, 3 * ADAM_CHUNK + 5, 257, 2 * ADAM_CHUNK - 1, 7]


@pytest.mark.parametrize('t', [1, 2, 7, 1000])
def test_adam_step_multi_against_float64_and_single_form(L, t):
    """vv_adam_step_multi over a table of nine variables of unequal sizes (a one-element variable, a last chunk of one element, chunk
    pointers that are 4-byte but not 16-byte aligned) against float64, and bit for bit against vv_adam_step on the same inputs."""
    lr_t = lr_t_of(t)
    data = [adam_inputs(n, seed=31 * k + t) for k, n in enumerate(ADAM_MULTI_VARS)]
    leads = [1 + (k % 3) for k in range(len(data))]                                            # 4, 8 or 12 bytes past a 16-byte boundary
    multi = [[_guarded(a, lead) for a in d[:4]] for d, lead in zip(data, leads)]
    single = [[_guarded(a, lead) for a in d[:4]] for d, lead in zip(data, leads)]
    for var, n in zip(multi, ADAM_MULTI_VARS):
        assert all(view.data_ptr() % 16 != 0 and view.data_ptr() % 4 == 0 for _, view in var)
    table = _chunk_table([tuple(view.data_ptr() for _, view in var) + (n,) for var, n in zip(multi, ADAM_MULTI_VARS)])
    assert table.shape[0] == sum((n + ADAM_CHUNK - 1) // ADAM_CHUNK for n in ADAM_MULTI_VARS) and int(table[:, 4].min()) == 1
    L.call('vv_adam_step_multi', L.ptr(table), table.shape[0], lr_t, ADAM_B1, ADAM_B2, ADAM_EPS, _st())
    for var, n in zip(single, ADAM_MULTI_VARS):
        L.call('vv_adam_step', *[L.ptr(view) for _, view in var], n, lr_t, ADAM_B1, ADAM_B2, ADAM_EPS, _st())
    torch.cuda.synchronize()
    worst = [0.0, 0.0, 0.0]
    for k, (d, lead, vm, vs, n) in enumerate(zip(data, leads, multi, single, ADAM_MULTI_VARS)):
        p, g, m, v, dead = d
        for (bm, wm), (bs, ws) in zip(vm, vs):
            assert _canaries_intact(bm, lead, n) and _canaries_intact(bs, lead, n), k
            assert torch.equal(wm, ws), 'variable %d: the two forms differ' % k                # "same arithmetic"
        gp, gg, gm, gv = (view.cpu().numpy() for _, view in vm)
        assert np.array_equal(gg, g)
        assert np.isfinite(gp).all() and np.isfinite(gm).all() and np.isfinite(gv).all()
        assert np.array_equal(gp[dead], p[dead]) and not gm[dead].any() and not gv[dead].any()
        worst = [max(a, b) for a, b in zip(worst, adam_units(gp, gm, gv, p, g, m, v, lr_t))]
    print('\n[adam multi t=%d] worst error in bound units: m %.2f  v %.2f  param %.2f  (bound %.0f)' % ((t,) + tuple(worst) + (ADAM_UNITS,)))
    assert max(worst) <= ADAM_UNITS, worst


# ------------------------------------------------------------------------------------------- backward of the latent step
def _reparam_kl_bwd_ref(e, eps, dz, mask, scale, Lz):
    """float64 autograd of mean_b KL(N(mean, exp lv) || N(0, 1)) + <dz, z> with the oracle's definitions (numpy_oracle.sampling /
    kl_loss / split_mean_logvar, restated on torch tensors so autograd sees them)."""
    et = torch.tensor(e, dtype=torch.float64, requires_grad=True)
    mu, lv = et[:, :Lz], torch.clamp(et[:, Lz:2 * Lz], -10.0, 10.0)                            # split_mean_logvar
    z = mu + torch.sqrt(torch.exp(lv)) * torch.tensor(eps, dtype=torch.float64)              # sampling
    if mask is not None:
        z = z * torch.tensor(mask, dtype=torch.float64) * scale
    kl = (0.5 * (0.0 - lv) + (torch.exp(lv) + mu ** 2) / 2.0 - 0.5).sum(-1)                  # kl_loss against N(0, 1)
    total = kl.mean() + (torch.tensor(dz, dtype=torch.float64) * z).sum()
    total.backward()
    return et.grad.numpy(), z.detach().numpy(), kl.detach().numpy()


@pytest.mark.parametrize('use_mask', [False, True])
@pytest.mark.parametrize('B,Lz', [(37, 16), (256, 64), (1, 32), (5, 100)])
def test_reparam_kl_bwd_against_float64_autograd(L, B, Lz, use_mask):
    """Raw log-variances inside, exactly on and outside the +-10 clip.  tf.clip_by_value's gradient is blocked where x < min or x > max
    and PASSES at equality (the oracle states the clip as torch.clamp, whose backward uses the same closed interval): the kernel's
    `raw >= -10 && raw <= 10` is pinned to that here -- at raw == +-10 the log-variance gradient is the unclipped formula, not 0."""
    rng = np.random.default_rng(1000 * B + Lz + use_mask)
    e = (rng.standard_normal((B, 2 * Lz)) * 6).astype(np.float32)                             # sigma 6: about one log-variance in ten is outside the clip
    raw = e[:, Lz:].reshape(-1)
    edge = np.array([10.0, -10.0, np.nextafter(np.float32(10), np.float32(11)), np.nextafter(np.float32(10), np.float32(0)),
                     np.nextafter(np.float32(-10), np.float32(-11)), np.nextafter(np.float32(-10), np.float32(0)), 0.0, -0.0, 1e-3, 25.0, -25.0],
                    np.float32)
    where = rng.permutation(raw.size)[:2 * edge.size]
    raw[where] = np.concatenate([edge, edge])
    e[:, Lz:] = raw.reshape(B, Lz)
    eps = rng.standard_normal((B, Lz)).astype(np.float32)
    dz = (rng.standard_normal((B, Lz)) * 10.0 ** rng.uniform(-3, 1, (B, Lz))).astype(np.float32)
    rate = 0.3
    mask = (rng.random((B, Lz)) > rate).astype(np.float32) if use_mask else None
    scale = 1.0 / (1.0 - rate) if use_mask else 1.0
    # the oracle's numpy definitions and their torch restatement above are the same functions
    ref, z_t, kl_t = _reparam_kl_bwd_ref(e, eps, dz, mask, scale, Lz)
    mu, lv = no.split_mean_logvar(e.astype(np.float64), Lz)
    z_n = no.sampling(mu, lv, eps) * (mask.astype(np.float64) * scale if use_mask else 1.0)
    np.testing.assert_allclose(z_t, z_n, rtol=1e-14, atol=1e-14)
    np.testing.assert_allclose(kl_t, no.kl_loss(mu, lv, 0 * mu, 0 * lv), rtol=1e-13)
    ed, epsd, dzd = _dev(e), _dev(eps), _dev(dz)
    md = _dev(mask) if use_mask else None
    ob, out = _guarded_empty(B * 2 * Lz)
    L.call('vv_reparam_kl_bwd', L.ptr(ed), L.ptr(epsd), L.ptr(dzd), L.ptr(md), scale, L.ptr(out), B, Lz, 1.0 / B, _st())
    torch.cuda.synchronize()
    assert _canaries_intact(ob, 0, B * 2 * Lz)
    got = out.cpu().numpy().reshape(B, 2 * Lz)
    atol = 2e-5 * float(np.abs(dz).max())
    np.testing.assert_allclose(got, ref, rtol=2e-5, atol=atol)
    r = e[:, Lz:]
    on = (r == 10.0) | (r == -10.0)
    out_of = (r > 10.0) | (r < -10.0)
    assert on.sum() >= 4 and out_of.sum() >= 4
    assert not got[:, Lz:][out_of].any()                                                     # blocked outside
    assert np.all(got[:, Lz:][on & (np.abs(ref[:, Lz:]) > atol)] != 0)                       # passed at equality
    print('\n[reparam_kl_bwd B=%d L=%d mask=%d] max abs err %.2e, worst error / tolerance %.2f' % (
        B, Lz, use_mask, np.abs(got - ref).max(), (np.abs(got - ref) / (atol + 2e-5 * np.abs(ref))).max()))


# ----------------------------------------------------------------------------------------------- backward of the shape loss
def _bce_edges():
    lo, one = np.float32(1e-7), np.float32(1.0)
    hi = one - lo
    zero = np.float32(0)
    return np.array([0.0, np.nextafter(zero, one), np.nextafter(lo, zero), lo, np.nextafter(lo, one),
                     np.nextafter(hi, zero), hi, np.nextafter(hi, one), 1.0, np.nextafter(one, zero)], np.float32)


def _bce_bwd_ref(p, y, B):
    """float64 autograd of mean_b binary_loss_b (numpy_oracle.binary_loss, gamma 0.6) with respect to the probabilities, times the
    sigmoid's dp/dlogit = p (1 - p).  The clip constants are the float32 ones (1 - 1e-7 is 0.99999988 in float32), as the oracle
    takes them; the probabilities are float32 values, so the float64 comparisons of the clamp are the float32 ones."""
    lo = float(np.float32(1e-7))
    hi = float(np.float32(1.0) - np.float32(1e-7))
    pt = torch.tensor(p, dtype=torch.float64, requires_grad=True)
    yt = torch.tensor(y, dtype=torch.float64)
    q = torch.clamp(pt, lo, hi)
    bce = -(0.6 * yt * torch.log(q) + (1.0 - 0.6) * (1.0 - yt) * torch.log(1.0 - q)).reshape(B, -1).sum(-1)
    bce.mean().backward()
    p64 = p.astype(np.float64)
    return pt.grad.numpy() * p64 * (1.0 - p64), bce.detach().numpy()


@pytest.mark.parametrize('B,D', [(1, 32), (5, 32), (256, 32), (17, 64)])
def test_bce_bwd_at_real_sizes_against_float64_autograd(L, B, D):
    rng = np.random.default_rng(B * 100 + D)
    vox = D ** 3
    n = B * vox
    logits = rng.standard_normal(n) * 4.0
    p = (1.0 / (1.0 + np.exp(-logits))).astype(np.float32)
    y = (rng.random(n) < 0.2).astype(np.float32)
    edges = _bce_edges()
    k = edges.size
    spots = [0, n - 2 * k]
    if n > GRID_CAP + 4 * k:
        spots += [GRID_CAP - k, GRID_CAP + 2 * k + 3]       # across and just behind the start of the stride loop's second pass
    for s in spots:
        p[s:s + 2 * k] = np.concatenate([edges, edges])
        y[s:s + 2 * k] = np.concatenate([np.zeros(k), np.ones(k)])
    if (B, D) in ((256, 32), (17, 64)):
        assert len(spots) == 4                                # only these two cases reach the second pass
    ref, bce = _bce_bwd_ref(p, y, B)
    if B <= 5:                                                # the torch restatement is the oracle's function (float32 there: 1e-4)
        np.testing.assert_allclose(bce, no.binary_loss(p.reshape(B, -1), y.reshape(B, -1), gamma=0.6), rtol=1e-4)
    pd, yd = _dev(p), _dev(y)
    gb, g = _guarded_empty(n)
    L.call('vv_bce_bwd', L.ptr(pd), L.ptr(yd), L.ptr(g), B, vox, 0.6, 1e-7, 1.0 / B, _st())
    torch.cuda.synchronize()
    assert _canaries_intact(gb, 0, n)
    got = g.cpu().numpy()
    # the expected-value rule of test_bce_backward_clip_semantics, from the float32 compare
    hi = np.float32(1.0) - np.float32(1e-7)
    inside = (p >= np.float32(1e-7)) & (p <= hi)
    exp = np.where(inside, (-0.6 * y.astype(np.float64) * (1 - p.astype(np.float64)) + 0.4 * (1 - y.astype(np.float64)) * p.astype(np.float64)) / B, 0.0)
    np.testing.assert_allclose(ref, exp, rtol=1e-12, atol=1e-300)                              # autograd agrees with the rule itself
    assert not got[~inside].any()
    # one term is live per voxel (binary targets): 1 - p, two or three products -- under 4 float32 ulps, rtol 1e-6 has room
    np.testing.assert_allclose(got, ref, rtol=1e-6, atol=TINY)
    for s in spots:
        blocked = np.array([1, 1, 1, 0, 0, 0, 0, 1, 1, 1] * 2, bool)
        assert not got[s:s + 2 * k][blocked].any()
        live = ~blocked & (ref[s:s + 2 * k] != 0)
        assert np.all(got[s:s + 2 * k][live] != 0)


# ---------------------------------------------------------------------------------- dense-panel packings and their adjoints
def _axis_taps(S):
    """T[a][b][t] = 1 where a - b + 1 == t, 0 <= t <= 3 (one axis of the k4 s1 SAME tap rule: pad 1 in front, 2 behind)."""
    T = np.zeros((S, S, 4))
    for a in range(S):
        for b in range(S):
            if 0 <= a - b + 1 <= 3:
                T[a, b, a - b + 1] = 1.0
    return T


def pack_meanpool_ref(w, S):
    """packed [Cout][S^3 * Cin], column (i, ci):  W_eff[i] = (1 / S^3) sum_o w[i - o + 1][ci][co]  (i input position, o output
    position, the tap index taken per axis and kept when it is one of the 4 taps); w Keras [4,4,4,Cin,Cout]."""
    cin, cout = w.shape[3], w.shape[4]
    M = _axis_taps(S).sum(axis=1)                          # [i][t]: how many output positions o use tap t at input position i
    out = np.einsum('ad,bh,cw,dhwio->oabci', M, M, M, w.astype(np.float64), optimize=True) / float(S ** 3)
    return out.reshape(cout, S ** 3 * cin)


def pack_convT_dense_ref(w, S):
    """packed [S^3 * Cout][S^3 * Cin], row (o, co), column (j, ci) = w[o - j + 1][co][ci], 0 when a tap index leaves 0..3;
    w Keras [4,4,4,Cout,Cin]."""
    cout, cin = w.shape[3], w.shape[4]
    T = _axis_taps(S)                                      # [o][j][t]
    out = np.einsum('xad,ybh,zcw,dhwoi->xyzoabci', T, T, T, w.astype(np.float64), optimize=True)
    return out.reshape(S ** 3 * cout, S ** 3 * cin)


PANEL_CASES = [(1, 512, 128), (2, 512, 128), (4, 512, 128), (2, 24, 40), (4, 64, 64)]        # encoder tail: shipped (512 -> 128) at 16^3 / 32^3 / 64^3, ragged, one tile
PANEL_CASES_T = [(1, 8, 512), (2, 8, 512), (4, 8, 512), (2, 5, 12), (4, 3, 7)]              # decoder head: shipped (8 -> 512), two ragged


def _pack_unpack(L, pack, unpack, S, cin, cout, wshape, pshape, ref_fn, seed):
    rng = np.random.default_rng(seed)
    w = rng.standard_normal(wshape).astype(np.float32)
    P = rng.standard_normal(pshape).astype(np.float32)
    wd, Pd = _dev(w), _dev(P)
    n_panel, n_w = int(np.prod(pshape)), int(np.prod(wshape))
    pb, packed = _guarded_empty(n_panel)
    ub, unpacked = _guarded_empty(n_w)
    L.call(pack, L.ptr(wd), L.ptr(packed), S, cin, cout, L.VV_F32, _st())
    L.call(unpack, L.ptr(Pd), L.ptr(unpacked), S, cin, cout, _st())
    torch.cuda.synchronize()
    assert _canaries_intact(pb, 0, n_panel) and _canaries_intact(ub, 0, n_w)
    got_panel = packed.cpu().numpy().reshape(pshape).astype(np.float64)
    got_dw = unpacked.cpu().numpy().reshape(wshape).astype(np.float64)
    # the packing against the layout as the header states it: sums of at most 27 float32 weights (8 at these sides) and one division
    ref_panel = ref_fn(w, S)
    np.testing.assert_allclose(got_panel, ref_panel, rtol=1e-6, atol=1e-6 * np.abs(ref_panel).max())
    # adjoint identity, both inner products in float64 from the downloaded arrays: <pack(w), P> = <w, unpack(P)>
    lhs = float((got_panel * P.astype(np.float64)).sum())
    rhs = float((w.astype(np.float64) * got_dw).sum())
    norm = float(np.abs(got_panel * P.astype(np.float64)).sum())
    assert abs(lhs - rhs) <= 1e-6 * norm, (lhs, rhs, norm)
    return P, got_dw


@pytest.mark.parametrize('S,cin,cout', PANEL_CASES)
def test_meanpool_panel_pack_layout_and_adjoint(L, S, cin, cout):
    P, got_dw = _pack_unpack(L, 'vv_pack_conv_k4s1_meanpool', 'vv_unpack_meanpool_grad', S, cin, cout, (4, 4, 4, cin, cout),
                                (cout, S ** 3 * cin), pack_meanpool_ref, seed=S * 1000 + cin)
    # dw[t][ci][co] = (1 / S^3) sum over the (i, o) pairs with i - o + 1 = t per axis of dpanel[co][i * cin + ci]
    T = _axis_taps(S)
    ref_dw = np.einsum('axd,byh,czw,oabci->dhwio', T, T, T, P.astype(np.float64).reshape(cout, S, S, S, cin), optimize=True) / float(S ** 3)
    np.testing.assert_allclose(got_dw, ref_dw, rtol=1e-6, atol=1e-6 * np.abs(ref_dw).max())


@pytest.mark.parametrize('S,cin,cout', PANEL_CASES_T)
def test_convT_dense_panel_pack_layout_and_adjoint(L, S, cin, cout):
    P, got_dw = _pack_unpack(L, 'vv_pack_convT_k4s1_dense', 'vv_unpack_convT_dense_grad', S, cin, cout, (4, 4, 4, cout, cin),
                                (S ** 3 * cout, S ** 3 * cin), pack_convT_dense_ref, seed=S * 1000 + cout)
    T = _axis_taps(S)
    ref_dw = np.einsum('xad,ybh,zcw,xyzoabci->dhwoi', T, T, T, P.astype(np.float64).reshape(S, S, S, cout, S, S, S, cin), optimize=True)
    np.testing.assert_allclose(got_dw, ref_dw, rtol=1e-6, atol=1e-6 * np.abs(ref_dw).max())


def test_meanpool_panel_is_the_conv_followed_by_the_mean(L):
    """The panel's meaning, against the oracle's own layer: x . W_eff^T == mean over positions of conv3d k4 s1 SAME (x, w)."""
    S, cin, cout = 2, 64, 64
    rng = np.random.default_rng(5)
    w = (rng.standard_normal((4, 4, 4, cin, cout)) / np.sqrt(64 * cin)).astype(np.float32)
    x = rng.standard_normal((3, S, S, S, cin))
    packed = torch.empty(cout * S ** 3 * cin, dtype=torch.float32, device=DEV)
    wd = _dev(w)
    L.call('vv_pack_conv_k4s1_meanpool', L.ptr(wd), L.ptr(packed), S, cin, cout, L.VV_F32, _st())
    torch.cuda.synchronize()
    panel = packed.cpu().numpy().astype(np.float64).reshape(cout, S ** 3 * cin)
    ref = no.conv3d_same(x, w.astype(np.float64), 1).mean(axis=(1, 2, 3))
    np.testing.assert_allclose(x.reshape(3, -1) @ panel.T, ref, rtol=1e-6, atol=1e-6 * np.abs(ref).max())


def test_convT_dense_panel_is_the_transposed_conv(L):
    S, cin, cout = 2, 8, 16
    rng = np.random.default_rng(6)
    w = (rng.standard_normal((4, 4, 4, cout, cin)) / np.sqrt(8 * cin)).astype(np.float32)
    x = rng.standard_normal((3, S, S, S, cin))
    packed = torch.empty(S ** 3 * cout * S ** 3 * cin, dtype=torch.float32, device=DEV)
    wd = _dev(w)
    L.call('vv_pack_convT_k4s1_dense', L.ptr(wd), L.ptr(packed), S, cin, cout, L.VV_F32, _st())
    torch.cuda.synchronize()
    panel = packed.cpu().numpy().astype(np.float64).reshape(S ** 3 * cout, S ** 3 * cin)
    ref = no.conv3d_transpose_same(x, w.astype(np.float64), 1).reshape(3, -1)
    np.testing.assert_allclose(x.reshape(3, -1) @ panel.T, ref, rtol=1e-12, atol=1e-12)


# --------------------------------------------------------------------------------------------------------- small helpers
@pytest.mark.parametrize('rows,cols', [(1, 1), (31, 33), (32, 32), (33, 65), (4096, 128), (5, 4099)])
def test_transpose_f32_exact(L, rows, cols):
    rng = np.random.default_rng(rows * 7 + cols)
    a = rng.standard_normal((rows, cols)).astype(np.float32)
    ad = _dev(a)
    ob, out = _guarded_empty(rows * cols)
    L.call('vv_transpose_f32', L.ptr(ad), L.ptr(out), rows, cols, _st())
    torch.cuda.synchronize()
    assert _canaries_intact(ob, 0, rows * cols)
    assert np.array_equal(out.cpu().numpy().reshape(cols, rows), a.T)


@pytest.mark.parametrize('with_bias', [False, True])
@pytest.mark.parametrize('channels,repeat', [(64, 1), (8, 64), (8, 8), (37, 1), (100, 8), (512, 1), (3, 64)])
def test_fold_bn_against_float64(L, channels, repeat, with_bias):
    rng = np.random.default_rng(channels * 10 + repeat + with_bias)
    gamma = rng.uniform(0.5, 1.5, channels).astype(np.float32) * rng.choice([-1.0, 1.0], channels).astype(np.float32)
    beta = rng.normal(0, 0.3, channels).astype(np.float32)
    mean = rng.normal(0, 1.0, channels).astype(np.float32)
    var = (10.0 ** rng.uniform(-6, 2, channels)).astype(np.float32)
    bias = rng.normal(0, 0.5, channels).astype(np.float32)
    eps = 1e-3
    n = channels * repeat
    (sb, scale), (hb, shift) = _guarded_empty(n), _guarded_empty(n)
    args = [_dev(a) for a in (gamma, beta, mean, var)]
    bd = _dev(bias) if with_bias else None
    L.call('vv_fold_bn', *[L.ptr(a) for a in args], L.ptr(bd), eps, L.ptr(scale), L.ptr(shift), channels, repeat, _st())
    torch.cuda.synchronize()
    assert _canaries_intact(sb, 0, n) and _canaries_intact(hb, 0, n)
    g64, b64, m64, v64 = (a.astype(np.float64) for a in (gamma, beta, mean, var))
    sc = g64 / np.sqrt(v64 + float(np.float32(eps)))
    prod = ((bias.astype(np.float64) if with_bias else 0.0) - m64) * sc
    sh = b64 + prod
    got_sc, got_sh = scale.cpu().numpy().astype(np.float64), shift.cpu().numpy().astype(np.float64)
    ulp = 2.0 ** -23
    # scale: an add, a square root and a division, at most one ulp each -> 4 ulps with room.  shift: the subtraction, the scale's own
    # error and the product on |(bias - mean) scale|, the final add on |shift| <= |beta| + |product| -> 4 ulps of (|beta| + |product|)
    assert np.all(np.abs(got_sc - np.tile(sc, repeat)) <= 4 * ulp * np.abs(np.tile(sc, repeat)))
    assert np.all(np.abs(got_sh - np.tile(sh, repeat)) <= 4 * ulp * np.tile(np.abs(b64) + np.abs(prod), repeat))


@pytest.mark.parametrize('in_place', [False, True])
def test_sigmoid_f32_against_float64(L, in_place):
    x = np.concatenate([np.linspace(-100.0, 100.0, 200001), [0.0, -0.0, -100.0, 100.0, -88.5, 88.5, -87.0, 87.0, -16.7, 16.7, 1e-8, -1e-8]]).astype(np.float32)
    n = x.size
    xb, xd = _guarded(x)
    yb, yd = (xb, xd) if in_place else _guarded_empty(n)
    L.call('vv_sigmoid_f32', L.ptr(xd), L.ptr(yd), n, _st())
    torch.cuda.synchronize()
    assert _canaries_intact(xb, 0, n) and _canaries_intact(yb, 0, n)
    if not in_place:
        assert np.array_equal(xd.cpu().numpy(), x)
    got = yd.cpu().numpy()
    assert not np.isnan(got).any() and got.min() >= 0.0 and got.max() <= 1.0
    ref = 1.0 / (1.0 + np.exp(-x.astype(np.float64)))
    # expf within 1 ulp, the add half an ulp, the division at most 2.5 (half when correctly rounded): 4 float32 ulps; below the smallest
    # normal float32 (x < -87.3, where exp(-x) nears or passes the float32 range) the result may be flushed to 0
    assert np.all(np.abs(got.astype(np.float64) - ref) <= 4 * 2.0 ** -23 * ref + TINY)
    assert got[x == 0].tolist() == [0.5] * int((x == 0).sum())


# ---------------------------------------------------------------------------- BatchNorm training ops and the column sum
# Inputs, references and the derivation of every bound: tests/_bn_inputs.py (host self-test in tests/test_tol_host.py).
_TDT = {'f32': torch.float32, 'bf16': torch.bfloat16}


def _bn_ws(L, rows, C):
    return torch.empty(max(L.load().vv_bn_workspace_bytes(rows, C), 16), dtype=torch.uint8, device=DEV)


def _within(got, ref, bound, what):
    """|got - ref| <= bound for every element (a NaN is over the bound) -> worst err / bound."""
    got, ref, bound = np.asarray(got, np.float64).ravel(), np.asarray(ref, np.float64).ravel(), np.asarray(bound, np.float64).ravel()
    err = np.abs(got - ref)
    bad = ~(err <= bound)
    if bad.any():
        i = int(np.argmax(np.where(bad, np.nan_to_num(err, nan=np.inf), -1.0)))
        raise AssertionError('%s: %d of %d elements over the bound; worst at %d: got %r ref %r err %.3e bound %.3e' % (
            what, int(bad.sum()), bad.size, i, got[i], ref[i], err[i], bound[i]))
    live = bound > 0
    return float((err[live] / bound[live]).max()) if live.any() else 0.0


@pytest.mark.parametrize('dtname,rows,C', BI.BN_STATS_CASES)
def test_bn_train_stats_on_integer_inputs(L, dtname, rows, C):
    """vv_bn_train_stats where the sums of x and x^2 are exact: the mean equals float32(s / R), the variance is within one float32
    spacing of float32(ss / R - m m), rstd / scale / shift and the moving statistics within the unit counts of _bn_inputs.stats_ref.
    C / V = 96, 65, 86, 255 leave threads of the workgroup without a row; rows go from one to past the 1024-block cap.
    Measured, worst err / bound over all cases: mean and var 0 (equal), rstd 0.49, scale 0.61, shift 0.48, moving statistics 0.49."""
    d = BI.inputs(rows, C)
    (ref, _, _) = BI.stats_ref(d)
    xb, xd = _guarded(d.x, dtype=_TDT[dtname])
    ins = {n: _guarded(getattr(d, n)) for n in ('gamma', 'beta')}
    mov = {'moving_mean': _guarded(d.mm0), 'moving_var': _guarded(d.mv0)}
    outs = {n: _guarded_nan(C) for n in ('mean', 'var', 'rstd', 'scale', 'shift')}
    ws = _bn_ws(L, rows, C)
    L.call('vv_bn_train_stats', L.ptr(xd), rows, C, L.ptr(ins['gamma'][1]), L.ptr(ins['beta'][1]), BI.EPS, BI.MOMENTUM, L.ptr(outs['mean'][1]),
           L.ptr(outs['var'][1]), L.ptr(outs['rstd'][1]), L.ptr(outs['scale'][1]), L.ptr(outs['shift'][1]), L.ptr(mov['moving_mean'][1]),
           L.ptr(mov['moving_var'][1]), L.DTYPES[dtname], L.ptr(ws), ws.numel(), _st())
    torch.cuda.synchronize()
    assert _canaries_intact(xb, 0, rows * C) and np.array_equal(xd.float().cpu().numpy().reshape(rows, C), d.x)
    for n, (buf, view) in list(ins.items()) + list(mov.items()) + list(outs.items()):
        assert _canaries_intact(buf, 0, C), n
    worst = {}
    for n in ('mean', 'var', 'rstd', 'scale', 'shift', 'moving_mean', 'moving_var'):
        got = (outs.get(n) or mov.get(n))[1].cpu().numpy()
        worst[n] = _within(got, ref[n][0], ref[n][1], 'bn_train_stats %s %s rows=%d C=%d' % (n, dtname, rows, C))
    print('\n[bn stats %s rows=%d C=%d] worst err / bound: %s' % (dtname, rows, C, ' '.join('%s %.2f' % kv for kv in worst.items())))


@pytest.mark.parametrize('dtname,rows,C,act', BI.BN_ACT_CASES)
def test_bn_act_fwd_against_float64(L, dtname, rows, C, act):
    """vv_bn_act_fwd for every activation code.  Identity, ReLU and LeakyReLU are exact on these inputs (check_exact); ELU is held to
    one rounding per element.  Elements with u == 0 exist and are pinned: 0 for every code (ReLU `v > 0 ? v : 0`, LeakyReLU 0.3 * 0,
    ELU expm1(0))."""
    d = BI.inputs(rows, C)
    u, ref = BI.act_fwd_ref(d, act, dtname)
    xb, xd = _guarded(d.x, dtype=_TDT[dtname])
    (sb, sd), (hb, hd) = _guarded(d.scale), _guarded(d.shift)
    yb, yd = _guarded_nan(rows * C, _TDT[dtname])
    L.call('vv_bn_act_fwd', L.ptr(xd), L.ptr(sd), L.ptr(hd), L.ptr(yd), rows, C, act, L.DTYPES[dtname], _st())
    torch.cuda.synchronize()
    assert _canaries_intact(xb, 0, rows * C) and _canaries_intact(yb, 0, rows * C) and _canaries_intact(sb, 0, C) and _canaries_intact(hb, 0, C)
    y = yd.float().cpu().numpy().reshape(rows, C)
    what = 'bn_act_fwd act=%d %s rows=%d C=%d' % (act, dtname, rows, C)
    if act == 1:
        T.check_one_rounding(y, ref, u, dtname, what)
    else:
        T.check_exact(y, ref, what)
    at0 = u == 0
    assert at0[0, ::4].all() and not y[at0].any(), what                                      # the value at u == 0


@pytest.mark.parametrize('dtname,rows,C,act', BI.BN_ACT_CASES)
def test_bn_act_bwd_against_float64(L, dtname, rows, C, act):
    """vv_bn_act_bwd for every activation code, on statistics the test supplies (mean an integer, rstd = 1/2, scale +-2^k, shift an
    integer).  Identity and ReLU: dbeta and dgamma EQUAL the float64 sums.  LeakyReLU and ELU: per channel within
    U sum |term| (k + c + e), k the longest chain of float32 additions (_bn_inputs.reduce_chain, act_bwd_ref).  dx per element against
    float64 from the device's own dgamma / dbeta: 3 float32 ulps of |scale| (|du| + |k1| + |x - mean| |k2|) (_bn_inputs.dx_ref), bf16
    one rounding on top of the float32 term of those three.  The derivative at u == 0 is part of every reference: 1 for identity
    and ELU (exp(0)), 0 for ReLU, 0.3 for LeakyReLU; dy is never 0, so another value there moves dx by |scale dy| times the difference.
    bf16 runs ELU on bn_reduce_kernel<1, T, ELU> and the other three codes on the run-time switch.
    Measured, worst err / bound over all cases: the sums of LeakyReLU 0.26 (f32) / 0.27 (bf16), of ELU 0.34 (f32) / 0.82 (bf16, a one-row
    case: the bound is __expf's alone there); dx 0.42 (f32), 0.99 (bf16: an element next to a rounding boundary takes the whole half ulp)."""
    d = BI.inputs(rows, C)
    du, dbeta, dgamma, bound_b, bound_g = BI.act_bwd_ref(d, act, dtname)
    tdt = _TDT[dtname]
    (xb, xd), (gb, gd) = _guarded(d.x, dtype=tdt), _guarded(d.dy, dtype=tdt)
    par = {n: _guarded(getattr(d, n)) for n in ('scale', 'shift', 'mean', 'rstd')}
    outs = {n: _guarded_nan(C) for n in ('dgamma', 'dbeta')}
    ob, od = _guarded_nan(rows * C, tdt)
    ws = _bn_ws(L, rows, C)
    L.call('vv_bn_act_bwd', L.ptr(xd), L.ptr(gd), L.ptr(par['scale'][1]), L.ptr(par['shift'][1]), L.ptr(par['mean'][1]), L.ptr(par['rstd'][1]),
           L.ptr(outs['dgamma'][1]), L.ptr(outs['dbeta'][1]), L.ptr(od), rows, C, act, L.DTYPES[dtname], L.ptr(ws), ws.numel(), _st())
    torch.cuda.synchronize()
    for buf in (xb, gb, ob):
        assert _canaries_intact(buf, 0, rows * C)
    for n, (buf, view) in list(par.items()) + list(outs.items()):
        assert _canaries_intact(buf, 0, C), n
    what = 'bn_act_bwd act=%d %s rows=%d C=%d' % (act, dtname, rows, C)
    got_b, got_g = outs['dbeta'][1].cpu().numpy(), outs['dgamma'][1].cpu().numpy()
    u = BI.pre_act(d)
    at0 = u == 0
    assert at0[0, ::4].all() and np.array_equal(BI.act_grad(u, act)[at0], np.full(int(at0.sum()), BI.ACT_GRAD_AT_0[act]))
    if act in (0, 2):
        T.check_exact(got_b, dbeta, what + ' dbeta')
        T.check_exact(got_g, dgamma, what + ' dgamma')
    else:
        rb, rg = _within(got_b, dbeta, bound_b, what + ' dbeta'), _within(got_g, dgamma, bound_g, what + ' dgamma')
        print('\n[%s] chain k = %d, worst err / bound: dbeta %.3f dgamma %.3f' % (what, BI.reduce_chain(rows, C, dtname), rb, rg))
    ref, terms = BI.dx_ref(d, du, got_g, got_b)
    dx = od.float().cpu().numpy().reshape(rows, C)
    if dtname == 'f32':
        r = _within(dx, ref, 3 * 2.0 ** -23 * (np.abs(terms[0]) + np.abs(terms[1]) + np.abs(terms[2])), what + ' dx')
    else:
        r = T.check_one_rounding(dx, ref, np.stack(terms), 'bf16', what + ' dx')
    print('\n[%s] dx worst err / bound %.3f' % (what, r))


@pytest.mark.parametrize('dtname', ['f32', 'bf16'])
@pytest.mark.parametrize('C', BI.COLSUM_C)
@pytest.mark.parametrize('rows', BI.COLSUM_ROWS)
def test_colsum_exact(L, dtname, rows, C):
    """vv_colsum on integers -4..4 (sums below 2^24: exact in any order): equality with the float64 sum, around the 8 row slices and
    the 32-row trip of colsum_kernel, with one column, a partial and a second column block."""
    x = BI.colsum_inputs(rows, C)
    xb, xd = _guarded(x, dtype=_TDT[dtname])
    ob, out = _guarded_nan(C)
    L.call('vv_colsum', L.ptr(xd), L.ptr(out), rows, C, L.DTYPES[dtname], _st())
    torch.cuda.synchronize()
    assert _canaries_intact(xb, 0, rows * C) and _canaries_intact(ob, 0, C)
    T.check_exact(out, x.astype(np.float64).sum(0), 'colsum %s rows=%d C=%d' % (dtname, rows, C))


# ------------------------------------------------------------------------------------------------------- argument checks
def test_training_entry_points_refuse_bad_arguments(L):
    """NULL pointer -> VV_ERR_NULL (-1), non-positive size -> VV_ERR_SHAPE (-2), unknown dtype -> VV_ERR_DTYPE (-3); a refused call
    launches nothing: the output it was given is untouched."""
    lib = L.load()
    ob, x = _guarded(np.full(4096, 0.5, np.float32))
    xp, st = L.ptr(x), _st()
    assert lib.vv_adam_step(None, xp, xp, xp, 16, 1e-3, 0.9, 0.999, 1e-7, st) == -1
    assert lib.vv_adam_step(xp, None, xp, xp, 16, 1e-3, 0.9, 0.999, 1e-7, st) == -1
    assert lib.vv_adam_step(xp, xp, None, xp, 16, 1e-3, 0.9, 0.999, 1e-7, st) == -1
    assert lib.vv_adam_step(xp, xp, xp, None, 16, 1e-3, 0.9, 0.999, 1e-7, st) == -1
    assert lib.vv_adam_step(xp, xp, xp, xp, 0, 1e-3, 0.9, 0.999, 1e-7, st) == -2
    assert lib.vv_adam_step(xp, xp, xp, xp, -5, 1e-3, 0.9, 0.999, 1e-7, st) == -2
    assert lib.vv_adam_step_multi(None, 3, 1e-3, 0.9, 0.999, 1e-7, st) == -1
    assert lib.vv_adam_step_multi(xp, 0, 1e-3, 0.9, 0.999, 1e-7, st) == -2
    assert lib.vv_adam_step_multi(xp, -1, 1e-3, 0.9, 0.999, 1e-7, st) == -2
    for k in range(4):                                                                       # enc_out, eps, dz, d_enc_out (drop_mask may be NULL)
        a = [xp, xp, xp, None, 1.0, xp, 2, 8, 0.5, st]
        a[(0, 1, 2, 5)[k]] = None
        assert lib.vv_reparam_kl_bwd(*a) == -1
    assert lib.vv_reparam_kl_bwd(xp, xp, xp, None, 1.0, xp, 0, 8, 0.5, st) == -2
    assert lib.vv_reparam_kl_bwd(xp, xp, xp, None, 1.0, xp, 2, 0, 0.5, st) == -2
    assert lib.vv_reparam_kl_bwd(xp, xp, xp, None, 1.0, xp, -2, 8, 0.5, st) == -2
    for k in range(3):
        a = [xp, xp, xp, 1, 8, 0.6, 1e-7, 1.0, st]
        a[k] = None
        assert lib.vv_bce_bwd(*a) == -1
    assert lib.vv_bce_bwd(xp, xp, xp, 0, 8, 0.6, 1e-7, 1.0, st) == -2
    assert lib.vv_bce_bwd(xp, xp, xp, 1, 0, 0.6, 1e-7, 1.0, st) == -2
    assert lib.vv_bce_bwd(xp, xp, xp, 1, -8, 0.6, 1e-7, 1.0, st) == -2
    for fn in (lib.vv_unpack_meanpool_grad, lib.vv_unpack_convT_dense_grad):
        assert fn(None, xp, 1, 2, 2, st) == -1
        assert fn(xp, None, 1, 2, 2, st) == -1
        assert fn(xp, xp, 0, 2, 2, st) == -2
        assert fn(xp, xp, 1, 0, 2, st) == -2
        assert fn(xp, xp, 1, 2, 0, st) == -2
        assert fn(xp, xp, -1, 2, 2, st) == -2
    assert lib.vv_transpose_f32(None, xp, 4, 4, st) == -1
    assert lib.vv_transpose_f32(xp, None, 4, 4, st) == -1
    assert lib.vv_transpose_f32(xp, xp, 0, 4, st) == -2
    assert lib.vv_transpose_f32(xp, xp, 4, -4, st) == -2
    for fn in (lib.vv_pack_conv_k4s1_meanpool, lib.vv_pack_convT_k4s1_dense):
        assert fn(None, xp, 1, 2, 2, L.VV_F32, st) == -1
        assert fn(xp, None, 1, 2, 2, L.VV_F32, st) == -1
        assert fn(xp, xp, 0, 2, 2, L.VV_F32, st) == -2
        assert fn(xp, xp, 1, 0, 2, L.VV_F32, st) == -2
        assert fn(xp, xp, 1, 2, -2, L.VV_F32, st) == -2
        assert fn(xp, xp, 1, 2, 2, 7, st) == -3
    for k in (0, 1, 2, 3, 6, 7):                                                             # gamma, beta, mean, var, scale, shift (bias may be NULL)
        a = [xp, xp, xp, xp, None, 1e-3, xp, xp, 8, 1, st]
        a[k] = None
        assert lib.vv_fold_bn(*a) == -1
    assert lib.vv_fold_bn(xp, xp, xp, xp, None, 1e-3, xp, xp, 0, 1, st) == -2
    assert lib.vv_fold_bn(xp, xp, xp, xp, None, 1e-3, xp, xp, 8, 0, st) == -2
    assert lib.vv_sigmoid_f32(None, xp, 16, st) == -1
    assert lib.vv_sigmoid_f32(xp, None, 16, st) == -1
    assert lib.vv_sigmoid_f32(xp, xp, 0, st) == -2
    assert lib.vv_sigmoid_f32(xp, xp, -16, st) == -2
    torch.cuda.synchronize()
    assert torch.all(ob[:4096] == 0.5).item() and _canaries_intact(ob, 0, 4096)
    with pytest.raises(L.VoxVaeError):
        L.call('vv_adam_step', None, None, None, None, 1, 1e-3, 0.9, 0.999, 1e-7, None)
