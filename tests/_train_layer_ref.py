"""Layer-wise, teacher-forced float64 references of one bf16 training step (tests/test_gpu_train_native.py).

capture() runs ONE Trainer.step with debug = {} and downloads what every launch read and wrote; check_step() recomputes each launch
in float64 from the operands the trainer actually held -- the stored bf16 tensors widened, the float32 weights rounded to bf16 where
the kernel reads a bf16 image -- and holds the stored result to a bound that is derived here or already the project's:

  stride-2 layers, first conv, dense layers, every data gradient   _tol.check_one_rounding(got, ref, pre_act=ref, type of the output)
  weight gradients (float32 from bf16 operands)                    |got - ref| <= _tol.f32_term(ref)   (test_gpu_ops.py::test_wgrad_kernels)
  the two panel-gradient reshapes                                  float64 sum of the DEVICE's panel gradient; a tap sums at most
                                                                   S^3 float32 entries in an unknown order: (n + 1) U sum |entry|
  BatchNorm statistics / forward / backward                        _bn_inputs' operation counts, extended below to inputs whose sums
                                                                   are not exact (bn_stats_bounds, check_bn)
  final layer                                                      the bounds of test_gpu_ops.py::test_convT3d_final_bce and
                                                                   test_gpu_train_ops.py::test_bce_bwd_at_real_sizes_against_float64_autograd

No bound here was measured on the code under test.  Written for any depth and width the trainer admits; ELU only (every config)."""
import numpy as np
import torch

import _bn_inputs as BI
import _tol as T
from oracle import torch_oracle as to

U = 2.0 ** -24
TINY = float(np.finfo(np.float32).tiny)
BN_EPS, BN_MOM = float(np.float32(1e-3)), float(np.float32(0.99))
F64 = torch.float64


def bf16_round(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(torch.bfloat16).to(torch.float32).numpy()


def _np(t):
    """Stored tensor (any float type) -> float64 numpy."""
    return t.detach().to(torch.float64).cpu().numpy() if hasattr(t, 'detach') else np.asarray(t, np.float64)


def _t64(a, grad=False):
    t = a.detach().to(F64).cpu() if hasattr(a, 'detach') else torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64))
    return t.requires_grad_(grad)


def _cpu(t):
    return None if t is None else t.detach().cpu()


# ------------------------------------------------------------------------------------------------------------------- capture
def _axis_taps(S):
    """T[a][b][t] = 1 where a - b + 1 == t, 0 <= t <= 3 (one axis of the k4 s1 SAME tap rule: pad 1 in front, 2 behind)."""
    M = np.zeros((S, S, 4))
    for a in range(S):
        for b in range(S):
            if 0 <= a - b + 1 <= 3:
                M[a, b, a - b + 1] = 1.0
    return M


def pack_meanpool_ref(w, S):
    """[Cout][S^3 Cin]: the last encoder conv (k4 s1 SAME) followed by the mean over positions, as one panel (include/voxvae.h)."""
    cin, cout = w.shape[3], w.shape[4]
    M = _axis_taps(S).sum(axis=1)
    return (np.einsum('ad,bh,cw,dhwio->oabci', M, M, M, np.asarray(w, np.float64), optimize=True) / float(S ** 3)).reshape(cout, S ** 3 * cin)


def pack_convT_dense_ref(w, S):
    """[S^3 Cout][S^3 Cin]: the first decoder layer (k4 s1 SAME transposed conv over the S^3 seed) as one panel."""
    cout, cin = w.shape[3], w.shape[4]
    M = _axis_taps(S)
    return np.einsum('xad,ybh,zcw,dhwoi->xyzoabci', M, M, M, np.asarray(w, np.float64), optimize=True).reshape(S ** 3 * cout, S ** 3 * cin)


def unpack_meanpool_ref(P, S, cin, cout):
    M = _axis_taps(S)
    return np.einsum('axd,byh,czw,oabci->dhwio', M, M, M, P.reshape(cout, S, S, S, cin), optimize=True) / float(S ** 3)


def unpack_convT_dense_ref(P, S, cin, cout):
    M = _axis_taps(S)
    return np.einsum('xad,ybh,zcw,xyzoabci->dhwoi', M, M, M, P.reshape(S, S, S, cout, S, S, S, cin), optimize=True)


def _bn_host(bn):
    return {n: getattr(bn, n).detach().cpu().numpy().astype(np.float64) for n in ('mean', 'var', 'rstd', 'scale', 'shift')}


def capture(tr, x, eps):
    """One Trainer.step(x, x, eps) with debug = {} -> everything check_step needs, on the host.  The weight-derived operands of the
    dense launches are taken BEFORE the step: the engines' packed panels, and the transposed panel of the encoder tail's data
    gradient rebuilt by the two calls _encoder_backward makes (the step's own copy is a temporary)."""
    from voxvae import lib as L
    from voxvae import train as TR
    enc, dec = tr.enc, tr.dec
    assert tr.dt == L.VV_BF16 and enc.act == L.ACT['elu'] and dec.act == L.ACT['elu']
    fe, fd = list(enc.filters), list(dec.filters)
    ne = len(fe) - 1
    cap = {'D': enc.D, 'fe': fe, 'fd': fd, 'Se': enc.S, 'Sd': dec.S, 'ch': dec.ch, 'Lz': dec.L, 'var': bool(tr.var), 'B': int(x.shape[0]),
           'world': tr.world}
    cap['ep'] = {k: v.detach().cpu().numpy().copy() for k, v in enc.params.items()}
    cap['dp'] = {k: v.detach().cpu().numpy().copy() for k, v in dec.params.items()}
    for e in (enc, dec):
        e.ensure_packed(fold=False)
    K5, E_out = enc.S ** 3 * fe[ne - 1], fe[ne]
    wef = torch.empty(E_out, K5, dtype=torch.float32, device=tr.dev)
    L.call('vv_pack_conv_k4s1_meanpool', L.ptr(enc.params['conv%d/kernel' % ne]), L.ptr(wef), enc.S, fe[ne - 1], E_out, L.VV_F32, TR._st())
    weT = torch.empty(K5, E_out, dtype=torch.bfloat16, device=tr.dev)
    L.call('vv_pack_dense', L.ptr(wef), L.ptr(weT), E_out, K5, L.VV_BF16, TR._st())
    cap['panels'] = {'enc_fwd': _cpu(enc.packed['w%d' % ne]), 'enc_f32': _cpu(wef), 'enc_bwd': _cpu(weT), 'dec_wd': _cpu(dec.packed['wd']),
                     'dec_w0': _cpu(dec.packed['w0'])}
    xd = torch.from_numpy(x).to(tr.dev)
    epsd = torch.from_numpy(eps).to(tr.dev) if tr.var else None
    tr.debug = {}
    kl, stats, metrics = tr.step(xd, xd, epsd)
    torch.cuda.synchronize()
    d = tr.debug
    cap['x'], cap['eps'] = x, eps
    cap['kl'], cap['stats'] = (None if kl is None else kl.cpu().numpy()), stats.cpu().numpy()
    for k in ('dlogit', 'probs', 'enc_out', 'z', 'z_act', 'dz', 'de', 'c_d0', 'dcv0', 't0', 'dt0', 'dpanel_dec', 'dpanel_enc'):
        cap[k] = _cpu(d[k])
    for k in ('h_enc', 'c_enc', 'dh_enc', 'dcv_enc', 'h_dec', 'c_dec', 'dh_dec', 'dcv_dec'):
        cap[k] = [_cpu(t) for t in d[k]]
    cap['bn_enc'], cap['bn_dec'], cap['bn_d0'] = [_bn_host(b) for b in d['bn_enc']], [_bn_host(b) for b in d['bn_dec']], _bn_host(d['bn_d0'])
    cap['grads'] = {n: tr.grads.views[n].detach().cpu().numpy().copy() for n, _ in tr.order}
    cap['ep_after'] = {k: v.detach().cpu().numpy().copy() for k, v in enc.params.items() if k.endswith(('moving_mean', 'moving_variance'))}
    cap['dp_after'] = {k: v.detach().cpu().numpy().copy() for k, v in dec.params.items() if k.endswith(('moving_mean', 'moving_variance'))}
    # how each BatchNorm's statistics were summed: the decoder's 'whole' layer leaves its own column sums (Trainer._decoder_forward)
    from voxvae import routes as R
    cap['fused_stats'] = [False] + [tr._route(R.CONVT, dec.S << (i - 1), fd[i - 1], fd[i]) == 'whole' and not tr.sw.no_stats_fusion
                                    for i in range(1, len(fd) - 1)]
    tr.debug = None
    return cap


# ----------------------------------------------------------------------------------------------------------------- BatchNorm
def bn_stats_bounds(c, gamma, beta, mm0, mv0, k_rel):
    """float64 statistics of c [R, C] and the bound of each output of bn_stats_finalize_kernel, {name: (ref, bound)}.

    _bn_inputs.stats_ref counts the operations behind the per-block sums, which are exact on its integer inputs.  Here they are
    not: a float32 partial sum that passes through k additions is off by at most k U sum |term| (k_rel = k U; the blocks' partials
    are added in double).  With A1 = mean |x| and A2 = mean x^2 per channel,
      mean   k U A1 + U |m|                                        (the sum, the rounding of m to float32)
      var    (k + 1) U A2 + 2 |m| k U A1 + U v                     (x * x rounds once more; d(m^2) = 2 |m| dm; v's own rounding)
      rstd   |1 / sqrt(v - dv + eps) - r| + 2 U r                  (monotone in v: the exact worst case, v - dv kept >= 0)
      scale  |gamma| d rstd + 3 U |scale|
      shift  |gamma r| dm + |m gamma| d rstd + 6 U (|beta| + |m gamma r|)
      moving (1 - momentum) d stat + 4 U (|old momentum| + |stat (1 - momentum)|)
    the U-multiples of the last four being _bn_inputs.stats_ref's."""
    R = float(c.shape[0])
    m, A1, A2 = c.mean(0), np.abs(c).mean(0), (c * c).mean(0)
    v = np.maximum(A2 - m * m, 0.0)
    dm_sum = k_rel * A1
    dm = dm_sum + U * np.abs(m)
    dv = (k_rel + U) * A2 + 2.0 * np.abs(m) * dm_sum + U * v
    r = 1.0 / np.sqrt(v + BN_EPS)
    dr = np.abs(1.0 / np.sqrt(np.maximum(v - dv, 0.0) + BN_EPS) - r) + 2 * U * r
    g, b = np.asarray(gamma, np.float64), np.asarray(beta, np.float64)
    out = {'mean': (m, dm), 'var': (v, dv), 'rstd': (r, dr), 'scale': (g * r, np.abs(g) * dr + 3 * U * np.abs(g * r)),
           'shift': (b - m * g * r, np.abs(g * r) * dm + np.abs(m * g) * dr + 6 * U * (np.abs(b) + np.abs(m * g * r)))}
    for name, old, stat, ds in (('moving_mean', mm0, m, dm), ('moving_var', mv0, v, dv)):
        p1, p2 = np.asarray(old, np.float64) * BN_MOM, stat * (1.0 - BN_MOM)
        out[name] = (p1 + p2, (1.0 - BN_MOM) * ds + 4 * U * (np.abs(p1) + np.abs(p2)))
    return out


def _within(got, ref, bound, what):
    got, ref, bound = (np.asarray(a, np.float64) for a in (got, ref, bound))
    bound = np.broadcast_to(bound, ref.shape)
    assert got.shape == ref.shape, '%s: shape %s, expected %s' % (what, got.shape, ref.shape)
    err = np.abs(got - ref)
    bad = ~(err <= bound)
    if bad.any():
        r = np.where(bad, np.nan_to_num(err / np.maximum(bound, 1e-300), nan=np.inf), 0.0)
        i = np.unravel_index(int(np.argmax(r)), r.shape)
        raise AssertionError('%s: %d of %d elements over the bound; worst at %s: got %r ref %r err %.3e bound %.3e' % (
            what, int(bad.sum()), bad.size, tuple(int(v) for v in i), got[i], ref[i], err[i], bound[i]))
    live = bound > 0
    return float((err[live] / bound[live]).max()) if live.any() else 0.0


def check_bn(what, c, h, dy, dx, bn, gamma, beta, mov0, mov1, dgamma, dbeta, fused, out):
    """One BatchNorm + ELU of the step: statistics of the stored c, forward to the stored h, backward of the stored dy to the stored dx
    and the two parameter gradients.  bn: the device's float32 mean / var / rstd / scale / shift; the forward and the backward are
    held to THOSE (what the kernels read), the statistics to float64 of c."""
    C = len(gamma)
    c = _np(c).reshape(-1, C)                              # (the dense layers' outputs are stored [B, positions * C])
    rows = c.shape[0]
    # the sweep's per-block sums pass through reduce_chain additions; the whole-sample layer's own column sums are held to what
    # test_gpu_ops.py::test_convT3d_whole_stats_form holds them to (2e-5 of sum |x|, of sum x^2)
    k_rel = 2e-5 if fused else BI.reduce_chain(rows, C, 'bf16') * U
    st = bn_stats_bounds(c, gamma, beta, mov0[0], mov0[1], k_rel)
    got = dict(bn, moving_mean=mov1[0], moving_var=mov1[1])
    for n in ('mean', 'var', 'rstd', 'scale', 'shift', 'moving_mean', 'moving_var'):
        out['%s stats %s' % (what, n)] = _within(got[n], st[n][0], st[n][1], '%s BatchNorm statistics: %s' % (what, n))
    sc, sh, mu, rs = bn['scale'], bn['shift'], bn['mean'], bn['rstd']
    u = c * sc + sh
    ref = np.where(u > 0, u, np.expm1(np.minimum(u, 0.0)))
    out[what + ' bn fwd'] = T.check_one_rounding(_np(h).reshape(rows, C), ref, u, 'bf16', what + ' BatchNorm + ELU forward')
    del ref
    # backward sums, _bn_inputs.act_bwd_ref's count for bf16 ELU: U sum |term| (k + c + e), k the addition chain, c = 1 (dbeta: d = dy act')
    # or 2 (dgamma: d * xhat), e = |min(u, 0)| + 2 for __expf.  On top of it here: u = x scale + shift is not exact (<= 2 U (|x scale| +
    # |shift|) absolute, the same amount relative to exp(u)), and xhat = (x - mean) rstd rounds twice (2 more on dgamma)
    dy = _np(dy).reshape(rows, C)
    du = dy * np.exp(np.minimum(u, 0.0))
    xm = c - mu
    tg = du * xm * rs
    k = BI.reduce_chain(rows, C, 'bf16')
    e = np.abs(np.minimum(u, 0.0)) + 2.0 + 2.0 * (np.abs(c * sc) + np.abs(sh))
    out[what + ' dbeta'] = _within(dbeta, du.sum(0), U * (np.abs(du) * (k + 1 + e)).sum(0), what + ' dbeta')
    out[what + ' dgamma'] = _within(dgamma, tg.sum(0), U * (np.abs(tg) * (k + 4 + e)).sum(0), what + ' dgamma')
    del tg, e
    # dx from the DEVICE's dgamma / dbeta (_bn_inputs.dx_ref): only the sweep is measured; bf16: one rounding on the float32 term of the three
    k1 = np.asarray(dbeta, np.float64) / rows
    k2 = np.asarray(dgamma, np.float64) * rs / rows
    t0, t1, t2 = sc * du, sc * k1, sc * xm * k2
    big = np.array([np.abs(t0).max(), np.abs(t1).max(), np.abs(t2).max()])
    out[what + ' bn bwd'] = T.check_one_rounding(_np(dx).reshape(rows, C), t0 - t1 - t2, big, 'bf16', what + ' BatchNorm + ELU backward (dx)')


# ------------------------------------------------------------------------------------------------------------------ the step
def _wgrad_ok(got, ref, what, out):
    out[what] = _within(got, ref, T.f32_term(ref), what)


def _stride2(direction, x, w, g):
    """float64 layer and, by autograd, its two gradients for the stored output gradient g -> (c, dx, dw) numpy."""
    xt, wt = _t64(x, True), _t64(w, True)
    c = (to._conv_same if direction == 'conv' else to._convT_same)(xt, wt, 2)
    dx, dw = torch.autograd.grad(c, [xt, wt], _t64(g).reshape(c.shape))
    return c.detach().numpy(), dx.numpy(), dw.numpy()


class Failures:
    """Runs every check, collects the failures: one broken launch must not hide the state of the others (teacher forcing makes
    them independent)."""

    def __init__(self):
        self.failed, self.ratios = [], {}

    def run(self, name, fn, *args):
        try:
            fn(*args)
        except AssertionError as e:
            self.failed.append((name, str(e)))

    def names(self):
        return [n for n, _ in self.failed]

    def raise_if_any(self):
        if self.failed:
            raise AssertionError('%d launches off their reference:\n%s' % (len(self.failed), '\n'.join('  [%s] %s' % f for f in self.failed)))


def check_encoder(cap, F):
    fe, B, D, S, out = cap['fe'], cap['B'], cap['D'], cap['Se'], F.ratios
    ne = len(fe) - 1
    ep, gr, pan = cap['ep'], cap['grads'], cap['panels']

    def bn(i):
        pre = 'bn%d' % i
        check_bn('E%d' % (i + 1), cap['c_enc'][i], cap['h_enc'][i], cap['dh_enc'][i], cap['dcv_enc'][i], cap['bn_enc'][i], ep[pre + '/gamma'],
                 ep[pre + '/beta'], (ep[pre + '/moving_mean'], ep[pre + '/moving_variance']),
                 (cap['ep_after'][pre + '/moving_mean'], cap['ep_after'][pre + '/moving_variance']),
                 gr['enc/%s/gamma' % pre], gr['enc/%s/beta' % pre], False, out)

    def first():
        # the occupancy grid is exact in bf16; the kernel reads the [64][64] bf16 image of the weights
        c, _, dw = _stride2('conv', cap['x'], bf16_round(ep['conv0/kernel']), cap['dcv_enc'][0])
        out['E1 fwd'] = T.check_one_rounding(cap['c_enc'][0], c, c, 'bf16', 'E1 first conv forward')
        _wgrad_ok(gr['enc/conv0/kernel'], dw, 'E1 weight gradient (cin = 1, side %d)' % D, out)

    F.run('E1', first)
    F.run('E1 bn', bn, 0)
    for i in range(1, ne):
        def layer(i=i):
            c, dx, dw = _stride2('conv', cap['h_enc'][i - 1], bf16_round(ep['conv%d/kernel' % i]), cap['dcv_enc'][i])
            what = 'E%d conv side %d %d->%d' % (i + 1, cap['h_enc'][i - 1].shape[1], fe[i - 1], fe[i])
            fs = Failures()
            fs.run(0, lambda: out.__setitem__(what + ' fwd', T.check_one_rounding(cap['c_enc'][i], c, c, 'bf16', what + ' forward')))
            fs.run(1, lambda: out.__setitem__(what + ' dgrad', T.check_one_rounding(cap['dh_enc'][i - 1], dx, dx, 'bf16', what + ' data gradient')))
            fs.run(2, lambda: _wgrad_ok(gr['enc/conv%d/kernel' % i], dw, what + ' weight gradient', out))
            assert not fs.failed, ' | '.join(m for _, m in fs.failed)
        F.run('E%d' % (i + 1), layer)
        F.run('E%d bn' % (i + 1), bn, i)

    def tail():
        cin, E_out = fe[ne - 1], fe[ne]
        K5 = S ** 3 * cin
        w = ep['conv%d/kernel' % ne]
        pref = pack_meanpool_ref(w, S)
        fs = Failures()
        # the panels: bf16 image of the float64 panel (one rounding on a float32 sum of <= 27 weights), the float32 panel of the backward
        # at test_gpu_train_ops.py's 1e-6, its transposed bf16 copy the exact rounding of the device's float32 panel
        fs.run(0, lambda: out.__setitem__('E tail panel', T.check_one_rounding(pan['enc_fwd'], pref, pref, 'bf16', 'encoder tail panel S=%d' % S)))
        fs.run(1, lambda: np.testing.assert_allclose(_np(pan['enc_f32']), pref, rtol=1e-6, atol=1e-6 * np.abs(pref).max()))
        fs.run(2, lambda: T.check_exact(pan['enc_bwd'], bf16_round(pan['enc_f32'].numpy()).astype(np.float64).T, 'encoder tail transposed panel'))
        h = _np(cap['h_enc'][ne - 1]).reshape(B, K5)
        ref = h @ _np(pan['enc_fwd']).T
        fs.run(3, lambda: out.__setitem__('E tail fwd', T.check_one_rounding(cap['enc_out'], ref, ref, 'f32', 'encoder tail forward (S=%d, K=%d)' % (S, K5))))
        de = _np(cap['de'])
        dp_ref = de.T @ h
        fs.run(4, lambda: _wgrad_ok(cap['dpanel_enc'], dp_ref, 'encoder tail panel gradient', out))
        P = _np(cap['dpanel_enc'])
        n_terms = S ** 3                                       # pairs (input position, output position) a tap can have: at most S per axis
        fs.run(5, lambda: out.__setitem__('E tail unpack', _within(gr['enc/conv%d/kernel' % ne], unpack_meanpool_ref(P, S, cin, E_out),
                                                                  (n_terms + 1) * U * unpack_meanpool_ref(np.abs(P), S, cin, E_out),
                                                                  'vv_unpack_meanpool_grad side %d' % S)))
        dh = _np(bf16_round(cap['de'].numpy())) @ _np(pan['enc_bwd']).T
        fs.run(6, lambda: out.__setitem__('E tail dgrad', T.check_one_rounding(cap['dh_enc'][ne - 1].reshape(B, K5), dh, dh, 'bf16', 'encoder tail data gradient')))
        assert not fs.failed, ' | '.join(m for _, m in fs.failed)

    F.run('E tail', tail)


def check_decoder(cap, F):
    fd, B, D, S, ch, Lz, out = cap['fd'], cap['B'], cap['D'], cap['Sd'], cap['ch'], cap['Lz'], F.ratios
    nd = len(fd) - 1
    dp, gr, pan = cap['dp'], cap['grads'], cap['panels']
    lin, n1 = S ** 3 * ch, S ** 3 * fd[0]
    inv_gb = 1.0 / float(B * cap['world'])

    def bn(what, pre, c, h, dy, dx, bnd, fused=False):
        check_bn(what, c, h, dy, dx, bnd, dp[pre + '/gamma'], dp[pre + '/beta'], (dp[pre + '/moving_mean'], dp[pre + '/moving_variance']),
                 (cap['dp_after'][pre + '/moving_mean'], cap['dp_after'][pre + '/moving_variance']),
                 gr['dec/%s/gamma' % pre], gr['dec/%s/beta' % pre], fused, out)

    def d0():
        fs = Failures()
        wk = bf16_round(dp['dense/kernel']).astype(np.float64)              # Keras [L][lin]
        fs.run(0, lambda: T.check_exact(pan['dec_wd'], wk.T, 'Dense panel'))
        fs.run(1, lambda: T.check_exact(cap['z_act'], bf16_round(cap['z'].numpy()), 'z in the activation dtype'))
        z = _np(cap['z_act'])
        ref = z @ wk + dp['dense/bias'].astype(np.float64)
        fs.run(2, lambda: out.__setitem__('D0 fwd', T.check_one_rounding(cap['c_d0'], ref, ref, 'bf16', 'D0 Dense forward')))
        g = _np(cap['dcv0'])
        fs.run(3, lambda: _wgrad_ok(gr['dec/dense/kernel'], z.T @ g, 'D0 Dense weight gradient', out))
        # vv_colsum over B rows: B - 1 float32 additions
        fs.run(4, lambda: out.__setitem__('D0 bias', _within(gr['dec/dense/bias'], g.sum(0), B * U * np.abs(g).sum(0), 'D0 bias gradient')))
        dz = g @ wk.T
        fs.run(5, lambda: out.__setitem__('D0 dgrad', T.check_one_rounding(cap['dz'], dz, dz, 'f32', 'D0 Dense data gradient')))
        assert not fs.failed, ' | '.join(m for _, m in fs.failed)

    def d1():
        fs = Failures()
        w = dp['convT0/kernel']
        pref = bf16_round(pack_convT_dense_ref(w, S)).astype(np.float64)      # a permutation with zeros: every entry one weight, rounded once
        fs.run(0, lambda: T.check_exact(pan['dec_w0'], pref, 'D1 panel S=%d' % S))
        t0 = _np(cap['t0'])
        ref = t0 @ pref.T
        fs.run(1, lambda: out.__setitem__('D1 fwd', T.check_one_rounding(cap['c_dec'][0].reshape(B, n1), ref, ref, 'bf16', 'D1 forward (S=%d, n1=%d)' % (S, n1))))
        g = _np(cap['dcv_dec'][0]).reshape(B, n1)
        fs.run(2, lambda: _wgrad_ok(cap['dpanel_dec'], g.T @ t0, 'D1 panel gradient', out))
        P = _np(cap['dpanel_dec'])
        n_terms = S ** 3
        fs.run(3, lambda: out.__setitem__('D1 unpack', _within(gr['dec/convT0/kernel'], unpack_convT_dense_ref(P, S, ch, fd[0]),
                                                              (n_terms + 1) * U * unpack_convT_dense_ref(np.abs(P), S, ch, fd[0]),
                                                              'vv_unpack_convT_dense_grad side %d' % S)))
        dt0 = g @ pref
        fs.run(4, lambda: out.__setitem__('D1 dgrad', T.check_one_rounding(cap['dt0'], dt0, dt0, 'bf16', 'D1 data gradient')))
        assert not fs.failed, ' | '.join(m for _, m in fs.failed)

    F.run('D0', d0)
    F.run('D0 bn', bn, 'D0', 'bn_dense', cap['c_d0'], cap['t0'], cap['dt0'], cap['dcv0'], cap['bn_d0'])
    F.run('D1', d1)
    F.run('D1 bn', bn, 'D1', 'bnT0', cap['c_dec'][0], cap['h_dec'][0], cap['dh_dec'][0], cap['dcv_dec'][0], cap['bn_dec'][0])
    for i in range(1, nd):
        def layer(i=i):
            side = S << (i - 1)
            c, dx, dw = _stride2('convT', cap['h_dec'][i - 1].reshape(B, side, side, side, fd[i - 1]), bf16_round(dp['convT%d/kernel' % i]), cap['dcv_dec'][i])
            what = 'D%d convT side %d %d->%d' % (i + 1, side, fd[i - 1], fd[i])
            fs = Failures()
            fs.run(0, lambda: out.__setitem__(what + ' fwd', T.check_one_rounding(cap['c_dec'][i], c, c, 'bf16', what + ' forward')))
            fs.run(1, lambda: out.__setitem__(what + ' dgrad', T.check_one_rounding(cap['dh_dec'][i - 1].reshape(dx.shape), dx, dx, 'bf16', what + ' data gradient')))
            fs.run(2, lambda: _wgrad_ok(gr['dec/convT%d/kernel' % i], dw, what + ' weight gradient', out))
            assert not fs.failed, ' | '.join(m for _, m in fs.failed)
        F.run('D%d' % (i + 1), layer)
        F.run('D%d bn' % (i + 1), bn, 'D%d' % (i + 1), 'bnT%d' % i, cap['c_dec'][i], cap['h_dec'][i], cap['dh_dec'][i], cap['dcv_dec'][i],
              cap['bn_dec'][i], cap['fused_stats'][i])

    def final():
        fs = Failures()
        y = cap['x'].astype(np.float64).reshape(B, -1)
        p = cap['probs'].numpy().reshape(B, -1)
        dl = cap['dlogit'].numpy().reshape(B, -1)
        # vv_bce_bwd from the device's own float32 probabilities: the rule and the tolerance of test_bce_bwd_at_real_sizes_against_float64_autograd
        inside = (p >= np.float32(1e-7)) & (p <= np.float32(1.0) - np.float32(1e-7))
        p64 = p.astype(np.float64)
        exp = np.where(inside, (-0.6 * y * (1 - p64) + 0.4 * (1 - y) * p64) * inv_gb, 0.0)
        fs.run(0, lambda: np.testing.assert_allclose(dl, exp, rtol=1e-6, atol=TINY, err_msg='vv_bce_bwd side %d' % D))
        # forward and both gradients: the layer is a transposed conv 64 -> 1; its weight gradient and its data gradient read dlogit
        # rounded to bf16 (the im2col rows of vv_wgrad_conv_k4s2 and the tiles of vv_conv3d_first_fwd are bf16)
        side = S << (nd - 1)
        lg, dx, dw = _stride2('convT', cap['h_dec'][nd - 1].reshape(B, side, side, side, fd[nd - 1]), bf16_round(dp['convT%d/kernel' % nd]), bf16_round(cap['dlogit'].numpy()))
        lg = lg.reshape(B, -1)
        pr = 1.0 / (1.0 + np.exp(-lg))
        # test_convT3d_final_bce: logits within 2e-5 max(1, max |logit|); a probability moves by at most a quarter of that, plus the
        # float32 sigmoid (4 ulps: test_sigmoid_f32_against_float64).  1e-5, the bound of that test, where |logit| <= 2
        fs.run(1, lambda: out.__setitem__('final probs', _within(p, pr, 0.25 * 2e-5 * max(1.0, float(np.abs(lg).max())) + 4 * 2.0 ** -23, 'final layer probabilities')))
        s = cap['stats'].astype(np.float64)
        q = np.clip(p, np.float32(1e-7), np.float32(1.0) - np.float32(1e-7))
        om = (np.float32(1.0) - q).astype(np.float64)
        bce_self = -(0.6 * y * np.log(q.astype(np.float64)) + 0.4 * (1 - y) * np.log(om)).sum(-1)
        fs.run(2, lambda: np.testing.assert_allclose(s[:, 0], bce_self, rtol=2e-5, err_msg='final layer bce on its own probabilities'))
        qr = np.clip(pr, 1e-7, 1.0 - 1e-7)
        fs.run(3, lambda: np.testing.assert_allclose(s[:, 0], -(0.6 * y * np.log(qr) + 0.4 * (1 - y) * np.log(1.0 - qr)).sum(-1), rtol=2e-3,
                                                    err_msg='final layer bce against float64'))
        flip = (p >= 0.5) != (lg >= 0)
        flips = int(flip.sum())

        def counts():
            assert flips == 0 or np.abs(lg[flip]).max() < 1e-5, 'occupancy flipped away from a zero logit'
            yh = lg >= 0
            for k, r in ((1, (y * yh).sum(-1)), (2, ((1 - y) * yh).sum(-1)), (3, (y * ~yh).sum(-1))):
                assert np.abs(s[:, k] - r).max() <= flips, 'TP / FP / FN column %d' % k
        fs.run(4, counts)
        fs.run(5, lambda: _wgrad_ok(gr['dec/convT%d/kernel' % nd], dw, 'final layer weight gradient [64 taps][%d] (side %d)' % (fd[nd - 1], D), out))
        fs.run(6, lambda: out.__setitem__('final dgrad', T.check_one_rounding(cap['dh_dec'][nd - 1].reshape(dx.shape), dx, dx, 'bf16', 'final layer data gradient (first-conv form, side %d)' % D)))
        assert not fs.failed, ' | '.join(m for _, m in fs.failed)

    F.run('D%d final' % (nd + 1), final)


def check_step(cap, parts=('encoder', 'decoder')):
    """-> Failures (its .ratios: worst err / bound of every check that passed)."""
    F = Failures()
    if 'encoder' in parts:
        check_encoder(cap, F)
    if 'decoder' in parts:
        check_decoder(cap, F)
    return F
