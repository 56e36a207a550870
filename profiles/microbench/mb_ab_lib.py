"""A/B of two library builds on the chip-wide MFMA layers at batch 256, back to back and interleaved: D4 (vv_convT3d_k4s2_whole_fwd),
E2 (vv_conv3d_k4s2_direct_fwd; E2fp8: vv_conv3d_k4s2_direct_fp8_fwd), E3 / D3 (vv_conv3d_k4s2_skip_fwd / vv_convT3d_k4s2_skip_fwd).  Outputs must be bit-identical.
E2 runs conv_direct16_kernel; its two other forms are reached only through VV_CD_SHAPE, so E2s32 (conv_direct_kernel) and E2h
(conv_direct16h_kernel) compare the two builds' HOOKS libraries and run only when the other build's hooks library is given.
Last and first layer: identity cases at small shapes (every output tensor compared, no timing) -- D5 = vv_convT3d_final_bce_metrics_fwd
(bf16 / f32 / fp8; with the hooks libraries each VV_FINAL_BCE form), D5mean = vv_convT3d_final_mean_fwd, metrics = vv_shape_metrics,
E1 = vv_conv3d_first_fwd_io (plane form at B 2 and 64, chain form at B 128) -- and the two timed ones at workload shapes, D5fp8_256 and D5mean_32x32.
AB_AA=<a second copy of the other library> adds it as '<name>_aa': its ratio to the other library is the A/A spread of the same job.
usage: mb_ab_lib.py <other lib .so> [name [other hooks lib .so]]      (the tree's library is 'tree'; AB_ONLY=case,case,...)"""
import ctypes, json, os, sys, time
import torch
_R = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))); sys.path.insert(0, _R); sys.path.insert(0, os.path.join(_R, 'anytime-3d-reconstruction_amd'))
from voxvae import lib as L
other = sys.argv[2] if len(sys.argv) > 2 else 'base'
libs = {other: ctypes.CDLL(os.path.join(_R, sys.argv[1])), 'tree': L.load()}
hooks_libs = {other: ctypes.CDLL(os.path.join(_R, sys.argv[3])), 'tree': ctypes.CDLL(L.HOOKS_LIB_PATH)} if len(sys.argv) > 3 else None
if os.environ.get('AB_AA'):
    libs[other + '_aa'] = ctypes.CDLL(os.path.join(_R, os.environ['AB_AA']))
DEV = 'cuda:0'; B = 256
cs = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
torch.manual_seed(0)
sc = torch.rand(256, device=DEV) + 0.5; sh = torch.randn(256, device=DEV) * 0.3


def bf(*shape):
    return torch.randn(*shape, device=DEV).to(torch.bfloat16)


def packed(fn, cin, cout, *extra):
    w = (torch.randn(4, 4, 4, cin, cout, device=DEV) / (8 * cin) ** 0.5).float().contiguous()
    o = torch.empty(64 * cin * cout, dtype=torch.bfloat16, device=DEV)
    L.call(fn, L.ptr(w), L.ptr(o), *extra, cs)
    return o


cases = {}
# D4: 8^3 x 128 -> 16^3 x 64 (Keras transposed kernel [4,4,4,cout,cin])
w = packed('vv_pack_convT_k4s2_skip', 64, 128, 128, 64)
x = bf(B, 8, 8, 8, 128)
cases['D4'] = ('vv_convT3d_k4s2_whole_fwd', lambda y: (L.ptr(x), L.ptr(w), L.ptr(sc), L.ptr(sh), L.ptr(y), B, 8, 128, 64, 1, L.VV_BF16, cs), (B, 16, 16, 16, 64))
# E2: 16^3 x 64 -> 8^3 x 128
w2 = packed('vv_pack_conv_k4', 64, 128, 64, 128, L.VV_BF16)
x2 = bf(B, 16, 16, 16, 64)
cases['E2'] = ('vv_conv3d_k4s2_direct_fwd', lambda y: (L.ptr(x2), L.ptr(w2), L.ptr(sc), L.ptr(sh), L.ptr(y), B, 16, 64, 128, 1, L.VV_BF16, cs), (B, 8, 8, 8, 128))
# E3: 8^3 x 128 -> 4^3 x 256
w3 = packed('vv_pack_conv_k4_skip', 128, 256, 128, 256)
x3 = bf(B, 8, 8, 8, 128)
cases['E3'] = ('vv_conv3d_k4s2_skip_fwd', lambda y: (L.ptr(x3), L.ptr(w3), L.ptr(sc), L.ptr(sh), L.ptr(y), B, 8, 128, 256, 1, L.VV_BF16, cs), (B, 4, 4, 4, 256))
# D3: 4^3 x 256 -> 8^3 x 128
w4 = packed('vv_pack_convT_k4s2_skip', 128, 256, 256, 128)
x4 = bf(B, 4, 4, 4, 256)
cases['D3'] = ('vv_convT3d_k4s2_skip_fwd', lambda y: (L.ptr(x4), L.ptr(w4), L.ptr(sc), L.ptr(sh), L.ptr(y), B, 4, 256, 128, 1, L.VV_BF16, cs), (B, 8, 8, 8, 128))

# E2 in fp8 (the direct fp8 kernel of the 'wide' policy): e4m3fn input and weights, bf16 output
w2f = torch.empty(64 * 64 * 128, dtype=torch.uint8, device=DEV)
_w2 = (torch.randn(4, 4, 4, 64, 128, device=DEV) / 64).float().contiguous()
L.call('vv_pack_conv_k4', L.ptr(_w2), L.ptr(w2f), 64, 128, L.VV_FP8, cs)
x2f = torch.randn(B, 16, 16, 16, 64, device=DEV).to(torch.float8_e4m3fn)
cases['E2fp8'] = ('vv_conv3d_k4s2_direct_fp8_fwd', lambda y: (L.ptr(x2f), L.ptr(w2f), L.ptr(sc), L.ptr(sh), L.ptr(y), B, 16, 64, 128, 1, L.VV_BF16, cs), (B, 8, 8, 8, 128))
if hooks_libs:       # (fn, args, output shape, environment of the hooks libraries: read at every call)
    cases['E2s32'] = cases['E2'] + ({'VV_CD_SHAPE': '32'},)
    cases['E2h'] = cases['E2'] + ({'VV_CD_SHAPE': '8'},)


# ---- last layer, first layer, metrics.  A case here is (fn, args(outputs), make_outputs[, environment]); outputs whose name starts with
# '_' (workspaces) are not compared.  Shapes: small for identity, the workload's for the two timed cases.
f32 = ctypes.c_float
timed = set(cases)
wk = (torch.randn(4, 4, 4, 1, 64, device=DEV) * 0.3).to(torch.bfloat16).float().contiguous()


def d5_case(dt, side, Bn):
    D = 2 * side
    xf = torch.randn(Bn, side, side, side, 64, device=DEV)
    xd = xf.contiguous() if dt == L.VV_F32 else xf.to(torch.bfloat16 if dt == L.VV_BF16 else torch.float8_e4m3fn)
    yd = (torch.rand(Bn, D, D, D, device=DEV) < 0.3).float()
    wsb = max(int(libs['tree'].vv_convT3d_final_bce_workspace_bytes(Bn, side)), 16)

    def mk():
        return {'probs': torch.full((Bn, D, D, D), -1.0, device=DEV), 'logits': torch.full((Bn, D, D, D), -1.0, device=DEV),
                'stats': torch.full((Bn, 4), -1.0, device=DEV), 'metrics': torch.full((4,), -1.0, device=DEV),
                '_ws': torch.empty(wsb, dtype=torch.uint8, device=DEV)}
    return ('vv_convT3d_final_bce_metrics_fwd', lambda o: (L.ptr(xd), L.ptr(wk), L.ptr(yd), L.ptr(o['probs']), L.ptr(o['logits']), L.ptr(o['stats']),
            L.ptr(o['metrics']), Bn, side, 64, f32(0.6), f32(1e-7), dt, L.ptr(o['_ws']), ctypes.c_size_t(wsb), cs), mk)


def mean_case(dt, Bn, K, side):
    D = 2 * side
    xf = torch.randn(Bn * K, side, side, side, 64, device=DEV)
    xd = xf.contiguous() if dt == L.VV_F32 else xf.to(torch.bfloat16)
    yd = (torch.rand(Bn, D, D, D, device=DEV) < 0.3).float()
    libs['tree'].vv_convT3d_final_mean_workspace_bytes.restype = ctypes.c_size_t
    wsb = max(int(libs['tree'].vv_convT3d_final_mean_workspace_bytes(Bn, K, side)), 16)

    def mk():
        return {'mean': torch.full((Bn, D, D, D), -1.0, device=DEV), 'stats': torch.full((Bn, 4), -1.0, device=DEV),
                '_ws': torch.empty(wsb, dtype=torch.uint8, device=DEV)}
    return ('vv_convT3d_final_mean_fwd', lambda o: (L.ptr(xd), L.ptr(wk), L.ptr(yd), L.ptr(o['mean']), L.ptr(o['stats']), Bn, K, side, 64,
            f32(0.6), f32(1e-7), dt, L.ptr(o['_ws']), ctypes.c_size_t(wsb), cs), mk)


def metrics_case(Bn):
    st = torch.cat([torch.rand(Bn, 1, device=DEV) * 900, torch.randint(0, 500, (Bn, 3), device=DEV).float()], 1).contiguous()
    return ('vv_shape_metrics', lambda o: (L.ptr(st), L.ptr(o['metrics']), Bn, cs), lambda: {'metrics': torch.full((4,), -1.0, device=DEV)})


def e1_case(Bn, side=32):
    xg = (torch.rand(Bn, side, side, side, device=DEV) < 0.3).float()
    w1 = packed('vv_pack_conv_k4', 1, 64, 1, 64, L.VV_BF16)
    h = side // 2
    return ('vv_conv3d_first_fwd_io', lambda o: (L.ptr(xg), L.ptr(w1), L.ptr(sc), L.ptr(sh), L.ptr(o['y']), Bn, side, 64, 1, L.VV_BF16, L.VV_BF16, cs),
            lambda: {'y': torch.full((Bn, h, h, h, 64), -1.0, dtype=torch.bfloat16, device=DEV)})


libs['tree'].vv_convT3d_final_bce_workspace_bytes.restype = ctypes.c_size_t
for side, Bn in ((8, 3), (16, 2)):
    cases['D5bf16_s%d' % side] = d5_case(L.VV_BF16, side, Bn)
    if hooks_libs:
        for form in ('box', 'sweep', 'sweepp'):
            cases['D5bf16_s%d_%s' % (side, form)] = cases['D5bf16_s%d' % side] + ({'VV_FINAL_BCE': form},)
cases['D5f32_s4'] = d5_case(L.VV_F32, 4, 3)
cases['D5f32_s32'] = d5_case(L.VV_F32, 32, 2)     # 512 partial blocks per sample: the separate reduce and metrics launches
cases['D5fp8_s8'] = d5_case(L.VV_FP8, 8, 3)
cases['D5mean_bf16_s8'] = mean_case(L.VV_BF16, 3, 8, 8)
cases['D5mean_bf16_s16'] = mean_case(L.VV_BF16, 2, 4, 16)
cases['D5mean_f32_s4'] = mean_case(L.VV_F32, 5, 3, 4)
cases['metrics_5'] = metrics_case(5)
cases['metrics_70'] = metrics_case(70)
cases['E1_B2'] = e1_case(2)           # plane form
cases['E1_B64'] = e1_case(64)         # 1,024 items = one per workgroup of the chained launcher: still the plane form
cases['E1_B128'] = e1_case(128)       # two consecutive planes per workgroup: the chain form
cases['D5fp8_256'] = d5_case(L.VV_FP8, 16, 256)
cases['D5mean_32x32'] = mean_case(L.VV_BF16, 32, 32, 16)
timed |= {'D5fp8_256', 'D5mean_32x32'}

only = os.environ.get('AB_ONLY', '').split(',') if os.environ.get('AB_ONLY') else list(cases)
N = 300
res = {}
release_libs = libs
for name in only:
    fn, args, oshape = cases[name][:3]
    env = cases[name][3] if len(cases[name]) > 3 else {}
    libs = hooks_libs if env else release_libs
    os.environ.update(env)
    ys = {k: oshape() if callable(oshape) else torch.empty(*oshape, dtype=torch.bfloat16, device=DEV) for k in libs}
    fs = {}
    for k in libs:
        f = getattr(libs[k], fn); f.restype = ctypes.c_int
        fs[k] = f
        assert f(*args(ys[k])) == 0
    torch.cuda.synchronize()
    if callable(oshape):     # every output, as bytes (NaN-proof)
        same = all(bool(torch.equal(ys[other][n].view(torch.uint8), ys['tree'][n].view(torch.uint8))) for n in ys['tree'] if n[0] != '_')
    else:
        same = bool(torch.equal(ys[other], ys['tree']))
    t = {k: [] for k in libs}
    for rnd in range(4 if name in timed else 0):
        for k in libs:
            a = args(ys[k])
            for i in range(30):
                fs[k](*a)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for i in range(N):
                fs[k](*a)
            torch.cuda.synchronize()
            t[k].append(1e6 * (time.perf_counter() - t0) / N)
    res[name] = {'bit_identical': same}
    if name in timed:
        res[name].update({'us_per_launch': {k: [round(v, 2) for v in t[k]] for k in libs}, 'tree_over_%s' % other: round(min(t['tree']) / min(t[other]), 4)})
        if other + '_aa' in libs:
            res[name]['%s_aa_over_%s' % (other, other)] = round(min(t[other + '_aa']) / min(t[other]), 4)
    for k in env:
        del os.environ[k]
    print(json.dumps({name: res[name]}), flush=True)
