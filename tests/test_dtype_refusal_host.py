"""CPU test: every entry of include/voxvae.h with a `*dtype` parameter refuses an element-type code outside the set it admits, before
anything is launched.  The entries come from the header (tests/_guarded.header_protos), so a new one without a recipe here fails.

Each call is the raw ctypes function on ONE 16-byte-aligned dummy HOST buffer standing in for every pointer, otherwise valid scalars of the
smallest shape the entry's shape check admits, a generous workspace, and exactly one dtype parameter set to a code it does not admit:
-1, 3 and 7 for every parameter, VV_FP8 (2) for every parameter that is not in FP8_ADMITTED.  No admitted combination is ever passed to
an entry that takes pointers, and the module is skipped where a device exists: the pointers are fake."""
import ctypes

import pytest
import torch

from _guarded import header_protos

pytestmark = pytest.mark.skipif(torch.cuda.is_available(), reason='fake host pointers: never where a kernel could be enqueued on them')

VV_F32, VV_BF16, VV_FP8 = 0, 1, 2
ERR_SHAPE, ERR_DTYPE = -2, -3
UNKNOWN = (-1, 3, 7)
BIG = 1 << 40

# (entry, parameter) pairs that admit VV_FP8 in some combination (from csrc/: small.hip, igemm.hip, conv_direct*.hip, convt_direct_fp8.hip,
# final_bce.hip)
FP8_ADMITTED = (
    ('vv_pack_conv_k4', 'dtype'), ('vv_pack_convT_k4s2', 'dtype'), ('vv_pack_conv_k4s1_meanpool', 'dtype'), ('vv_pack_conv_k4s1_full', 'dtype'),
    ('vv_pack_convT_k4s1_dense', 'dtype'), ('vv_pack_dense', 'dtype'),
    ('vv_conv3d_first_fwd_io', 'out_dtype'),
    ('vv_conv3d_k4s2_fwd', 'dtype'), ('vv_convT3d_k4s2_fwd', 'dtype'),
    ('vv_conv3d_k4s2_fwd_io', 'dtype'), ('vv_conv3d_k4s2_fwd_io', 'out_dtype'),
    ('vv_convT3d_k4s2_fwd_io', 'dtype'), ('vv_convT3d_k4s2_fwd_io', 'out_dtype'),
    ('vv_dense_fwd', 'dtype'), ('vv_dense_fwd', 'out_dtype'),
    ('vv_conv3d_k4s2_direct_fwd_io', 'out_dtype'), ('vv_conv3d_k4s2_direct_fp8_fwd', 'out_dtype'), ('vv_convT3d_k4s2_direct_fp8_fwd', 'out_dtype'),
    ('vv_convT3d_final_bce_fwd', 'dtype'), ('vv_convT3d_final_bce_metrics_fwd', 'dtype'),
    ('vv_convert', 'src_dtype'), ('vv_convert', 'dst_dtype'),
)

# The single-type (bf16) layer entries have no dtype check of their own: `dtype` is an argument of their `*_supported` predicate, and what
# that refuses is VV_ERR_SHAPE.  (entry, parameter) -> the codes that come back as VV_ERR_SHAPE instead of VV_ERR_DTYPE.
# vv_conv3d_k4s2_direct_fwd passes dtype on as out_dtype too, whose check comes first: only VV_FP8 gets as far as the predicate.
_ALL = UNKNOWN + (VV_FP8,)
SHAPE_REFUSED = {
    ('vv_conv3d_k4s2_direct_fwd', 'dtype'): (VV_FP8,), ('vv_conv3d_k4s2_direct_fwd_io', 'dtype'): _ALL,
    ('vv_convT3d_k4s2_direct_fwd', 'dtype'): _ALL,
    ('vv_conv3d_k4s2_skip_fwd', 'dtype'): _ALL, ('vv_convT3d_k4s2_skip_fwd', 'dtype'): _ALL,
    ('vv_convT3d_k4s2_whole_fwd', 'dtype'): _ALL, ('vv_convT3d_k4s2_whole_stats_fwd', 'dtype'): _ALL,
    ('vv_conv3d_k4s2_pos_fwd', 'dtype'): _ALL, ('vv_convT3d_k4s2_pos_fwd', 'dtype'): _ALL,
    ('vv_latent_tail_fwd', 'dtype'): _ALL, ('vv_conv_pos_latent_tail_fwd', 'dtype'): _ALL,
}

_DIRECT = dict(batch=1, side=16, cin=64, cout=128, act=0)
_DIRECT_T = dict(batch=1, side=8, cin=128, cout=64, act=0)
_TAIL = dict(batch=1, E=64, L=32, lin=32, n1=16, variational=1, act=0, dtype=VV_BF16)
_MM = dict(batch=1, lc=1, li=1, classes=1, act_dtype=VV_F32)
# entry -> its valid scalars (dtype parameters included); float scalars are 0.5, pointers the dummy buffer, streams NULL.
# 'null': pointers passed as NULL.
RECIPES = {
    'vv_pack_conv_k4': dict(cin=1, cout=1, dtype=VV_F32),
    'vv_pack_convT_k4s2': dict(cin=1, cout=1, dtype=VV_F32),
    'vv_pack_conv_k4s1_meanpool': dict(side=1, cin=1, cout=1, dtype=VV_F32),
    'vv_pack_conv_k4s1_full': dict(side=1, cin=1, cout=1, dtype=VV_F32),
    'vv_pack_convT_k4s1_dense': dict(side=1, cin=1, cout=1, dtype=VV_F32),
    'vv_pack_dense': {'in': 1, 'out': 1, 'dtype': VV_F32},
    'vv_conv3d_first_fwd': dict(batch=1, side=2, cout=4, act=0, dtype=VV_F32),
    'vv_conv3d_first_fwd_io': dict(batch=1, side=2, cout=4, act=0, dtype=VV_BF16, out_dtype=VV_BF16),
    'vv_conv3d_k4s2_fwd': dict(batch=1, side=2, cin=64, cout=8, act=0, dtype=VV_BF16),
    'vv_conv3d_k4s2_fwd_io': dict(batch=1, side=2, cin=64, cout=8, act=0, dtype=VV_BF16, out_dtype=VV_BF16),
    'vv_convT3d_k4s2_fwd': dict(batch=1, side=1, cin=64, cout=8, act=0, dtype=VV_BF16),
    'vv_convT3d_k4s2_fwd_io': dict(batch=1, side=1, cin=64, cout=8, act=0, dtype=VV_BF16, out_dtype=VV_BF16),
    'vv_conv3d_k4s2_direct_fwd': dict(_DIRECT, dtype=VV_BF16),
    'vv_conv3d_k4s2_direct_fwd_io': dict(_DIRECT, dtype=VV_BF16, out_dtype=VV_BF16),
    'vv_conv3d_k4s2_direct_fp8_fwd': dict(_DIRECT, out_dtype=VV_BF16),
    'vv_convT3d_k4s2_direct_fwd': dict(_DIRECT_T, dtype=VV_BF16),
    'vv_convT3d_k4s2_direct_fp8_fwd': dict(_DIRECT_T, out_dtype=VV_BF16),
    'vv_conv3d_k4s2_skip_fwd': dict(batch=1, side=8, cin=64, cout=64, act=0, dtype=VV_BF16),
    'vv_convT3d_k4s2_skip_fwd': dict(batch=1, side=4, cin=64, cout=128, act=0, dtype=VV_BF16),
    'vv_convT3d_k4s2_whole_fwd': dict(_DIRECT_T, dtype=VV_BF16),
    'vv_convT3d_k4s2_whole_stats_fwd': dict(batch=1, side=8, cin=128, cout=64, dtype=VV_BF16),
    'vv_conv3d_k4s2_pos_fwd': dict(batch=1, side=4, cin=64, cout=8, act=0, dtype=VV_BF16),
    'vv_convT3d_k4s2_pos_fwd': dict(batch=1, side=2, cin=64, cout=8, act=0, dtype=VV_BF16),
    'vv_dense_fwd': dict(m=1, n=8, k=8, act=0, dtype=VV_BF16, out_dtype=VV_BF16),
    'vv_latent_tail_fwd': dict(_TAIL, K5=64),
    'vv_conv_pos_latent_tail_fwd': dict(_TAIL, cin4=64, cout4=256),
    'vv_reparam_kl_fwd': dict(batch=1, latent=1, act_dtype=VV_F32),
    'vv_convT3d_final_bce_fwd': dict(batch=1, side=4, cin=64, dtype=VV_F32),
    'vv_convT3d_final_bce_metrics_fwd': dict(batch=1, side=4, cin=64, dtype=VV_F32),
    'vv_sample_latents': dict(objects=1, samples=1, latent=1, act_dtype=VV_F32),
    'vv_convT3d_final_mean_fwd': dict(objects=1, samples=1, side=4, cin=64, dtype=VV_F32),
    'vv_latent_mask_fill': dict(classes=1, batch=1, latent=1, act_dtype=VV_F32),
    'vv_latent_correct': dict(batch=1, latent=1, act_dtype=VV_F32),
    'vv_mm_latent_eval': dict(_MM, insts=1, null=('mask', 'eps2')),
    'vv_mm_latent_eval_host': dict(_MM, insts=1, null=('mask', 'eps2')),
    'vv_mm_latent_train_fwd': _MM,
    'vv_mm_latent_train_fwd_host': _MM,
    'vv_pack_conv2d': dict(ksize=1, cin=3, cout=1, dtype=VV_F32),
    'vv_conv2d_fwd': dict(batch=1, rows=1, cols=1, cin=32, cout=1, ksize=1, act=0, dtype=VV_F32, out_dtype=VV_F32),
    'vv_conv2d_ex_fwd': dict(batch=1, rows=1, cols=1, cin=32, cout=1, ksize=1, stride=1, act=0, dtype=VV_F32, out_dtype=VV_F32),
    'vv_maxpool2d_same_fwd': dict(batch=1, rows=1, cols=1, channels=1, dtype=VV_F32),
    'vv_maxpool2d_s1_same_fwd': dict(batch=1, rows=1, cols=1, channels=1, dtype=VV_F32),
    'vv_bn_train_stats': dict(rows=1, channels=8, dtype=VV_F32),
    'vv_bn_act_fwd': dict(rows=1, channels=8, act=0, dtype=VV_F32),
    'vv_bn_act_bwd': dict(rows=1, channels=8, act=0, dtype=VV_F32),
    'vv_wgrad_dense': dict(rows=1, m=4, n=4, lda=4, a_dtype=VV_F32, g_dtype=VV_F32),
    'vv_wgrad_conv_k4s2': dict(batch=1, side=2, cin=64, cout=4, src_dtype=VV_F32, g_dtype=VV_F32),
    'vv_colsum': dict(rows=1, cols=1, dtype=VV_F32),
    'vv_convert': dict(n=1, src_dtype=VV_F32, dst_dtype=VV_F32),
}

# `*_supported` predicates: a shape they accept with VV_BF16; any other code, VV_FP8 included, answers 0
SUPPORTED = {
    'vv_conv3d_k4s2_direct_supported': dict(side=16, cin=64, cout=128, dtype=VV_BF16),
    'vv_convT3d_k4s2_direct_supported': dict(side=8, cin=128, cout=64, dtype=VV_BF16),
    'vv_conv3d_k4s2_skip_supported': dict(side=8, cin=64, cout=64, dtype=VV_BF16),
    'vv_convT3d_k4s2_skip_supported': dict(side=4, cin=64, cout=128, dtype=VV_BF16),
    'vv_convT3d_k4s2_whole_supported': dict(side=8, cin=128, cout=64, dtype=VV_BF16),
    'vv_conv3d_k4s2_pos_supported': dict(side=4, cin=64, cout=8, dtype=VV_BF16),
    'vv_convT3d_k4s2_pos_supported': dict(side=2, cin=64, cout=8, dtype=VV_BF16),
    'vv_latent_tail_supported': dict(K5=64, E=64, L=32, lin=32, n1=16, variational=1, dtype=VV_BF16),
    'vv_conv_pos_latent_tail_supported': dict(cin4=64, cout4=256, E=64, L=32, lin=32, n1=16, variational=1, dtype=VV_BF16),
    'vv_conv2d_supported': dict(ksize=1, cin=32, cout=1, dtype=VV_BF16, out_dtype=VV_BF16),
    'vv_conv2d_ex_supported': dict(ksize=1, stride=1, cin=32, cout=1, dtype=VV_BF16, out_dtype=VV_BF16),
}
# size queries that answer 0 for a code they do not admit, at a shape where an admitted code gives a size (one row, K cut into shares)
BYTES = {
    'vv_conv2d_packed_bytes': dict(ksize=1, cin=32, cout=1, dtype=VV_BF16),
    'vv_conv2d_workspace_bytes': dict(batch=1, rows=1, cols=1, ksize=3, cin=1024, cout=64, dtype=VV_BF16),
    'vv_conv2d_ex_workspace_bytes': dict(batch=1, rows=1, cols=1, ksize=3, stride=1, cin=1024, cout=64, dtype=VV_BF16),
}
# size queries that check nothing: `dtype` only picks the K chunk of the split-K plan, any other code counts as float32
NO_REFUSAL = ('vv_conv3d_k4s2_workspace_bytes', 'vv_convT3d_k4s2_workspace_bytes', 'vv_dense_workspace_bytes')


@pytest.fixture(scope='module')
def lib():
    from voxvae import build as vb
    vb.build()
    from voxvae import lib as L
    return L.load()


@pytest.fixture(scope='module')
def mem():
    raw = ctypes.create_string_buffer(4096 + 16)
    return raw, ctypes.c_void_p((ctypes.addressof(raw) + 15) & ~15)       # (keep-alive, 16-byte aligned)


def _dtype_params(proto):
    return [p[0] for p in proto.params if p[0].endswith('dtype')]


def _args(lib, proto, recipe, p, **override):
    argtypes = getattr(lib, proto.name).argtypes
    out = []
    for (name, is_ptr, _), ctype in zip(proto.params, argtypes):
        if name in override:
            out.append(override[name])
        elif is_ptr:
            out.append(None if name in ('stream', 'hip_stream') or name in recipe.get('null', ()) else p)
        elif name in ('workspace_bytes', 'stats_bytes'):
            out.append(BIG)
        elif ctype in (ctypes.c_float, ctypes.c_double):
            out.append(0.5)
        else:
            out.append(recipe[name])             # KeyError: the recipe misses a scalar of the header
    return out


def test_every_entry_with_a_dtype_parameter_is_covered():
    with_dtype = {n for n, pr in header_protos().items() if _dtype_params(pr)}
    tables = [set(RECIPES), set(SUPPORTED), set(BYTES), set(NO_REFUSAL)]
    assert sum(len(t) for t in tables) == len(set().union(*tables)), 'an entry is in two tables'
    assert with_dtype == set().union(*tables)
    pairs = {(n, q) for n in RECIPES for q in _dtype_params(header_protos()[n])}
    assert set(FP8_ADMITTED) <= pairs and len(set(FP8_ADMITTED)) == len(FP8_ADMITTED)
    assert set(SHAPE_REFUSED) <= pairs and not set(SHAPE_REFUSED) & set(FP8_ADMITTED)


@pytest.mark.parametrize('name', sorted(RECIPES))
def test_entry_refuses_codes_outside_its_set(lib, mem, name):
    proto, recipe, p = header_protos()[name], RECIPES[name], mem[1]
    assert proto.ret == 'int'
    for q in _dtype_params(proto):
        for code in UNKNOWN + (() if (name, q) in FP8_ADMITTED else (VV_FP8,)):
            want = ERR_SHAPE if code in SHAPE_REFUSED.get((name, q), ()) else ERR_DTYPE
            got = getattr(lib, name)(*_args(lib, proto, recipe, p, **{q: code}))
            assert got == want, '%s(%s = %d) returned %d, not %d' % (name, q, code, got, want)


def test_convert_refuses_fp8_to_fp8(lib, mem):
    """Both codes are admitted one by one; the pair has no kernel."""
    assert lib.vv_convert(mem[1], mem[1], 8, VV_FP8, VV_FP8, None) == ERR_DTYPE


def test_single_channel_wgrad_source_is_float32_only(lib, mem):
    proto = header_protos()['vv_wgrad_conv_k4s2']
    recipe = dict(RECIPES['vv_wgrad_conv_k4s2'], cin=1)
    assert lib.vv_wgrad_conv_k4s2(*_args(lib, proto, recipe, mem[1], src_dtype=VV_BF16)) == ERR_DTYPE


@pytest.mark.parametrize('name', sorted(SUPPORTED))
def test_supported_predicates_answer_no(lib, name):
    proto, recipe = header_protos()[name], SUPPORTED[name]
    for q in _dtype_params(proto):
        for code in UNKNOWN + (VV_FP8,):
            assert getattr(lib, name)(*_args(lib, proto, recipe, None, **{q: code})) == 0, (name, q, code)


@pytest.mark.parametrize('name', sorted(BYTES))
def test_size_queries_answer_zero(lib, name):
    proto, recipe = header_protos()[name], BYTES[name]
    assert getattr(lib, name)(*_args(lib, proto, recipe, None)) > 0          # no pointers: a query launches nothing
    for code in UNKNOWN + (VV_FP8,):
        assert getattr(lib, name)(*_args(lib, proto, recipe, None, dtype=code)) == 0, (name, code)
