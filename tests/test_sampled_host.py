"""CPU tests of the sampled-mean reconstruction's C ABI (final_mean.hip): the entries exist and are bound, arguments are validated before
any launch, and the workspace keeps the conditions the design sets (no growth with K for K >= 8, at most 8 float32 grids per object)."""
import ctypes

import pytest

ENTRIES = ('vv_sample_latents', 'vv_convT3d_final_mean_workspace_bytes', 'vv_convT3d_final_mean_fwd')
OK, ERR_NULL, ERR_SHAPE, ERR_DTYPE, ERR_ALIGN, ERR_WORKSPACE = 0, -1, -2, -3, -4, -5


@pytest.fixture(scope='module')
def lib():
    from voxvae import build as vb
    vb.build()
    from voxvae import lib as L
    return L.load()


@pytest.fixture(scope='module')
def mem():
    """Host memory standing in for device pointers: every call below is refused by the argument checks, nothing is launched."""
    raw = ctypes.create_string_buffer(4096 + 16)
    base = (ctypes.addressof(raw) + 15) & ~15
    return raw, ctypes.c_void_p(base), ctypes.c_void_p(base + 4)       # (keep-alive, 16-byte aligned, misaligned)


def test_entries_exported_and_bound(lib):
    from voxvae import lib as L
    raw = ctypes.CDLL(L.LIB_PATH)
    hooks = ctypes.CDLL(L.HOOKS_LIB_PATH)
    for name in ENTRIES:
        assert hasattr(raw, name), 'libvoxvae.so does not export %s' % name
        assert hasattr(hooks, name), 'libvoxvae_hooks.so does not export %s' % name
        assert name in L.SIGNATURES
    assert len(L.SIGNATURES['vv_sample_latents'][1]) == 10
    assert len(L.SIGNATURES['vv_convT3d_final_mean_workspace_bytes'][1]) == 3
    assert len(L.SIGNATURES['vv_convT3d_final_mean_fwd'][1]) == 15
    assert lib.vv_abi_version() == 1


def _fwd(lib, x, w, target, mean, stats, objects=2, samples=4, side=8, cin=64, dtype=1, ws=None, ws_bytes=None):
    if ws_bytes is None:
        ws_bytes = lib.vv_convT3d_final_mean_workspace_bytes(max(objects, 1), max(samples, 1), side)
    return lib.vv_convT3d_final_mean_fwd(x, w, target, mean, stats, objects, samples, side, cin, 0.6, 1e-7, dtype, ws, ws_bytes, None)


def test_final_mean_validates_before_any_launch(lib, mem):
    _, p, odd = mem
    assert _fwd(lib, None, p, None, p, None, ws=p) == ERR_NULL
    assert _fwd(lib, p, None, None, p, None, ws=p) == ERR_NULL
    assert _fwd(lib, p, p, None, None, None, ws=p) == ERR_NULL
    assert _fwd(lib, p, p, p, p, None, ws=p) == ERR_NULL                # a target without stats
    assert _fwd(lib, p, p, None, p, p, ws=p) == ERR_NULL                # stats without a target
    for samples in (0, 1025):
        assert _fwd(lib, p, p, None, p, None, samples=samples, ws=p) == ERR_SHAPE
    assert _fwd(lib, p, p, None, p, None, cin=32, ws=p) == ERR_SHAPE
    assert _fwd(lib, p, p, None, p, None, objects=0, ws=p) == ERR_SHAPE
    assert _fwd(lib, p, p, None, p, None, objects=64, samples=1024, ws=p) == ERR_SHAPE      # objects * samples > 65535
    for side in (2, 12):
        assert _fwd(lib, p, p, None, p, None, side=side, ws=p, ws_bytes=1 << 30) == ERR_SHAPE
    assert _fwd(lib, p, p, None, p, None, dtype=2, ws=p) == ERR_DTYPE                         # VV_FP8
    assert _fwd(lib, p, p, None, p, None, dtype=7, ws=p) == ERR_DTYPE
    assert _fwd(lib, odd, p, None, p, None, ws=p) == ERR_ALIGN
    assert _fwd(lib, p, p, None, odd, None, ws=p) == ERR_ALIGN
    assert _fwd(lib, p, p, odd, p, p, ws=p) == ERR_ALIGN
    assert _fwd(lib, p, p, None, p, None, ws=None) == ERR_WORKSPACE
    assert _fwd(lib, p, p, None, p, None, ws=odd) == ERR_WORKSPACE
    need = lib.vv_convT3d_final_mean_workspace_bytes(2, 4, 8)
    assert _fwd(lib, p, p, None, p, None, ws=p, ws_bytes=need - 1) == ERR_WORKSPACE


def test_sample_latents_validates_before_any_launch(lib, mem):
    _, p, _ = mem
    f = lib.vv_sample_latents
    assert f(None, p, p, p, None, 0, 2, 4, 64, None) == ERR_NULL
    assert f(p, None, p, p, None, 0, 2, 4, 64, None) == ERR_NULL
    assert f(p, p, None, p, None, 0, 2, 4, 64, None) == ERR_NULL
    assert f(p, p, p, None, None, 1, 2, 4, 64, None) == ERR_NULL       # neither output
    assert f(p, p, p, None, p, 2, 2, 4, 64, None) == ERR_DTYPE         # VV_FP8 latents do not exist
    for shape in ((0, 4, 64), (2, 0, 64), (2, 4, 0)):
        assert f(p, p, p, p, None, 0, *shape, None) == ERR_SHAPE


@pytest.mark.parametrize('side', [4, 8, 16, 32])
@pytest.mark.parametrize('B', [1, 8, 256])
def test_workspace_conditions(lib, B, side):
    ws = lib.vv_convT3d_final_mean_workspace_bytes
    grid = (2 * side) ** 3 * 4
    bound = 8 * B * grid + lib.vv_convT3d_final_bce_workspace_bytes(B * 8, side)
    assert ws(B, 64, side) == ws(B, 8, side)                          # no growth with K for K >= 8
    assert ws(B, 1024, side) == ws(B, 8, side)
    for K in (1, 2, 3, 7, 8, 32, 64, 1024):
        n = ws(B, K, side)
        assert 0 < n <= bound, (B, K, side, n, bound)
        assert n >= B * grid                                           # at least the one grid of sums the finish kernel reads
