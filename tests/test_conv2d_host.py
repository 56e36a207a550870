"""CPU tests of the 2D convolution's host side (csrc/conv2d.hip, csrc/conv2d_plan.h, voxvae/conv2d.py): the size queries are pure host
arithmetic, validation precedes any launch, the Python engine's plan / permutation / staleness key, and the MAC accounting."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

from _common import build_and_run_sanitized
import _conv2d_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32, BF16 = 0, 1
NULL, SHAPE, DTYPE = -1, -2, -3
DARKNET = [(3, 32, 3), (32, 64, 3), (64, 128, 3), (128, 64, 1), (64, 128, 3), (128, 256, 3), (256, 128, 1), (128, 256, 3), (256, 512, 3),
           (512, 256, 1), (256, 512, 3), (512, 256, 1), (256, 512, 3), (512, 1024, 3), (1024, 512, 1), (512, 1024, 3), (1024, 512, 1), (512, 1024, 3)]
HEAD = [(1024, 1024, 3), (1024, 1024, 3), (1024, 1024, 3), (1024, 245, 1)]


@pytest.fixture(scope='module')
def lib():
    from voxvae import build as vb
    vb.build()
    from voxvae import lib as L
    return L.load()


def test_supported_and_packed_bytes(lib):
    for cin, cout, k in DARKNET + HEAD:
        for dt, size in ((F32, 4), (BF16, 2)):
            assert lib.vv_conv2d_supported(k, cin, cout, dt, F32) == 1 and lib.vv_conv2d_supported(k, cin, cout, dt, BF16) == 1
            kchunks, npad = -(-k * k * cin // 32), -(-cout // 64) * 64
            assert lib.vv_conv2d_packed_bytes(k, cin, cout, dt) == kchunks * npad * 32 * size
    assert lib.vv_conv2d_packed_bytes(3, 3, 32, BF16) == 1 * 64 * 32 * 2              # K = 27 in one chunk, 32 channels padded to 64
    assert lib.vv_conv2d_packed_bytes(1, 1024, 245, F32) == 32 * 256 * 32 * 4
    for k, cin, cout, dt, odt in [(2, 32, 32, 0, 0), (5, 32, 32, 0, 0), (3, 48, 32, 0, 0), (3, 16, 32, 0, 0), (3, 0, 32, 0, 0), (3, 32, 0, 0, 0),
                                  (3, 32, 32, 2, 0), (3, 32, 32, 0, 2), (3, 32, 32, 7, 0)]:
        assert lib.vv_conv2d_supported(k, cin, cout, dt, odt) == 0, (k, cin, cout, dt, odt)
    assert lib.vv_conv2d_packed_bytes(2, 32, 32, F32) == 0
    for cout in (1, 31, 33, 245, 1000):
        assert lib.vv_conv2d_supported(1, 32, cout, BF16, F32) == 1


def test_split_schedule_and_workspace(lib):
    # one 13 x 13 frame through the head's 1024 -> 1024 k3: 3 x 16 tiles, 288 chunks -> ceil(512 / 48) = 11 shares
    assert lib.vv_conv2d_splits(1, 13, 13, 3, 1024, 1024) == 11
    assert lib.vv_conv2d_workspace_bytes(1, 13, 13, 3, 1024, 1024, BF16) == 11 * 169 * 1024 * 4
    # 72 frames of 8 x 8 (config 3): 72 x 16 tiles fill the device, no split, no workspace
    assert lib.vv_conv2d_splits(72, 8, 8, 3, 1024, 1024) == 1
    assert lib.vv_conv2d_workspace_bytes(72, 8, 8, 3, 1024, 1024, F32) == 0
    # the image layer has one form
    assert lib.vv_conv2d_splits(1, 416, 416, 3, 3, 32) == 1 and lib.vv_conv2d_splits(1, 2, 2, 3, 3, 32) == 1
    # a share is at least 4 chunks: k1 with cin 64 (2 chunks) never splits
    assert lib.vv_conv2d_splits(1, 13, 13, 1, 64, 128) == 1
    assert lib.vv_conv2d_splits(1, 13, 13, 1, 1024, 245) == 8                        # 3 x 4 tiles, 32 chunks
    # shares never exceed 32, tiles x shares reaches for 512 workgroups
    for cin, cout, k in DARKNET[1:] + HEAD:
        for B, g in ((1, 13), (1, 3), (4, 8), (72, 8)):
            s = lib.vv_conv2d_splits(B, g, g, k, cin, cout)
            assert 1 <= s <= 32 and s <= max(1, -(-k * k * cin // 32) // 4)
            assert lib.vv_conv2d_workspace_bytes(B, g, g, k, cin, cout, F32) == (s * B * g * g * cout * 4 if s > 1 else 0)
    # the slab size per row does not grow with the batch beyond the split count's fall: total bytes / (M * cout * 4) = splits, non-increasing
    prev = None
    for B in (1, 2, 4, 8, 16, 64, 128):
        s = lib.vv_conv2d_splits(B, 13, 13, 3, 512, 1024)
        assert prev is None or s <= prev
        prev = s
    assert lib.vv_conv2d_splits(0, 13, 13, 3, 512, 1024) == 0 and lib.vv_conv2d_splits(1, 13, 13, 2, 512, 1024) == 0


def _fwd(lib, x, w, y, batch=1, rows=4, cols=4, cin=32, cout=32, k=3, act=0, dt=F32, odt=F32, ws=None, ws_bytes=0):
    return lib.vv_conv2d_fwd(x, w, None, None, y, batch, rows, cols, cin, cout, k, act, 0.1, dt, odt, ws, ws_bytes, None)


@pytest.mark.skipif(torch.cuda.is_available(), reason='pointers that are never dereferenced: validation precedes the launch, so this runs only where no launch can follow')
def test_validation_precedes_the_launch(lib):
    p = ctypes.c_void_p(4096)                                   # non-null, 16-byte aligned, never dereferenced
    assert _fwd(lib, None, p, p) == NULL and _fwd(lib, p, None, p) == NULL and _fwd(lib, p, p, None) == NULL
    assert _fwd(lib, p, p, p, k=2) == SHAPE
    assert _fwd(lib, p, p, p, cin=48) == SHAPE
    assert _fwd(lib, p, p, p, rows=0) == SHAPE and _fwd(lib, p, p, p, cols=0) == SHAPE and _fwd(lib, p, p, p, batch=0) == SHAPE
    assert _fwd(lib, p, p, p, cout=0) == SHAPE
    assert _fwd(lib, p, p, p, act=9) == SHAPE
    assert _fwd(lib, p, p, p, dt=2) == DTYPE and _fwd(lib, p, p, p, odt=2) == DTYPE
    # a declared tensor past 2^31 - 1 elements: 2^16 x 2^10 rows x 32 channels = 2^31
    assert _fwd(lib, p, p, p, batch=1, rows=65536, cols=1024) == SHAPE
    assert _fwd(lib, p, p, p, batch=1 << 20, rows=1 << 10, cols=1 << 10) == SHAPE      # rows x cols x batch overflows int
    assert _fwd(lib, p, p, p, batch=4, rows=4096, cols=4096, cin=32, cout=64) == SHAPE    # the OUTPUT is the tensor past the limit
    assert lib.vv_pack_conv2d(None, p, 3, 32, 32, F32, None) == NULL and lib.vv_pack_conv2d(p, None, 3, 32, 32, F32, None) == NULL
    assert lib.vv_pack_conv2d(p, p, 2, 32, 32, F32, None) == SHAPE and lib.vv_pack_conv2d(p, p, 3, 48, 32, F32, None) == SHAPE
    assert lib.vv_maxpool2d_same_fwd(None, p, 1, 4, 4, 32, F32, None) == NULL and lib.vv_maxpool2d_same_fwd(p, None, 1, 4, 4, 32, F32, None) == NULL
    assert lib.vv_maxpool2d_same_fwd(p, p, 1, 0, 4, 32, F32, None) == SHAPE and lib.vv_maxpool2d_same_fwd(p, p, 1, 4, 4, 0, F32, None) == SHAPE
    assert lib.vv_maxpool2d_same_fwd(p, p, 1, 65536, 1024, 32, F32, None) == SHAPE
    assert lib.vv_maxpool2d_same_fwd(p, p, 1, 4, 4, 32, 2, None) == DTYPE
    # misaligned pointers and a missing workspace are refused too
    assert _fwd(lib, ctypes.c_void_p(4100), p, p) == -4
    assert _fwd(lib, p, p, p, rows=13, cols=13, cin=1024, cout=1024) == -5


def test_null_pointers_are_refused_everywhere(lib):
    """NULL is refused before anything else, with or without a GPU: nothing is launched."""
    assert _fwd(lib, None, None, None) == NULL
    assert lib.vv_pack_conv2d(None, None, 3, 32, 32, F32, None) == NULL
    assert lib.vv_maxpool2d_same_fwd(None, None, 1, 4, 4, 32, F32, None) == NULL


# ------------------------------------------------------------------------------------------------------------ the Python side
@pytest.mark.skipif(torch.cuda.is_available(), reason='checks the no-GPU failure mode')
def test_hip_engine_without_gpu_is_an_error():
    import voxvae
    from voxvae import lib as L
    import src.net_core.darknet as darknet
    with pytest.raises(L.VoxVaeError):
        darknet.Darknet19(name='b', activation='lrelu', engine='hip')
    with pytest.raises(L.VoxVaeError):
        darknet.head2D('h', (None, None, 64), 245, [64], [3], engine='hip')
    assert voxvae.image_engine() == 'torch'
    voxvae.set_image_engine('hip')
    try:
        with pytest.raises(L.VoxVaeError):
            darknet.Darknet19(name='b')
    finally:
        voxvae.set_image_engine('torch')
    with pytest.raises(ValueError):
        voxvae.set_image_engine('miopen')
    with pytest.raises(ValueError):
        darknet.Darknet19(name='b', engine='other')
    m = darknet.Darknet19(name='b', device='cpu')                         # the default: the stock path, no chain
    assert m._chain is None and m._engine == 'torch'


def test_layer_plan_of_the_modules():
    import src.net_core.darknet as darknet
    from voxvae import conv2d as C
    m = darknet.Darknet19(name='b', activation='lrelu', device='cpu')
    plan = C.module_plan(m)
    assert [s[0] for s in plan] == ['pool' if it == 'M' else 'conv' for it in darknet._Darknet19._PLAN]
    convs = [s for s in plan if s[0] == 'conv']
    assert [(s[1].in_channels, s[1].out_channels, s[1].kernel_size[0]) for s in convs] == DARKNET
    assert all(s[3] == 'lrelu' and s[4] == pytest.approx(0.1) and s[2] is not None for s in convs)
    shapes = C.plan_shapes(plan, 416, 416)
    assert shapes[0] == ('conv', 416, 416, 3, 32, 3) and shapes[1] == ('pool', 416, 416, 32, 32, 2) and shapes[-1] == ('conv', 13, 13, 512, 1024, 3)
    assert C.plan_shapes(plan, 96, 160)[-1][1:3] == (3, 5) and C.plan_shapes(plan, 65, 33)[-1][1:3] == (3, 2)     # ceil at every pool
    h = darknet.head2D('h', (None, None, 1024), 245, [1024, 1024, 1024], [3, 3, 3], activation='elu', device='cpu')
    hp = C.module_plan(h)
    assert [(s[1].in_channels, s[1].out_channels, s[1].kernel_size[0]) for s in hp] == HEAD
    assert [s[3] for s in hp] == ['elu', 'elu', 'elu', None] and hp[-1][2] is None


def test_keras_permutation():
    from voxvae import conv2d as C
    w = torch.arange(5 * 4 * 3 * 3, dtype=torch.float32).reshape(5, 4, 3, 3)          # [cout, cin, kr, kc]
    k = C.keras_kernel(w).numpy()
    assert k.shape == (3, 3, 4, 5) and k.flags['C_CONTIGUOUS']
    want = np.empty((3, 3, 4, 5), dtype=np.float32)
    for co in range(5):
        for ci in range(4):
            for tr in range(3):
                for tc in range(3):
                    want[tr, tc, ci, co] = w[co, ci, tr, tc]
    assert np.array_equal(k, want)
    # and it is the layout the float64 definition takes: conv2d_ref(x, keras) = torch's own convolution with the OIHW weight
    x = np.random.default_rng(0).standard_normal((1, 4, 5, 4)).astype(np.float32)
    ref = torch.nn.functional.conv2d(torch.from_numpy(x).double().permute(0, 3, 1, 2), w.double(), padding=1).permute(0, 2, 3, 1).numpy()
    assert np.abs(R.conv2d_ref(x, k)[0] - ref).max() < 1e-9
    assert np.abs(R.conv2d_direct(x, k) - ref).max() < 1e-9


def test_version_key_sees_every_kind_of_update(tmp_path):
    import src.net_core.darknet as darknet
    from voxvae import conv2d as C
    m = darknet.head2D('h', (None, None, 32), 8, [32], [3], device='cpu')
    tensors = list(m.parameters()) + list(m.buffers())
    k0 = C.version_key(tensors)
    assert C.version_key(tensors) == k0
    m(np.zeros((1, 2, 2, 32), np.float32), training=False)
    assert C.version_key(tensors) == k0                                            # an inference call changes nothing
    opt = torch.optim.Adam(m.parameters(), lr=1e-3)
    m(np.ones((2, 2, 2, 32), np.float32), training=True).sum().backward()
    k1 = C.version_key(tensors)
    assert k1 != k0                                                                # the training forward moved the running statistics
    opt.step()
    k2 = C.version_key(tensors)
    assert k2 != k1
    m.save_weights(str(tmp_path / 'w'))
    m.load_weights(str(tmp_path / 'w'))
    assert C.version_key(tensors) != k2
    assert all(a is b for a, b in zip(tensors, list(m.parameters()) + list(m.buffers())))      # still the same tensor objects


def test_reference_helpers():
    x = np.arange(2 * 5 * 7 * 2, dtype=np.float64).reshape(2, 5, 7, 2) - 60
    p = R.pool_ref(x)
    assert p.shape == (2, 3, 4, 2) and p[0, 2, 3, 0] == x[0, 4, 6, 0] and p[0, 0, 0, 1] == x[0, 1, 1, 1] and p[1, 2, 0, 0] == x[1, 4, 1, 0]
    assert np.array_equal(R.pool_ref(x[:, :1, :1]), x[:, :1, :1])
    xi, wk = np.random.default_rng(1).standard_normal((2, 5, 7, 32)), np.random.default_rng(2).standard_normal((3, 3, 32, 8))
    assert np.abs(R.conv2d_ref(xi, wk)[0] - R.conv2d_direct(R.round_to(xi, 'f32'), R.round_to(wk, 'f32'))).max() < 1e-12
    s, t = R.fold_ref([2.0], [1.0], [3.0], [4.0 - 1e-3])
    assert s[0] == pytest.approx(1.0) and t[0] == pytest.approx(-2.0)
    assert R.round_to([1.0 + 2.0 ** -9], 'bf16')[0] == 1.0 and R.round_to([1.0 + 2.0 ** -9], 'f32')[0] == 1.0 + 2.0 ** -9


def test_image_encoder_mac_accounting():
    from voxvae import workload as W
    lm = W.image_encoder_macs(416, 416)
    d = {n: (v, dn) for n, v, dn in lm}
    assert len(lm) == 18 + 4
    assert d['B1'] == ((3 * 416 - 2) ** 2 * 3 * 32, 416 * 416 * 27 * 32)               # k3: 3n - 2 (output, tap) pairs per axis
    assert d['B18'] == (37 * 37 * 512 * 1024, 169 * 9 * 512 * 1024)
    assert d['H1'] == (37 * 37 * 1024 * 1024, 169 * 9 * 1024 * 1024) and d['HL'] == (169 * 1024 * 245,) * 2
    assert d['B4'] == (104 * 104 * 128 * 64,) * 2                                      # a 1x1 layer has no padding
    back = sum(dn for n, _, dn in lm if n[0] == 'B')
    assert abs(back - 9.45e9) < 0.01e9                                                 # "about 9 G MAC"
    assert abs(sum(dn for n, _, dn in lm if n[0] == 'H') - 4.83e9) < 0.01e9            # "about 5 G MAC"
    lm = W.image_encoder_macs(256, 256, head=None)
    assert len(lm) == 18 and lm[-1] == ('B18', 22 * 22 * 512 * 1024, 64 * 9 * 512 * 1024)
    assert lm[0][2] == 256 * 256 * 27 * 32
    assert W.image_encoder_macs(65, 33, head=None)[-1][2] == 3 * 2 * 9 * 512 * 1024
    assert W.DARKNET19_PLAN == __import__('src.net_core.darknet', fromlist=['x'])._Darknet19._PLAN


@pytest.mark.skipif(torch.cuda.is_available(), reason='sanitizer programs run on CPU-only machines')
def test_plan_header_under_the_host_sanitizers(tmp_path):
    """csrc/conv2d_plan.h compiles for the host: the row split, tap validity, the tap offset and the split-K schedule run in a stand-alone
    program under the address and undefined-behaviour sanitizers (nothing loaded into Python is run under a sanitizer)."""
    build_and_run_sanitized('conv2d_plan_main.cpp', tmp_path, 'conv2d_plan_main')
