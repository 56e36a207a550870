"""CPU tests of the counter-based keep masks (csrc/keep_mask.h through vv_keep_mask_host): a numpy restatement of Philox4x32-10 and the
keep rule, written here, reproduces the published known answers and the library's masks bit for bit; determinism, separation of
offsets and seeds, the keep fraction, the refusals that need no GPU, the ABI of the three entries, and KeepMasks' offset layout."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, 'include', 'voxvae.h')
M0, M1, W0, W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85
MASK32 = np.uint64(0xFFFFFFFF)
ENTRIES = {'vv_keep_mask': 7, 'vv_keep_mask_host': 6, 'vv_mask_scale': 7}
SHAPES = [(1, 1), (1, 3), (3, 5), (5, 64), (256, 64)]
RATES = [0.0, 0.1, 0.35, 0.5, 0.9, float(np.nextafter(np.float32(1), np.float32(0)))]
SEEDS = [0, 1, 2 ** 63 + 5]
OFFSETS = [0, 1, 2 ** 40, 2 ** 56 + 7]


# ------------------------------------------------------------------------------------------------ the restatement
def philox4x32_10(counter, key):
    """counter: four uint64 arrays holding 32-bit words (broadcastable), key: two.  -> four uint64 arrays of 32-bit words."""
    c = [np.asarray(w, dtype=np.uint64) & MASK32 for w in counter]
    c = list(np.broadcast_arrays(*c))
    k0, k1 = (np.uint64(int(k) & 0xFFFFFFFF) for k in key)
    for _ in range(10):
        p0, p1 = np.uint64(M0) * c[0], np.uint64(M1) * c[2]          # 32 x 32 -> 64 bits: no overflow in uint64
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ k0, p1 & MASK32, (p0 >> np.uint64(32)) ^ c[3] ^ k1, p0 & MASK32]
        k0, k1 = (k0 + np.uint64(W0)) & MASK32, (k1 + np.uint64(W1)) & MASK32
    return c


def restated_mask(B, Lz, rate, seed, offset):
    n = B * Lz
    blk = np.arange((n + 3) // 4, dtype=np.uint64)
    words = philox4x32_10((blk & MASK32, blk >> np.uint64(32), np.uint64(offset & 0xFFFFFFFF), np.uint64(offset >> 32)),
                          (seed & 0xFFFFFFFF, seed >> 32))
    w = np.stack(words, axis=1).reshape(-1)[:n]                       # element e: word e & 3 of block e >> 2
    u = (w >> np.uint64(8)).astype(np.float32) * np.float32(2.0 ** -24)
    assert u.dtype == np.float32
    return (u >= np.float32(rate)).astype(np.float32).reshape(B, Lz)


# ------------------------------------------------------------------------------------------------ the library
@pytest.fixture(scope='module')
def lib():
    from voxvae import build as vb
    vb.build()
    from voxvae import lib as L
    return L.load()


def host_mask(lib, B, Lz, rate, seed, offset):
    keep = np.full((B, Lz), np.nan, dtype=np.float32)
    rc = lib.vv_keep_mask_host(keep.ctypes.data_as(ctypes.c_void_p), B, Lz, rate, seed, offset)
    assert rc == 0, rc
    return keep


def test_restatement_reproduces_the_known_answers():
    cases = [((0, 0, 0, 0), (0, 0), '6627e8d5 e169c58d bc57ac4c 9b00dbd8'),
             ((0xffffffff,) * 4, (0xffffffff,) * 2, '408f276d 41c83b0e a20bc7c6 6d5451fd'),
             ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), 'd16cfe09 94fdcceb 5001e420 24126ea1')]
    for counter, key, want in cases:
        got = ' '.join('%08x' % int(w) for w in philox4x32_10([np.uint64(c) for c in counter], key))
        assert got == want, (counter, key, got)


@pytest.mark.parametrize('B,Lz', SHAPES)
def test_host_entry_equals_the_restatement_bit_for_bit(lib, B, Lz):
    for rate in RATES:
        for seed in SEEDS:
            for offset in OFFSETS:
                got, want = host_mask(lib, B, Lz, rate, seed, offset), restated_mask(B, Lz, rate, seed, offset)
                assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (B, Lz, rate, seed, offset)
                if rate == 0.0:
                    assert bool((got == 1.0).all())


def test_determinism_and_separation(lib):
    a = host_mask(lib, 256, 64, 0.5, 7, 0)
    assert np.array_equal(a, host_mask(lib, 256, 64, 0.5, 7, 0))
    other_offset, other_seed = host_mask(lib, 256, 64, 0.5, 7, 1), host_mask(lib, 256, 64, 0.5, 8, 0)
    assert not np.array_equal(a, other_offset) and not np.array_equal(a, other_seed)
    for b in (other_offset, other_seed):
        agree = float((a == b).mean())
        print('agreement %.4f' % agree)
        assert 0.45 <= agree <= 0.55, agree           # independent fair bits agree half the time; 16384 of them: sigma = 0.0039


@pytest.mark.parametrize('B,Lz', [(5, 64), (256, 64)])
def test_keep_fraction(lib, B, Lz):
    """|mean(keep) - (1 - rate)| <= 4 sigma of a Bernoulli mean over n draws.  The inputs are fixed, so this is no flaky test: the
    restatement's worst case over them is 2.38 sigma."""
    n, worst = B * Lz, 0.0
    for rate in (0.1, 0.35, 0.5, 0.9):
        r32 = float(np.float32(rate))
        sigma = np.sqrt(r32 * (1.0 - r32) / n)
        for seed in (1, 2, 3):
            for offset in (0, 1, 2):
                dev = abs(float(host_mask(lib, B, Lz, rate, seed, offset).mean(dtype=np.float64)) - (1.0 - r32))
                worst = max(worst, dev / sigma)
                assert dev <= 4.0 * sigma, (rate, seed, offset, dev / sigma)
    print('n = %d: worst deviation %.2f sigma' % (n, worst))


def test_refusals_need_no_gpu(lib):
    keep = np.zeros((2, 4), dtype=np.float32)
    p = keep.ctypes.data_as(ctypes.c_void_p)
    null, shape = -1, -2
    for fn, tail in ((lib.vv_keep_mask_host, ()), (lib.vv_keep_mask, (None,))):
        assert fn(None, 2, 4, 0.5, 0, 0, *tail) == null
        assert fn(p, 0, 4, 0.5, 0, 0, *tail) == shape
        assert fn(p, 2, 0, 0.5, 0, 0, *tail) == shape
        assert fn(p, -1, 4, 0.5, 0, 0, *tail) == shape
        for rate in (-0.1, 1.0, float('nan')):
            assert fn(p, 2, 4, rate, 0, 0, *tail) == shape, rate
    assert bool((keep == 0).all())                     # nothing was written
    x = np.ones((2, 4), dtype=np.float32)
    px, py = x.ctypes.data_as(ctypes.c_void_p), np.empty_like(x).ctypes.data_as(ctypes.c_void_p)
    assert lib.vv_mask_scale(None, p, 1.0, py, 2, 4, None) == null
    assert lib.vv_mask_scale(px, None, 1.0, py, 2, 4, None) == null
    assert lib.vv_mask_scale(px, p, 1.0, None, 2, 4, None) == null
    assert lib.vv_mask_scale(px, p, 1.0, py, 0, 4, None) == shape
    assert lib.vv_mask_scale(px, p, 1.0, py, 2, 0, None) == shape


def test_the_three_entries_are_declared_exported_and_bound(lib):
    from voxvae import build as vb
    from voxvae import lib as L
    src = re.sub(r'/\*.*?\*/', '', open(HEADER).read(), flags=re.S)
    nm = subprocess.run(['nm', '-D', '--defined-only', vb.LIB], capture_output=True, text=True).stdout
    for name, nargs in ENTRIES.items():
        m = re.search(r'\bint\s+%s\s*\(([^;]*?)\)\s*;' % name, src, flags=re.S)
        assert m, '%s is not declared in include/voxvae.h' % name
        params = [a.strip() for a in m.group(1).split(',') if a.strip()]
        assert len(params) == nargs == len(L.SIGNATURES[name][1]), (name, params)
        assert re.search(r' T %s$' % name, nm, flags=re.M), '%s is not exported' % name
        assert 'stream' not in [re.findall(r'\w+', a)[-1] for a in params], name      # new entries name it hip_stream
        assert not any(a.endswith('dtype') for a in params), name


def test_keepmasks_host_packs_kind_rank_and_step_into_the_offset(lib):
    from voxvae import masks as M
    assert M.pack_offset('dropout', 0, 0) == 0
    assert M.pack_offset('dropout', 0, 5) == 5
    assert M.pack_offset('dropout', 3, 0) == 3 << 40
    assert M.pack_offset('missing', 0, 0) == 1 << 56
    assert M.pack_offset('missing', 0xFFFF, 2 ** 40 - 1) == (1 << 56) | (0xFFFF << 40) | (2 ** 40 - 1)
    for bad in (('dropout', 1 << 16, 0), ('dropout', 0, 1 << 40), ('dropout', -1, 0)):
        with pytest.raises(ValueError):
            M.pack_offset(*bad)
    km = M.KeepMasks('cpu', seed=2 ** 63 + 5, rank=3)
    for kind, code in (('dropout', 0), ('missing', 1)):
        for step in (0, 1, 9):
            want = host_mask(lib, 5, 64, 0.35, 2 ** 63 + 5, (code << 56) | (3 << 40) | step)
            assert np.array_equal(km.host(kind, 5, 64, 0.35, step), want), (kind, step)
    assert km.steps == {'dropout': 0, 'missing': 0}     # the host twin does not advance the stream
    # without torch.distributed the rank is 0, and manual_seed supplies the seed
    M.manual_seed(11)
    try:
        auto = M.KeepMasks('cpu')
        assert (auto.rank, auto.seed) == (0, 11)
        assert np.array_equal(auto.host('missing', 3, 5, 0.5, 2), host_mask(lib, 3, 5, 0.5, 11, (1 << 56) | 2))
    finally:
        M.manual_seed(None)


def test_an_unset_seed_is_taken_once_from_np_random():
    from voxvae import masks as M
    M.manual_seed(None)
    try:
        np.random.seed(123)
        first = M.seed()
        np.random.seed(123)
        expect = int(np.random.randint(0, 2 ** 63 - 1, dtype=np.int64))
        assert first == expect and M.seed() == first     # the second call draws nothing
    finally:
        M.manual_seed(None)


def test_mask_source_switch():
    import voxvae
    assert voxvae.mask_source() in ('host', 'device')
    before = voxvae.mask_source()
    try:
        voxvae.set_mask_source('device')
        assert voxvae.mask_source() == 'device'
        with pytest.raises(ValueError):
            voxvae.set_mask_source('gpu')
    finally:
        voxvae.set_mask_source(before)
