"""CPU tests of the host-side logic around the hot path: the dataset-loader contract, the gradient buckets of the
data-parallel training path under a real 2-rank gloo group, and the training oracle's forward against the numpy
definition oracle."""
import os
import sys

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, 'anytime-3d-reconstruction_amd')


def test_dataset_loader_contract():
    from src.dataset_loader.modelnet_dataset import dataLoader
    np.random.seed(0)
    dl = dataLoader(data_path='synthetic:50:16', trainortest='test')
    assert dl.dataLength == 50 and dl.epoch == 0 and dl.batchStart == 0
    b = dl.getNextBatch(batchSize=8)
    assert set(b) == {'input_images', 'class_list', 'inst_list'}
    assert b['input_images'].shape == (8, 16, 16, 16, 1) and b['input_images'].dtype == np.float32
    assert b['class_list'].shape == (8, 40) and np.all(b['class_list'].sum(-1) == 1)
    assert dl.batchStart == 8
    seen = [b['inst_list'].ravel()]
    for _ in range(5):
        seen.append(dl.getNextBatch(8)['inst_list'].ravel())
    assert dl.epoch == 0 and len(np.unique(np.concatenate(seen))) == 48       # a shuffled permutation, no repeats
    dl.getNextBatch(8)                                                        # 48 + 8 > 50 -> new epoch, reshuffle
    assert dl.epoch == 1 and dl.batchStart == 8


def test_dataset_loader_reads_reference_layout(tmp_path):
    from src.dataset_loader.modelnet_dataset import dataLoader
    d = tmp_path / '32to64_4rot_64sqr' / 'test'
    d.mkdir(parents=True)
    for i in range(5):
        np.save(d / ('%dFull.npy' % i), np.full((3, 8, 8, 8, 1), i, np.float32))
        np.save(d / ('%dClass.npy' % i), np.eye(40, dtype=np.float32)[[i, i, i]])
        np.save(d / ('%dInst.npy' % i), np.arange(3, dtype=np.float32).reshape(3, 1))
    dl = dataLoader(data_path=str(tmp_path), trainortest='test')
    assert dl.dataLength == 15
    b = dl.getNextBatch(15)
    assert sorted(np.unique(b['input_images'])) == [0, 1, 2, 3, 4]


def test_entry_config_is_the_reference_literal():
    sys.path.insert(0, PKG)
    import _entry_common as C
    cfg = C.make_config(64, 64, True)
    # reference test_modelnet_VAE.py:169-192
    assert cfg == {
        'z_category_dim': 64,
        'encoder': {'name': 'encoder3D', 'input_shape': [64, 64, 64, 1], 'filter_num_list': [64, 128, 256, 512, 128],
                    'filter_size_list': [4, 4, 4, 4, 4], 'strides_list': [2, 2, 2, 2, 1], 'final_pool': 'average',
                    'activation': 'elu', 'final_activation': 'None'},
        'decoder': {'name': 'decoder', 'input_dim': 64, 'output_shape': [64, 64, 64, 1], 'filter_num_list': [512, 256, 128, 64, 1],
                    'filter_size_list': [4, 4, 4, 4, 4], 'strides_list': [1, 2, 2, 2, 2], 'activation': 'elu',
                    'final_activation': 'sigmoid'},
    }
    assert C.make_config(64, 64, False)['encoder']['filter_num_list'][-1] == 64     # AE: test_modelnet_AE.py:175


def _bucket_worker(rank, world, port, out):
    os.environ['MASTER_ADDR'] = '127.0.0.1'
    os.environ['MASTER_PORT'] = str(port)
    dist.init_process_group('gloo', rank=rank, world_size=world)
    sys.path.insert(0, PKG)
    from voxvae.train import GradBuckets
    shapes = [('dec/convT4/kernel', (4, 4, 4, 1, 64)), ('dec/bnT3/gamma', (64,)), ('enc/conv1/kernel', (4, 4, 4, 64, 128)),
              ('enc/bn0/beta', (63,)), ('enc/conv0/kernel', (4, 4, 4, 1, 64))]
    gb = GradBuckets(shapes, 'cpu', bucket_bytes=1 << 20)
    assert len(gb.buckets) >= 2                                   # the 2 MiB kernel forces a second bucket
    for i, (n, s) in enumerate(shapes):
        assert gb.views[n].shape == torch.Size(s) and gb.views[n].data_ptr() % 16 == 0
        gb.views[n].fill_(float(rank + 1) * (i + 1))
    gb.all_reduce()
    ok = all(torch.all(gb.views[n] == float(sum(r + 1 for r in range(world)) * (i + 1))) for i, (n, _) in enumerate(shapes))
    # overlapped form: a bucket is reduced the moment its last member is reported ready, in backward order
    for i, (n, s) in enumerate(shapes):
        gb.views[n].fill_(float(rank + 1) * (i + 1))
    gb.begin_step()
    launched = []
    for n, _ in shapes:
        gb.ready([n])
        launched.append(len(gb.launch_order))
    first_bucket = len(gb.members[0])
    ok = ok and launched[first_bucket - 2] == 0 and launched[first_bucket - 1] == 1 and gb.launch_order == sorted(gb.launch_order)
    gb.finish()
    ok = ok and len(gb.launch_order) == len(gb.buckets)
    ok = ok and all(torch.all(gb.views[n] == float(sum(r + 1 for r in range(world)) * (i + 1))) for i, (n, _) in enumerate(shapes))
    out[rank] = bool(ok)
    dist.destroy_process_group()


def test_gradient_buckets_allreduce_gloo_world2():
    """The N>1 training path sums gradients with bucketed all-reduces: exercised with two real processes over gloo."""
    mgr = mp.Manager()
    out = mgr.dict()
    port = 29500 + (os.getpid() % 2000)
    mp.spawn(_bucket_worker, args=(2, port, out), nprocs=2, join=True)
    assert dict(out) == {0: True, 1: True}


def _bf16_bucket_worker(rank, world, port, out):
    os.environ['MASTER_ADDR'] = '127.0.0.1'
    os.environ['MASTER_PORT'] = str(port)
    dist.init_process_group('gloo', rank=rank, world_size=world)
    sys.path.insert(0, PKG)
    from voxvae.train import GradBuckets
    shapes = [('dec/convT4/kernel', (4, 4, 4, 1, 64)), ('dec/bnT3/gamma', (64,)), ('enc/conv1/kernel', (4, 4, 4, 64, 128)),
              ('enc/bn0/beta', (63,)), ('enc/conv0/kernel', (4, 4, 4, 1, 64))]
    res = {}
    for wire in ('f32', 'bf16'):
        gb = GradBuckets(shapes, 'cpu', bucket_bytes=1 << 20, wire=wire, world_size=world)
        assert all(b.numel() % (8 * world) == 0 for b in gb.buckets)
        g = torch.Generator().manual_seed(100 + rank)
        for n, s in shapes:
            gb.views[n].copy_(torch.randn(s, generator=g) * (10.0 ** ((hash(n) % 5) - 2)))
        mine = {n: gb.views[n].clone() for n, _ in shapes}
        gb.begin_step()
        for n, _ in shapes:
            gb.ready([n])
        gb.finish()
        res[wire] = {n: gb.views[n].clone() for n, _ in shapes}
        res[wire + '_bytes'] = gb.wire_bytes_per_step()
    ok = res['bf16_bytes'] * 2 == res['f32_bytes']
    # every rank holds the same bits; the bf16 form = round_bf16( sum_r float32(round_bf16(g_r)) ): checked exactly, and against f32
    gathered = [None] * world
    dist.all_gather_object(gathered, {n: mine[n] for n in mine})
    for n, _ in shapes:
        exact = sum(gathered[r][n].to(torch.bfloat16).float() for r in range(world)).to(torch.bfloat16).float()
        ok = ok and torch.equal(res['bf16'][n], exact)
        ref = res['f32'][n]
        ok = ok and torch.equal(ref, sum(gathered[r][n] for r in range(world)))
        denom = sum(gathered[r][n].abs() for r in range(world)).clamp_min(1e-30)
        ok = ok and float(((res['bf16'][n] - ref).abs() / denom).max()) <= 2.0 ** -7       # two roundings of 2^-9 relative each, with slack
    out[rank] = bool(ok)
    dist.destroy_process_group()


def test_gradient_buckets_bf16_wire_gloo_world2():
    """GradBuckets(wire='bf16'): bf16 on the wire, float32 accumulation (all-to-all -> float32 sum in rank order -> all-gather), half the
    bytes of the float32 all-reduce; two real processes over gloo, compared with the float32 path and with the exact formula."""
    mgr = mp.Manager()
    out = mgr.dict()
    port = 31500 + (os.getpid() % 2000)
    mp.spawn(_bf16_bucket_worker, args=(2, port, out), nprocs=2, join=True)
    assert dict(out) == {0: True, 1: True}


def test_training_oracle_forward_matches_numpy_oracle():
    """BN in training mode with batch statistics: the torch statement equals the numpy definition-level statement."""
    from oracle import numpy_oracle as no
    from oracle import torch_oracle as to
    from voxvae import synthetic as syn
    cfg = syn.make_config(16, 64, True)
    ep = syn.make_encoder_params(cfg['encoder'], nontrivial_affine=True)
    dp = syn.make_decoder_params(cfg['decoder'], nontrivial_affine=True)
    x, eps = syn.make_voxels(3, 16), syn.make_eps(3, 64)
    P = {('enc/' + k): to._t(v) for k, v in ep.items()}
    P.update({('dec/' + k): to._t(v) for k, v in dp.items()})
    kl, shape, p, stats = to.forward_train(cfg, P, to._t(x), to._t(x), to._t(eps))
    e, st = no.encoder3D_forward(cfg['encoder'], ep, x, training=True, return_stats=True)
    mu, lv = no.split_mean_logvar(e, 64)
    z = no.sampling(mu, lv, eps)
    lg, pr, st2 = no.decoder3D_forward(cfg['decoder'], dp, z, training=True, return_stats=True)
    np.testing.assert_allclose(p.numpy(), pr, rtol=0, atol=1e-12)
    assert abs(float(kl) - no.kl_loss(mu, lv, 0 * mu, 0 * lv).mean()) < 1e-12
    assert abs(float(shape) - no.binary_loss(pr, x.astype(np.float64), gamma=0.6).mean()) < 1e-8
    np.testing.assert_allclose(stats['enc/bn2'][1], st['bn2'][1], rtol=1e-12)
    np.testing.assert_allclose(stats['dec/bnT1'][0], st2['bnT1'][0], rtol=1e-10, atol=1e-14)


def test_adam_rule_of_training_oracle():
    """Keras Adam: first step moves each weight by lr * g / (|g| + eps*sqrt(1-b2)) ~ lr * sign(g)."""
    from oracle import torch_oracle as to
    from voxvae import synthetic as syn
    cfg = syn.make_config(16, 64, False)
    ep, dp = syn.make_encoder_params(cfg['encoder']), syn.make_decoder_params(cfg['decoder'], final_gain=2.0)
    x = syn.make_voxels(2, 16)
    r = to.fit_step(cfg, ep, dp, x, x, syn.make_eps(2, 64), lr=1e-3, variational=False)
    g = r['grads']['dec/convT4/kernel']
    step = r['params']['dec/convT4/kernel'] - dp['convT4/kernel']
    big = np.abs(g) > 1e-4 * np.abs(g).max()
    np.testing.assert_allclose(step[big], -1e-3 * np.sign(g[big]), rtol=2e-2)
    assert r['adam']['t'] == 1


def test_darknet19_and_head2d_shapes_and_keras_attributes():
    """src/net_core/darknet.py mirror (reference darknet.py:83-173), CPU torch: 5 ceil-mode poolings (MaxPool2D 'same'),
    1024 output channels, head = 1x1 conv + max pool to [B, output_dim], l2 terms only on the head's kernels."""
    import src.net_core.darknet as darknet
    bb = darknet.Darknet19(name='bb', device='cpu')
    assert bb.output_shape == (None, None, None, 1024)
    x = np.random.default_rng(0).random((2, 72, 40, 3)).astype('float32')
    f = bb(x)
    assert tuple(f.shape) == (2, 3, 2, 1024)                     # ceil(72/32), ceil(40/32)
    assert len([m for m in bb.modules() if m.__class__.__name__ == '_ConvBNAct']) == 18 and bb.losses == []
    hd = darknet.head2D('hd', bb.output_shape[1:], 32, [64], [3], last_pooling='max', device='cpu')
    o = hd(f)
    assert tuple(o.shape) == (2, 32) and not o.requires_grad
    ref_l2 = 0.0005 * float((hd.last.weight.detach() ** 2).sum())
    assert len(hd.losses) == 2 and abs(float(hd.losses[1].detach()) - ref_l2) <= 1e-6 * ref_l2
    o2 = hd(bb(x, training=True), training=True)
    assert o2.requires_grad and len(bb.trainable_variables) == 18 * 3
    # BatchNormalization defaults of Keras: epsilon 1e-3, momentum 0.99 (torch momentum 0.01)
    bn = bb.layers[0].bn
    assert bn.eps == 1e-3 and bn.momentum == 0.01


def test_pascal_synthetic_loader_contract():
    import src.dataset_loader.pascal3D as pascal3D
    ld = pascal3D.dataLoaderSingleObject(trainOrVal='val', Pascal3DDataPath='synthetic:10:16')
    inst, cls, s, c, img, vox = ld.getNextBatch(batchSizeof3DShape=4, imageSize=(48, 32), augmentation=False)
    assert img.shape == (4, 32, 48, 3) and img.dtype == np.float32 and vox.shape == (4, 16, 16, 16, 1)
    assert cls.shape == (4, 12) and np.all(cls.sum(1) == 1) and set(np.unique(vox)) <= {0.0, 1.0}
    np.testing.assert_allclose(s ** 2 + c ** 2, 1.0, atol=1e-6)
    for _ in range(2):
        ld.getNextBatch(batchSizeof3DShape=4, imageSize=(48, 32), augmentation=False)
    assert ld.epoch == 1 and ld.dataLength == 10
    with pytest.raises(FileNotFoundError):
        pascal3D.dataLoaderSingleObject(Pascal3DDataPath='/nonexistent')


def test_fp8_weight_quantisation_host_side():
    """'fp8' inference mode, host side (voxvae/engine.py:quant_fp8): per-output-channel scales keep every channel inside
    e4m3fn's range whatever its magnitude, and w ~= fp8(w / s) * s to 3 mantissa bits.  No GPU involved (the import of the
    engine module must not need one either)."""
    if not hasattr(torch, 'float8_e4m3fn'):
        pytest.skip('torch.float8_e4m3fn not available')
    from voxvae import engine as E
    rng = np.random.default_rng(0)
    w = torch.from_numpy((rng.standard_normal((4, 4, 4, 8, 16)) * np.exp(rng.uniform(-8, 8, 16))).astype(np.float32))   # Keras conv layout, cout last
    wq, s = E.quant_fp8(w, 4)
    assert wq.shape == w.shape and s.shape == (16,)
    assert float(wq.abs().amax()) <= 256.0 + 1e-3 and torch.allclose(wq.abs().amax(dim=(0, 1, 2, 3)), torch.full((16,), 256.0), rtol=1e-5)
    assert torch.equal(wq, wq.to(torch.float8_e4m3fn).float())                       # returned ON the e4m3fn grid (round 4)
    back = wq.to(torch.float8_e4m3fn).float() * s
    big = w.abs() > w.abs().amax(dim=(0, 1, 2, 3), keepdim=True) * 2.0 ** -6          # above the subnormal floor of the scaled channel
    assert float(((back - w).abs() / w.abs())[big].max()) <= 2.0 ** -4 + 1e-6
    wt = w.permute(0, 1, 2, 4, 3).contiguous()                                        # transposed-conv layout: cout at axis 3
    wq2, s2 = E.quant_fp8(wt, 3)
    assert torch.equal(s2, s) and torch.equal(wq2, wq.permute(0, 1, 2, 4, 3))


def test_fp8_weight_error_diffusion_host_side():
    """Round 4: the fp8 weight images are rounded with error diffusion over the taps one output sums (engine.quant_fp8 with tap groups).
    round_e4m3 is the e4m3fn cast bit for bit; every value stays on the e4m3fn grid and within one ulp of the weight; the rounding errors
    of a (cin, cout) pair sum to at most half an ulp over a whole tap group AND over every raster prefix of it (what a SAME-padding
    border sums), where independent rounding leaves ~sqrt(n / 12) ulps; the transposed layout diffuses inside its 8 parity classes."""
    if not hasattr(torch, 'float8_e4m3fn'):
        pytest.skip('torch.float8_e4m3fn not available')
    from voxvae import engine as E
    g = torch.Generator().manual_seed(3)
    x = torch.randn(100000, generator=g) * torch.exp2(torch.randint(-12, 9, (100000,), generator=g).float())
    x = torch.cat([x, torch.tensor([0., 448., 500., -500., 2.0 ** -9, 2.0 ** -10, 1.5 * 2.0 ** -9, 2.0 ** -11, 0.9375, 0.96875, 1.0625])])
    assert torch.equal(E.round_e4m3(x), x.clamp(-448, 448).to(torch.float8_e4m3fn).float())
    w = torch.randn(4, 4, 4, 16, 32, generator=g) * 0.05
    q0, s0 = E.quant_fp8(w, 4)
    q1, s1 = E.quant_fp8(w, 4, E.CONV_TAP_GROUPS)
    assert torch.equal(s0, s1)
    for q in (q0, q1):
        assert torch.equal(q, q.to(torch.float8_e4m3fn).float())                    # on the grid: the pack kernel converts exactly
    ws = (w / s0).reshape(64, 16, 32)
    e0, e1 = (q0.reshape(64, 16, 32) - ws), (q1.reshape(64, 16, 32) - ws)
    top = torch.exp2(torch.floor(torch.log2(ws.abs().amax(0))) - 3)                    # the largest ulp in the group
    # a weight's error = (carry in) - (carry out), each at most half an ulp of the value it was rounded at: bounded by the group's
    # largest ulp (one binade of slack for a value the carry pushed up), and the error POWER is twice independent rounding's, not more
    assert float((e1.abs() / top).max()) <= 2.0 + 1e-4
    assert float(e1.pow(2).mean()) <= 2.6 * float(e0.pow(2).mean())
    pre1 = e1.cumsum(0).abs().amax(0)                                                # worst raster prefix of the diffused errors
    assert float((pre1 / top).max()) <= 0.5 + 1e-4
    assert float(e0.sum(0).pow(2).mean().sqrt()) > 4 * float(e1.sum(0).pow(2).mean().sqrt())
    wt = w.permute(0, 1, 2, 4, 3).contiguous()
    q2, _ = E.quant_fp8(wt, 3, E.CONVT_TAP_GROUPS)
    e2 = (q2 - wt / s0.view(1, 1, 1, -1, 1)).reshape(64, 32, 16)
    assert sorted(t for grp in E.CONVT_TAP_GROUPS for t in grp) == list(range(64)) and all(len(grp) == 8 for grp in E.CONVT_TAP_GROUPS)
    for grp in E.CONVT_TAP_GROUPS:
        idx = torch.tensor(grp)
        topg = torch.exp2(torch.floor(torch.log2((wt / s0.view(1, 1, 1, -1, 1)).reshape(64, 32, 16)[idx].abs().amax(0))) - 3)
        assert float((e2[idx].sum(0).abs() / topg).max()) <= 0.5 + 1e-4
    # parity class (pd, ph, pw) of an OUTPUT voxel reads taps 1 - p + 2a per axis: group 0 = taps with all-even indices = output parity (1,1,1)
    assert E.CONVT_TAP_GROUPS[0] == (0, 2, 8, 10, 32, 34, 40, 42)


def test_default_dtype_switch_accepts_the_three_modes():
    import voxvae
    keep = voxvae.default_dtype()
    try:
        for name in ('f32', 'bf16', 'fp8'):
            voxvae.set_default_dtype(name)
            assert voxvae.default_dtype() == name
        with pytest.raises(ValueError):
            voxvae.set_default_dtype('fp16')
    finally:
        voxvae.set_default_dtype(keep)
    from voxvae import lib as L
    assert (L.DTYPES['f32'], L.DTYPES['bf16'], L.DTYPES['fp8']) == (L.VV_F32, L.VV_BF16, L.VV_FP8) == (0, 1, 2)   # include/voxvae.h vv_dtype


def _run_bench(*args, timeout=300):
    import subprocess
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY='0')
    return subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py')] + list(args), stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                          env=env, text=True, timeout=timeout)


def test_bench_self_launches_two_ranks_and_reduces_metrics_gloo():
    """bench.py --gpus 2 outside a launcher must start the two ranks itself and relay rank 0's line: rehearsed on the CPU
    with the gloo backend (--dry-run: no kernel runs, the launcher, the SUM of the 8 metric scalars and the MAX of the timed
    region are the real code; reference DP semantics AE3D.py:92-104)."""
    import json
    p = _run_bench('--gpus', '2', '--dry-run', '--backend', 'gloo', '--steps', '5', '--warmup', '1')
    assert p.returncode == 0, p.stderr[-2000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith('{')]
    assert len(lines) == 1                                   # ONE JSON line, from rank 0
    got = json.loads(lines[0])
    assert got['n_gpus'] == 2 and got['rccl_world_size'] == 2 and got['dry_run'] is True
    # rank r fabricates sum_bce = 10 (r + 1) B over B samples, elapsed = steps (1 + r) ms: SUM / MAX over the ranks
    assert got['global_metrics']['samples'] == 512 and abs(got['global_metrics']['loss_shape'] - 15.0) < 1e-9
    assert abs(got['ms_per_step'] - 2.0) < 1e-9


def test_bench_dry_run_at_the_target_world_size_of_8():
    """The launcher, the per-rank shard seeds, the 8-scalar metric reduction and the gradient buckets (bf16 on the wire) at the
    world size BASELINE configs[3] / [4] name: 8 ranks over gloo on the CPU (no scaling curve can be measured here; this pins that
    the code paths the 8-GPU run takes are the ones rehearsed)."""
    import json
    p = _run_bench('--gpus', '8', '--dry-run', '--backend', 'gloo', '--steps', '4', '--warmup', '1', '--grad-wire', 'bf16', timeout=600)
    assert p.returncode == 0, p.stderr[-2000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith('{')]
    assert len(lines) == 1
    got = json.loads(lines[0])
    assert got['n_gpus'] == 8 and got['rccl_world_size'] == 8 and got['dry_run'] is True
    assert got['global_metrics']['samples'] == 8 * 256
    assert abs(got['global_metrics']['loss_shape'] - 10.0 * sum(range(1, 9)) / 8) < 1e-9       # SUM over ranks of 10 (r + 1) B, over 8 B samples
    assert abs(got['ms_per_step'] - 8.0) < 1e-9                                                  # MAX over ranks of (1 + r) ms
    assert got['shard_seeds'] == [[1234 + r, 7 + r] for r in range(8)]                           # every rank draws its own voxels / epsilon
    gb = got['gradient_buckets']
    assert gb['wire'] == 'bf16' and gb['summed_correctly'] is True and gb['buckets'] >= 2


def test_bench_dump_outputs_stays_within_budget_and_is_reproducible(tmp_path):
    """bench.py --dump-outputs: float32 (float64 and integer counts as float64), whole arrays while they fit, a fixed seeded sample of
    the largest one when they do not (64^3 at batch 64 = 67 MB of probabilities), the same files from run to run."""
    sys.path.insert(0, ROOT)
    import bench
    rng = np.random.default_rng(3)
    small = [('stats', torch.from_numpy(rng.random((16, 4)).astype(np.float32))), ('metrics', torch.arange(4, dtype=torch.int32)),
             ('kl', torch.from_numpy(rng.random(16)))]
    bench.dump_outputs(str(tmp_path / 'a'), [('pred', torch.from_numpy(rng.random((16, 32, 32, 32, 1), np.float32)))] + small + [('none', None)])
    got = {f[:-4]: np.load(tmp_path / 'a' / f) for f in os.listdir(tmp_path / 'a')}
    assert set(got) == {'pred', 'stats', 'metrics', 'kl'}
    assert got['pred'].shape == (16, 32, 32, 32, 1) and got['pred'].dtype == np.float32
    assert got['metrics'].dtype == np.float64 and list(got['metrics']) == [0, 1, 2, 3] and got['kl'].dtype == np.float64
    big = torch.from_numpy(rng.random((64, 64, 64, 64, 1), np.float32))
    for d in ('b', 'c'):
        bench.dump_outputs(str(tmp_path / d), [('pred', big)] + small)
    files = sorted(os.listdir(tmp_path / 'b'))
    assert sum(os.path.getsize(tmp_path / 'b' / f) for f in files) <= 64 * 10 ** 6
    p = np.load(tmp_path / 'b' / 'pred.npy')
    assert p.ndim == 1 and 0.9 * bench.DUMP_BYTES / 4 < p.size < big.numel()
    assert np.isin(p[:100], big.numpy().ravel()).all()
    assert all(np.array_equal(np.load(tmp_path / 'b' / f), np.load(tmp_path / 'c' / f)) for f in files)


def test_bench_refuses_more_gpus_than_visible():
    """--gpus N with fewer than N visible GPUs fails loudly instead of running one rank (no GPU exists in this container)."""
    if torch.cuda.device_count() >= 2:
        pytest.skip('two GPUs are visible here')
    p = _run_bench('--gpus', '2', '--steps', '1', timeout=120)
    assert p.returncode != 0
    assert '2 GPUs requested, %d visible' % torch.cuda.device_count() in (p.stderr + p.stdout)
    assert not [ln for ln in p.stdout.splitlines() if ln.startswith('{')]


# ------------------------------------------------------------------------------------------------ TensorFlow checkpoint files
def test_tf_checkpoint_tensor_crcs_are_written_and_verified(tmp_path):
    """Round-3 advisor finding: write_checkpoint stored crc32c = 0 in every BundleEntryProto, which TensorFlow's BundleReader::GetValue
    rejects (DataLoss).  The entries now carry the masked crc32c of the tensor bytes (numpy lane-parallel crc32c_bulk == the byte-wise
    crc32c on every input), and the reader checks it: a flipped bit in the data shard is an error, not a silently different weight."""
    from voxvae import tf_checkpoint as tc
    rng = np.random.default_rng(0)
    for n in (0, 1, 4095, 4096 * 4, 4096 * 4 + 1, 100003, 4096 * 37 + 17):
        d = rng.integers(0, 256, n, dtype=np.uint8)
        assert tc.crc32c_bulk(d) == tc.crc32c(d.tobytes()), n
    p = str(tmp_path / 'ck')
    tens = {'a/b': rng.standard_normal((300, 70)).astype(np.float32), 'c': np.arange(5, dtype=np.int64)}
    tc.write_checkpoint(p, tens)
    stored = {k.decode(): tc._parse_proto(v).get(6, [0])[0] for k, v in tc.read_index(p + '.index')[1:]}
    assert stored['a/b'] == tc._mask(tc.crc32c(tens['a/b'].tobytes())) != 0
    out = tc.read_checkpoint(p)
    assert all(np.array_equal(out[k], tens[k]) for k in tens)
    raw = bytearray(open(p + '.data-00000-of-00001', 'rb').read())
    raw[100] ^= 1
    open(p + '.data-00000-of-00001', 'wb').write(raw)
    with pytest.raises(ValueError, match='crc32c mismatch'):
        tc.read_checkpoint(p)


def test_tf_checkpoint_crc32c_known_answers_and_table_round_trip(tmp_path):
    """voxvae/tf_checkpoint.py: CRC32C against RFC 3720's vectors, LevelDB's mask, and a multi-block index round trip."""
    from voxvae import tf_checkpoint as tc
    assert tc.crc32c(b'123456789') == 0xE3069283
    assert tc.crc32c(bytes(32)) == 0x8A9136AA and tc.crc32c(b'\xff' * 32) == 0x62A8AB43
    assert tc.crc32c(bytes(range(32))) == 0x46DD794E
    assert tc.crc32c(b'world', tc.crc32c(b'hello ')) == tc.crc32c(b'hello world')
    assert tc._mask(0) == 0xa282ead8                             # rotate right 15, add kMaskDelta
    rng = np.random.default_rng(0)
    names = ['conv%d/%s' % (i, leaf) for i in range(40) for leaf in ('kernel', 'bias')]
    names += ['bn%d/%s' % (i, leaf) for i in range(40) for leaf in ('gamma', 'beta', 'moving_mean', 'moving_variance')]
    tensors = {'layer_with_weights-%d/%s/.ATTRIBUTES/VARIABLE_VALUE' % (i, n): rng.standard_normal((3, i % 5 + 1, 2)).astype(np.float32)
               for i, n in enumerate(names)}
    tensors['save_counter/.ATTRIBUTES/VARIABLE_VALUE'] = np.array(7, dtype=np.int64)
    prefix = str(tmp_path / 'ck' / 'encoder')
    tc.write_checkpoint(prefix, tensors, block_bytes=512)         # many data blocks: exercises the index block and key prefixes
    keys = [k for k, _ in tc.read_index(prefix + '.index')]
    assert keys[0] == b'' and keys[1:] == sorted(k.encode() for k in tensors)
    back = tc.read_checkpoint(prefix)
    assert set(back) == set(tensors)
    for k in tensors:
        assert back[k].dtype == tensors[k].dtype and back[k].shape == tensors[k].shape and np.array_equal(back[k], tensors[k])
    # a flipped byte inside a block is caught by the block CRC; a foreign file by the magic
    raw = bytearray(open(prefix + '.index', 'rb').read())
    raw[20] ^= 0x40
    open(prefix + '.index', 'wb').write(bytes(raw))
    with pytest.raises(ValueError, match='CRC'):
        tc.read_checkpoint(prefix)
    open(prefix + '.index', 'wb').write(b'not a table' * 10)
    with pytest.raises(ValueError, match='magic'):
        tc.read_checkpoint(prefix)


def test_tf_checkpoint_keras_object_graph_keys_follow_creation_order(tmp_path):
    """`layer_with_weights-<i>` counts the layers that own variables in creation order (autoencoder3D.py:26-139 creates
    Conv3D then BatchNormalization per block); shapes are checked, bfloat16 entries widen to float32."""
    from voxvae import tf_checkpoint as tc
    shapes = {'conv0/kernel': (4, 4, 4, 1, 8), 'conv0/bias': (8,), 'bn0/gamma': (8,), 'bn0/beta': (8,), 'bn0/moving_mean': (8,),
              'bn0/moving_variance': (8,), 'dense/kernel': (8, 6), 'dense/bias': (6,)}
    keys = tc.keras_object_graph_keys(list(shapes))
    assert keys[0] == ('layer_with_weights-0/kernel/.ATTRIBUTES/VARIABLE_VALUE', 'conv0/kernel')
    assert keys[2] == ('layer_with_weights-1/gamma/.ATTRIBUTES/VARIABLE_VALUE', 'bn0/gamma')
    assert keys[-1] == ('layer_with_weights-2/bias/.ATTRIBUTES/VARIABLE_VALUE', 'dense/bias')
    rng = np.random.default_rng(1)
    params = {k: rng.standard_normal(s).astype(np.float32) for k, s in shapes.items()}
    prefix = str(tmp_path / 'enc')
    tc.save_keras_checkpoint(prefix, params)
    back = tc.load_keras_checkpoint(prefix, shapes)
    assert list(back) == list(shapes) and all(np.array_equal(back[k], params[k]) for k in shapes)
    with pytest.raises(ValueError, match='shape'):
        tc.load_keras_checkpoint(prefix, dict(shapes, **{'dense/bias': (7,)}))
    with pytest.raises(ValueError, match='lacks'):
        tc.load_keras_checkpoint(prefix, dict(shapes, **{'extra/kernel': (1,)}))
    # a bfloat16 entry (DT_BFLOAT16 = 14), built by hand: value 1.5 = 0x3FC0
    entry = tc._entry_proto(14, (2,), 0, 0, 4, 0)
    e = tc._parse_proto(entry)
    assert e[1] == [14] and tc._shape_of(e[2][0]) == (2,) and e[5] == [4]
