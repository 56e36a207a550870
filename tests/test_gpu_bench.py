"""bench.py's plain run (no --full) with --dump-outputs: the line carries the headline figure and nothing that needs legs of its own,
and the arrays it writes are the outputs of the last timed step (the line's `global_metrics` are recomputed from them)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench(*args):
    p = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py')] + list(args), stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                       text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-3000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith('{')]
    assert len(lines) == 1, p.stdout[-2000:]
    return json.loads(lines[0])


def _metrics_of(d, r):
    sys.path.insert(0, ROOT)
    import bench
    kl = torch.from_numpy(np.load(os.path.join(d, 'kl.npy')))
    stats = torch.from_numpy(np.load(os.path.join(d, 'stats.npy')))
    got = bench.global_metrics(bench.metric_vector(stats, kl))
    for k, v in r['global_metrics'].items():
        assert abs(got[k] - v) <= 1e-9 * max(1.0, abs(v)), (k, got[k], v)


def test_bench_plain_eval_run_dumps_the_last_timed_step(tmp_path):
    d = str(tmp_path / 'eval')
    r = _bench('--gpus', '1', '--steps', '3', '--warmup', '1', '--batch', '16', '--dump-outputs', d)
    assert r['steps'] == 3 and r['warmup'] == 1 and r['full'] is False and r['ms_per_step'] > 0
    assert abs(r['value'] - 16e3 / r['ms_per_step']) <= 1e-6 * r['value']
    assert r['roofline'] is None and r['cpu_baseline'] is None and r['parity'] is None and r['layer_ms'] is None
    assert sorted(os.listdir(d)) == ['kl.npy', 'metrics.npy', 'pred.npy', 'stats.npy']
    pred = np.load(os.path.join(d, 'pred.npy'))
    assert pred.shape == (16, 32, 32, 32, 1) and pred.dtype == np.float32 and 0.0 <= pred.min() and pred.max() <= 1.0
    assert np.load(os.path.join(d, 'stats.npy')).shape == (16, 4) and np.load(os.path.join(d, 'kl.npy')).shape == (16,)
    _metrics_of(d, r)


def test_bench_plain_train_run_dumps_the_last_timed_step(tmp_path):
    d = str(tmp_path / 'train')
    r = _bench('--gpus', '1', '--mode', 'train', '--steps', '2', '--warmup', '1', '--batch', '16', '--dump-outputs', d)
    assert r['steps'] == 2 and r['full'] is False and r['ms_per_step'] > 0
    assert r['gradient_all_reduce'] is None and r['roofline'] is None and r['cpu_baseline'] is None
    assert sorted(os.listdir(d)) == ['kl.npy', 'metrics.npy', 'stats.npy', 'weights_decoder.npy', 'weights_encoder.npy']
    w = np.load(os.path.join(d, 'weights_encoder.npy'))
    assert w.dtype == np.float32 and w.ndim == 1 and w.size > 0 and np.isfinite(w).all()
    _metrics_of(d, r)
