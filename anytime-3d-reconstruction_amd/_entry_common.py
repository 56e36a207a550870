"""Shared by the train_*/test_* entry points: the config dict literals of the reference scripts
(test_modelnet_VAE.py:169-192, train_modelnet_category_VAE.py:109-132) with the voxel side as a parameter, and the
argparse overrides SURVEY §5 asks for (--voxel, --batch, --dtype, --synthetic ...)."""
import argparse
import os


def make_config(latent_dim=64, voxel=64, variational=True):
    return {
        'z_category_dim': latent_dim,
        'encoder': {
            'name': 'encoder3D',
            'input_shape': [voxel, voxel, voxel, 1],  # or [None,None,None,1]
            'filter_num_list': [64, 128, 256, 512, (2 if variational else 1) * latent_dim],
            'filter_size_list': [4, 4, 4, 4, 4],
            'strides_list': [2, 2, 2, 2, 1],
            'final_pool': 'average',
            'activation': 'elu',
            'final_activation': 'None',
        },
        'decoder': {
            'name': 'decoder',
            'input_dim': latent_dim,
            'output_shape': [voxel, voxel, voxel, 1],
            'filter_num_list': [512, 256, 128, 64, 1],
            'filter_size_list': [4, 4, 4, 4, 4],
            'strides_list': [1, 2, 2, 2, 2],
            'activation': 'elu',
            'final_activation': 'sigmoid'
        },
    }


def parse(description, train=False, extra=None):
    """extra(ap): a script's own options.  A script that defines them reads --sampling itself (test_modelnet_PR.py: the curve of the
    sampled-mean reconstruction) and nothing is installed for it below."""
    ap = argparse.ArgumentParser(description=description)
    ap.add_argument('--dataset-path', default=None, help="ModelNet shard directory; default: seeded synthetic voxels")
    ap.add_argument('--voxel', type=int, default=32, help='voxel side (the reference ships 64; BASELINE.json asks for 32)')
    ap.add_argument('--latent', type=int, default=64)
    ap.add_argument('--batch', type=int, default=64 if train else 72)
    ap.add_argument('--dtype', default='f32', choices=['f32', 'bf16'] + ([] if train else ['fp8']),
                    help="'f32': the reference's arithmetic; 'bf16'; 'fp8' (test_* scripts only: e4m3fn MFMA layers, inference)")
    ap.add_argument('--load-path', default=None)
    ap.add_argument('--save-path', default=None)
    ap.add_argument('--max-iter', type=int, default=None, help='stop after this many iterations (smoke runs)')
    ap.add_argument('--missing-pr', type=float, default=0.9)
    ap.add_argument('--epochs', type=int, default=1000)
    ap.add_argument('--lr', type=float, default=1e-4)
    ap.add_argument('--device-data', action='store_true', help='keep the split in HBM as packed bits (deviceDataLoader)')
    ap.add_argument('--packed-data', action='store_true', help='host loader that keeps the split as bits and serves PackedVoxels batches (1 bit per voxel over PCIe)')
    ap.add_argument('--pipeline', type=int, default=1, help='test_modelnet_VAE.py: batches in flight (voxvae.streams.HostPipeline); 1 = the reference\'s synchronous loop')
    ap.add_argument('--dump-dir', default=None, help='test_modelnet_VAE.py: save <missing_pr>_cl_label/_gt/_pred.npy here (reference :159-165)')
    ap.add_argument('--points-dir', default=None, help='test_modelnet_VAE.py: save every batch\'s predictions as point clouds here (batch_<n>_points.npy [N,3], batch_<n>_offsets.npy [B+1]; voxvae.points); needs --pipeline 1')
    ap.add_argument('--sampling', type=int, default=0, help='test_modelnet_VAE.py: also score the sampled-mean reconstruction over this many latents per object (0 = off); needs --pipeline 1.  test_modelnet_PR.py: also accumulate that reconstruction\'s curve')
    ap.add_argument('--mask-source', default=None, choices=['host', 'device'],
                    help="where uninjected dropout / missing-latent masks are drawn: 'host' (np.random, the reference's calls) or 'device' "
                         "(voxvae.masks, no upload); default: VOXVAE_MASK_SOURCE, else 'host'")
    ap.add_argument('--seed', type=int, default=None, help='seed of the device mask source (voxvae.manual_seed) and of np.random')
    if extra is not None:
        extra(ap)
    a = ap.parse_args()
    # both are read when a model is built, which every script does after parse(): passed on from here, once for all of them
    import voxvae
    if a.mask_source is not None:
        voxvae.set_mask_source(a.mask_source)
    if a.seed is not None:
        voxvae.manual_seed(a.seed)
        np.random.seed(a.seed % 2 ** 32)
    if a.points_dir and extra is None:
        if os.path.basename(sys.argv[0]) != SAMPLING_SCRIPT:
            ap.error('--points-dir is an option of %s' % SAMPLING_SCRIPT)
        if a.pipeline > 1:
            ap.error('--points-dir writes every batch synchronously: use --pipeline 1')
        save_point_clouds(a.points_dir)
    if a.sampling and extra is None:
        # one script owns the option: elsewhere (train + test getEval in one loop, other model classes) its numbers would mean something else
        if os.path.basename(sys.argv[0]) != SAMPLING_SCRIPT:
            ap.error('--sampling is an option of %s' % SAMPLING_SCRIPT)
        if a.sampling < 0:
            ap.error('--sampling must be >= 0')
        if a.pipeline > 1:
            ap.error('--sampling scores every batch synchronously: use --pipeline 1')
        score_sampled_mean(a.sampling)
    return a


# --sampling K of test_modelnet_VAE.py.  That script is a fixed point of this repository (it is not edited), and its loop is
# getEval -> RunningMeans.add -> Progress.show with the model and the batch out of this module's reach, so the option is served from here:
# every getEval of the model classes is followed, for the same (input, target) pair, by getSampledEval over K latents per object (the
# reference's nolbo_test.py:167-180), and Progress.show appends the running means of its loss / pr / rc as sloss / spr / src.
# getEval's own result is returned untouched.  parse() installs this for that one script only, with --pipeline 1 only (the conversion to
# floats synchronises); without --sampling nothing is installed.
SAMPLING_SCRIPT = 'test_modelnet_VAE.py'
SAMPLED = None          # {'k': K, 'n': batches scored, 'sums': [loss, pr, rc]} while --sampling is active


def score_sampled_mean(k):
    global SAMPLED
    import src.module.nolbo as nolbo
    SAMPLED = {'k': int(k), 'n': 0, 'sums': np.zeros(3)}
    base = nolbo._ModelnetBase
    single = base.getEval

    def getEval(self, inputs, *args, **kw):
        out = single(self, inputs, *args, **kw)
        if self._variational:
            s = self.getSampledEval((inputs[0], inputs[1]), SAMPLED['k'])
            SAMPLED['sums'] += np.array([float(v) for v in s[1:4]])
            SAMPLED['n'] += 1
        return out

    base.getEval = getEval



# --points-dir D of test_modelnet_VAE.py, served from here for the same reason as --sampling: every getEval of the model classes is
# followed by voxvae.points.voxel_points on its prediction (the cells with p > 0.5 in row-major order, largest extent scaled to 1,
# centred: ModelNet carries no size or pose), made on the device and saved as D/batch_<n>_points.npy [N,3] and D/batch_<n>_offsets.npy
# [B+1] (object b = rows offsets[b] .. offsets[b+1] - 1), n counting the calls from 0.  getEval's own result is returned untouched;
# without --points-dir nothing is installed.
def save_point_clouds(points_dir):
    import src.module.nolbo as nolbo
    from voxvae.points import voxel_points
    base = nolbo._ModelnetBase
    single = base.getEval
    state = {'n': 0}

    def getEval(self, inputs, *args, **kw):
        out = single(self, inputs, *args, **kw)
        os.makedirs(points_dir, exist_ok=True)
        cloud = voxel_points(out[0], np.ones((len(out[0]), 3), dtype=np.float32))
        stem = os.path.join(points_dir, 'batch_%05d' % state['n'])
        np.save(stem + '_points.npy', cloud.points.cpu().numpy())
        np.save(stem + '_offsets.npy', cloud.offsets.cpu().numpy())
        state['n'] += 1
        return out

    base.getEval = getEval

# ---------------------------------------------------------------------------------------------------------------------
# Shared loop plumbing of the train_* / test_* entry points.  The reference scripts each carry their own copy of the
# same bookkeeping (running means reset at epoch boundaries, one status line rewritten in place, a NaN stop); here it
# lives once.  The printed fields and their order are those of the reference scripts.
import sys
import time

import numpy as np


class RunningMeans:
    """Per-epoch running means of several result tuples (the `loss = (loss * it + new) / (it + 1)` idiom)."""

    def __init__(self, **widths):
        self.n = 0
        self.sums = {k: np.zeros(w) for k, w in widths.items()}

    def reset(self):
        self.n = 0
        for v in self.sums.values():
            v[:] = 0

    def add(self, **values):
        for k, v in values.items():
            self.sums[k] += np.array([float(x) for x in v])
        self.n += 1

    def __getitem__(self, key):
        return self.sums[key] / max(self.n, 1)

    def finite(self):
        return all(np.all(np.isfinite(v)) for v in self.sums.values())


class Progress:
    """One carriage-return status line: iteration, mean step time, epoch, loader position, then labelled groups."""

    def __init__(self, width=4, head_fmt="it:{it:04d} rt:{rt:.2f} Ep_o:{ep:03d} ", pos_label="cur_o/tot_o"):
        """head_fmt / pos_label: the names a script's reference prints for iteration, mean step time, epoch and loader position."""
        self.head_fmt = head_fmt
        self.pos_fmt = pos_label + ":{:0%dd}/{:0%dd} " % (width, width)
        self.elapsed, self.n = 0.0, 0
        self._t0 = None

    def reset(self):
        self.elapsed, self.n = 0.0, 0

    def tic(self):
        self._t0 = time.time()

    def toc(self):
        self.elapsed += time.time() - self._t0
        self.n += 1

    @staticmethod
    def group(pairs, sep=", "):
        return sep.join("%s:%.4f" % (k, v) for k, v in pairs)

    def show(self, epoch, position, total, *groups):
        head = self.head_fmt.format(it=self.n, rt=self.elapsed / max(self.n, 1), ep=int(epoch) + 1)
        if SAMPLED is not None and SAMPLED['n']:
            groups = groups + (self.group(zip(('sloss', 'spr', 'src'), SAMPLED['sums'] / SAMPLED['n'])),)
        sys.stdout.write(head + self.pos_fmt.format(position, total) + " ".join(groups) + "  \r")
        sys.stdout.flush()


def epochs_of(loader, limit, position_attr, on_new_epoch=None, every=None):
    """Yields (epoch, position, total) before every batch until `limit` epochs have been served; calls `on_new_epoch()`
    when the loader's epoch counter has advanced (the scripts save the model and restart their running means there) and,
    with `every`, also after every `every` batches since it last did."""
    epoch, since = loader.epoch, 0
    while loader.epoch < limit:
        if since and (loader.epoch != epoch or since == every):
            epoch, since = loader.epoch, 0
            if on_new_epoch is not None:
                on_new_epoch()
        since += 1
        yield loader.epoch, getattr(loader, position_attr), loader.dataLength


def stop_on_nan(means):
    if means.finite():
        return False
    print('')
    print('NaN')
    return True
