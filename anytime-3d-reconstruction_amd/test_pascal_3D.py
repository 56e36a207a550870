"""Entry point mirroring the reference's test_pascal_3D.py (:118-173), the paper's comparison: one training and one validation batch
through the multi-modal model (at twice the missing rate: only its category half is masked), the AE baseline and the VAE baseline,
at the reference's four missing rates; per object the target and the four reconstructions are written as text, [D*D, D] each:
    OUT_DIR/{train,test}/<2 * missing_pr>/3D/NNN_{gt,mVAE,mVAE_c,AE,VAE}.txt
`python test_pascal_3D.py --batch 4 --image 128 --voxel 32 --out-dir /tmp/data_3D --max-iter 2` (max-iter: how many rates)."""
import os
import sys

import numpy as np

import _entry_common as C
import voxvae
import src.dataset_loader.pascal3D as pascal3D
import src.net_core.darknet as Darknet
from train_pascal import indices_of, inputs_of, make_config

MISSING_PR = (0.15, 0.25, 0.35, 0.45)
DUMPS = ('gt', 'mVAE', 'mVAE_c', 'AE', 'VAE')


def make_baseline_config(latent_dim=16, voxel=64, variational=True):
    """config_AE / config_VAE of the reference (:64-116): one latent of the full width; the VAE's head emits (mean | logVar)."""
    return {
        'encoder_backbone': {'name': 'nolbo_backbone', 'z_dim': latent_dim, 'activation': 'elu'},
        'encoder_head': {'name': 'nolbo_head', 'output_dim': (2 if variational else 1) * latent_dim, 'filter_num_list': [],
                         'filter_size_list': [], 'activation': 'elu'},
        'decoder': C.make_config(latent_dim, voxel, True)['decoder'],
    }


def train(config=None, config_AE=None, config_VAE=None, load_path=None, load_path_AE=None, load_path_VAE=None, out_dir='data_3D',
          batch_size=72, image_size=(256, 256), max_iter=None, dataset_path=None):
    import src.module.nolbo as nolbo
    model = nolbo.nolboSingleObject(nolbo_structure=config, backbone_style=Darknet.Darknet19, learning_rate=None)
    model_AE = nolbo.nolboSingleObject_AE(nolbo_structure=config_AE, backbone_style=Darknet.Darknet19, learning_rate=None)
    model_VAE = nolbo.nolboSingleObject_VAE(nolbo_structure=config_VAE, backbone_style=Darknet.Darknet19, learning_rate=None)
    voxel, idx = config['decoder']['output_shape'][0], indices_of(config)
    data = {}
    for name, split in (('train', 'train'), ('test', 'val')):
        loader = pascal3D.dataLoaderSingleObject(trainOrVal=split, Pascal3DDataPath=dataset_path, voxel=voxel, instances=idx['inst_indices'].shape[0])
        data[name] = inputs_of(loader.getNextBatch(batchSizeof3DShape=batch_size, imageSize=image_size, augmentation=False))
    for m, path in ((model, load_path), (model_AE, load_path_AE), (model_VAE, load_path_VAE)):
        if path is not None:
            m.loadModel(path)
    written = 0
    for name, inputs in data.items():
        for missing_pr in MISSING_PR[:max_iter]:
            print(name, missing_pr)
            out = model.getEval(inputs=inputs, missing_prob=missing_pr * 2, **idx)        # :151
            pred_AE = model_AE.getEval(inputs=inputs[0:2], missing_prob=missing_pr)[0]    # :152-153
            pred_VAE = model_VAE.getEval(inputs=inputs[0:2], missing_prob=missing_pr)[0]
            save_dir = os.path.join(out_dir, name, str(missing_pr * 2), '3D')
            os.makedirs(save_dir, exist_ok=True)
            grids = [np.asarray(g, dtype=np.float32) for g in (inputs[1], out[0], out[6], pred_AE, pred_VAE)]
            for i in range(len(grids[0])):
                for tag, g in zip(DUMPS, grids):
                    np.savetxt(os.path.join(save_dir, '{:03d}_{}.txt'.format(i, tag)), np.reshape(g[i], (voxel * voxel, voxel)))
                    written += 1
    return written


latent_dim = 16
config = make_config(latent_dim, 64)
config_AE = make_baseline_config(latent_dim, 64, False)
config_VAE = make_baseline_config(latent_dim, 64, True)

if __name__ == '__main__':
    import argparse
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument('--voxel', type=int, default=64)
    ap.add_argument('--latent', type=int, default=16)
    ap.add_argument('--batch', type=int, default=72)
    ap.add_argument('--image', type=int, default=256)
    ap.add_argument('--dtype', default='f32', choices=['f32', 'bf16'])
    ap.add_argument('--load-path', default=None)
    ap.add_argument('--load-path-AE', default=None)
    ap.add_argument('--load-path-VAE', default=None)
    ap.add_argument('--out-dir', default='data_3D')
    ap.add_argument('--max-iter', type=int, default=None, help='how many of the four missing rates to run')
    ap.add_argument('--dataset-path', default=None)
    a = ap.parse_args()
    voxvae.set_default_dtype(a.dtype)
    n = train(config=make_config(a.latent, a.voxel), config_AE=make_baseline_config(a.latent, a.voxel, False),
              config_VAE=make_baseline_config(a.latent, a.voxel, True), load_path=a.load_path, load_path_AE=a.load_path_AE,
              load_path_VAE=a.load_path_VAE, out_dir=a.out_dir, batch_size=a.batch, image_size=(a.image, a.image), max_iter=a.max_iter,
              dataset_path=a.dataset_path)
    print('%d files -> %s' % (n, a.out_dir))
    sys.exit(0 if n else 1)
