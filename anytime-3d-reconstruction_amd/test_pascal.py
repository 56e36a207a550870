"""Entry point mirroring the reference's test_pascal.py (loop :125-185): one epoch of nolboSingleObject.getEval over the validation
split with `missing_pr` of the category latent missing -- reconstruction, category / instance accuracy, and the same after the
correction against the category prior.
`python test_pascal.py --batch 16 --image 128 --missing-pr 0.3 --max-iter 2`."""
import sys

import _entry_common as C
import voxvae
import src.dataset_loader.pascal3D as pascal3D
import src.net_core.darknet as Darknet
from train_pascal import indices_of, inputs_of, make_config


def train(
        learning_rate=1e-4,
        config=None,
        load_path=None,
        load_encoder_backbone_path=None, load_encoder_backbone_name=None,
        load_decoder_path=None, load_decoder_name=None,
        missing_pr=0.3,
        batch_size=72, image_size=(256, 256), max_iter=None, dataset_path=None,
):
    import src.module.nolbo as nolbo
    model = nolbo.nolboSingleObject(nolbo_structure=config, backbone_style=Darknet.Darknet19, learning_rate=learning_rate)
    voxel, idx = config['decoder']['output_shape'][0], indices_of(config)
    loader = pascal3D.dataLoaderSingleObject(trainOrVal='val', Pascal3DDataPath=dataset_path, voxel=voxel, instances=idx['inst_indices'].shape[0])
    if load_path is not None:
        print('load weights...')
        model.loadModel(load_path=load_path)
        print('done!')
    if load_encoder_backbone_path is not None:
        model.loadEncoderBackbone(load_path=load_encoder_backbone_path, file_name=load_encoder_backbone_name)
    if load_decoder_path is not None:
        model.loadDecoder(load_path=load_decoder_path, file_name=load_decoder_name)

    means = C.RunningMeans(eval=9)
    bar = C.Progress(width=5)
    print('start training...')
    for epoch, position, total in C.epochs_of(loader, 1, 'dataStart'):
        bar.tic()
        batch = loader.getNextBatch(batchSizeof3DShape=batch_size, imageSize=image_size, augmentation=False)
        out = model.getEval(inputs=inputs_of(batch), missing_prob=missing_pr, **idx)
        means.add(eval=out[1:6] + out[7:11])
        bar.toc()
        m = means['eval']
        bar.show(epoch, position, total, bar.group(zip(('loss', 'pr', 'rc', 'c', 'i'), m[:5])) + ",",
                 bar.group(zip(('closs', 'cpr', 'crc', 'cc'), m[5:])))
        if C.stop_on_nan(means):
            return None
        if max_iter is not None and means.n >= max_iter:
            break
    print('')
    return means['eval']


latent_dim = 16
config = make_config(latent_dim, 64)

if __name__ == '__main__':
    import argparse
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument('--voxel', type=int, default=64)
    ap.add_argument('--latent', type=int, default=16)
    ap.add_argument('--batch', type=int, default=72)
    ap.add_argument('--image', type=int, default=256)
    ap.add_argument('--dtype', default='f32', choices=['f32', 'bf16'])
    ap.add_argument('--load-path', default=None)
    ap.add_argument('--missing-pr', type=float, default=0.3)
    ap.add_argument('--max-iter', type=int, default=None)
    ap.add_argument('--dataset-path', default=None)
    a = ap.parse_args()
    if not a.missing_pr > 0:
        ap.error('--missing-pr must be > 0: the loop reads the corrected half of getEval')
    voxvae.set_default_dtype(a.dtype)
    sys.exit(0 if train(config=make_config(a.latent, a.voxel), load_path=a.load_path, missing_pr=a.missing_pr, batch_size=a.batch,
                        image_size=(a.image, a.image), max_iter=a.max_iter, dataset_path=a.dataset_path) is not None else 1)
