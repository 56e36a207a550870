"""Entry point mirroring the reference's test_pascal_category.py (loop :118-171): one epoch of nolboSingleObject_category_only.getEval
over the validation split with `missing_pr` of the latent missing -- reconstruction and category accuracy, and the same after the
correction against the category prior.
`python test_pascal_category.py --batch 16 --image 128 --missing-pr 0.3 --max-iter 2`."""
import sys

import _entry_common as C
import voxvae
import src.dataset_loader.pascal3D as pascal3D
import src.net_core.darknet as Darknet
from train_pascal_category import inputs_of, make_config


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
    model = nolbo.nolboSingleObject_category_only(nolbo_structure=config, backbone_style=Darknet.Darknet19, learning_rate=learning_rate)
    loader = pascal3D.dataLoaderSingleObject(trainOrVal='val', Pascal3DDataPath=dataset_path, voxel=config['decoder']['output_shape'][0])
    if load_path is not None:
        print('load weights...')
        model.loadModel(load_path=load_path)
        print('done!')
    if load_encoder_backbone_path is not None:
        model.loadEncoderBackbone(load_path=load_encoder_backbone_path, file_name=load_encoder_backbone_name)
    if load_decoder_path is not None:
        model.loadDecoder(load_path=load_decoder_path, file_name=load_decoder_name)

    means = C.RunningMeans(eval=8)
    bar = C.Progress(width=5)
    print('start training...')
    for epoch, position, total in C.epochs_of(loader, 1, 'dataStart'):
        bar.tic()
        batch = loader.getNextBatch(batchSizeof3DShape=batch_size, imageSize=image_size, augmentation=False)
        out = model.getEval(inputs=inputs_of(batch), missing_prob=missing_pr)
        means.add(eval=out[1:5] + out[6:10])
        bar.toc()
        m = means['eval']
        bar.show(epoch, position, total, bar.group(zip(('loss', 'pr', 'rc', 'c'), m[:4])) + ",",
                 bar.group(zip(('closs', 'cpr', 'crc', 'cc'), m[4:])))
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
    ap.add_argument('--missing-pr', type=float, default=0.0, help='the reference runs 0.0, 0.3, 0.5 and 0.7')
    ap.add_argument('--max-iter', type=int, default=None)
    ap.add_argument('--dataset-path', default=None)
    a = ap.parse_args()
    voxvae.set_default_dtype(a.dtype)
    sys.exit(0 if train(config=make_config(a.latent, a.voxel), load_path=a.load_path, missing_pr=a.missing_pr, batch_size=a.batch,
                        image_size=(a.image, a.image), max_iter=a.max_iter, dataset_path=a.dataset_path) is not None else 1)
