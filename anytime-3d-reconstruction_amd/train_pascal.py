"""Entry point mirroring the reference's train_pascal.py (loop :118-171, config :173-214): nolboSingleObject.fit on the training
split, getEval on the same batch and on a validation batch -- Darknet19 + head2D image encoder, category latent 8 + instance
latent 8, a prior network for each, 64^3 decoder.
`python train_pascal.py --batch 16 --image 128 --max-iter 2`."""
import sys

import numpy as np

import _entry_common as C
import voxvae
import src.dataset_loader.pascal3D as pascal3D
import src.net_core.darknet as Darknet

INSTANCES = 10


def make_config(latent_dim=16, voxel=64, instances=INSTANCES):
    lc = latent_dim // 2
    prior = lambda name, n, out: {'name': name, 'input_dim': n, 'unit_num_list': [32, out], 'core_activation': 'elu', 'const_log_var': 0.0}
    return {
        'encoder_backbone': {'name': 'nolbo_backbone', 'z_category_dim': lc, 'z_inst_dim': latent_dim - lc, 'activation': 'elu'},
        'encoder_head': {'name': 'nolbo_head', 'output_dim': 2 * latent_dim, 'filter_num_list': [], 'filter_size_list': [],
                         'activation': 'elu'},
        'decoder': C.make_config(latent_dim, voxel, True)['decoder'],
        'prior_class': prior('priornet_class', pascal3D.CLASSES, lc),
        'prior_inst': prior('priornet_inst', pascal3D.CLASSES + instances, latent_dim - lc),
    }


def inputs_of(batch):
    """The loader's positional tuple -> the model's (images, voxels, category one-hots, instance one-hots)."""
    inst_list, category_list, _, _, input_images, output_images = batch
    return input_images, output_images, category_list, inst_list


def indices_of(config):
    """The identity tables getEval classifies against: every category, every instance."""
    classes = config['prior_class']['input_dim']
    return {'category_indices': np.identity(classes), 'inst_indices': np.identity(config['prior_inst']['input_dim'] - classes)}


def train(
        training_epoch=1000,
        learning_rate=1e-4,
        config=None,
        save_path=None, load_path=None,
        load_encoder_backbone_path=None, load_encoder_backbone_name=None,
        load_decoder_path=None, load_decoder_name=None,
        batch_size=72, image_size=(256, 256), max_iter=None, dataset_path=None, loader='host', colour_ops='invert_add',
):
    import src.module.nolbo as nolbo
    make_loader = pascal3D.loader_factory(loader, colour_ops)
    model = nolbo.nolboSingleObject(nolbo_structure=config, backbone_style=Darknet.Darknet19, learning_rate=learning_rate)
    voxel, idx = config['decoder']['output_shape'][0], indices_of(config)
    instances = idx['inst_indices'].shape[0]
    loader = make_loader(trainOrVal='train', Pascal3DDataPath=dataset_path, voxel=voxel, instances=instances)
    loader_test = make_loader(trainOrVal='val', Pascal3DDataPath=dataset_path, voxel=voxel, instances=instances)
    if load_path is not None:
        print('load weights...')
        model.loadModel(load_path=load_path)
        print('done!')
    if load_encoder_backbone_path is not None:
        model.loadEncoderBackbone(load_path=load_encoder_backbone_path, file_name=load_encoder_backbone_name)
    if load_decoder_path is not None:
        model.loadDecoder(load_path=load_decoder_path, file_name=load_decoder_name)

    means = C.RunningMeans(fit=5, train=5, test=5)
    bar = C.Progress(width=4)

    def on_new_epoch():
        print('')
        means.reset()
        bar.reset()
        if save_path is not None:
            print('save model...')
            model.saveModel(save_path=save_path)

    print('start training...')
    for epoch, position, total in C.epochs_of(loader, training_epoch, 'dataStart', on_new_epoch):
        bar.tic()
        inputs = inputs_of(loader.getNextBatch(batchSizeof3DShape=batch_size, imageSize=image_size))
        inputs_test = inputs_of(loader_test.getNextBatch(batchSizeof3DShape=batch_size, imageSize=image_size, augmentation=False))
        means.add(fit=model.fit(inputs=inputs), train=model.getEval(inputs=inputs, **idx)[1:], test=model.getEval(inputs=inputs_test, **idx)[1:])
        bar.toc()
        f, tr, te = means['fit'], means['train'], means['test']
        bar.show(epoch, position, total, bar.group(zip(('kl', 'shape', 'reg', 'pr', 'rc'), f)) + ", " + bar.group(zip(('c', 'i'), tr[3:])),
                 bar.group(zip(('shape', 'pr', 'rc', 'c', 'i'), te)))
        if C.stop_on_nan(means):
            return None
        if max_iter is not None and means.n >= max_iter:
            break
    print('')
    return means['fit']


latent_dim = 16
config = make_config(latent_dim, 64)

if __name__ == '__main__':
    import argparse
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument('--voxel', type=int, default=64)
    ap.add_argument('--latent', type=int, default=16)
    ap.add_argument('--batch', type=int, default=72)
    ap.add_argument('--image', type=int, default=256)
    ap.add_argument('--epochs', type=int, default=1000)
    ap.add_argument('--lr', type=float, default=1e-4)
    ap.add_argument('--save-path', default=None)
    ap.add_argument('--load-path', default=None)
    ap.add_argument('--max-iter', type=int, default=None)
    ap.add_argument('--dataset-path', default=None)
    ap.add_argument('--loader', choices=('host', 'device'), default='host',
                    help="'device': pascal3D.deviceDataLoaderSingleObject builds the image batch on the GPU")
    ap.add_argument('--colour-ops', choices=('invert_add', 'all'), default='invert_add',
                    help="with --loader device: 'all' also applies GaussianBlur and AddToHueAndSaturation, the reference's other two")
    a = ap.parse_args()
    voxvae.set_default_dtype('f32')        # the 2D encoder trains by float32 autograd
    sys.exit(0 if train(training_epoch=a.epochs, learning_rate=a.lr, config=make_config(a.latent, a.voxel), save_path=a.save_path,
                        load_path=a.load_path, batch_size=a.batch, image_size=(a.image, a.image), max_iter=a.max_iter,
                        dataset_path=a.dataset_path, loader=a.loader, colour_ops=a.colour_ops) is not None else 1)
