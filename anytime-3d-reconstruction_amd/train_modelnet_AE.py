"""Entry point with the role of the reference's train_modelnet_AE.py: the data-parallel 3D autoencoder src.module.AE3D on the MI355X
path, with the fields its status line prints (Epoch, iter, runtime, batch, cur/tot, rloss, ploss, tloss, pr, rc), a save at every new
epoch and every 1000 iterations, and a stop on NaN.  One GPU: `python train_modelnet_AE.py --voxel 32 --batch 64 --dtype bf16`;
several: `torchrun --nproc_per_node=8 train_modelnet_AE.py ...` (one process per GPU; --batch is per replica)."""
import os
import sys

import numpy as np

import _entry_common as C
import voxvae
from src.dataset_loader.modelnet_dataset import dataLoader

SAVE_EVERY = 1000
latent_dim = 16


def structures(latent, voxel):
    cfg = C.make_config(latent, voxel, False)
    return cfg['encoder'], dict(cfg['decoder'], name='decoder3D')


def train(training_epoch=1000, learning_rate=1e-4, batch_per_replica=32, dataset_path=None, encoder_structure=None, decoder_structure=None,
          save_path=None, load_path=None, max_iter=None):
    import torch.distributed as dist
    import src.module.AE3D as AE3D
    from voxvae.train import ReplicaStrategy
    strategy = ReplicaStrategy()
    world = strategy.num_replicas_in_sync
    rank = dist.get_rank() if world > 1 else 0
    with strategy.scope():
        model = AE3D.AE3D(encoder_structure=encoder_structure, decoder_structure=decoder_structure, BATCH_SIZE_PER_REPLICA=batch_per_replica,
                          strategy=strategy, learning_rate=learning_rate)
    if world > 1:
        np.random.seed(0)          # the loader shuffles with np.random: every rank walks the split in the same order and takes its own rows
    loader = dataLoader(data_path=dataset_path, voxel=encoder_structure['input_shape'][0])
    if load_path is not None:
        print('load weights...')
        model.loadModel(load_path=load_path)
        print('done!')
    global_batch = batch_per_replica * world
    rows = slice(rank * batch_per_replica, (rank + 1) * batch_per_replica)
    means = C.RunningMeans(loss=3, pr=2)
    bar = C.Progress(width=5, head_fmt="Epoch:{ep:03d} iter:{it:04d} runtime:{rt:.2f} batch:%d " % global_batch, pos_label='cur/tot')

    def save():
        if save_path is not None and rank == 0:
            print('save model...')
            model.saveModel(save_path)

    def restart():
        print('')
        means.reset()
        bar.reset()
        save()

    print('start training...')
    done = 0
    for epoch, position, total in C.epochs_of(loader, training_epoch, 'batchStart', restart, every=SAVE_EVERY):
        bar.tic()
        x = loader.getNextBatch(batchSize=global_batch)['input_images'][rows]
        out = model.distributed_fit(inputs=(x, x))
        means.add(loss=out[:3], pr=out[3:])
        bar.toc()
        if rank == 0:
            bar.show(epoch, position, total, bar.group(zip(('rloss', 'ploss', 'tloss'), means['loss'])), bar.group(zip(('pr', 'rc'), means['pr'])))
        if C.stop_on_nan(means):
            return None
        done += 1
        if max_iter is not None and done >= max_iter:
            break
    print('')
    save()
    return means['loss'], means['pr']


encoder_structure, decoder_structure = structures(latent_dim, 64)      # the reference's size (64^3); main rebuilds them for --voxel / --latent

if __name__ == '__main__':
    parser = []
    a = C.parse(__doc__, train=True, extra=lambda ap: (parser.append(ap), ap.set_defaults(latent=latent_dim)))
    if a.device_data or a.packed_data:
        parser[0].error('--device-data / --packed-data: this script reads the host loader only')
    voxvae.set_default_dtype(a.dtype)        # 'f32': exact-f32 parity mode; 'bf16': mixed precision (float32 master weights)
    if int(os.environ.get('WORLD_SIZE', '1')) > 1:
        import torch
        import torch.distributed as dist
        local = int(os.environ.get('LOCAL_RANK', '0'))
        torch.cuda.set_device(local)
        voxvae.set_default_device('cuda:%d' % local)
        dist.init_process_group('nccl')
    enc, dec = structures(a.latent, a.voxel)
    sys.exit(0 if train(training_epoch=a.epochs, learning_rate=a.lr, batch_per_replica=a.batch, dataset_path=a.dataset_path,
                        encoder_structure=enc, decoder_structure=dec, save_path=a.save_path, load_path=a.load_path,
                        max_iter=a.max_iter) is not None else 1)
