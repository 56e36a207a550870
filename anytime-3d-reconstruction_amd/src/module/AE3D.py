"""Drop-in for the reference's src/module/AE3D.py: the data-parallel 3D autoencoder, the reference's one multi-GPU class.

Same constructor arguments, methods and return tuples.  A replica is a process with its own GPU (torch.distributed, one rank per
device) instead of a tf.distribute replica; `strategy` only has to carry `num_replicas_in_sync` and a `scope()`
(voxvae.train.ReplicaStrategy).  What the class computes, with the reference's lines:

  * the encoder sees 2x - 1, the loss target stays 0/1 (AE3D.py:70, 74);
  * every replica's loss is pred_loss / GLOBAL_BATCH + the UNSCALED reg_loss = 5e-4 * sum w^2 over every kernel and the Dense bias
    (AE3D.py:46-48, 82-84), and the gradients are summed across replicas (:86-87): the summed gradient carries world * 2 * 5e-4 * w,
    and distributed_fit reports rl = world * reg_loss (:95);
  * TP / FP / FN are summed over the GLOBAL batch and precision / recall formed from the sums (:51-59, 98-103), not averaged per sample.

The regulariser costs no pass of its own: its gradient enters inside the optimiser launch, which also leaves sum w^2 of the weights
the forward used (vv_adam_step_multi_l2), and the six scalars of a step come from one small launch (vv_ae3d_step_scalars).
`predict` is the one method beyond the reference.
"""
import os

import torch

import src.net_core.autoencoder3D as ae
from src.module.function import *  # noqa: F401,F403  (the reference's module does the same; binary_loss / voxelPrecisionRecall below)
from src.module import function as _F
from voxvae import lib as _L
from voxvae import synthetic as _syn
from voxvae import train as _T
from voxvae.tensor import DeviceArray, as_device_f32

# The module-level architecture example of the reference's file (its encoder ends in 400 channels against a decoder input_dim of 200 and
# cannot run; this pair is consistent): the 64^3 configuration with latent 200, from the one place the schema is written.
_example = _syn.make_config(64, 200, False, enc_name='encoder', dec_name='decoder')
encoder_structure, decoder_structure = _example['encoder'], _example['decoder']


class AE3D(object):
    def __init__(self, encoder_structure, decoder_structure,
                 BATCH_SIZE_PER_REPLICA=64, strategy=None,
                 learning_rate=1e-4):
        self._enc_str = encoder_structure
        self._dec_str = decoder_structure
        self._learning_rate = learning_rate
        if encoder_structure['filter_num_list'][-1] != decoder_structure['input_dim']:
            raise ValueError('the encoder ends in %d channels and the decoder takes input_dim %d: they must be equal'
                             % (encoder_structure['filter_num_list'][-1], decoder_structure['input_dim']))
        self._strategy = _T.ReplicaStrategy() if strategy is None else strategy
        self._world = _T.group_size()
        if int(self._strategy.num_replicas_in_sync) != self._world:
            raise ValueError('strategy.num_replicas_in_sync is %d but the process group has %d ranks'
                             % (int(self._strategy.num_replicas_in_sync), self._world))
        self._BATCH_SIZE_PER_REPLICA = BATCH_SIZE_PER_REPLICA
        self._GLOBAL_BATCH_SIZE = self._BATCH_SIZE_PER_REPLICA * self._world
        self._x_scaled = None          # the step's 2x - 1, a reused float32 buffer
        self.always_reduce = False     # True: issue the collectives in a one-rank group too (exercises the RCCL path on one GPU)
        with self._strategy.scope():
            self._buildModel()
            self._trainer = _T.Trainer(self._enc_eng, self._dec_eng, variational=False, learning_rate=self._learning_rate,
                                       world_size=self._world, weight_l2=ae.L2_REG)

    def _lossObject(self, y_target, y_pred, gamma=0.60):
        """AE3D.py:46-48: sum_b binary_loss_b / GLOBAL_BATCH."""
        loss = _F.binary_loss(xTarget=y_target, xPred=y_pred, gamma=gamma, b_range=False)
        return DeviceArray(loss.t.sum() / self._GLOBAL_BATCH_SIZE)

    def _evaluation(self, y_target, y_pred):
        """AE3D.py:51-59: (TP, FP, FN), each summed over the samples / GLOBAL_BATCH."""
        return tuple(DeviceArray(c.t.sum() / self._GLOBAL_BATCH_SIZE) for c in _F.voxelPrecisionRecall(xTarget=y_target, xPred=y_pred))

    def _buildModel(self):
        print('build Models...')
        self._encoder = ae.encoder3D(structure=self._enc_str)
        self._decoder = ae.decoder3D(structure=self._dec_str)
        self._enc_eng, self._dec_eng = self._encoder._engine, self._decoder._engine
        self._device = self._enc_eng.device
        print('done')

    def _rescaled(self, x):
        """2x - 1 (AE3D.py:70) written once per step into a buffer kept between steps."""
        if self._x_scaled is None or self._x_scaled.shape != x.shape:
            self._x_scaled = torch.empty_like(x)
            self._minus_one = torch.full((), -1.0, dtype=torch.float32, device=x.device)
        return torch.add(self._minus_one, x, alpha=2.0, out=self._x_scaled)      # one launch; 2x is exact, so one rounding as in 2x - 1

    def _fit_scalars(self, inputs):
        """One optimisation step -> the six per-replica scalars as one float32 device tensor."""
        input_images, output_images = inputs
        if len(input_images) != self._BATCH_SIZE_PER_REPLICA:
            # the losses and counts are scaled by GLOBAL_BATCH = BATCH_SIZE_PER_REPLICA * replicas (AE3D.py:38, 46-59), a constant of the
            # model; the step scales by the batch it is given.  One number only when the two agree.
            raise ValueError('a replica\'s batch has %d samples, BATCH_SIZE_PER_REPLICA is %d' % (len(input_images), self._BATCH_SIZE_PER_REPLICA))
        x = as_device_f32(input_images, self._device)
        y = x if output_images is input_images else as_device_f32(output_images, self._device)     # an (x, x) pair is uploaded once
        self._trainer.grads.always_reduce = self.always_reduce
        _, stats, _ = self._trainer.step(self._rescaled(x), y)
        return self._trainer.step_scalars(stats)

    def fit(self, inputs):
        """AE3D.py:67-90 -> (reg_loss, pred_loss, total_loss, TP, FP, FN) of THIS replica, GLOBAL_BATCH scaling included."""
        s = self._fit_scalars(inputs)
        return tuple(DeviceArray(s[i]) for i in range(6))

    def distributed_fit(self, inputs):
        """AE3D.py:92-104 -> (rl, pl, tl, p, r): every replica runs fit on its shard, the six scalars are summed across the replicas by
        ONE all-reduce, and precision / recall are formed from the summed counts.  One replica: no collective."""
        s = self._fit_scalars(inputs)
        if self._world > 1 or self.always_reduce:
            import torch.distributed as dist
            if dist.is_available() and dist.is_initialized():
                dist.all_reduce(s, op=dist.ReduceOp.SUM)
        p, r = self._precision_recall(s[3], s[4], s[5])
        return DeviceArray(s[0]), DeviceArray(s[1]), DeviceArray(s[2]), DeviceArray(p), DeviceArray(r)

    @staticmethod
    def _precision_recall(TP, FP, FN):
        """AE3D.py:102-103 on the counts SUMMED over the global batch (not the batch mean of per-sample ratios the other classes return)."""
        return TP / (TP + FP + 1e-10), TP / (TP + FN + 1e-10)

    def predict(self, input_images):
        """decoder(encoder(2x - 1)) with the moving statistics (the inference engines) -> occupancy probabilities [B,D,D,D,1]."""
        x = as_device_f32(input_images, self._device)
        z = self._enc_eng.forward(x * 2.0 - 1.0)
        out, _, _ = self._dec_eng.forward(z if self._dec_eng.dt == _L.VV_F32 else z.to(torch.bfloat16))
        return DeviceArray(out)

    def saveEncoder(self, save_path):
        file_name = self._enc_str['name']
        self._encoder.save_weights(os.path.join(save_path, file_name))

    def saveDecoder(self, save_path):
        file_name = self._dec_str['name']
        self._decoder.save_weights(os.path.join(save_path, file_name))

    def saveModel(self, save_path):
        self.saveEncoder(save_path=save_path)
        self.saveDecoder(save_path=save_path)

    def loadEncoder(self, load_path):
        file_name = self._enc_str['name']
        self._encoder.load_weights(os.path.join(load_path, file_name))

    def loadDecoder(self, load_path):
        file_name = self._dec_str['name']
        self._decoder.load_weights(os.path.join(load_path, file_name))

    def loadModel(self, load_path):
        self.loadEncoder(load_path=load_path)
        self.loadDecoder(load_path=load_path)
