"""The image classifier that pre-trains the 2D backbones, mirror of the reference's src/module/classifier.py:7-131: a darknet backbone
(Darknet19, Darknet53, Darknet53Tiny) under a `head2D` with `last_pooling='average'`, trained with softmax cross entropy.

Same constructor arguments, method names and return tuples as the reference.  Training runs on the torch modules, as all 2D training
does here (fit / distributed_fit call the models with training=True, which never enters the HIP engine); inference calls (`predict`)
follow the image engine of the models: `voxvae.set_image_engine('hip')` or `engine='hip'` models run csrc/conv2d.hip.  `strategy=None`
is one replica; a strategy object only has to carry `num_replicas_in_sync`.
"""
import os

import numpy as np
import torch

import src.net_core.darknet as darknet


class classifier(object):
    def __init__(self, backbone_style=None, model_backbone=None, name=None, BATCH_SIZE_PER_REPLICA=64, strategy=None,
                 output_dim=1000, is_training=True,
                 backbone_activation='elu', head_activation='elu',
                 last_filter_num_list=[],
                 last_filter_size_list=[],
                 last_pooling='average',
                 learning_rate=1e-4):
        if name is None:
            name = 'None'
        self._name = name
        self._backbone_style = backbone_style
        self.model_backbone = model_backbone
        self._output_dim = output_dim
        self._is_training = is_training
        self._b_act, self._h_act = backbone_activation, head_activation
        self._last_fnl = last_filter_num_list
        self._last_fsl = last_filter_size_list
        self._last_pooling = last_pooling
        self._learning_rate = learning_rate

        self._strategy = strategy
        self._BATCH_SIZE_PER_REPLICA = BATCH_SIZE_PER_REPLICA
        replicas = 1 if strategy is None else int(strategy.num_replicas_in_sync)
        if replicas != 1:
            raise NotImplementedError('classifier trains on one replica; %d asked for' % replicas)
        self._GLOBAL_BATCH_SIZE = self._BATCH_SIZE_PER_REPLICA * replicas

        self._buildModel()
        self._optimizer = torch.optim.Adam(self.model_backbone.trainable_variables + self.model_head.trainable_variables,
                                           lr=self._learning_rate, eps=1e-7)                  # Keras Adam's epsilon

    def _lossObject(self, y_target, y_pred):
        """classifier.py:37-41: sum_b -sum(y log(softmax(pred) + 1e-9)) / global batch."""
        y_pred = torch.softmax(y_pred, dim=-1)
        loss = -(y_target * torch.log(y_pred + 1e-9)).sum(-1)
        return loss.sum() / self._GLOBAL_BATCH_SIZE

    def _evaluation(self, y_target, y_pred):
        """classifier.py:43-59: (top-1, top-5) hits summed over the batch / global batch."""
        gt = y_target.argmax(-1)
        acc_top1 = (y_pred.argmax(-1) == gt).float()
        k = min(5, y_pred.shape[-1])
        # tf.math.in_top_k: the target is in the top k when fewer than k classes score strictly higher
        higher = (y_pred > y_pred.gather(-1, gt[:, None])).sum(-1)
        acc_top5 = (higher < k).float()
        return acc_top1.sum() / self._GLOBAL_BATCH_SIZE, acc_top5.sum() / self._GLOBAL_BATCH_SIZE

    def _buildModel(self):
        print('build Models...')
        if self.model_backbone is None:
            self.model_backbone = self._backbone_style(name=self._name + '_backbone', activation=self._b_act)
        # ================================= set model head
        self.model_head = darknet.head2D(name='head_' + self._name,
                                         input_shape=self.model_backbone.output_shape[1:],
                                         output_dim=self._output_dim,
                                         filter_num_list=self._last_fnl, filter_size_list=self._last_fsl,
                                         last_pooling=self._last_pooling, activation=self._h_act,
                                         device=getattr(self.model_backbone, '_device', None))

    def _labels(self, y, like):
        if not torch.is_tensor(y):
            y = torch.from_numpy(np.ascontiguousarray(y, dtype=np.float32))
        return y.to(like.device, torch.float32)

    def predict(self, input_images):
        """Inference: the class scores [B, output_dim] (float32, on the models' device), on the image engine the models were built with."""
        features = darknet.last_output(self.model_backbone(input_images, training=False))
        return self.model_head(features, training=False)

    def fit(self, inputs):
        """classifier.py:73-96: one Adam step on backbone + head.  -> (reg_loss, pred_loss, total_loss, acc_top1, acc_top5) as floats;
        total = pred_loss (the reference leaves the l2 terms out of the step and only reports them)."""
        input_images, output_labels_gt = inputs
        self._optimizer.zero_grad(set_to_none=True)
        output_backbone = darknet.last_output(self.model_backbone(input_images, training=True))
        output_labels_pred = self.model_head(output_backbone, training=True)
        output_labels_gt = self._labels(output_labels_gt, output_labels_pred)
        with torch.no_grad():
            reg_loss = torch.stack(list(self.model_backbone.losses) + list(self.model_head.losses)).sum()
        pred_loss = self._lossObject(y_target=output_labels_gt, y_pred=output_labels_pred)
        total_loss = pred_loss  # + reg_loss
        total_loss.backward()
        self._optimizer.step()
        with torch.no_grad():
            acc_top1, acc_top5 = self._evaluation(y_pred=output_labels_pred.detach(), y_target=output_labels_gt)
        return float(reg_loss), float(pred_loss.detach()), float(total_loss.detach()), float(acc_top1), float(acc_top5)

    def distributed_fit(self, inputs):
        """classifier.py:98-107 on one replica: the per-replica results ARE the sums."""
        return self.fit(inputs)

    def saveBackbone(self, save_path):
        file_name = self._name + '_backbone'
        self.model_backbone.save_weights(os.path.join(save_path, file_name))

    def saveHead(self, save_path):
        file_name = self._name + '_head'
        self.model_head.save_weights(os.path.join(save_path, file_name))

    def saveModel(self, save_path):
        self.saveBackbone(save_path=save_path)
        self.saveHead(save_path=save_path)

    def loadBackbone(self, load_path):
        file_name = self._name + '_backbone'
        self.model_backbone.load_weights(os.path.join(load_path, file_name))

    def loadHead(self, load_path):
        file_name = self._name + '_head'
        self.model_head.load_weights(os.path.join(load_path, file_name))

    def loadModel(self, load_path):
        self.loadBackbone(load_path=load_path)
        self.loadHead(load_path=load_path)
