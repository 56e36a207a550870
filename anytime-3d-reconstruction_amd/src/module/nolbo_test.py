"""Drop-in for the reference's multi-object inference class, src/module/nolbo_test.py: `config`, `nolbo_test(nolbo_structure,
backbone_style, encoder_backbone)`, `getPred(...)` and the load methods, with the reference's names, arguments and return tuples.

The image encoder (Darknet19 + head2D, last_pooling=None) is the stock-PyTorch mirror of src/net_core/darknet.py, as everywhere in
this package; everything after the head runs on the HIP path: voxvae.detect.decode_detections (activations, per-cell candidates,
greedy NMS: one launch), the sampled-mean decoder (getSampledShape of the model classes, the same code), and -- through getObjects,
an extension -- voxvae.pose.object_poses and voxvae.points.voxel_points, so that image -> detections -> shapes -> poses -> point
clouds stays on the device and only the counts are read back.

Drawing the boxes into `image_bbox2D` needs cv2; without it the undrawn copy is returned.
"""
import os

import numpy as np
import torch

import src.module.nolbo as _nolbo
import src.net_core.autoencoder3D as ae3D
import src.net_core.darknet as darknet
import voxvae
from voxvae.detect import channel_width, decode_detections, partition

config = {
    'encoder_backbone': {
        'name': 'nolbo_backbone',
        'predictor_num': 5,
        'bbox2D_dim': 4, 'bbox3D_dim': 3, 'orientation_dim': 3,
        'inst_dim': 10, 'z_inst_dim': 16,
        'activation': 'elu',
    },
    'encoder_head': {
        'name': 'nolbo_head',
        'output_dim': 5 * (1 + 4 + 3 + (2 * 3 + 3) + 2 * 16),
        'filter_num_list': [1024, 1024, 1024, 1024],
        'filter_size_list': [3, 3, 3, 1],
        'activation': 'elu',
    },
    'decoder': {
        'name': 'docoder',
        'input_dim': 16,
        'output_shape': [64, 64, 64, 1],
        'filter_num_list': [512, 256, 128, 64, 1],
        'filter_size_list': [4, 4, 4, 4, 4],
        'strides_list': [1, 2, 2, 2, 2],
        'activation': 'elu',
        'final_activation': 'sigmoid',
    },
}


class nolbo_test(object):
    SAMPLING_NUM = 32       # nolbo_test.py:171

    def __init__(self, nolbo_structure, backbone_style=None, encoder_backbone=None):
        self._enc_backbone_str = nolbo_structure['encoder_backbone']
        self._enc_head_str = nolbo_structure['encoder_head']
        self._dec_str = nolbo_structure['decoder']
        self._backbone_style = backbone_style
        self._encoder_backbone = encoder_backbone
        bb = self._enc_backbone_str
        if bb.get('bbox2D_dim', 4) != 4 or bb.get('bbox3D_dim', 3) != 3 or bb.get('orientation_dim', 3) != 3:
            raise ValueError('the detection decode is written for bbox2D_dim 4, bbox3D_dim 3, orientation_dim 3')
        self._buildModel()

    def _buildModel(self):
        print('build Models...')
        dev = voxvae.default_device() if torch.cuda.is_available() else 'cpu'
        if self._encoder_backbone is None:
            self._encoder_backbone = self._backbone_style(name=self._enc_backbone_str['name'], device=dev)
        self._encoder_head = darknet.head2D(name=self._enc_head_str['name'], input_shape=self._encoder_backbone.output_shape[1:],
                                            output_dim=self._enc_head_str['output_dim'],
                                            filter_num_list=self._enc_head_str['filter_num_list'],
                                            filter_size_list=self._enc_head_str['filter_size_list'], last_pooling=None,
                                            activation=self._enc_head_str['activation'], device=dev)
        # the decoder is HIP only: it is built on first use, so that the detection half (getPred(get_3D_shape=False, host=True)) also
        # works where there is no GPU; using it without one is the decoder's own error
        self._decoder_model = None
        print('done')

    @property
    def _decoder(self):
        if self._decoder_model is None:
            self._decoder_model = ae3D.decoder3D(structure=self._dec_str)
        return self._decoder_model

    # the sampled-mean path IS the model classes' (src/module/nolbo.py): these methods touch self._dev, _dec_eng, _device and _act_dt only
    _dev = _nolbo.nolboSingleObject_VAE._dev
    _scored = staticmethod(_nolbo._ModelnetBase._scored)
    getSampledShape = _nolbo._ModelnetBase.getSampledShape
    getSampledObjects = _nolbo._ModelnetBase.getSampledObjects

    @property
    def _dec_eng(self):
        return self._decoder._engine

    @property
    def _device(self):
        return self._dec_eng.device

    @property
    def _act_dt(self):
        return self._dec_eng.dt

    # ---------------------------------------------------------------- the head output
    def _encOutPartitioning(self):
        """The channel ranges of the head output's fields for this structure's predictor_num / z_inst_dim (nolbo_test.py:214-246);
        the activations of :247-255 are applied inside the decode kernel."""
        self._partition = partition(self._enc_backbone_str['predictor_num'], self._enc_backbone_str['z_inst_dim'])
        return self._partition

    def _head_output(self, input_image):
        """-> (images [B,row,col,3] as the caller gave them, head output [B,grid_row,grid_col,channels] where the head left it)."""
        input_image = np.asarray(input_image) if not torch.is_tensor(input_image) else input_image
        if input_image.shape[-1] != 3:              # a gray image
            input_image = (torch if torch.is_tensor(input_image) else np).stack([input_image] * 3, -1)
        if input_image.ndim != 4:
            input_image = input_image[None]
        P, Z = self._enc_backbone_str['predictor_num'], self._enc_backbone_str['z_inst_dim']
        self._enc_output = self._encoder_head(self._encoder_backbone(input_image, training=False), training=False)
        if self._enc_output.shape[-1] != P * channel_width(Z):
            raise ValueError('the head gives %d channels, predictor_num %d x z_inst_dim %d needs %d'
                             % (self._enc_output.shape[-1], P, Z, P * channel_width(Z)))
        return input_image, self._enc_output

    def _detect(self, input_image, obj_thresh, IOU_thresh, top_1_pred, image_reduced, host=False):
        input_image, enc = self._head_output(input_image)
        _, rows, cols, _ = input_image.shape
        self._gridSize = [int(cols / image_reduced), int(rows / image_reduced)]
        if [int(enc.shape[2]), int(enc.shape[1])] != self._gridSize:
            raise ValueError('the head output is a %d x %d grid, the image / image_reduced gives %d x %d'
                             % (enc.shape[1], enc.shape[2], self._gridSize[1], self._gridSize[0]))
        bb = self._enc_backbone_str
        det = decode_detections(enc[:1], bb['predictor_num'], bb['z_inst_dim'], obj_thresh, IOU_thresh, top_1_pred, host=host)   # frame 0, as the reference
        return input_image, det

    def getPred(self, input_image, obj_thresh=0.5, IOU_thresh=0.5, top_1_pred=True, get_3D_shape=True, is_sampling=True, image_reduced=32,
                *, host=False, _eps=None):
        """nolbo_test.py:81-188 -> (image_bbox2D, bbox2D_selected, bbox3D_selected, sin_mean_selected, cos_mean_selected,
        rad_log_var_selected[, outputs_3D_shape]) as numpy.  The shapes: the sampled mean over 32 latents per detection (is_sampling;
        `_eps` [M,32,Z] injects the draw) or the plain decode of the means.  host=True (an extension) decodes the detections with the
        host entry; the shapes need the GPU either way."""
        input_image, det = self._detect(input_image, obj_thresh, IOU_thresh, top_1_pred, image_reduced, host)
        bbox2D, bbox3D, sin, cos, rad, mean, logvar = det.numpy(0)
        first = input_image[0]
        image_bbox2D = np.array(first.cpu() if torch.is_tensor(first) else first).copy()
        try:
            import cv2
        except ImportError:
            cv2 = None
        if cv2 is not None:
            imrow, imcol, _ = image_bbox2D.shape
            for b in bbox2D:
                cv2.rectangle(img=image_bbox2D, pt1=(int(b[0] * imcol), int(b[1] * imrow)), pt2=(int(b[2] * imcol), int(b[3] * imrow)),
                              color=(0, 255, 0), thickness=2)
        if not get_3D_shape:
            return image_bbox2D, bbox2D, bbox3D, sin, cos, rad
        if len(mean) == 0:
            return image_bbox2D, bbox2D, bbox3D, sin, cos, rad, np.array([])
        _, _, _, _, _, mean_d, logvar_d = det.frame(0)
        if is_sampling:
            shapes = self.getSampledShape(mean_d, logvar_d, self.SAMPLING_NUM, _eps=_eps)
        else:
            shapes = self._decoder(mean_d)
        D = self._dec_eng.D
        return image_bbox2D, bbox2D, bbox3D, sin, cos, rad, np.array(shapes).reshape(-1, D, D, D)

    def getObjects(self, input_image, image_size=None, proj_mat=None, sampling_num=32, obj_thresh=0.5, IOU_thresh=0.5, top_1_pred=True,
                   image_reduced=32, proj_mat_inv=None, prob=0.5, surface_only=False, *, _eps=None):
        """The whole chain for one frame on the device: head output -> Detections -> sampled-mean shapes -> ObjectPoses -> PointCloud
        (getPred followed by visualizer.getObjectInRealWorld in the reference).  image_size = (cols, rows), None: the input image's.
        Returns (Detections, ObjectPoses or None, PointCloud or None): both None without a detection, the cloud None when no pose
        is kept.  Read back: the detection count, the kept-pose count and the cloud's total."""
        input_image, det = self._detect(input_image, obj_thresh, IOU_thresh, top_1_pred, image_reduced)
        if det.counts()[0] == 0:
            return det, None, None
        b2, b3, sn, cs, _, mean, logvar = det.frame(0)
        if image_size is None:
            image_size = (int(input_image.shape[2]), int(input_image.shape[1]))
        poses, cloud = self.getSampledObjects(mean, logvar, b2, b3, sn, cs, image_size, sampling_num, proj_mat, proj_mat_inv, prob,
                                              surface_only, _eps=_eps)
        return det, poses, cloud

    # ---------------------------------------------------------------- checkpoints (nolbo_test.py:190-212)
    def loadEncoderBackbone(self, load_path, file_name=None):
        if file_name == None:
            file_name = self._enc_backbone_str['name']
        self._encoder_backbone.load_weights(os.path.join(load_path, file_name))

    def loadEncoderHead(self, load_path, file_name=None):
        if file_name == None:
            file_name = self._enc_head_str['name']
        self._encoder_head.load_weights(os.path.join(load_path, file_name))

    def loadEncoder(self, load_path):
        self.loadEncoderBackbone(load_path=load_path)
        self.loadEncoderHead(load_path=load_path)

    def loadDecoder(self, load_path, file_name=None):
        if file_name == None:
            file_name = self._dec_str['name']
        self._decoder.load_weights(os.path.join(load_path, file_name))

    def loadModel(self, load_path):
        self.loadEncoder(load_path=load_path)
        self.loadDecoder(load_path=load_path)
