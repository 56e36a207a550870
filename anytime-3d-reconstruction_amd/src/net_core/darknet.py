"""2D image encoders of the image -> 3D models, mirror of the reference's src/net_core/darknet.py.

Outside the voxel hot path: stock PyTorch ops by default; `engine='hip'` (or voxvae.set_image_engine('hip'))
runs the inference form on the HIP 2D convolution instead (voxvae/conv2d.py, csrc/conv2d.hip).  Same builder
names and arguments as the reference -- `Darknet19(name, activation)` (darknet.py:96-135) and
`head2D(name, input_shape, output_dim, filter_num_list, filter_size_list, last_pooling, activation)`
(darknet.py:152-173) -- returning callables `model(x, training=False)` over channels-last images [B,H,W,3] with the
Keras attributes the model classes use: `.output_shape`, `.trainable_variables`, `.losses`, `.save_weights`,
`.load_weights`.

Keras semantics restated: Conv2D 'same' stride 1 without bias, BatchNormalization(momentum 0.99, epsilon 1e-3),
ELU / LeakyReLU(0.1) / ReLU, MaxPool2D(2, 2, 'same') (= ceil-mode pooling), Glorot-uniform kernels, and the
kernel_regularizer l2(0.0005) that the head's convolutions (darknet.py:140-141,160-161) and every Darknet53Conv (:20) carry.

`Darknet53(name, activation)` / `Darknet53Tiny(name, activation)` (darknet.py:11-81) return TUPLES of feature maps, (x_36, x_61, x) and
(x_8, x); `.output_shape` is the last one's, `.output_shapes` lists all, and `last_output` is the rule every caller picks by.
"""
import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F


def _act(name):
    if name == 'lrelu':
        return nn.LeakyReLU(0.1)
    if name == 'elu':
        return nn.ELU()
    if name == 'relu':
        return nn.ReLU()
    return nn.Identity()


class _ConvBNAct(nn.Module):
    """Darknet19Conv / convHead (darknet.py:83-94, 137-150): Conv2D(same, no bias) -> BatchNormalization -> activation."""

    def __init__(self, cin, cout, k, activation, l2=0.0, stride=1):
        super().__init__()
        # Darknet53Conv(strides=2) (darknet.py:11-18): ZeroPadding2D(((1, 0), (1, 0))) in forward, then a 'valid' convolution
        self.stride = stride
        self.conv = nn.Conv2d(cin, cout, k, stride=stride, padding=k // 2 if stride == 1 else 0, bias=False)
        nn.init.xavier_uniform_(self.conv.weight)
        self.bn = nn.BatchNorm2d(cout, eps=1e-3, momentum=0.01)   # Keras momentum 0.99 = torch momentum 0.01
        self.act = _act(activation)
        self.l2 = l2

    def forward(self, x):
        if self.stride != 1:
            x = F.pad(x, (1, 0, 1, 0))
        return self.act(self.bn(self.conv(x)))


class _Pool1Same(nn.Module):
    """MaxPool2D(2, 1, 'same') (darknet.py:77): the input's grid, padding only at the end."""

    def forward(self, x):
        return F.max_pool2d(F.pad(x, (0, 1, 0, 1), value=float('-inf')), 2, 1)


def last_output(out):
    """The feature map a head takes from a backbone's output: the last element of Darknet53's / Darknet53Tiny's tuple (the reference's
    classifier.py:78-81), the output itself for every other backbone.  Every module here applies it to what it is called on, so
    `head(backbone(x))` -- the form nolbo_test and the image models use -- works for all three backbones; classifier and the image models
    also call it themselves where they take the backbone's output."""
    return out[-1] if isinstance(out, tuple) else out


class _Keras2D(nn.Module):
    """Channels-last in / out, `model(x, training=...)` call form, and the handful of Keras attributes the callers use."""

    def __init__(self, name, device=None, engine=None):
        super().__init__()
        self.name = name
        self._device = torch.device(device if device is not None else ('cuda:0' if torch.cuda.is_available() else 'cpu'))
        import voxvae
        self._engine = voxvae.image_engine() if engine is None else engine
        if self._engine not in ('torch', 'hip'):
            raise ValueError(self._engine)
        self._chain = None

    def _finish(self):
        self.to(self._device)
        self.eval()
        if self._engine == 'hip':
            # inference calls run csrc/conv2d.hip (voxvae.conv2d.Conv2dChain); this module keeps the parameters and the training form.
            # No GPU: VoxVaeError, as for the 3D builders -- no fallback to the torch ops.
            from voxvae.conv2d import Conv2dChain
            self._chain = Conv2dChain(self)
        return self

    def body(self, x):
        raise NotImplementedError

    def _hip_forward(self, x):
        """[B,R,C,Cin] -> the chain's float32 channels-last output, pooled as the module's forward pools it."""
        return self._chain(x)

    def __call__(self, x, training=False):
        x = last_output(x)                                  # a head called on Darknet53's / Darknet53Tiny's tuple takes the last map
        if not torch.is_tensor(x):
            x = torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32))
        x = x.to(self._device, torch.float32)
        if self._chain is not None and not training:
            self.train(False)
            with torch.no_grad():
                return self._hip_forward(x)
        self.train(bool(training))
        with torch.set_grad_enabled(bool(training)):
            return nn.Module.__call__(self, x)

    def forward(self, x):
        return self.body(x.permute(0, 3, 1, 2))

    @property
    def trainable_variables(self):
        return [p for p in self.parameters() if p.requires_grad]

    @property
    def losses(self):
        """Keras `model.losses`: one l2 term per regularised kernel."""
        return [m.l2 * (m.conv.weight ** 2).sum() for m in self.modules() if isinstance(m, _ConvBNAct) and m.l2 > 0] + \
               [l2 * (w ** 2).sum() for w, l2 in getattr(self, '_extra_l2', [])]

    def save_weights(self, path):
        torch.save(self.state_dict(), path + '.pt')

    def load_weights(self, path):
        self.load_state_dict(torch.load(path + '.pt', map_location=self._device))


class _Darknet19(_Keras2D):
    # (filters, kernel) runs separated by 'M' = MaxPool2D(2, 2, 'same'); darknet.py:99-133
    _PLAN = [(32, 3), 'M', (64, 3), 'M', (128, 3), (64, 1), (128, 3), 'M', (256, 3), (128, 1), (256, 3), 'M',
             (512, 3), (256, 1), (512, 3), (256, 1), (512, 3), 'M', (1024, 3), (512, 1), (1024, 3), (512, 1), (1024, 3)]

    def __init__(self, name=None, activation='elu', device=None, engine=None):
        super().__init__(name, device, engine)
        layers, cin = [], 3
        for item in self._PLAN:
            if item == 'M':
                layers.append(nn.MaxPool2d(2, 2, ceil_mode=True))
            else:
                layers.append(_ConvBNAct(cin, item[0], item[1], activation))
                cin = item[0]
        self.layers = nn.Sequential(*layers)
        self.output_shape = (None, None, None, cin)
        self._finish()

    def body(self, x):
        return self.layers(x).permute(0, 2, 3, 1)


class _Head2D(_Keras2D):
    def __init__(self, name, input_shape, output_dim, filter_num_list, filter_size_list, last_pooling=None, activation='elu',
                 device=None, engine=None):
        super().__init__(name, device, engine)
        cin, layers = int(input_shape[-1]), []
        for c, k in zip(filter_num_list, filter_size_list):
            layers.append(_ConvBNAct(cin, c, k, activation, l2=0.0005))
            cin = c
        self.layers = nn.Sequential(*layers)
        self.last = nn.Conv2d(cin, output_dim, 1, bias=False)
        nn.init.xavier_uniform_(self.last.weight)
        self._extra_l2 = [(self.last.weight, 0.0005)]
        self.last_pooling = last_pooling
        self.output_shape = (None, output_dim) if last_pooling in ('max', 'average') else (None, None, None, output_dim)
        self._finish()

    def forward(self, x):                                  # input is the backbone's channels-last feature map
        x = self.last(self.layers(x.permute(0, 3, 1, 2)))
        if self.last_pooling == 'max':
            return x.amax(dim=(2, 3))
        if self.last_pooling == 'average':
            return x.mean(dim=(2, 3))
        return x.permute(0, 2, 3, 1)

    def _hip_forward(self, x):
        y = self._chain(x)                                  # float32 [B,R,C,output_dim]
        if self.last_pooling == 'max':
            from voxvae.conv2d import max_over_positions
            return max_over_positions(y)
        if self.last_pooling == 'average':
            return y.mean(dim=(1, 2))                       # a torch reduction on the float32 head output (include/voxvae.h says so)
        return y


class _Darknet53(_Keras2D):
    """Darknet53 / Darknet53Tiny (darknet.py:11-81) as a flat list of steps: `layers[i]` is a _ConvBNAct or a pool, `_res[i]` the step
    whose output is added behind step i (Darknet53Residual: inputs + conv3x3(conv1x1(inputs))), `_taps` the steps whose outputs leave
    the model in front of the last one.  Every kernel carries l2 0.0005 (darknet.py:20)."""
    L2 = 0.0005

    def __init__(self, name=None, activation='elu', device=None, engine=None, tiny=False):
        super().__init__(name, device, engine)
        self.layers, self._res, self._taps, self._widths = nn.ModuleList(), {}, [], []
        self._cin = 3
        if tiny:
            self._build_tiny(activation)
        else:
            self._build_53(activation)
        self.output_shapes = [(None, None, None, self._widths[t]) for t in self._taps] + [(None, None, None, self._cin)]
        self.output_shape = self.output_shapes[-1]       # what head2D(input_shape=backbone.output_shape[1:]) needs: the LAST output's
        self._finish()

    def _conv(self, cout, k, activation, stride=1, res=None):
        self.layers.append(_ConvBNAct(self._cin, cout, k, activation, l2=self.L2, stride=stride))
        self._cin = cout
        self._widths.append(cout)
        if res is not None:
            self._res[len(self.layers) - 1] = res

    def _pool(self, stride):
        self.layers.append(nn.MaxPool2d(2, 2, ceil_mode=True) if stride == 2 else _Pool1Same())
        self._widths.append(self._cin)

    def _build_53(self, activation):
        self._conv(32, 3, activation)
        for filters, blocks, tap in ((64, 1, False), (128, 2, False), (256, 8, True), (512, 8, True), (1024, 4, False)):
            self._conv(filters, 3, activation, stride=2)
            for _ in range(blocks):
                src = len(self.layers) - 1
                self._conv(filters // 2, 1, activation)
                self._conv(filters, 3, 'elu', res=src)   # darknet.py:35 passes no activation: always ELU, whatever the backbone's is
            if tap:
                self._taps.append(len(self.layers) - 1)  # x_36, x_61

    def _build_tiny(self, activation):
        for filters in (16, 32, 64, 128):
            self._conv(filters, 3, activation)
            self._pool(2)
        self._conv(256, 3, activation)
        self._taps.append(len(self.layers) - 1)          # x_8
        self._pool(2)
        self._conv(512, 3, activation)
        self._pool(1)
        self._conv(1024, 3, activation)

    def body(self, x):
        keep, held = set(self._res.values()) | set(self._taps), {}
        for i, m in enumerate(self.layers):
            x = m(x)
            if i in self._res:
                src = self._res[i]
                x = (held[src] if src in self._taps else held.pop(src)) + x      # a block's input is added once: let it go
            if i in keep:
                held[i] = x
        outs = [held[t] for t in self._taps] + [x]
        return tuple(o.permute(0, 2, 3, 1) for o in outs)


def Darknet53(name=None, activation='elu', device=None, engine=None):
    """-> model(x) = (x_36, x_61, x): strides 8, 16 and 32 (darknet.py:46-56).  engine as for Darknet19."""
    print('Darknet53', name)
    m = _Darknet53(name=name, activation=activation, device=device, engine=engine)
    print('end Darknet53')
    return m


def Darknet53Tiny(name=None, activation='elu', device=None, engine=None):
    """-> model(x) = (x_8, x): strides 16 and 32 (darknet.py:58-81)."""
    print('Darknet53Tiny', name)
    m = _Darknet53(name=name, activation=activation, device=device, engine=engine, tiny=True)
    print('end Darknet53Tiny')
    return m


def Darknet19(name=None, activation='elu', device=None, engine=None):
    """engine: 'torch' | 'hip' | None = voxvae.image_engine() now.  'hip' runs calls with training=False on csrc/conv2d.hip."""
    print('Darknet19', name)
    m = _Darknet19(name=name, activation=activation, device=device, engine=engine)
    print('end Darknet19')
    return m


def head2D(name, input_shape, output_dim, filter_num_list, filter_size_list, last_pooling=None, activation='elu', device=None, engine=None):
    print('head start')
    m = _Head2D(name, input_shape, output_dim, filter_num_list, filter_size_list, last_pooling, activation, device, engine)
    print('end head2D')
    return m
