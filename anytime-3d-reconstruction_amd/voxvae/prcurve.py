"""Precision / recall-vs-threshold curves accumulated on the device (csrc/pr_curve.hip behind vv_pr_curve_accumulate).

The reference's test scripts collect `_gt.npy` / `_pred.npy` (test_modelnet_VAE.py:128-130, 159-165) and its notebooks sweep a list of
thresholds over them on the host, one numpy pass over all the data per threshold (modelnetAE3.ipynb / pascalAE3.ipynb cell 2), then
save the table (cell 3).  Here the prediction and the target are already in device memory when getEval returns, so one streaming pass
over them counts every threshold at once and only the integer counts ever leave the device:

    curve = PRCurve(thresholds)                  # or notebook_curve(div) for the notebook's own list
    for batch in split:
        model.getPRCurve(inputs, curve, ...)     # = getEval + curve.update(target, pred)
    table = notebook_table(curve, div)           # the array cell 3 saves

Counts are exact integers and additive: two updates equal one update of the concatenated batch, curves of shards are summed with
merge() / all_reduce().
"""
import ctypes

import numpy as np
import torch

MAX_THRESHOLDS = 256


def normalise_thresholds(thresholds, inclusive=False):
    """-> (eff, order, inverse).  eff: the float32 thresholds the kernel compares with `>` -- an inclusive one (p >= t) is replaced by
    its float32 predecessor, since p >= t <=> p > nextafter(t, -inf) for every finite float32 t; order: the stable permutation that
    sorts eff (the kernel gets eff[order], non-decreasing); inverse: position of the caller's threshold j in the sorted list, so
    result[..., inverse] is in the caller's order, duplicates included."""
    thr = np.asarray(thresholds, dtype=np.float32).reshape(-1)
    if not 1 <= thr.size <= MAX_THRESHOLDS:
        raise ValueError('between 1 and %d thresholds, got %d' % (MAX_THRESHOLDS, thr.size))
    inc = np.broadcast_to(np.asarray(inclusive, dtype=bool), thr.shape)
    eff = np.where(inc, np.nextafter(thr, np.float32(-np.inf), dtype=np.float32), thr).astype(np.float32)
    order = np.argsort(eff, kind='stable')
    inverse = np.empty_like(order)
    inverse[order] = np.arange(order.size)
    return eff, order, inverse


class PRCurve(object):
    """Pooled TP / FP / FN counts at `thresholds` for `groups` groups of samples (group = class index: per-category curves; group =
    sample index: per-sample counts).  `inclusive`: one bool or one per threshold -- False counts p > t (the notebook's sweep), True
    p >= t (function.py:110; the notebook's `>= 1.0` rows).  The int64 accumulators and the kernel's workspace live on `device`
    (default: voxvae's default device).  A curve on 'cpu' can hold, merge, reduce and tabulate counts; update() needs the GPU."""

    def __init__(self, thresholds, inclusive=False, groups=1, device=None):
        import voxvae
        self.thresholds = np.asarray(thresholds, dtype=np.float64).reshape(-1).copy()
        self.inclusive = np.broadcast_to(np.asarray(inclusive, dtype=bool), self.thresholds.shape).copy()
        self._eff, self._order, self._inverse = normalise_thresholds(self.thresholds, self.inclusive)
        self.groups = int(groups)
        if self.groups < 1:
            raise ValueError('groups must be >= 1, got %r' % (groups,))
        self.device = torch.device(voxvae.default_device() if device is None else device)
        self._acc = None          # int64 [G*T*2 + G*2]: (TP, FP) per (group, sorted threshold), then (occupied, voxels) per group
        self._thr_dev = None
        self._ws = None

    T = property(lambda self: self.thresholds.size)

    # ------------------------------------------------------------------------------------------------ storage
    def _accumulators(self):
        if self._acc is None:
            self._acc = torch.zeros(self.groups * (2 * self.T + 2), dtype=torch.int64, device=self.device)
        return self._acc

    def _split(self, acc):
        G, T = self.groups, self.T
        return acc[:G * T * 2].reshape(G, T, 2), acc[G * T * 2:].reshape(G, 2)      # views (contiguous slices), torch or numpy

    def reset(self):
        if self._acc is not None:
            self._acc.zero_()
        return self

    # ------------------------------------------------------------------------------------------------ accumulation
    def update(self, target, pred, group=None):
        """Adds one batch.  target / pred: torch CUDA tensor, DeviceArray, HostPrediction (its device tensor is used: nothing is
        re-uploaded), numpy array, or (target only) PackedVoxels, which is uploaded as bits and counted as bits.  Any shape [B, ...];
        a float target voxel is occupied iff y > 0.5.  group: None (everything in group 0), an int array [B], or a one-hot [B, G]
        (arg-max taken on the device); a sample whose group is outside [0, groups) is counted nowhere.  Runs on the current stream and
        does not synchronise."""
        from . import lib as L
        from .hostio import PackedVoxels
        from .tensor import DeviceArray, as_device_f32
        if self.device.type != 'cuda':
            raise L.VoxVaeError('PRCurve.update runs on the GPU only (this curve lives on %s); there is no CPU fallback' % self.device)
        p = as_device_f32(pred, self.device)
        B = int(p.shape[0]) if p.dim() else 0
        if B == 0:
            return self
        V = p.numel() // B
        if isinstance(target, PackedVoxels):
            if int(np.prod(target.shape)) != p.numel():
                raise ValueError('target %s and pred %s differ in size' % (tuple(target.shape), tuple(p.shape)))
            t, packed = torch.from_numpy(target.bits).to(self.device), 1
        else:
            t, packed = as_device_f32(target, self.device), 0
            if t.numel() != p.numel():
                raise ValueError('target %s and pred %s differ in size' % (tuple(t.shape), tuple(p.shape)))
        g = None
        if group is not None:
            if isinstance(group, DeviceArray):
                group = group.t
            g = group if isinstance(group, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(group))
            g = g.to(self.device)
            if g.dim() == 2 and g.shape[1] != 1:
                g = g.argmax(dim=1)
            g = g.reshape(-1).to(torch.int32).contiguous()
            if g.numel() != B:
                raise ValueError('group must have one entry (or one one-hot row) per sample: %d for a batch of %d' % (g.numel(), B))
        if self._thr_dev is None:
            self._thr_dev = torch.from_numpy(self._eff[self._order].copy()).to(self.device)
        need = L.load().vv_pr_curve_workspace_bytes(B, V, self.T)
        if self._ws is None or self._ws.numel() < need:
            self._ws = torch.empty(need, dtype=torch.uint8, device=self.device)
        tp_fp, totals = self._split(self._accumulators())
        L.call('vv_pr_curve_accumulate', L.ptr(p), L.ptr(t), packed, L.ptr(self._thr_dev), self.T, 1, L.ptr(g), self.groups,
               L.ptr(tp_fp), L.ptr(totals), L.ptr(self._ws), self._ws.numel(), B, V,
               ctypes.c_void_p(torch.cuda.current_stream(self.device).cuda_stream))
        return self

    def merge(self, other):
        """Adds another curve's counts (same thresholds and groups), e.g. of another shard or stream."""
        if not isinstance(other, PRCurve) or other.groups != self.groups or not np.array_equal(other._eff, self._eff):
            raise ValueError('curves with different thresholds or groups cannot be merged')
        if other._acc is not None:
            self._accumulators().add_(other._acc.to(self.device))
        return self

    def all_reduce(self):
        """Sums the counts over the initialised torch.distributed group (counts are additive, so every rank evaluates its own shard
        of the split); a no-op without one."""
        import torch.distributed as dist
        if not (dist.is_available() and dist.is_initialized()):
            return self
        acc = self._accumulators()
        if acc.is_cuda and dist.get_backend() == 'gloo':
            host = acc.cpu()                      # gloo reduces host tensors: the counts (a few KB) make the round trip
            dist.all_reduce(host)
            acc.copy_(host)
        else:
            dist.all_reduce(acc)
        return self

    def set_counts(self, TP, FP, occupied, voxels):
        """Replaces the counts (caller's threshold order): TP, FP [G, T]; occupied, voxels [G].  For counts saved earlier."""
        G, T = self.groups, self.T
        tp_fp = np.stack([np.asarray(TP, dtype=np.int64).reshape(G, T), np.asarray(FP, dtype=np.int64).reshape(G, T)], axis=-1)[:, self._order]
        totals = np.stack([np.asarray(occupied, dtype=np.int64).reshape(G), np.asarray(voxels, dtype=np.int64).reshape(G)], axis=-1)
        flat = np.concatenate([tp_fp.reshape(-1), totals.reshape(-1)])
        self._accumulators().copy_(torch.from_numpy(flat))
        return self

    # ------------------------------------------------------------------------------------------------ results
    def counts_device(self):
        """(TP, FP, FN [G, T], occupied, voxels [G]) as int64 tensors on the curve's device, caller's threshold order; no synchronise."""
        tp_fp, totals = self._split(self._accumulators())
        inv = torch.from_numpy(self._inverse).to(self.device)
        tp, fp = tp_fp[:, :, 0].index_select(1, inv), tp_fp[:, :, 1].index_select(1, inv)
        return tp, fp, totals[:, 0:1] - tp, totals[:, 0], totals[:, 1]

    def counts(self):
        """{'TP', 'FP', 'FN': int64 [G, T]; 'occupied', 'voxels': int64 [G]} as numpy, in the caller's threshold order.  The one call
        that synchronises."""
        acc = self._accumulators().cpu().numpy()
        tp_fp, totals = self._split(acc)
        tp, fp = tp_fp[:, self._inverse, 0], tp_fp[:, self._inverse, 1]
        return {'TP': tp.copy(), 'FP': fp.copy(), 'FN': totals[:, 0:1] - tp, 'occupied': totals[:, 0].copy(), 'voxels': totals[:, 1].copy()}

    def precision_recall(self):
        """float64 [G, T, 2] = (TP / (TP + FP + 1e-10), TP / (TP + FN + 1e-10)), the notebook's guards."""
        c = self.counts()
        return _precision_recall(c['TP'].astype(np.float64), c['FP'].astype(np.float64), c['FN'].astype(np.float64))


def _precision_recall(tp, fp, fn):
    return np.stack([tp / (tp + fp + 1e-10), tp / (tp + fn + 1e-10)], axis=-1)


# ---------------------------------------------------------------------------------------------------------------------------------
# The notebook's sweep, restated from its text (modelnetAE3.ipynb / pascalAE3.ipynb cell 2; the lists are printed by cell 0).

def notebook_thresholds(div, full=False):
    """The thresholds `test(yTarget, yPred, div)` of modelnetAE3.ipynb cell 2 sweeps with `yPred > prob`: the active list
    r2 = [(i+1)/div for i in range(div-1)], or with full=True the commented r1 + r2 + r3 list (r1 = 0.01^(2(div-i))/div down into the
    float32 denormals, r3 = 1 - 0.1^i/div; it holds (div-1)/div twice).  Python floats, as the notebook has them."""
    div = int(div)
    r2 = [(i + 1) * 1.0 / div for i in range(div - 1)]
    if not full:
        return r2
    r1 = [0.01 ** (2 * (div - i)) / div for i in range(div)]
    r3 = [1.0 - 0.1 ** (i) / div for i in range(div)]
    return r1 + r2 + r3


def notebook_curve(div, full=False, groups=1, device=None):
    """The PRCurve notebook_table needs: the notebook's exclusive thresholds followed by one inclusive 1.0 (the `np.greater_equal(yPred,
    1.0)` of its thinning rows)."""
    thr = notebook_thresholds(div, full)
    return PRCurve(thr + [1.0], [False] * len(thr) + [True], groups=groups, device=device)


def notebook_table(curve, div, rng=None, group=None):
    """The array cell 2 of modelnetAE3.ipynb returns and cell 3 saves: [len(thresholds) + div, 2] = (precision, recall), pooled over
    all groups (or of one `group`).  `curve`: a notebook_curve(div, ...) -- its last threshold is the inclusive 1.0.  Rows
    0 .. len-1 are the deterministic sweep.  Row len + i keeps each voxel with p >= 1.0 with probability a = 0.1^i: the notebook draws
    a full-size np.random.choice mask per row; here the rows are built from the single (TP1, FP1) pair counted at p >= 1.0 --
    rng=None: the expectation TP = a TP1, FP = a FP1, FN = occupied - a TP1;  rng (np.random.Generator / RandomState): TP ~
    Binomial(TP1, a), FP ~ Binomial(FP1, a), FN = occupied - TP, which is the distribution of the notebook's masked sums."""
    div = int(div)
    if curve.T < 2 or curve.thresholds[-1] != 1.0 or not curve.inclusive[-1]:
        raise ValueError('notebook_table needs a curve whose last threshold is the inclusive 1.0 (notebook_curve)')
    c = curve.counts()
    sel = slice(None) if group is None else [int(group)]
    tp, fp = c['TP'][sel].sum(axis=0).astype(np.float64), c['FP'][sel].sum(axis=0).astype(np.float64)
    occ = float(c['occupied'][sel].sum())
    tp1, fp1 = tp[-1], fp[-1]
    rows_tp, rows_fp = list(tp[:-1]), list(fp[:-1])
    for i in range(div):
        a = 0.1 ** i
        if rng is None:
            rows_tp.append(a * tp1)
            rows_fp.append(a * fp1)
        else:
            rows_tp.append(float(rng.binomial(int(tp1), a)))
            rows_fp.append(float(rng.binomial(int(fp1), a)))
    rows_tp, rows_fp = np.array(rows_tp), np.array(rows_fp)
    return _precision_recall(rows_tp, rows_fp, occ - rows_tp)
