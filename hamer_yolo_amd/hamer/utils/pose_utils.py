"""hamer/utils/pose_utils.py of the reference, on one HIP kernel per batch (hm_pose_eval, csrc/pose_eval.hip).

Same names and call signatures: ``compute_similarity_transform``, ``reconstruction_error``, ``eval_pose``, ``Evaluator``,
``EvaluatorPCK``.  The similarity Procrustes, both error means, the root subtraction and the keypoint selection run inside the
kernel (fp64 sums and 3 x 3 solve, one rounding to fp32); nothing is copied to the host unless the reference's return type is
a numpy array.  There is no CPU fallback: without the library or a GPU every call raises ``HipLibraryError``.
"""
from __future__ import annotations

import ctypes as C
from typing import Dict, List, Optional, Tuple

import numpy as np
import torch

from ... import lib as L

MAX_POINTS = 1024


def _device() -> torch.device:
    L.load()                                            # HipLibraryError when the library is missing
    if not torch.cuda.is_available():
        raise L.HipLibraryError("hm_pose_eval needs a GPU; there is no CPU path")
    return torch.device("cuda", torch.cuda.current_device())


def _f32(t, dev: torch.device) -> torch.Tensor:
    """Any float tensor or array, host or device -> contiguous fp32 on the device (a new tensor unless it already is one)."""
    t = torch.as_tensor(t)
    return t.detach().to(device=dev, dtype=torch.float32).contiguous()


def _sel_words(sel, P: int):
    words = (C.c_uint64 * 16)()
    if sel is None:
        return words, P
    sel = [int(i) for i in sel]
    if len(set(sel)) != len(sel):
        raise ValueError("keypoint_list holds an index twice: the selection is a mask, every point counts once")
    if any(i < 0 or i >= P for i in sel):
        raise ValueError(f"keypoint_list holds an index outside 0..{P - 1}")
    for i in sel:
        words[i >> 6] |= 1 << (i & 63)
    return words, (len(sel) if sel else P)


def pose_eval(pred: torch.Tensor, gt: torch.Tensor, root: int = -1, sel=None, err: Optional[torch.Tensor] = None,
              pa_err: Optional[torch.Tensor] = None, want=("err", "pa_err")) -> Dict[str, torch.Tensor]:
    """One hm_pose_eval launch.  pred (B, P, 3) and gt (B, P, 3 or 4) fp32 contiguous device tensors; ``sel``: point indices
    (None: all); ``root``: index subtracted from every point first, or -1.  ``want`` names the outputs to compute out of
    ``err``, ``pa_err``, ``aligned``, ``transform``; ``err`` / ``pa_err`` may be given as (B,) fp32 device slices to fill.
    Asynchronous on the current stream."""
    if not (pred.is_cuda and gt.is_cuda):
        raise L.HipLibraryError("libhamer_hip kernels take device tensors; there is no CPU path")
    if pred.dim() != 3 or gt.dim() != 3 or pred.shape[2] != 3 or gt.shape[:2] != pred.shape[:2] or gt.shape[2] not in (3, 4):
        raise ValueError(f"pose_eval: pred {tuple(pred.shape)} / gt {tuple(gt.shape)}: expected (B, P, 3) and (B, P, 3 or 4)")
    assert pred.dtype == torch.float32 and gt.dtype == torch.float32 and pred.is_contiguous() and gt.is_contiguous()
    B, P = int(pred.shape[0]), int(pred.shape[1])
    if B == 0:
        raise ValueError("pose_eval: empty batch")
    words, n_sel = _sel_words(sel, P)
    out: Dict[str, torch.Tensor] = {}
    for name, given in (("err", err), ("pa_err", pa_err)):
        if given is not None:
            assert given.is_cuda and given.dtype == torch.float32 and given.shape == (B,) and given.is_contiguous()
            out[name] = given
        elif name in want:
            out[name] = torch.empty(B, device=pred.device, dtype=torch.float32)
    if "aligned" in want:
        out["aligned"] = torch.empty(B, n_sel, 3, device=pred.device, dtype=torch.float32)
    if "transform" in want:
        out["transform"] = torch.empty(B, 13, device=pred.device, dtype=torch.float32)
    a = L.PoseEvalArgs(pred=L.ptr(pred), gt=L.ptr(gt), B=B, P=P, gt_stride=int(gt.shape[2]), root=int(root), sel=words,
                       err=L.ptr(out.get("err")), pa_err=L.ptr(out.get("pa_err")), aligned=L.ptr(out.get("aligned")),
                       transform=L.ptr(out.get("transform")))
    L.check(L.load().hm_pose_eval(C.byref(a), L.current_stream()), "hm_pose_eval")
    return out


def compute_similarity_transform(S1: torch.Tensor, S2: torch.Tensor) -> torch.Tensor:
    """pose_utils.py:9-58: S1 (B, N, 3) aligned onto S2 (B, N, 3) by the best similarity (scale, rotation, translation);
    returns S1_hat (B, N, 3), an fp32 device tensor.  N <= 1024."""
    dev = _device()
    return pose_eval(_f32(S1, dev), _f32(S2, dev), want=("aligned",))["aligned"]


def reconstruction_error(S1, S2) -> torch.Tensor:
    """pose_utils.py:60-71: mean distance of S1 to S2 after the Procrustes alignment, (B,) fp32 on the device."""
    dev = _device()
    return pose_eval(_f32(S1, dev), _f32(S2, dev), want=("pa_err",))["pa_err"]


def eval_pose(pred_joints, gt_joints) -> Tuple[np.ndarray, np.ndarray]:
    """pose_utils.py:73-87: joint errors in mm before and after Procrustes alignment, two numpy arrays (one copy)."""
    dev = _device()
    o = pose_eval(_f32(pred_joints, dev), _f32(gt_joints, dev))
    both = torch.stack([o["err"], o["pa_err"]]).double().cpu().numpy()      # (float64: the factor adds no second rounding)
    return 1000 * both[0], 1000 * both[1]


_MM = ('mode_mpjpe', 'mode_re', 'min_mpjpe', 'min_re', 'opt_mpjpe', 'opt_re')
# metric name -> (device buffer, factor): mode_* and min_* share a buffer because num_samples is 1, in the reference too
_STORE = {'mode_mpjpe': ('mpjpe', 1000.0), 'min_mpjpe': ('mpjpe', 1000.0), 'mode_re': ('re', 1000.0), 'min_re': ('re', 1000.0),
          'opt_mpjpe': ('opt_mpjpe', 1000.0), 'opt_re': ('opt_re', 1000.0), 'mode_kpl2': ('kpl2', 1.0), 'min_kpl2': ('kpl2', 1.0)}


class Evaluator:
    """pose_utils.py:89-223.  The per-sample metrics live in device buffers of ``dataset_length`` (metres, fp32) which the
    kernel fills at ``counter``; ``evaluator.mode_mpjpe`` etc. are read-only properties that copy them into float64 numpy
    arrays of that length in mm, as the reference's attributes are (the factor 1000 is applied in float64: no second
    rounding).  Every read of such a property synchronises and copies, and returns a fresh array: unlike the reference's
    attributes, writing into the result changes nothing in the evaluator.  Read it once, or use ``get_metrics_dict()``.

    Unlike the reference (:164 subtracts the pelvis from a view of ``output['pred_keypoints_3d']``, in place), a call leaves
    the caller's tensors alone: the root subtraction happens inside the kernel."""

    def __init__(self,
                 dataset_length: int,
                 keypoint_list: List,
                 pelvis_ind: int,
                 metrics: List = ['mode_mpjpe', 'mode_re', 'min_mpjpe', 'min_re'],
                 pck_thresholds: Optional[List] = None):
        kl = [int(i) for i in keypoint_list]
        if len(set(kl)) != len(kl):
            raise ValueError("keypoint_list holds an index twice: the selection is a mask, every point counts once")
        if any(i < 0 or i >= MAX_POINTS for i in kl) or not kl:
            raise ValueError(f"keypoint_list must hold indices in 0..{MAX_POINTS - 1}")
        self.dataset_length = int(dataset_length)
        self.keypoint_list = keypoint_list
        self.pelvis_ind = int(pelvis_ind)
        self.metrics = metrics
        self._buf: Dict[str, torch.Tensor] = {}         # allocated at the first call (the constructor needs no GPU)
        self.counter = 0
        self.pck_evaluator = None if pck_thresholds is None else EvaluatorPCK(pck_thresholds)
        for metric in self.metrics:                     # a name this class does not compute: the reference's zeros
            if metric not in _STORE:
                setattr(self, metric, np.zeros((self.dataset_length,)))

    def _arrays(self, names) -> Dict[str, np.ndarray]:
        """Metric name -> float64 array of dataset_length: the buffers behind ``names`` in ONE copy."""
        keys = sorted({_STORE[n][0] for n in names if n in _STORE and _STORE[n][0] in self._buf})
        host = dict(zip(keys, torch.stack([self._buf[k].double() for k in keys]).cpu().numpy())) if keys else {}
        zeros = np.zeros((self.dataset_length,))
        return {n: (host[_STORE[n][0]] * _STORE[n][1] if n in _STORE and _STORE[n][0] in host else zeros.copy()) for n in names}

    def _buffer(self, key: str, wanted, dev, dtype=torch.float32) -> Optional[torch.Tensor]:
        if not any(m in self.metrics for m in wanted):
            return None
        if key not in self._buf:
            self._buf[key] = torch.zeros(self.dataset_length, device=dev, dtype=dtype)
        return self._buf[key]

    def log(self):
        if self.counter == 0:
            print('Evaluation has not started')
            return
        print(f'{self.counter} / {self.dataset_length} samples')
        if self.pck_evaluator is not None:
            self.pck_evaluator.log()
        d = self._means()
        for metric in self.metrics:
            print(f"{metric}: {d[metric]} {'mm' if metric in _MM else ''}")
        print('***')

    def _means(self) -> Dict:
        return {m: a[:self.counter].mean() for m, a in self._arrays(list(self.metrics)).items()}

    def get_metrics_dict(self) -> Dict:
        d1 = self._means()
        if self.pck_evaluator is not None:
            d1.update(self.pck_evaluator.get_metrics_dict())
        return d1

    def __call__(self, output: Dict, batch: Dict, opt_output: Optional[Dict] = None, sync: bool = True):
        """Evaluate a batch: ``output['pred_keypoints_3d']`` (B, J, 3), ``output['pred_keypoints_2d']`` (B, J, 2),
        ``batch['keypoints_3d']`` (B, J, 4), ``batch['keypoints_2d']`` (B, J, 3), ``opt_output['model_joints']`` (B, J, 3).
        Returns ``{'mode_mpjpe', 'mode_re'}`` in mm: numpy arrays (one synchronising copy) or, with ``sync=False``, device
        tensors and no synchronisation anywhere.  The caller's tensors are not modified."""
        dev = _device()
        pred = _f32(output['pred_keypoints_3d'], dev)
        gt = _f32(batch['keypoints_3d'], dev)
        B, J = int(pred.shape[0]), int(pred.shape[1])
        if self.counter + B > self.dataset_length:
            raise ValueError(f"Evaluator: {self.counter} + {B} samples exceed dataset_length {self.dataset_length}")
        if any(int(i) >= J for i in self.keypoint_list) or not (0 <= self.pelvis_ind < J):
            raise ValueError(f"Evaluator: keypoint_list / pelvis_ind outside the {J} keypoints of the batch")
        if self.pck_evaluator is not None:
            self.pck_evaluator(output, batch, opt_output)
        lo, hi = self.counter, self.counter + B

        def window(key, wanted):
            buf = self._buffer(key, wanted, dev)
            return None if buf is None else buf[lo:hi]

        # ONE launch; the kernel writes the windows of the metric buffers (unrecorded metrics go to scratch tensors)
        o = pose_eval(pred, gt, root=self.pelvis_ind, sel=self.keypoint_list, err=window('mpjpe', ('mode_mpjpe', 'min_mpjpe')),
                      pa_err=window('re', ('mode_re', 'min_re')))
        if "mode_kpl2" in self.metrics or "min_kpl2" in self.metrics:
            p2 = _f32(output['pred_keypoints_2d'], dev).double()
            g2 = _f32(batch['keypoints_2d'], dev).double()
            self._buffer('kpl2', ('mode_kpl2', 'min_kpl2'), dev, torch.float64)[lo:hi] = \
                (g2[:, :, -1] * ((p2 - g2[:, :, :-1]) ** 2).sum(-1)).mean(-1)
        if opt_output is not None and ("opt_mpjpe" in self.metrics or "opt_re" in self.metrics):
            pose_eval(_f32(opt_output['model_joints'], dev), gt, root=self.pelvis_ind, sel=self.keypoint_list,
                      err=window('opt_mpjpe', ('opt_mpjpe',)), pa_err=window('opt_re', ('opt_re',)))
        self.counter = hi
        if 'mode_mpjpe' in self.metrics and 'mode_re' in self.metrics:
            both = torch.stack([o["err"], o["pa_err"]]).double() * 1000.0
            if not sync:
                return {'mode_mpjpe': both[0], 'mode_re': both[1]}
            both = both.cpu().numpy()
            return {'mode_mpjpe': both[0], 'mode_re': both[1]}
        return {}


def _metric_property(name: str) -> property:
    def get(self):
        if name not in self.metrics:                    # hasattr(evaluator, name) is False, as in the reference
            raise AttributeError(name)
        return self._arrays([name])[name]
    return property(get, doc=f"{name}: float64 array of dataset_length, a fresh copy of the device buffer per read")


for _name in _STORE:
    setattr(Evaluator, _name, _metric_property(_name))


def pck_accuracy(pred: torch.Tensor, gt: torch.Tensor, mask: torch.Tensor, thr: float):
    """mmpose's keypoint_pck_accuracy with normalize = 1, restated (unpinned against mmpose): pred / gt (N, K, 2), mask (N, K)
    bool, on one device.  acc[k] = share of the valid samples of keypoint k with |pred - gt| < thr, -1 where it has none;
    avg_acc = mean of the acc[k] >= 0, 0 when there is none; cnt = their number.  Returns numpy acc (K,), float, int."""
    d = torch.sqrt(((pred.double() - gt.double()) ** 2).sum(-1))
    valid = mask.sum(0)
    hit = ((d < thr) & mask).sum(0)
    acc = torch.where(valid > 0, hit.double() / valid.clamp(min=1).double(), torch.full_like(hit, -1, dtype=torch.float64))
    acc = acc.cpu().numpy()
    good = acc[acc >= 0]
    return acc, (float(good.mean()) if len(good) else 0.0), int(len(good))


class EvaluatorPCK:
    """pose_utils.py:226-306, with predictions and ground truth kept on the device between calls."""

    def __init__(self, thresholds: List = [0.05, 0.1, 0.2, 0.3, 0.4, 0.5],):
        self.thresholds = thresholds
        self.pred_kp_2d = []
        self.gt_kp_2d = []
        self.gt_conf_2d = []
        self.counter = 0

    def log(self):
        if self.counter == 0:
            print('Evaluation has not started')
            return
        print(f'{self.counter} samples')
        metrics_dict = self.get_metrics_dict()
        for metric in metrics_dict:
            print(f'{metric}: {metrics_dict[metric]}')
        print('***')

    def get_metrics_dict(self) -> Dict:
        pcks = self.compute_pcks()
        metrics = {}
        for thr, (acc, avg_acc, cnt) in zip(self.thresholds, pcks):
            metrics.update({f'kp{i}_pck_{thr}': float(a) for i, a in enumerate(acc) if a >= 0})
            metrics.update({f'kpAvg_pck_{thr}': float(avg_acc)})
        return metrics

    def compute_pcks(self):
        pred, gt, conf = torch.cat(self.pred_kp_2d), torch.cat(self.gt_kp_2d), torch.cat(self.gt_conf_2d)
        assert pred.shape == gt.shape and pred[..., 0].shape == conf.shape
        return [pck_accuracy(pred, gt, conf > 0.5, thr) for thr in self.thresholds]

    def __call__(self, output: Dict, batch: Dict, opt_output: Optional[Dict] = None):
        dev = _device()
        p2 = _f32(output['pred_keypoints_2d'], dev)
        g2 = _f32(batch['keypoints_2d'], dev)
        self.pred_kp_2d.append(p2[:, :, :2].clone())
        self.gt_kp_2d.append(g2[:, :, :2].clone())
        self.gt_conf_2d.append(g2[:, :, -1].clone())
        self.counter += int(p2.shape[0])
