"""yolo/yolov7/utils/metrics.py and the statistics of yolo/yolov7/test.py of the reference, on three HIP entry points
(hm_det_match, hm_det_ap, hm_det_ap_curve, csrc/det_eval.hip).

Same names and call signatures where the reference has them: ``ap_per_class`` (metrics.py:18-78) and ``compute_ap``
(:81-110).  ``match_predictions`` is the matching loop that test.py has inline (:178-209), ``DetEvaluator`` the accumulation
around it and the numbers test.py prints (:129-139, :211-212, :222-238); ``load_label_file`` / ``save_label_file`` read and
write the text format of test.py:146-152.  numpy in gives numpy out; device tensors in give device tensors out.

One rule is narrower than the reference's: predictions are sorted by descending confidence STABLY (equal confidences keep
their input order), where the reference's ``np.argsort(-conf)`` leaves ties unspecified.

Synchronisation.  ``match_predictions``, ``DetEvaluator.__call__`` and ``compute_ap`` never synchronise.  ``ap_per_class`` on
device tensors does not either when ``target_cls`` is a host array; a device ``target_cls`` costs the one synchronisation
``torch.unique`` needs to size its result.  ``DetEvaluator.result()`` returns host numbers and therefore waits.

There is no CPU fallback: without the library or a GPU every call raises ``HipLibraryError``.  Out of scope, and absent here:
``ConfusionMatrix``, the plot helpers (``plot_pr_curve``, ``plot_mc_curve``; ``plot=True`` raises) and ``fitness``.
"""
from __future__ import annotations

from typing import Dict, Optional

import numpy as np
import torch

from .. import lib as L
from .. import ops

MAX_PRED_ROWS, MAX_LABEL_ROWS = 4096, 1024


def _device() -> torch.device:
    L.load()                                            # HipLibraryError when the library is missing
    if not torch.cuda.is_available():
        raise L.HipLibraryError("the detector evaluation needs a GPU; there is no CPU path")
    return torch.device("cuda", torch.cuda.current_device())


_GRIDS: Dict[str, tuple] = {}


def _grids(dev: torch.device):
    """np.linspace(0, 1, 101) and np.linspace(0, 1, 1000) on the device: the reference's knots, bit for bit."""
    key = str(dev)
    if key not in _GRIDS:
        _GRIDS[key] = (torch.from_numpy(np.linspace(0, 1, 101)).to(dev), torch.from_numpy(np.linspace(0, 1, 1000)).to(dev))
    return _GRIDS[key]


def default_iouv(dev=None) -> torch.Tensor:
    """test.py:78."""
    t = torch.linspace(0.5, 0.95, 10)
    return t if dev is None else t.to(dev)


def _is_host(x) -> bool:
    return not (torch.is_tensor(x) and x.is_cuda)


def xywh2xyxy(x: np.ndarray) -> np.ndarray:
    """general.py:268-275 on an (n, 4) array, in its dtype."""
    y = np.copy(x)
    y[:, 0] = x[:, 0] - x[:, 2] / 2
    y[:, 1] = x[:, 1] - x[:, 3] / 2
    y[:, 2] = x[:, 0] + x[:, 2] / 2
    y[:, 3] = x[:, 1] + x[:, 3] / 2
    return y


def xyxy2xywh(x: np.ndarray) -> np.ndarray:
    """general.py:258-265."""
    y = np.copy(x)
    y[:, 0] = (x[:, 0] + x[:, 2]) / 2
    y[:, 1] = (x[:, 1] + x[:, 3]) / 2
    y[:, 2] = x[:, 2] - x[:, 0]
    y[:, 3] = x[:, 3] - x[:, 1]
    return y


def compute_ap(recall, precision, v5_metric=False):
    """metrics.py:81-110: (ap, mpre, mrec).  numpy / lists in: a float and two float64 arrays; device tensors in: three fp64
    device tensors (ap of shape ()), no synchronisation."""
    dev = _device()
    host = _is_host(recall)
    rec = torch.as_tensor(np.asarray(recall, np.float64) if host else recall).to(device=dev, dtype=torch.float64).contiguous().reshape(-1)
    pre = torch.as_tensor(np.asarray(precision, np.float64) if _is_host(precision) else precision).to(device=dev, dtype=torch.float64).contiguous().reshape(-1)
    if rec.numel() != pre.numel() or rec.numel() < 1:
        raise ValueError("compute_ap: recall and precision must have the same length, at least 1")
    ap, mpre, mrec = ops.det_ap_curve(rec, pre, _grids(dev)[0], v5_metric)
    if host:
        return float(ap.cpu().numpy()[0]), mpre.cpu().numpy(), mrec.cpu().numpy()
    return ap.reshape(()), mpre, mrec


def _ap_device(tp: torch.Tensor, conf: torch.Tensor, pred_cls: torch.Tensor, classes: torch.Tensor, n_labels: torch.Tensor,
               v5_metric: bool):
    """metrics.py:33-78 on the device for a known class list: (p, r, ap, f1, i), p / r / f1 at column i, the first arg-max of
    f1.mean(0) (a 0-d device tensor); no sync."""
    dev = tp.device
    order = torch.sort(conf, descending=True, stable=True).indices
    x101, px = _grids(dev)
    ap, p, r = ops.det_ap(tp[order].contiguous(), conf[order].contiguous(), pred_cls[order].contiguous(), classes, n_labels, x101,
                          px, v5_metric)
    f1 = 2 * p * r / (p + r + 1e-16)
    m = f1[0]
    for c in range(1, f1.shape[0]):                                    # np.mean(0): the rows added in order, then one division
        m = m + f1[c]
    m = m / f1.shape[0]
    cols = torch.arange(m.numel(), device=dev)
    i = torch.where(m == m.max(), cols, torch.full_like(cols, m.numel())).min().clamp(max=m.numel() - 1)   # the first maximum
    col = i.reshape(1)
    return p.index_select(1, col)[:, 0], r.index_select(1, col)[:, 0], ap, f1.index_select(1, col)[:, 0], i


def ap_per_class(tp, conf, pred_cls, target_cls, v5_metric=False, plot=False, save_dir='.', names=()):
    """metrics.py:18-78: (p, r, ap, f1, unique_classes int32), p / r / f1 at the arg-max of f1.mean(0) (the first maximum).
    tp (n, niou) booleans, conf (n,), pred_cls (n,), target_cls (m,).  numpy in, numpy out; device tensors in, device tensors
    out (see the module docstring on synchronisation).  The sort by confidence is stable.  ``plot=True`` is not implemented."""
    if plot:
        raise NotImplementedError("ap_per_class(plot=True): the plot helpers of utils/metrics.py are not part of this package")
    dev = _device()
    host = _is_host(tp)

    def up(x, dtype):
        x = torch.as_tensor(np.asarray(x) if _is_host(x) and not torch.is_tensor(x) else x)
        return x.to(device=dev, dtype=dtype).contiguous()

    n = len(conf)
    tp_d = up(tp, torch.uint8).reshape(n, -1)
    conf_d, cls_d = up(conf, torch.float32).reshape(-1), up(pred_cls, torch.float32).reshape(-1)
    if _is_host(target_cls):
        t_host = np.asarray(target_cls.numpy() if torch.is_tensor(target_cls) else target_cls)
        uc_host, counts = np.unique(t_host, return_counts=True)
        classes = torch.from_numpy(uc_host.astype(np.float32)).to(dev)
        n_labels = torch.from_numpy(counts.astype(np.int32)).to(dev)
        uc = uc_host.astype('int32') if host else classes.to(torch.int32)
    else:
        u, counts = torch.unique(target_cls.reshape(-1), return_counts=True)         # the one sync of the device route
        classes, n_labels = u.to(torch.float32), counts.to(torch.int32)
        uc = u.to(torch.int32)
    nc = int(classes.numel())
    if nc == 0:
        raise ValueError("ap_per_class: target_cls is empty (the reference's arg-max of an empty array raises too)")
    p, r, ap, f1, _ = _ap_device(tp_d, conf_d, cls_d, classes.contiguous(), n_labels.contiguous(), v5_metric)
    if host:
        both = torch.stack([p, r, f1]).cpu().numpy()
        return both[0], both[1], ap.cpu().numpy(), both[2], uc
    return p, r, ap, f1, uc


def match_predictions(pred, pred_count, labels, label_count, iouv=None):
    """test.py:178-209 for a batch: pred (N, stride, 6) [xyxy, conf, cls], pred_count (N,), labels (N, lmax, 5) [cls, xyxy] in
    the predictions' units, label_count (N,) -> (correct (N, stride, niou) bool, best_iou (N, stride) fp32,
    matched (N, stride) int32: the target's index or -1).  ``iouv``: default test.py:78's ten thresholds.  numpy in, numpy out;
    device tensors in, device tensors out, no synchronisation.  A flat (N * stride, 6) ``pred``, the layout of the detector
    plan's ``dets``, is taken as N = len(pred_count) images."""
    dev = _device()
    host = _is_host(pred)
    f32 = lambda x: torch.as_tensor(x).to(device=dev, dtype=torch.float32).contiguous()      # noqa: E731
    i32 = lambda x: torch.as_tensor(x).to(device=dev, dtype=torch.int32).contiguous().reshape(-1)      # noqa: E731
    pc, lc = i32(pred_count), i32(label_count)
    N = int(pc.numel())
    p = f32(pred)
    if p.dim() == 2:
        p = p.reshape(N, -1, 6)
    lb = f32(labels)
    if lb.dim() != 3 or lb.shape[0] != N or lb.shape[2] != 5:
        raise ValueError(f"match_predictions: labels {tuple(lb.shape)}: expected ({N}, lmax, 5)")
    if lb.shape[1] == 0:                                               # no label anywhere: one unread row keeps the shape legal
        lb = torch.zeros(N, 1, 5, dtype=torch.float32, device=dev)
    iv = default_iouv(dev) if iouv is None else f32(iouv).reshape(-1)
    correct, best, matched = ops.det_match(p, pc, lb, lc, iv)
    if host:
        return correct.cpu().numpy().astype(bool), best.cpu().numpy(), matched.cpu().numpy()
    return correct.bool(), best, matched


class DetEvaluator:
    """The statistics of test.py around the matching: ``__call__`` scores one batch and appends to device buffers (no
    synchronisation), ``result()`` forms what test.py:222-238 prints."""

    def __init__(self, nc: int, iouv=None, v5_metric: bool = False):
        self.nc = int(nc)
        self.dev = _device()
        self.iouv = default_iouv(self.dev) if iouv is None else torch.as_tensor(iouv).to(device=self.dev, dtype=torch.float32).contiguous().reshape(-1)
        self.niou = int(self.iouv.numel())
        self.v5_metric = bool(v5_metric)
        self.seen = 0
        self._stats = []          # per call: correct (N, stride, niou) u8, conf, cls (N, stride), pred_count, label cls (N, lmax), label_count

    def __call__(self, pred, pred_count, labels, label_count):
        """pred (N, stride, 6) or the plan's flat (N * 300, 6) ``dets``; pred_count (N,) (the plan's ``count``);
        labels (N, lmax, 5) [cls, xyxy] in the predictions' units; label_count (N,).  Returns (correct, best_iou, matched) as
        device tensors.  What is kept is copied, so the plan's buffers may be overwritten by the next pass."""
        dev = self.dev
        pc = torch.as_tensor(pred_count).to(device=dev, dtype=torch.int32).contiguous().reshape(-1)
        lc = torch.as_tensor(label_count).to(device=dev, dtype=torch.int32).contiguous().reshape(-1)
        N = int(pc.numel())
        p = torch.as_tensor(pred).to(device=dev, dtype=torch.float32).contiguous()
        p = p.reshape(N, -1, 6)
        lb = torch.as_tensor(labels).to(device=dev, dtype=torch.float32).contiguous()
        if lb.dim() != 3 or lb.shape[0] != N or lb.shape[2] != 5:
            raise ValueError(f"DetEvaluator: labels {tuple(lb.shape)}: expected ({N}, lmax, 5)")
        if lb.shape[1] == 0:
            lb = torch.zeros(N, 1, 5, dtype=torch.float32, device=dev)
        correct, best, matched = ops.det_match(p, pc, lb, lc, self.iouv)
        self._stats.append((correct, p[:, :, 4].clone(), p[:, :, 5].clone(), pc.clamp(0, p.shape[1]), lb[:, :, 0].clone(),
                            lc.clamp(0, lb.shape[1])))
        self.seen += N
        return correct, best, matched

    def _flat(self):
        """(tp (P, niou) u8, conf (P,), pred_cls (P,), target_cls (T,)) on the device, the padding rows dropped (this sizes
        tensors by their content, so it waits for the device)."""
        tps, confs, clss, tcls = [], [], [], []
        for correct, conf, cls, pc, lcls, lc in self._stats:
            keep = torch.arange(conf.shape[1], device=self.dev)[None, :] < pc[:, None]
            tps.append(correct[keep]); confs.append(conf[keep]); clss.append(cls[keep])
            tcls.append(lcls[torch.arange(lcls.shape[1], device=self.dev)[None, :] < lc[:, None]])
        if not tps:
            e = torch.zeros(0, device=self.dev)
            return torch.zeros(0, self.niou, dtype=torch.uint8, device=self.dev), e, e, e
        return torch.cat(tps), torch.cat(confs), torch.cat(clss), torch.cat(tcls)

    def result(self) -> Dict:
        """test.py:222-238: ``seen``, ``nt`` (labels per class, (nc,) int64), ``mp``, ``mr``, ``map50``, ``map``, and per
        class of ``ap_class`` (int32): ``p``, ``r``, ``ap50``, ``ap``, ``f1``.  All zeros (and empty per-class arrays) when no
        prediction is correct anywhere (:223)."""
        tp, conf, cls, tcls = self._flat()
        out = {"seen": self.seen, "nt": np.zeros(self.nc, np.int64), "mp": 0.0, "mr": 0.0, "map50": 0.0, "map": 0.0,
               "p": np.zeros(0), "r": np.zeros(0), "ap50": np.zeros(0), "ap": np.zeros(0), "f1": np.zeros(0),
               "ap_class": np.zeros(0, np.int32)}
        if tp.numel() and bool(tp.any()):
            t_host = tcls.cpu().numpy()
            p, r, ap, f1, ap_class = ap_per_class(tp, conf, cls, t_host, v5_metric=self.v5_metric)
            p, r, ap, f1 = p.cpu().numpy(), r.cpu().numpy(), ap.cpu().numpy(), f1.cpu().numpy()
            ap50, ap = ap[:, 0], ap.mean(1)
            out.update(p=p, r=r, ap50=ap50, ap=ap, f1=f1, ap_class=ap_class.cpu().numpy(), mp=float(p.mean()), mr=float(r.mean()),
                       map50=float(ap50.mean()), map=float(ap.mean()),
                       nt=np.bincount(t_host.astype(np.int64), minlength=self.nc))
        return out


def load_label_file(path: str, conf: bool = False) -> np.ndarray:
    """One text file of test.py:146-152 / the dataset's labels: a line is ``cls cx cy w h [conf]``, normalised xywh, parsed
    as the reference's reader does (``np.array(rows, dtype=np.float32)``, datasets.py:509) and converted with xywh2xyxy in
    fp32.  conf=False: (n, 5) [cls, x1, y1, x2, y2], a sixth column is ignored.  conf=True: (n, 6) [x1, y1, x2, y2, conf, cls],
    the prediction layout; a line without the sixth column is an error.  An empty file gives zero rows."""
    with open(path) as f:
        rows = [ln.split() for ln in f.read().strip().splitlines() if ln.strip()]
    width = 6 if conf else 5
    if not rows:
        return np.zeros((0, width), np.float32)
    if any(len(r) < width for r in rows):
        raise ValueError(f"{path}: every line needs {width} columns (cls cx cy w h{' conf' if conf else ''})")
    a = np.array([r[:6] if conf else r[:5] for r in rows], dtype=np.float32)
    box = xywh2xyxy(a[:, 1:5])
    if conf:
        return np.concatenate([box, a[:, 5:6], a[:, 0:1]], 1)
    return np.concatenate([a[:, 0:1], box], 1)


def save_label_file(path: str, pred, size=None, conf: bool = False) -> None:
    """test.py:146-152: pred (n, 6) [x1, y1, x2, y2, conf, cls] -> one line ``cls cx cy w h [conf]`` per row, ``%g``.
    ``size=(W, H)``: pixel boxes, divided by the gain [W, H, W, H] as the reference does; None: already normalised.  The
    arithmetic is fp32, as the reference's torch tensors are.  The file is rewritten, not appended to."""
    a = np.asarray(pred.detach().cpu().numpy() if torch.is_tensor(pred) else pred, np.float32).reshape(-1, 6)
    xywh = xyxy2xywh(a[:, :4])
    if size is not None:
        xywh = xywh / np.array([size[0], size[1], size[0], size[1]], np.float32)
    with open(path, "w") as f:
        for row, b in zip(a, xywh):
            line = (float(row[5]), *[float(v) for v in b], float(row[4])) if conf else (float(row[5]), *[float(v) for v in b])
            f.write(('%g ' * len(line)).rstrip() % line + '\n')
