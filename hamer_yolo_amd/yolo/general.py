"""``non_max_suppression`` of the reference's yolo/yolov7/utils/general.py (:611-703), same name and signature, on one HIP
entry point (hm_yolo_nms_batch, csrc/nms_batch.hip): every image of ``prediction`` in one call, a workgroup per image.

Both branches: best class per row, and ``multi_label=True`` (one candidate per (row, class) with obj * cls > conf_thres; turned
off for a one-class model, as the reference does).  Class-aware unless ``agnostic``.  300 boxes per image at most, the best
30000 candidates enter the suppression.  Equal scores are ordered by ascending row * nc + class -- the reference leaves that to
its sort and to torchvision -- see DESIGN.md section 11.

Not offered: ``labels`` (the apriori labels of autolabelling, test.py --save-hybrid) raises ``NotImplementedError``; ``merge``
is a constant False inside the reference's function and has no counterpart here.

Cost: one enqueue (a memset and two launches, whatever the number of images) and one host synchronisation for the counts,
which size the returned tensors.  There is no CPU fallback: without the library or a GPU the call raises ``HipLibraryError``.
"""
from __future__ import annotations

from typing import List, Optional, Sequence

import torch

from .. import lib as L

MAX_DET = 300         # general.py:624


def non_max_suppression(prediction, conf_thres: float = 0.25, iou_thres: float = 0.45, classes: Optional[Sequence[int]] = None,
                        agnostic: bool = False, multi_label: bool = False, labels=()) -> List[torch.Tensor]:
    """prediction (nb, n, 5+nc) fp32, a device tensor (a host tensor is uploaded) -> list of nb (k, 6) device tensors
    [x1, y1, x2, y2, conf, cls] in the prediction's (letterbox) coordinates, by descending confidence."""
    if labels is not None and len(labels):
        raise NotImplementedError("non_max_suppression: labels (autolabelling, test.py --save-hybrid) is not implemented")
    lib = L.load()
    if not torch.cuda.is_available():
        raise L.HipLibraryError("non_max_suppression needs a GPU; there is no CPU path")
    pred = torch.as_tensor(prediction)
    if pred.dim() != 3 or pred.shape[2] < 6:
        raise ValueError(f"prediction must be (nb, n, 5+nc), got {tuple(pred.shape)}")
    if not pred.is_cuda:
        pred = pred.to(torch.device("cuda", torch.cuda.current_device()))
    pred = pred.to(torch.float32).contiguous()
    nb, n, no = pred.shape
    nc = no - 5
    if nb == 0 or n == 0:
        return [torch.zeros(0, 6, device=pred.device) for _ in range(nb)]
    ml = int(bool(multi_label))
    mask = 0xFFFFFFFF if classes is None else sum(1 << int(c) for c in classes)
    with torch.cuda.device(pred.device):
        ws = torch.empty(max(lib.hm_nms_batch_workspace_bytes(nb, n, nc, ml), 16), dtype=torch.uint8, device=pred.device)
        dets = torch.empty(nb, MAX_DET, 6, dtype=torch.float32, device=pred.device)
        count = torch.empty(nb, dtype=torch.int32, device=pred.device)
        L.check(lib.hm_yolo_nms_batch(pred.data_ptr(), n * no, nb, n, nc, float(conf_thres), float(iou_thres), mask, int(bool(agnostic)),
                                      ml, MAX_DET, None, dets.data_ptr(), MAX_DET, count.data_ptr(), ws.data_ptr(), ws.numel(),
                                      L.current_stream()), "hm_yolo_nms_batch")
        counts = count.tolist()                                        # the one synchronisation
    return [dets[i, :int(k)].clone() for i, k in enumerate(counts)]
