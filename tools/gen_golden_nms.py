#!/usr/bin/env python3
"""Generate tests/golden/nms_multi.npz from the REFERENCE's ``yolo/yolov7/utils/general.py`` ``non_max_suppression``, run in
place (CPU, torch) with the import stand-ins of tools/gen_golden_yolo.py: ``cv2``, the ``torchvision`` package tree, ``seaborn``.

``torchvision.ops.nms`` is absent from this image; the reference's function runs with the oracle's greedy NMS
(``oracle/yolo_ref.nms_greedy``) plugged into that one call.  So the fixture pins everything around it -- the confidence
filter, conf = obj * cls, the multi-label and best-class branches, the class filter, xywh -> xyxy, the 30000 cut, the class
offset, the 300 cap -- but not ``nms`` itself, and the order of EQUAL scores inside ``nms`` is the stand-in's stable sort, i.e.
this project's tie rule (lower candidate first), not something the reference defines.

Cases (inputs from tests/nms_rule.py's seeded generators, stored once and shared):
  nc3/...    nc = 3, n = 300, two images (the second without a survivor): multi_label x agnostic x classes None / [1] x
             conf / IoU 0.001 / 0.65 and 0.25 / 0.35
  nc1_multi  nc = 1 with multi_label=True: the reference turns it off (general.py:628)
  nc32_cut   nc = 32, n = 1000, multi_label, conf 0.001: 32000 candidates, so general.py:681-682 cuts to 30000.  That argsort
             is not stable: the tool asserts that all candidate scores are distinct and refuses to write the file otherwise
  ties/...   duplicated score rows, far below 30000 candidates: their order is the stand-in's (see above)
Per case: ``<case>/pred`` (the key of the stored input), ``conf``, ``iou``, ``agnostic``, ``multi_label``, ``classes`` (empty =
None), ``count`` and ``out<i>`` per image.  Data only, no code."""
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import nms_rule as NR  # noqa: E402
from oracle import yolo_ref  # noqa: E402

REF = os.environ.get("HAMER_REFERENCE", "/root/reference")
OUT = os.path.join(ROOT, "tests", "golden", "nms_multi.npz")
LIMIT = 400 * 1000


def load_reference():
    cv2 = types.ModuleType("cv2"); cv2.setNumThreads = lambda n: None
    sys.modules["cv2"] = cv2
    for name in ("torchvision", "torchvision.ops", "torchvision.utils", "torchvision.models", "torchvision.transforms", "seaborn"):
        sys.modules.setdefault(name, types.ModuleType(name))
    sys.modules["torchvision"].ops = sys.modules["torchvision.ops"]
    sys.modules["torchvision.ops"].nms = lambda boxes, scores, thr: yolo_ref.nms_greedy(boxes, scores, thr)
    sys.path.insert(0, REF)
    sys.path.insert(0, os.path.join(REF, "yolo"))
    from yolo.yolov7.utils import general
    return general


def main():
    general = load_reference()
    preds = {
        "a": NR.pass_nc3(11, 2, 300, ties=0),
        "b": NR.make_image(np.random.default_rng(12), 300, 1)[None],
        "c": NR.image_truncated()[None],
        "d": NR.pass_nc3(13, 2, 300, ties=40),
    }
    cases = {}
    for ml in (False, True):
        for ag in (False, True):
            for cl in (None, [1]):
                for conf, iou in ((0.001, 0.65), (0.25, 0.35)):
                    name = f"nc3/ml{int(ml)}_ag{int(ag)}_{'all' if cl is None else 'c1'}_{conf:g}"
                    cases[name] = ("a", conf, iou, cl, ag, ml)
    cases["nc1_multi"] = ("b", 0.001, 0.65, None, False, True)
    cases["nc32_cut"] = ("c", 0.001, 0.65, None, False, True)
    cases["ties/ml1"] = ("d", 0.001, 0.65, None, False, True)
    cases["ties/ml0"] = ("d", 0.25, 0.35, None, True, False)

    c = preds["c"][0]
    s = (c[:, 5:] * c[:, 4:5])[c[:, 4] > np.float32(0.001)]
    s = s[s > np.float32(0.001)]
    assert s.size > 30000 and np.unique(s).size == s.size, "nc32_cut: candidate scores must be distinct (the cut's argsort is not stable)"
    d = preds["d"][0]
    assert np.unique(d[:, 5:] * d[:, 4:5]).size < d[:, 5:].size, "ties: no duplicated scores"

    store = {f"pred/{k}": v for k, v in preds.items()}
    store["cases"] = np.array(list(cases))
    store["notes"] = np.array(
        "torchvision.ops.nms is a stand-in (oracle/yolo_ref.nms_greedy): pinned is everything around it.  Equal scores in the "
        "ties/ cases are ordered by the stand-in's stable sort (lower row * nc + class first): this project's tie rule, which "
        "the reference does not define.  nc32_cut: all candidate scores distinct, so the unstable argsort of the 30000 cut is "
        "determined.")
    for name, (key, conf, iou, cl, ag, ml) in cases.items():
        with torch.no_grad():
            out = general.non_max_suppression(torch.from_numpy(preds[key].copy()), conf, iou, classes=cl, agnostic=ag, multi_label=ml)
        store[f"{name}/pred"] = np.array(key)
        store[f"{name}/conf"] = np.float64(conf)
        store[f"{name}/iou"] = np.float64(iou)
        store[f"{name}/agnostic"] = np.int32(ag)
        store[f"{name}/multi_label"] = np.int32(ml)
        store[f"{name}/classes"] = np.array([] if cl is None else cl, np.int32)
        store[f"{name}/count"] = np.array([len(o) for o in out], np.int32)
        for i, o in enumerate(out):
            store[f"{name}/out{i}"] = o.numpy().astype(np.float32).reshape(-1, 6)
        mine = NR.nms(preds[key], conf, iou, cl, ag, ml)
        same = all(np.array_equal(a, o.numpy().reshape(-1, 6)) for a, o in zip(mine, out))
        print(f"{name}: kept {[len(o) for o in out]}, tests/nms_rule.py equal: {same}")
    assert store["nc3/ml1_ag0_all_0.001/count"][1] == 0 and store["nc32_cut/count"][0] == 300
    np.savez_compressed(OUT, **store)
    size = os.path.getsize(OUT)
    print(OUT, size, "bytes")
    assert size < LIMIT, "the fixture must stay under 400 KB"


if __name__ == "__main__":
    main()
