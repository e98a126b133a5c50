"""Host side of the batched multi-label NMS: the numpy rule (tests/nms_rule.py) against the reference's recorded outputs
(tests/golden/nms_multi.npz); the two entry points (header, binding, library, build list, HM_VERSION); hm_yolo_nms_batch's
argument limits, refused without a device; the workspace formula; the driver's new switches; the unsupported ``labels``."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import nms_rule as NR
from hamer_yolo_amd import build as B
from hamer_yolo_amd import lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PATH = os.path.join(ROOT, "tests", "golden", "nms_multi.npz")
G = np.load(PATH)
CASES = [str(c) for c in G["cases"]]


def case_args(case):
    cl = G[f"{case}/classes"]
    return dict(conf_thres=float(G[f"{case}/conf"]), iou_thres=float(G[f"{case}/iou"]), classes=None if cl.size == 0 else cl.tolist(),
                agnostic=bool(G[f"{case}/agnostic"]), multi_label=bool(G[f"{case}/multi_label"]))


@pytest.mark.parametrize("case", CASES)
def test_rule_equals_the_fixture(case):
    pred = G[f"pred/{str(G[f'{case}/pred'])}"]
    out = NR.nms(pred, **case_args(case))
    assert [len(o) for o in out] == G[f"{case}/count"].tolist()
    for i, o in enumerate(out):
        want = G[f"{case}/out{i}"]
        assert o.dtype == np.float32 and o.shape == want.shape and np.array_equal(o.view(np.uint32), want.view(np.uint32)), (case, i)


def test_fixture_cases_and_size():
    assert os.path.getsize(PATH) < 400 * 1000
    assert len([c for c in CASES if c.startswith("nc3/")]) == 16 and {"nc1_multi", "nc32_cut", "ties/ml1", "ties/ml0"} <= set(CASES)
    assert all(G[f"{c}/count"][1] == 0 for c in CASES if c.startswith("nc3/"))           # an image without a survivor
    assert G["nc32_cut/count"][0] == 300 and "stable" in str(G["notes"])
    c = G["pred/c"][0]
    s = c[:, 5:] * c[:, 4:5]
    assert (s > np.float32(0.001)).sum() > 30000 and np.unique(s).size == s.size       # cut applies; no tie decides it
    assert np.array_equal(c, NR.image_truncated())                                       # the GPU test's image 0
    # multi-label keeps boxes that best-class drops, and nc == 1 ignores the switch
    assert G["nc3/ml1_ag0_all_0.25/count"][0] > G["nc3/ml0_ag0_all_0.25/count"][0]
    b = G["pred/b"]
    assert np.array_equal(NR.nms(b, 0.001, 0.65, multi_label=True)[0], NR.nms(b, 0.001, 0.65, multi_label=False)[0])


NEW = ("hm_nms_batch_workspace_bytes", "hm_yolo_nms_batch")


def test_surface():
    header = open(os.path.join(ROOT, "include", "hamer_hip.h")).read()
    lib = L.load()
    for name in NEW:
        assert re.search(r"\b(int|size_t) %s\(" % name, header), name
        assert name in L.EXPORTS and hasattr(lib, name), name
    assert "nms_batch.hip" in B.SOURCES and os.path.exists(os.path.join(B.CSRC, "nms_batch.hip"))
    assert re.search(r"#define HM_VERSION 402\b", header) and L.HM_VERSION == 402 and lib.hm_version() == 402
    assert lib.hm_nms_batch_workspace_bytes.restype is C.c_size_t


def _buf(n=4096):
    return C.addressof(C.create_string_buffer(n + 16)) + 15 & ~15      # a non-null aligned address; errors return before device work


def _nms(**kw):
    a = dict(pred=_buf(), stride=8 * 8, nb=1, n=8, nc=3, conf=0.25, iou=0.45, mask=7, agnostic=0, ml=0, max_det=300, dets=_buf(8192),
             dstride=300, count=_buf(), ws=_buf(), ws_bytes=4096)
    a.update(kw)
    return L.load().hm_yolo_nms_batch(a["pred"], a["stride"], a["nb"], a["n"], a["nc"], a["conf"], a["iou"], a["mask"], a["agnostic"],
                                      a["ml"], a["max_det"], None, a["dets"], a["dstride"], a["count"], a["ws"], a["ws_bytes"], None)


BAD = {"pred=None": dict(pred=None), "dets=None": dict(dets=None), "count=None": dict(count=None), "workspace=None": dict(ws=None),
       "nb=0": dict(nb=0), "nb=4097": dict(nb=4097), "nc=0": dict(nc=0), "nc=33": dict(nc=33), "max_det=0": dict(max_det=0),
       "max_det=1025": dict(max_det=1025, dstride=2000), "n=0": dict(n=0), "n=2^20+1": dict(n=(1 << 20) + 1, ws_bytes=1 << 40),
       "n*nc=2^20+2-multi": dict(n=(1 << 20) // 3 + 1, ml=1, ws_bytes=1 << 40), "conf=-0.1": dict(conf=-0.1),
       "conf=nan": dict(conf=float("nan")), "workspace-128-bytes-short": dict(ws_bytes=256 + 8 * 8 + 8 * 16),
       "workspace-misaligned": dict(ws=_buf() + 8), "dets_stride=299": dict(dstride=299)}


@pytest.mark.parametrize("kw", list(BAD.values()), ids=list(BAD))
def test_argument_limits_are_refused_without_a_device(kw):
    rc = _nms(**kw)
    msg = L.load().hm_last_error_string().decode()
    assert rc != 0 and "hm_yolo_nms_batch" in msg, (rc, msg)


def test_the_default_arguments_pass_the_checks_up_to_the_device():
    """The refusals above come from the one changed argument: the workspace of the default call is exactly large enough."""
    assert L.load().hm_nms_batch_workspace_bytes(1, 8, 3, 0) == 256 + 8 * 8 + 8 * 16 + 8 * 16 <= 4096


def pow2(x):
    p = 1
    while p < x:
        p <<= 1
    return p


def formula(nb, n, nc, ml):
    c = n * (nc if ml and nc > 1 else 1)
    return (nb * 4 + 255) // 256 * 256 + nb * (pow2(c) * 8 + n * 16 + min(c, 30000) * 16)


def test_workspace_bytes():
    f = L.load().hm_nms_batch_workspace_bytes
    for shape in ((0, 100, 3, 0), (4097, 100, 3, 0), (1, 0, 3, 0), (1, 100, 0, 0), (1, 100, 33, 0), (1, (1 << 20) + 1, 3, 0),
                  (1, (1 << 20) // 3 + 1, 3, 1), (-1, 100, 3, 1)):
        assert f(*shape) == 0, shape
    assert f(1, 1 << 20, 3, 0) > 0 and f(1, (1 << 20) // 3, 3, 1) > 0 and f(1, 1 << 20, 1, 1) > 0      # nc == 1: multi_label is off
    assert f(48, 15120, 3, 1) == formula(48, 15120, 3, 1) == 256 + 48 * (65536 * 8 + 15120 * 16 + 30000 * 16)
    assert f(65, 1000, 32, 0) == formula(65, 1000, 32, 0) == 512 + 65 * (1024 * 8 + 1000 * 16 + 1000 * 16)
    for ml in (0, 1):
        last = 0
        for nb in (1, 2, 63, 64, 65, 4096):
            assert f(nb, 15120, 3, ml) >= last
            last = f(nb, 15120, 3, ml)
        last = 0
        for n in (1, 2, 255, 256, 257, 5461, 5462, 15120, 25200, 1 << 18):
            assert f(4, n, 3, ml) >= last
            last = f(4, n, 3, ml)


def test_parser_protocol():
    from hamer_yolo_amd import evaluate_det as E
    a = E._parser().parse_args(["--labels", "l", "--images", "i", "--protocol", "test", "--multi-label"])
    assert a.protocol == "test" and a.multi_label is True and a.conf_thres is None and a.iou_thres is None
    d = E._parser().parse_args(["--labels", "l", "--images", "i"])
    assert d.protocol == "deployed" and d.multi_label is False and d.conf_thres is None and d.iou_thres is None
    with pytest.raises(SystemExit):
        E._parser().parse_args(["--labels", "l", "--images", "i", "--protocol", "coco"])


def test_labels_are_not_implemented():
    import torch
    from hamer_yolo_amd.yolo import general
    with pytest.raises(NotImplementedError, match="labels"):
        general.non_max_suppression(torch.zeros(1, 4, 8), labels=[torch.zeros(1, 5)])
    import inspect
    assert list(inspect.signature(general.non_max_suppression).parameters) == ["prediction", "conf_thres", "iou_thres", "classes", "agnostic",
                                                                                "multi_label", "labels"]
