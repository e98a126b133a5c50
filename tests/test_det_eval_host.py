"""Host (no GPU): the CPU rule of the detector evaluation (tests/det_eval_rule.py) against the reference's recorded outputs
(tests/golden/det_eval.npz, written by tools/gen_golden_det_eval.py) and against hand-worked matching cases; the surface of
the three entry points (header, binding, library, build list, HM_VERSION); their argument checks; the label-file format."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import det_eval_cases as DC
import det_eval_rule as DR
from hamer_yolo_amd import build as B
from hamer_yolo_amd import lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = np.load(os.path.join(ROOT, "tests", "golden", "det_eval.npz"))
CASES = [str(c) for c in G["cases"]]
TOL = 1e-12


def _inputs(case):
    return G[f"{case}/tp"], G[f"{case}/conf"], G[f"{case}/pred_cls"], G[f"{case}/target_cls"]


@pytest.mark.parametrize("v5", (False, True))
@pytest.mark.parametrize("case", CASES)
def test_rule_matches_the_reference(case, v5):
    p, r, ap, f1, cls, _ = DR.ap_per_class(*_inputs(case), v5)
    k = f"{case}/v5_{int(v5)}"
    for name, got in (("p", p), ("r", r), ("ap", ap), ("f1", f1)):
        assert got.shape == G[f"{k}/{name}"].shape and np.abs(got - G[f"{k}/{name}"]).max() <= TOL, (case, name)
    assert cls.dtype == np.int32 and np.array_equal(cls, G[f"{k}/classes"])


@pytest.mark.parametrize("v5", (False, True))
@pytest.mark.parametrize("case", [str(c) for c in G["curves"]])
def test_rule_compute_ap_matches_the_reference(case, v5):
    ap, mpre, mrec = DR.compute_ap(G[f"{case}/curve/recall"], G[f"{case}/curve/precision"], v5)
    k = f"{case}/curve/v5_{int(v5)}"
    assert abs(ap - float(G[k + "/ap"])) <= TOL
    assert np.array_equal(mpre, G[k + "/mpre"]) and np.array_equal(mrec, G[k + "/mrec"])


def test_fixture_holds_what_the_issue_asks_for():
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "det_eval.npz")) < 200 * 1024
    assert len(CASES) >= 12 and {"nl4", "nl10", "class_without_pred", "class_without_label", "single_tp", "single_fp"} <= set(CASES)
    assert len(np.unique(G["nl4/target_cls"])) == 1 and len(G["nl4/target_cls"]) == 4 and len(G["nl10/target_cls"]) == 10
    for case in CASES:
        tp, conf, pred_cls, target_cls = _inputs(case)
        assert conf.dtype == np.float32 and len(np.unique(conf)) == len(conf), case              # distinct confidences
        for v5 in (False, True):                                                                 # the arg-max has a margin
            _, p, r, _ = DR.ap_curves(tp, conf, pred_cls, target_cls, v5)
            m = (2 * p * r / (p + r + 1e-16)).mean(0)
            rest = m[m != m.max()]
            assert not len(rest) or m.max() - rest.max() >= 1e-9, case
    assert not np.isin(1.0, G["class_without_pred/pred_cls"]) and not np.isin(1.0, G["class_without_label/target_cls"])
    assert np.all(G["class_without_pred/v5_0/ap"][1] == 0)                                       # the reference's `continue`


def test_rule_box_iou_equals_the_reference():
    for name in G["iou_sets"]:
        got, want = DR.box_iou(G[f"iou/{name}/a"], G[f"iou/{name}/b"]), G[f"iou/{name}/iou"]
        assert got.dtype == np.float32 and np.array_equal(np.isnan(got), np.isnan(want)), name
        assert np.array_equal(got[~np.isnan(got)].view(np.uint32), want[~np.isnan(want)].view(np.uint32)), name      # bit for bit
    s = G["iou/special/iou"]
    assert s[0, 0] == 0.5 and np.isnan(s[2, 2]) and s[1, 0] == 1.0 and s[3, 4] == 0.0


@pytest.mark.parametrize("name", list(DC.HAND))
def test_rule_matches_the_hand_worked_cases(name):
    pred, lab, _, _, _ = DC.hand_arrays(name)
    DC.check_hand(name, *DR.match_image(pred, lab, DC.IOUV))


def test_rule_batch_padding_and_clamping():
    rng = np.random.default_rng(3)
    imgs = [DC.random_image(rng, 5, 3), DC.random_image(rng, 0, 2), DC.random_image(rng, 4, 0)]
    pred, pc, lab, lc = DC.pack(imgs, 6, 4, fill=np.nan)
    c, b, m = DR.match_batch(pred, pc, lab, lc, DC.IOUV)
    assert not np.isnan(b).any() and (c[0, 5:] == 0).all() and (m[0, 5:] == -1).all() and (m[1] == -1).all() and (b[2] == 0).all()
    c2, b2, m2 = DR.match_batch(pred, pc + np.array([100, -3, 0], np.int32), lab, lc, DC.IOUV)      # clamped to [0, stride]
    assert np.array_equal(m2[1], m[1]) and np.array_equal(m2[2], m[2]) and np.array_equal(c2[2], c[2])


NEW = ("hm_det_match", "hm_det_ap_workspace_bytes", "hm_det_ap", "hm_det_ap_curve")


def test_surface():
    header = open(os.path.join(ROOT, "include", "hamer_hip.h")).read()
    lib = L.load()
    for name in NEW:
        assert re.search(r"\b(int|size_t) %s\(" % name, header), name
        assert name in L.EXPORTS and hasattr(lib, name), name
    assert "det_eval.hip" in B.SOURCES and os.path.exists(os.path.join(B.CSRC, "det_eval.hip"))
    assert re.search(r"#define HM_VERSION 402\b", header) and L.HM_VERSION == 402 and lib.hm_version() == 402
    src = open(os.path.join(B.CSRC, "det_eval.hip")).read()
    assert "#pragma clang fp contract(off)" in src and "getenv" not in src and "hipMalloc" not in src
    assert lib.hm_det_ap_workspace_bytes(1000000, 3, 10) == 0


def _buf(n=4096):
    return C.addressof(C.create_string_buffer(n))      # a non-null address; an argument error returns before any device work


def _match(**kw):
    a = dict(pred=_buf(), pred_count=_buf(), labels=_buf(), label_count=_buf(), iouv=_buf(), N=1, stride=4, lmax=4, niou=10,
             correct=_buf(), best_iou=_buf(), matched=_buf())
    a.update(kw)
    return L.load().hm_det_match(a["pred"], a["pred_count"], a["labels"], a["label_count"], a["iouv"], a["N"], a["stride"],
                                 a["lmax"], a["niou"], a["correct"], a["best_iou"], a["matched"], None)


def _ap(**kw):
    a = dict(tp=_buf(), conf=_buf(), pred_cls=_buf(), P=4, classes=_buf(), n_labels=_buf(), nc=1, niou=10, x101=_buf(),
             px=_buf(8192), v5=0, ap=_buf(), p=_buf(8192), r=_buf(8192))
    a.update(kw)
    return L.load().hm_det_ap(a["tp"], a["conf"], a["pred_cls"], a["P"], a["classes"], a["n_labels"], a["nc"], a["niou"],
                              a["x101"], a["px"], a["v5"], a["ap"], a["p"], a["r"], None, 0, None)


def _curve(**kw):
    a = dict(recall=_buf(), precision=_buf(), n=4, x101=_buf(), v5=0, ap=_buf(), mpre=_buf(), mrec=_buf())
    a.update(kw)
    return L.load().hm_det_ap_curve(a["recall"], a["precision"], a["n"], a["x101"], a["v5"], a["ap"], a["mpre"], a["mrec"], None)


BAD = [(_match, "hm_det_match", kw) for kw in
       [dict(pred=None), dict(pred_count=None), dict(labels=None), dict(label_count=None), dict(iouv=None), dict(correct=None),
        dict(best_iou=None), dict(matched=None), dict(N=0), dict(stride=0), dict(stride=4097), dict(lmax=1025), dict(niou=0),
        dict(niou=17)]] + \
      [(_ap, "hm_det_ap", kw) for kw in
       [dict(tp=None), dict(conf=None), dict(pred_cls=None), dict(classes=None), dict(n_labels=None), dict(x101=None),
        dict(px=None), dict(ap=None), dict(p=None), dict(r=None), dict(P=-1), dict(nc=0), dict(niou=0), dict(niou=17)]] + \
      [(_curve, "hm_det_ap_curve", kw) for kw in
       [dict(recall=None), dict(precision=None), dict(x101=None), dict(ap=None), dict(mpre=None), dict(mrec=None), dict(n=0),
        dict(n=-1)]]


@pytest.mark.parametrize("fn,name,kw", BAD, ids=[f"{n}-{'-'.join(f'{k}={v}' for k, v in kw.items())}" for _, n, kw in BAD])
def test_argument_checks(fn, name, kw):
    rc = fn(**kw)
    msg = L.load().hm_last_error_string().decode()
    assert rc == -1 and msg.startswith(name + ":"), (rc, msg)          # HM_ERR_ARG, the entry point's own name


def test_ap_per_class_plot_raises():
    from hamer_yolo_amd.yolo import metrics as M
    with pytest.raises(NotImplementedError):
        M.ap_per_class(np.zeros((1, 10), bool), np.ones(1), np.zeros(1), np.zeros(1), plot=True)
    for missing in ("ConfusionMatrix", "fitness", "plot_pr_curve"):
        assert not hasattr(M, missing) and missing in M.__doc__


def test_signatures_equal_the_reference():
    import inspect
    from hamer_yolo_amd.yolo import metrics as M
    assert list(inspect.signature(M.ap_per_class).parameters) == ["tp", "conf", "pred_cls", "target_cls", "v5_metric", "plot",
                                                                  "save_dir", "names"]
    assert list(inspect.signature(M.compute_ap).parameters) == ["recall", "precision", "v5_metric"]
    d = {k: v.default for k, v in inspect.signature(M.ap_per_class).parameters.items()}
    assert (d["v5_metric"], d["plot"], d["save_dir"], d["names"]) == (False, False, '.', ())


def test_label_file_round_trip(tmp_path):
    """%g text, then the floats the reference's reader parses: np.array(rows, dtype=np.float32) and xywh2xyxy in fp32."""
    from hamer_yolo_amd.yolo import metrics as M
    pred = np.array([[100.25, 50.5, 300.75, 250.125, 0.87654321, 1], [0, 0, 1920, 1080, 0.25, 0], [3.3, 4.4, 5.5, 6.6, 1.0, 2]], np.float32)
    path = str(tmp_path / "a.txt")
    M.save_label_file(path, pred, size=(1920, 1080), conf=True)
    lines = open(path).read().splitlines()
    g = np.array([1920, 1080, 1920, 1080], np.float32)
    xywh = M.xyxy2xywh(pred[:, :4]) / g
    assert xywh.dtype == np.float32
    for ln, row, b in zip(lines, pred, xywh):
        assert ln == ('%g ' * 6).rstrip() % (float(row[5]), *[float(v) for v in b], float(row[4]))      # test.py:150-152
    assert lines[1] == "0 0.5 0.5 1 1 0.25"
    want = np.array([ln.split() for ln in lines], dtype=np.float32)                                     # datasets.py:509
    back = M.load_label_file(path, conf=True)
    assert back.dtype == np.float32 and back.shape == (3, 6)
    assert np.array_equal(back[:, :4], M.xywh2xyxy(want[:, 1:5])) and np.array_equal(back[:, 4], want[:, 5]) and np.array_equal(back[:, 5], want[:, 0])
    lab = M.load_label_file(path)                                                                       # the sixth column ignored
    assert lab.shape == (3, 5) and np.array_equal(lab[:, 0], want[:, 0]) and np.array_equal(lab[:, 1:], back[:, :4])
    assert np.abs(back[:, :4] * g - pred[:, :4]).max() < 1920 * 1e-5                                    # %g keeps 6 digits
    M.save_label_file(path, pred[:1], size=(1920, 1080))
    assert len(open(path).read().split()) == 5
    with pytest.raises(ValueError):
        M.load_label_file(path, conf=True)
    open(path, "w").close()
    assert M.load_label_file(path).shape == (0, 5) and M.load_label_file(path, conf=True).shape == (0, 6)
    M.save_label_file(path, np.array([[0.1, 0.2, 0.3, 0.6, 0.5, 1]], np.float32), conf=True)            # already normalised
    assert open(path).read() == "1 0.2 0.4 0.2 0.4 0.5\n"


def test_evaluate_det_parser_and_table():
    from hamer_yolo_amd import evaluate_det as E
    a = E._parser().parse_args(["--pred", "A", "--labels", "B", "--size", "1920", "1080"])
    assert (a.pred, a.labels, a.size, a.images, a.json) == ("A", "B", [1920, 1080], None, None)
    a = E._parser().parse_args(["--images", "I", "--labels", "B", "--precise-detector", "--save-txt", "O", "--save-conf"])
    assert a.precise_detector and a.save_conf and a.conf_thres is None and a.iou_thres is None
    res = {"seen": 3, "labels": 7, "mp": 0.5, "mr": 0.25, "map50": 0.125, "map": 0.0625,
           "classes": [{"name": "1", "labels": 7, "p": 0.5, "r": 0.25, "ap50": 0.125, "ap": 0.0625}]}
    lines = E.format_table(res).splitlines()
    pf = '%20s' + '%12i' * 2 + '%12.3g' * 4                                                             # test.py:232
    assert lines[1] == pf % ('all', 3, 7, 0.5, 0.25, 0.125, 0.0625) and lines[2] == pf % ('1', 3, 7, 0.5, 0.25, 0.125, 0.0625)
    assert lines[0].split() == ['Class', 'Images', 'Labels', 'P', 'R', 'mAP@.5', 'mAP@.5:.95']
    with pytest.raises(SystemExit):
        E.main(["--labels", "B"])
