"""The detector evaluation on the GPU against the same work stated in torch / numpy ops.

  python tools/bench_det_eval.py [--images 64] [--labels 8] [--P 19200 1000000] [--rounds 10] [--warmup 3]

Match (``--images`` x 300 rows, ``--labels`` labels per image, ~20 valid predictions each):
  kernel   DetEvaluator.__call__ on device tensors: one hm_det_match launch plus the copies it keeps; no host sync
  torch    test.py:178-209 restated in torch ops, image by image, on the same device tensors (``.nonzero()`` and ``.item()``
           synchronise, as they do in the reference's loop)
  host     the same loop on CPU tensors
AP (P predictions of 3 classes, 10 thresholds):
  kernel   what metrics.ap_per_class runs on device tensors once the class list is known: stable sort, one hm_det_ap launch,
           F1 and the arg-max in torch ops; no host sync.  ``hm_det_ap_alone``: that one launch on presorted inputs
  torch    metrics.py:18-110 restated in torch ops on the device (cumsum, flipped cummax, searchsorted interpolation)
  host     metrics.py:18-110 restated in numpy (np.interp, np.trapz's sum)
Every figure is the median over ``--rounds`` of the time between two device events (host side: perf_counter) around ``calls``
back-to-back calls, after ``--warmup`` rounds, the sides alternating.  One JSON line."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def torch_match(pred, pc, labels, lc, iouv):
    """test.py:178-209 in torch ops for a batch held as padded tensors (any device)."""
    import torch
    out = []
    pcs, lcs = pc.tolist(), lc.tolist()
    for si in range(pred.shape[0]):
        p, lb = pred[si, :pcs[si]], labels[si, :lcs[si]]
        correct = torch.zeros(p.shape[0], iouv.numel(), dtype=torch.bool, device=pred.device)
        nl = lb.shape[0]
        if nl and p.shape[0]:
            detected = []
            tcls = lb[:, 0]
            tbox = lb[:, 1:5]
            for cls in torch.unique(tcls):
                ti = (cls == tcls).nonzero(as_tuple=False).view(-1)
                pi = (cls == p[:, 5]).nonzero(as_tuple=False).view(-1)
                if pi.shape[0]:
                    b1, b2 = p[pi, :4], tbox[ti]
                    a1, a2 = (b1[:, 2] - b1[:, 0]) * (b1[:, 3] - b1[:, 1]), (b2[:, 2] - b2[:, 0]) * (b2[:, 3] - b2[:, 1])
                    inter = (torch.min(b1[:, None, 2:], b2[:, 2:]) - torch.max(b1[:, None, :2], b2[:, :2])).clamp(0).prod(2)
                    ious, i = (inter / (a1[:, None] + a2 - inter)).max(1)
                    seen = set()
                    for j in (ious > iouv[0]).nonzero(as_tuple=False):
                        d = ti[i[j]]
                        if d.item() not in seen:
                            seen.add(d.item())
                            detected.append(d)
                            correct[pi[j]] = ious[j] > iouv
                            if len(detected) == nl:
                                break
        out.append(correct)
    return out


def numpy_ap(tp, conf, pred_cls, target_cls):
    i = np.argsort(-conf, kind="stable")
    tp, conf, pred_cls = tp[i], conf[i], pred_cls[i]
    uc = np.unique(target_cls)
    px, x101 = np.linspace(0, 1, 1000), np.linspace(0, 1, 101)
    ap, p, r = np.zeros((len(uc), tp.shape[1])), np.zeros((len(uc), 1000)), np.zeros((len(uc), 1000))
    for ci, c in enumerate(uc):
        sel = pred_cls == c
        n_l = (target_cls == c).sum()
        if sel.sum() == 0 or n_l == 0:
            continue
        fpc, tpc = (1 - tp[sel]).cumsum(0), tp[sel].cumsum(0)
        recall, precision = tpc / (n_l + 1e-16), tpc / (tpc + fpc)
        r[ci] = np.interp(-px, -conf[sel], recall[:, 0], left=0)
        p[ci] = np.interp(-px, -conf[sel], precision[:, 0], left=1)
        for j in range(tp.shape[1]):
            mrec = np.concatenate(([0.0], recall[:, j], [recall[-1, j] + 0.01]))
            mpre = np.flip(np.maximum.accumulate(np.flip(np.concatenate(([1.0], precision[:, j], [0.0])))))
            y = np.interp(x101, mrec, mpre)
            ap[ci, j] = (np.diff(x101) * (y[1:] + y[:-1]) / 2.0).sum()
    f1 = 2 * p * r / (p + r + 1e-16)
    k = f1.mean(0).argmax()
    return p[:, k], r[:, k], ap, f1[:, k]


def torch_interp(x, xp, fp, left):
    import torch
    j = torch.searchsorted(xp, x, right=True) - 1
    jc = j.clamp(0, xp.numel() - 2)
    v = fp[jc] + (x - xp[jc]) * ((fp[jc + 1] - fp[jc]) / (xp[jc + 1] - xp[jc]))
    v = torch.where(x >= xp[-1], fp[-1], v)
    return torch.where(j < 0, torch.full_like(v, left), v)


def torch_ap(tp, conf, pred_cls, classes, n_labels):
    """metrics.py:18-110 in torch ops on device tensors; classes / n_labels host lists (no sync inside but boolean masks)."""
    import torch
    dev = tp.device
    i = torch.sort(conf, descending=True, stable=True).indices
    tp, conf, pred_cls = tp[i].to(torch.int64), conf[i].double(), pred_cls[i]
    px, x101 = torch.linspace(0, 1, 1000, dtype=torch.float64, device=dev), torch.linspace(0, 1, 101, dtype=torch.float64, device=dev)
    ap, p, r = [], [], []
    one, zero = torch.ones(1, dtype=torch.float64, device=dev), torch.zeros(1, dtype=torch.float64, device=dev)
    for c, n_l in zip(classes, n_labels):
        sel = pred_cls == c
        t = tp[sel]                                                    # (sizes its result: a sync)
        tpc, fpc = t.cumsum(0), (1 - t).cumsum(0)
        recall, precision = tpc / (n_l + 1e-16), tpc / (tpc + fpc)
        xp = -conf[sel]
        if xp.numel() < 2:
            xp, recall, precision = xp.repeat(2), recall.repeat(2, 1), precision.repeat(2, 1)
        r.append(torch_interp(-px, xp, recall[:, 0].contiguous(), 0.0))
        p.append(torch_interp(-px, xp, precision[:, 0].contiguous(), 1.0))
        row = []
        for j in range(tp.shape[1]):
            mrec = torch.cat([zero, recall[:, j], recall[-1:, j] + 0.01])
            mpre = torch.cat([one, precision[:, j], zero]).flip(0).cummax(0).values.flip(0)
            y = torch_interp(x101, mrec.contiguous(), mpre.contiguous(), 1.0)
            row.append(((x101[1:] - x101[:-1]) * (y[1:] + y[:-1]) / 2.0).sum())
        ap.append(torch.stack(row))
    ap, p, r = torch.stack(ap), torch.stack(p), torch.stack(r)
    f1 = 2 * p * r / (p + r + 1e-16)
    k = f1.mean(0).argmax()
    return p[:, k], r[:, k], ap, f1[:, k]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=64)
    ap.add_argument("--labels", type=int, default=8)
    ap.add_argument("--P", type=int, nargs="+", default=[19200, 1000000])
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()
    import torch
    import det_eval_cases as DC
    from hamer_yolo_amd.yolo import metrics as M
    if not torch.cuda.is_available():
        raise SystemExit("bench_det_eval.py measures on the GPU; none is visible")

    def dev_ms(fn, calls):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(calls):
            fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b) / calls

    def host_ms(fn, calls):
        t = time.perf_counter()
        for _ in range(calls):
            fn()
        return (time.perf_counter() - t) * 1e3 / calls

    def measure(sides):
        """sides: name -> (fn, calls, timer); alternating rounds, median after warm-up."""
        ms = {k: [] for k in sides}
        for r in range(args.warmup + args.rounds):
            for k, (fn, calls, timer) in sides.items():
                v = timer(fn, calls)
                if r >= args.warmup:
                    ms[k].append(v)
        return {k: {"ms_per_call": round(float(np.median(v)), 5), "min_max": [round(min(v), 5), round(max(v), 5)],
                    "calls": sides[k][1]} for k, v in ms.items()}

    out = {"bench": "det_eval", "device": torch.cuda.get_device_name(0), "rounds": args.rounds, "warmup": args.warmup}
    # ---- the match
    rng = np.random.default_rng(1)
    imgs = [DC.random_image(rng, 20, args.labels) for _ in range(args.images)]
    pred, pc, lab, lc = [torch.from_numpy(a) for a in DC.pack(imgs, 300, args.labels)]
    iouv = torch.from_numpy(DC.IOUV)
    d = [t.cuda() for t in (pred, pc, lab, lc, iouv)]

    def kernel_match():
        ev = M.DetEvaluator(3)                                         # a fresh one each call: the buffers do not pile up
        ev(d[0], d[1], d[2], d[3])

    got = M.match_predictions(d[0], d[1], d[2], d[3])[0].cpu()
    want = torch_match(pred, pc, lab, lc, iouv)
    assert all(torch.equal(got[i, :len(w)], w) for i, w in enumerate(want)), "the torch statement and the kernel disagree"
    out["match"] = {"images": args.images, "rows": 300, "labels": args.labels,
                    **measure({"kernel": (kernel_match, 200, dev_ms), "torch_device": (lambda: torch_match(*d), 2, dev_ms),
                               "torch_host": (lambda: torch_match(pred, pc, lab, lc, iouv), 2, host_ms)})}
    print(json.dumps(out["match"]), file=sys.stderr)
    # ---- AP
    out["ap"] = []
    for P in args.P:
        tp, conf, pred_cls, target_cls = DC.ap_case(P, P)
        uc, cnt = np.unique(target_cls, return_counts=True)
        dtp, dconf, dcls = torch.from_numpy(tp).cuda(), torch.from_numpy(conf).cuda(), torch.from_numpy(pred_cls).cuda()
        k = M.ap_per_class(dtp, dconf, dcls, target_cls)
        t = torch_ap(dtp, dconf, dcls, [float(c) for c in uc], [int(n) for n in cnt])
        h = numpy_ap(tp, conf, pred_cls, target_cls)
        diff = max(float(np.abs(a.cpu().numpy() - b).max()) for a, b in zip(k[:4], h))
        diff_t = max(float(np.abs(a.cpu().numpy() - b).max()) for a, b in zip(t, h))
        calls = 50 if P <= 100000 else 5
        cls_d, nl_d = torch.from_numpy(uc.astype(np.float32)).cuda(), torch.from_numpy(cnt.astype(np.int32)).cuda()
        order = torch.sort(dconf, descending=True, stable=True).indices
        stp, sconf, scls = dtp[order].contiguous(), dconf[order].contiguous(), dcls[order].contiguous()
        x101, px = M._grids(dtp.device)
        row = {"P": P, "max_abs_diff_kernel_host": diff, "max_abs_diff_torch_host": diff_t,
               **measure({"kernel": (lambda: M._ap_device(dtp, dconf, dcls, cls_d, nl_d, False), calls, dev_ms),
                          "hm_det_ap_alone": (lambda: M.ops.det_ap(stp, sconf, scls, cls_d, nl_d, x101, px), calls, dev_ms),
                          "torch_device": (lambda: torch_ap(dtp, dconf, dcls, [float(c) for c in uc], [int(n) for n in cnt]), 2, dev_ms),
                          "torch_host": (lambda: numpy_ap(tp, conf, pred_cls, target_cls), 1, host_ms)})}
        out["ap"].append(row)
        print(json.dumps(row), file=sys.stderr)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
