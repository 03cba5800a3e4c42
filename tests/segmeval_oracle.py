"""Numpy restatement of the COCO API's evaluation for iouType "segm" (rleIou on boolean masks, COCOeval.evaluateImg over area
ranges, accumulate over (class, area range, maxDets), summarize), the specification of ep24.segmeval and of the ep24_segm_*
kernels.  Written from the contract in include/ep24.h section E6 and the API's documented semantics, one statement per step;
Python's float and numpy's float64 are the C double and every operation rounds on its own.

A *group* is one (image, category): ``{"cls", "seq", "iou" [D, G] float64 (detection-major), "gt_crowd" [G], "gt_ignore0" [G]
(the annotation's ignore OR iscrowd), "gt_area" [G] float64, "dt_area" [D] float64, "dt_score" [D] float64}`` with the
detections already in (score descending, input order) order and cut at the largest maxDets.
"""
import numpy as np

IOU_THRS = np.linspace(0.5, 0.95, int(np.round((0.95 - 0.5) / 0.05)) + 1, endpoint=True)
REC_THRS = np.linspace(0.0, 1.0, int(np.round((1.0 - 0.0) / 0.01)) + 1, endpoint=True)
AREA_RANGES = ((0 ** 2, 1e5 ** 2), (0 ** 2, 32 ** 2), (32 ** 2, 96 ** 2), (96 ** 2, 1e5 ** 2))
AREA_LABELS = ("all", "small", "medium", "large")
MAX_DETS = (1, 10, 100)
EPS = float(np.spacing(1))


def mask_iou(dt_masks, gt_masks, gt_crowd):
    """rleIou: (inter int64 [D, G], iou float64 [D, G]) of boolean masks; a crowd GT divides by the detection's area."""
    D, G = len(dt_masks), len(gt_masks)
    inter = np.zeros((D, G), dtype=np.int64)
    iou = np.zeros((D, G), dtype=np.float64)
    for d in range(D):
        md = np.asarray(dt_masks[d]).astype(bool)
        ad = int(md.sum())
        for g in range(G):
            mg = np.asarray(gt_masks[g]).astype(bool)
            i = int((md & mg).sum())
            inter[d, g] = i
            if i == 0:
                continue
            den = ad if gt_crowd[g] else int(mg.sum()) + ad - i
            iou[d, g] = float(i) / float(den)
    return inter, iou


def evaluate_img(group, area_rng, thrs=IOU_THRS):
    """evaluateImg for one area range -> dict: ``gt_order`` (original GT indices, the non-ignored first, stable), ``gt_ignore``
    (in that order), ``dt_match`` [T, D] (the matched GT's ORIGINAL index, -1 for none), ``dt_ignore`` [T, D] bool."""
    iou = np.asarray(group["iou"], dtype=np.float64)
    G, D = len(group["gt_area"]), len(group["dt_area"])
    lo, hi = area_rng
    ig = [bool(group["gt_ignore0"][g]) or group["gt_area"][g] < lo or group["gt_area"][g] > hi for g in range(G)]
    order = sorted(range(G), key=lambda g: int(ig[g]))              # sorted() is stable
    gt_ig = [ig[g] for g in order]
    T = len(thrs)
    gtm = np.zeros((T, G), dtype=bool)
    dtm = np.full((T, D), -1, dtype=np.int64)
    dt_ig = np.zeros((T, D), dtype=bool)
    for t in range(T):
        for d in range(D):
            best = min(float(thrs[t]), 1 - 1e-10)
            m = -1
            for gi in range(G):
                g = order[gi]
                if gtm[t, gi] and not group["gt_crowd"][g]:
                    continue
                if m > -1 and not gt_ig[m] and gt_ig[gi]:
                    break
                if iou[d, g] < best:
                    continue
                best = iou[d, g]
                m = gi
            if m > -1:
                dt_ig[t, d] = gt_ig[m]
                dtm[t, d] = order[m]
                gtm[t, m] = True
            elif group["dt_area"][d] < lo or group["dt_area"][d] > hi:
                dt_ig[t, d] = True
    return {"gt_order": order, "gt_ignore": gt_ig, "dt_match": dtm, "dt_ignore": dt_ig}


def score_ranks(scores):
    """Dense rank of every float64 score among the distinct scores, 0 = the highest."""
    s = np.asarray(scores, dtype=np.float64).reshape(-1)
    u = np.unique(s)
    return (len(u) - 1 - np.searchsorted(u, s)).astype(np.int64)


def records(groups, num_classes, area_ranges=AREA_RANGES, thrs=IOU_THRS):
    """One record per detection, in group order: dict of arrays ``cls``, ``score``, ``seq``, ``rank`` (position in its group),
    ``m`` [n, NA] int32 = 10 TP bits | 10 ignore bits << 16, and ``npig`` [K, NA] = the non-ignored GTs."""
    NA = len(area_ranges)
    cls, score, seq, rank, m = [], [], [], [], []
    npig = np.zeros((num_classes, NA), dtype=np.int64)
    for gr in groups:
        D = len(gr["dt_area"])
        mm = np.zeros((D, NA), dtype=np.int64)
        for a, rng in enumerate(area_ranges):
            e = evaluate_img(gr, rng, thrs)
            npig[gr["cls"], a] += sum(1 for x in e["gt_ignore"] if not x)
            for t in range(len(thrs)):
                mm[:, a] |= (e["dt_match"][t] >= 0).astype(np.int64) << t
                mm[:, a] |= e["dt_ignore"][t].astype(np.int64) << (16 + t)
        cls += [gr["cls"]] * D
        seq += [gr["seq"]] * D
        rank += list(range(D))
        score += [float(s) for s in gr["dt_score"]]
        m.append(mm)
    m = np.concatenate(m) if m else np.zeros((0, NA), dtype=np.int64)
    return {"cls": np.array(cls, dtype=np.int64), "score": np.array(score, dtype=np.float64), "seq": np.array(seq, dtype=np.int64),
            "rank": np.array(rank, dtype=np.int64), "m": m.astype(np.int32).reshape(-1, NA), "npig": npig}


def accumulate(rec, num_classes, max_dets=MAX_DETS, num_thrs=10, rec_thrs=REC_THRS, eps=EPS):
    """accumulate over the records -> (precision [T, R, K, A, M], recall [T, K, A, M]).  ``eps``: the COCO API's
    ``tp / (fp + tp + np.spacing(1))``; ``eps=None`` forms the precision as the C++ port of the API does, ``tp / (tp + fp)`` with
    0 for 0 / 0 - the two differ in exactly one case, tp + fp == 1 (1 + eps is the next double after 1; from 2 on the sum
    rounds back to the integer)."""
    K, NA, M, T, R = num_classes, rec["m"].shape[1], len(max_dets), num_thrs, len(rec_thrs)
    precision = -np.ones((T, R, K, NA, M))
    recall = -np.ones((T, K, NA, M))
    for k in range(K):
        sel = np.flatnonzero(rec["cls"] == k)
        sel = sel[np.lexsort((rec["rank"][sel], rec["seq"][sel]))]                  # image by image, each in its own order
        for a in range(NA):
            npig = int(rec["npig"][k, a])
            if npig == 0:
                continue
            for mi, md in enumerate(max_dets):
                s = sel[rec["rank"][sel] < md]
                s = s[np.argsort(-rec["score"][s], kind="mergesort")]
                mm = rec["m"][s, a].astype(np.int64)
                for t in range(T):
                    ig = (mm >> (16 + t)) & 1
                    tps = ((mm >> t) & 1) & (1 - ig)
                    fps = (1 - ((mm >> t) & 1)) & (1 - ig)
                    tp = np.cumsum(tps).astype(np.float64)
                    fp = np.cumsum(fps).astype(np.float64)
                    nd = len(tp)
                    rc = tp / npig
                    if eps is None:
                        pr = np.array([tp[i] / (tp[i] + fp[i]) if tp[i] + fp[i] > 0 else 0.0 for i in range(nd)])
                    else:
                        pr = tp / (fp + tp + eps)
                    recall[t, k, a, mi] = rc[-1] if nd else 0
                    pr = pr.tolist()
                    for i in range(nd - 1, 0, -1):
                        if pr[i] > pr[i - 1]:
                            pr[i - 1] = pr[i]
                    q = np.zeros(R)
                    inds = np.searchsorted(rc, rec_thrs, side="left")
                    for ri, pi in enumerate(inds):
                        if pi < nd:
                            q[ri] = pr[pi]
                    precision[t, :, k, a, mi] = q
    return precision, recall


def _mean_valid(x):
    v = x[x > -1]
    return float(np.mean(v)) if v.size else -1.0


def summarize(precision, recall, max_dets=MAX_DETS, area_labels=AREA_LABELS, thrs=IOU_THRS):
    """COCOeval.summarize: the 12 numbers (for three maxDets and the four standard ranges) and their printed lines."""
    def one(ap, iou_thr, a, mi):
        s = precision if ap else recall
        if iou_thr is not None:
            s = s[np.where(iou_thr == thrs)[0]]
        s = s[:, :, :, a, mi] if ap else s[:, :, a, mi]
        v = _mean_valid(s)
        iou_str = "{:0.2f}:{:0.2f}".format(thrs[0], thrs[-1]) if iou_thr is None else "{:0.2f}".format(iou_thr)
        line = " {:<18} {} @[ IoU={:<9} | area={:>6s} | maxDets={:>3d} ] = {:0.3f}".format(
            "Average Precision" if ap else "Average Recall", "(AP)" if ap else "(AR)", iou_str, area_labels[a], max_dets[mi], v)
        return v, line
    last = len(max_dets) - 1
    rows = [one(True, None, 0, last), one(True, thrs[0], 0, last), one(True, thrs[5], 0, last)]
    rows += [one(True, None, a, last) for a in range(1, len(area_labels))]
    rows += [one(False, None, 0, mi) for mi in range(len(max_dets))]
    rows += [one(False, None, a, last) for a in range(1, len(area_labels))]
    return [r[0] for r in rows], [r[1] for r in rows]


def evaluate(groups, num_classes, area_ranges=AREA_RANGES, max_dets=MAX_DETS):
    """groups -> (stats, lines, precision, recall, records)."""
    rec = records(groups, num_classes, area_ranges)
    precision, recall = accumulate(rec, num_classes, max_dets)
    stats, lines = summarize(precision, recall, max_dets)
    return stats, lines, precision, recall, rec
