"""Numpy restatement of the evaluation semantics of ep24.evaluate (COCO-style AP, one area range, no crowd / ignore).

Written from the contract, independently of the kernels: IoU functions of its own (float32 circle24, float64 rect) and the
matching / accumulation over IoU matrices that the caller passes in, so that the kernels' own IoUs can be fed to it.

An image is a dict ``gt_cls [G] int``, ``det_cls [D] int``, ``det_score [D] float32`` (in the image's postprocess order p)
and ``iou [G, D] float64``.
"""
import numpy as np

IOU_THRS = np.linspace(0.5, 0.95, 10)
REC_THRS = np.linspace(0.0, 1.0, 101)
PI_F = np.float32(np.pi)
F = np.float32


def num_gt(labels):
    """labels [L, 51]: the first n rows, n = rows whose values sum to > 0."""
    return int((labels.astype(np.float64).sum(-1) > 0).sum())


def ray_cos_sin():
    th = np.arange(24, dtype=np.float64) * (15.0 * np.pi / 180.0)
    return np.cos(th).astype(np.float32), np.sin(th).astype(np.float32)


def _gt_radii(gt50):
    g = np.asarray(gt50, dtype=np.float32)
    vx = g[:, 2::2] - g[:, 0:1]
    vy = g[:, 3::2] - g[:, 1:2]
    return np.sqrt(vx * vx + vy * vy).astype(np.float32)


def _ray_inter(r1, r2, d):
    """Intersection area of two circles (radii r1, r2, centre distance d), fp32, geom.h's case order."""
    with np.errstate(all="ignore"):
        rmin, rmax = np.minimum(r1, r2), np.maximum(r1, r2)
        rmin2, rmax2, d2 = rmin * rmin, rmax * rmax, d * d
        contained = np.abs(r1 - r2) >= d
        disjoint = d >= r1 + r2
        c1 = (rmin2 + d2 - rmax2) / (F(2) * rmin * d + F(1e-8))
        c2 = (rmax2 + d2 - rmin2) / (F(2) * rmax * d + F(1e-8))
        c1 = np.minimum(np.maximum(c1, F(-0.99)), F(0.99))
        c2 = np.minimum(np.maximum(c2, F(-0.99)), F(0.99))
        a1, a2 = np.arccos(c1), np.arccos(c2)
        lens = a1 * rmin2 + a2 * rmax2 - rmin * d * np.sin(a1)
        inter = np.where(contained, PI_F * rmin2, F(0))
        inter = np.where(disjoint, F(0), inter)
        inter = np.where(contained | disjoint, inter, lens)
    return inter.astype(np.float32)


def iou_circle24(gt50, det26):
    """[G, D] float32: mean over the 24 rays of inter / (pi r^2 + pi r'^2 - inter + 1e-6), summed in ray order."""
    g = np.asarray(gt50, dtype=np.float32)
    q = np.asarray(det26, dtype=np.float32)
    rg = _gt_radii(g)[:, None, :]
    rq = q[None, :, 2:26]
    ddx = g[:, None, 0] - q[None, :, 0]
    ddy = g[:, None, 1] - q[None, :, 1]
    d = np.sqrt(ddx * ddx + ddy * ddy).astype(np.float32)
    acc = np.zeros(d.shape, dtype=np.float32)
    for k in range(24):
        r1, r2 = np.broadcast_to(rg[..., k], d.shape), np.broadcast_to(rq[..., k], d.shape)
        inter = _ray_inter(r1, r2, d)
        acc = acc + inter / (PI_F * (r1 * r1) + PI_F * (r2 * r2) - inter + F(1e-6))
    return (acc / F(24)).astype(np.float32)


def gt_boxes(gt50):
    g = np.asarray(gt50, dtype=np.float32)
    xs, ys = g[:, 2::2], g[:, 3::2]
    return np.stack([xs.min(1), ys.min(1), xs.max(1), ys.max(1)], 1)


def det_boxes(det26):
    q = np.asarray(det26, dtype=np.float32)
    c, s = ray_cos_sin()
    xs = q[:, 0:1] + q[:, 2:26] * c[None]
    ys = q[:, 1:2] + q[:, 2:26] * s[None]
    return np.stack([xs.min(1), ys.min(1), xs.max(1), ys.max(1)], 1).astype(np.float32)


def iou_rect(gt50, det26):
    """[G, D] float64 box IoU of the vertex boxes against c + r_k (cos, sin)(15 deg k), no +1."""
    g = gt_boxes(gt50).astype(np.float64)[:, None, :]
    d = det_boxes(det26).astype(np.float64)[None, :, :]
    w = np.maximum(0.0, np.minimum(g[..., 2], d[..., 2]) - np.maximum(g[..., 0], d[..., 0]))
    h = np.maximum(0.0, np.minimum(g[..., 3], d[..., 3]) - np.maximum(g[..., 1], d[..., 1]))
    inter = w * h
    ag = (g[..., 2] - g[..., 0]) * (g[..., 3] - g[..., 1])
    ad = (d[..., 2] - d[..., 0]) * (d[..., 3] - d[..., 1])
    with np.errstate(all="ignore"):
        return inter / (ag + ad - inter)


def match_image(img, max_dets=100):
    """-> list of records (cls, score, p, rank, tp_mask) of one image, per class in (score desc, p asc) order."""
    gt_cls = np.asarray(img["gt_cls"], dtype=np.int64)
    det_cls = np.asarray(img["det_cls"], dtype=np.int64)
    score = np.asarray(img["det_score"], dtype=np.float32)
    iou = np.asarray(img["iou"], dtype=np.float64)
    recs = []
    for c in sorted(set(det_cls.tolist())):
        ds = sorted(np.nonzero(det_cls == c)[0].tolist(), key=lambda p: (-float(score[p]), p))[:max_dets]
        gs = np.nonzero(gt_cls == c)[0].tolist()
        tp = [0] * len(ds)
        for t, thr in enumerate(IOU_THRS):
            taken = set()
            for r, p in enumerate(ds):
                best, m = min(thr, 1 - 1e-10), -1
                for g in gs:
                    if g in taken or iou[g, p] < best:
                        continue
                    best, m = iou[g, p], g
                if m >= 0:
                    taken.add(m)
                    tp[r] |= 1 << t
        recs += [(c, score[p], p, r, tp[r]) for r, p in enumerate(ds)]
    return recs


def evaluate(images, num_classes, max_dets=100):
    """images in update order -> dict: records (sorted by class, score desc, seq, p), precision [10, 101, C], recall [10, C]."""
    per_class = {k: [] for k in range(num_classes)}
    npig = np.zeros(num_classes, dtype=np.int64)
    for seq, img in enumerate(images):
        for c in np.asarray(img["gt_cls"], dtype=np.int64):
            npig[c] += 1
        for (c, s, p, r, tp) in match_image(img, max_dets):
            per_class[c].append((s, seq, p, r, tp))
    T, R = len(IOU_THRS), len(REC_THRS)
    precision = -np.ones((T, R, num_classes))
    recall = -np.ones((T, num_classes))
    records = []
    for k in range(num_classes):
        recs = per_class[k]
        scores = np.array([x[0] for x in recs], dtype=np.float32)
        inds = np.argsort(-scores, kind="mergesort")
        recs = [recs[i] for i in inds]
        records += [(k,) + x for x in recs]
        if npig[k] == 0:
            continue
        tps = np.array([[(x[4] >> t) & 1 for x in recs] for t in range(T)], dtype=bool).reshape(T, len(recs))
        tp_sum = np.cumsum(tps, axis=1).astype(float)
        fp_sum = np.cumsum(~tps, axis=1).astype(float)
        for t in range(T):
            tp, fp = tp_sum[t], fp_sum[t]
            nd = len(tp)
            rc = tp / npig[k]
            pr = tp / (fp + tp + np.spacing(1))
            recall[t, k] = rc[-1] if nd else 0
            pr = pr.tolist()
            for i in range(nd - 1, 0, -1):
                if pr[i] > pr[i - 1]:
                    pr[i - 1] = pr[i]
            q = np.zeros(R)
            for ri, pi in enumerate(np.searchsorted(rc, REC_THRS, side="left")):
                if pi >= nd:
                    break
                q[ri] = pr[pi]
            precision[t, :, k] = q
    return {"records": records, "precision": precision, "recall": recall, "npig": npig}


def summarize(precision, recall):
    def mean(x):
        v = x[x > -1]
        return float(np.mean(v)) if v.size else -1.0
    return {"AP": mean(precision), "AP50": mean(precision[0]), "AP75": mean(precision[5]), "AR100": mean(recall),
            "per_class_AP": np.array([mean(precision[:, :, k]) for k in range(precision.shape[2])])}
