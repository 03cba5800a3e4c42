"""Numpy restatement of the stratified 24-point evaluation (include/ep24.h section E8, ep24.evaluate.Evaluator24(strata=...)).

Written from the contract: the two measures in float64 with the header's expressions, pycocotools' ``evaluateImg`` with the stratum
predicate in its own loop form (GTs in a stable order with the non-ignored first, the walk that stops at the first ignored GT once
a non-ignored match is held) - NOT the closed form the kernel reduces it to - and the records over [C, NA].  The accumulation is
``segmeval_oracle.accumulate``.

A stratum is ``(area_lo, area_hi, z_lo, z_hi)``.  An image is a dict ``gt_cls [G]``, ``gt_area [G]``, ``gt_zone [G]``, ``det_cls [D]``,
``det_score [D] float32`` (in the image's postprocess order p), ``det_area [D]``, ``det_zone [D]`` and ``iou [G, D] float64``.
"""
import numpy as np

import eval24_oracle as O
import segmeval_oracle as S

IOU_THRS = O.IOU_THRS
ZT_D = 16


def outside(area, zone, st):
    return bool(area < st[0] or area > st[1] or zone < st[2] or zone >= st[3])


# ---- measures ------------------------------------------------------------------------------------------
def det_points(det26):
    """[n, 48] float32: c + r_k * (cos, sin)(15 deg * k) as (x, y) pairs, product and sum in fp32."""
    q = np.asarray(det26, dtype=np.float32).reshape(-1, det26.shape[-1])
    c, s = O.ray_cos_sin()
    out = np.empty((len(q), 48), dtype=np.float32)
    out[:, 0::2] = q[:, 0:1] + q[:, 2:26] * c[None]
    out[:, 1::2] = q[:, 1:2] + q[:, 2:26] * s[None]
    return out


def area24(points48, scale):
    """0.5 * |sum_k x_k y_{k+1} - x_{k+1} y_k| / (s * s), the sum from 0.0 in k order, float64."""
    p = np.asarray(points48, dtype=np.float32).astype(np.float64).reshape(-1, 48)
    x, y = p[:, 0::2], p[:, 1::2]
    s = np.zeros(len(p), dtype=np.float64)
    for k in range(24):
        k1 = (k + 1) % 24
        s = s + (x[:, k] * y[:, k1] - x[:, k1] * y[:, k])
    sc = np.asarray(scale, dtype=np.float64)
    return 0.5 * np.abs(s) / (sc * sc)


def zone(X, Y, zt):
    """zt [n, 16] float64 (one row per object).  kind 0: 0, kind 1: rd, kind 2: the incidence angle in degrees, inf beyond the field."""
    X, Y = np.asarray(X, dtype=np.float32).astype(np.float64), np.asarray(Y, dtype=np.float32).astype(np.float64)
    zt = np.asarray(zt, dtype=np.float64).reshape(-1, ZT_D)
    kind = zt[:, 0].astype(np.int64)
    with np.errstate(all="ignore"):                                            # a kind-0 row holds zeros: its rd is never used
        x = (X - zt[:, 3]) / zt[:, 1]
        y = (Y - zt[:, 4]) / zt[:, 2]
        rd = np.sqrt(x * x + y * y)
    k1, k2, k3, k4, tmax, tdmax = (zt[:, i] for i in range(5, 11))
    td = np.fmin(rd, tdmax)
    th = td.copy()
    with np.errstate(all="ignore"):
        for _ in range(12):
            t2 = th * th
            f = th * (1.0 + t2 * (k1 + t2 * (k2 + t2 * (k3 + t2 * k4)))) - td
            fp = 1.0 + t2 * (3.0 * k1 + t2 * (5.0 * k2 + t2 * (7.0 * k3 + t2 * (9.0 * k4))))
            th = th - f / fp
            th = np.fmin(np.fmax(th, 0.0), tmax)
        deg = np.where(rd > tdmax, np.inf, th * (180.0 / np.pi))
    return np.where(kind == 1, rd, np.where(kind == 2, deg, 0.0))


def measure_labels(rows51, image, scales, zt):
    """[n, 2] float64 (area, zone) of label rows; ``image [n]`` names each row's scale and zone-table row."""
    r = np.asarray(rows51, dtype=np.float32).reshape(-1, 51)
    image = np.asarray(image, dtype=np.int64)
    return np.stack([area24(r[:, 3:51], np.asarray(scales, dtype=np.float64)[image]),
                     zone(r[:, 1], r[:, 2], np.asarray(zt, dtype=np.float64)[image])], 1)


def measure_dets(rows, image, scales, zt):
    r = np.asarray(rows, dtype=np.float32)
    r = r.reshape(-1, r.shape[-1])
    image = np.asarray(image, dtype=np.int64)
    return np.stack([area24(det_points(r), np.asarray(scales, dtype=np.float64)[image]),
                     zone(r[:, 0], r[:, 1], np.asarray(zt, dtype=np.float64)[image])], 1)


# ---- evaluateImg ---------------------------------------------------------------------------------------
def evaluate_img(iou, gt_out, dt_out, thrs=IOU_THRS):
    """pycocotools' loop for one (image, class, stratum).  ``iou [G, D]``, ``gt_out [G]`` / ``dt_out [D]``: the object lies outside
    the stratum; the detections stand in matching order.  -> (match [T, D] the GT's original index or -1, ignore [T, D] bool)."""
    G, D = len(gt_out), len(dt_out)
    order = sorted(range(G), key=lambda g: int(gt_out[g]))
    gt_ig = [bool(gt_out[g]) for g in order]
    T = len(thrs)
    dtm = np.full((T, D), -1, dtype=np.int64)
    dt_ig = np.zeros((T, D), dtype=bool)
    by_det = [[float(iou[g, d]) for g in order] for d in range(D)]          # plain floats: the loops below are Python's
    for t in range(T):
        gtm = [False] * G
        for d in range(D):
            best, m = min(float(thrs[t]), 1 - 1e-10), -1
            row = by_det[d]
            for gi in range(G):
                if gtm[gi]:
                    continue
                if m > -1 and not gt_ig[m] and gt_ig[gi]:
                    break
                if row[gi] < best:
                    continue
                best, m = row[gi], gi
            if m > -1:
                dt_ig[t, d] = gt_ig[m]
                dtm[t, d] = order[m]
                gtm[m] = True
            elif dt_out[d]:
                dt_ig[t, d] = True
    return dtm, dt_ig


def class_dets(img, c, max_dets):
    score = np.asarray(img["det_score"], dtype=np.float32)
    return sorted(np.nonzero(np.asarray(img["det_cls"]) == c)[0].tolist(), key=lambda p: (-float(score[p]), p))[:max_dets]


def records(images, num_classes, strata, max_dets=100, stats=None):
    """Images in update order -> the records sorted by (class, score desc, seq, rank): dict of ``cls``, ``score`` (float32), ``seq``,
    ``p``, ``rank``, ``m [n, NA]`` (10 TP bits | 10 ignore bits << 16), ``area``, ``zone`` and ``npig [C, NA]``.  ``max_dets``: the
    largest maxDets.  ``stats``: a dict that receives the counts of the matching cases the scenes are built to contain."""
    NA = len(strata)
    npig = np.zeros((num_classes, NA), dtype=np.int64)
    rows = []
    st = stats if stats is not None else {}
    for k in ("to_ignored", "unmatched_outside", "tie_non_ignored", "ignored_larger_iou"):
        st.setdefault(k, 0)
    for seq, img in enumerate(images):
        gt_cls = np.asarray(img["gt_cls"], dtype=np.int64)
        iou = np.asarray(img["iou"], dtype=np.float64)
        g_out = np.array([[outside(img["gt_area"][g], img["gt_zone"][g], s) for s in strata] for g in range(len(gt_cls))],
                         dtype=bool).reshape(len(gt_cls), NA)
        for g, c in enumerate(gt_cls):
            if 0 <= c < num_classes:
                npig[c] += ~g_out[g]
        for c in sorted(set(int(x) for x in img["det_cls"])):
            if not 0 <= c < num_classes:
                continue
            ds = class_dets(img, c, max_dets)
            gs = np.nonzero(gt_cls == c)[0]
            sub = iou[np.ix_(gs, ds)] if len(gs) else np.zeros((0, len(ds)))
            mm = np.zeros((len(ds), NA), dtype=np.int64)
            for a, s in enumerate(strata):
                d_out = [outside(img["det_area"][p], img["det_zone"][p], s) for p in ds]
                dtm, dig = evaluate_img(sub, g_out[gs, a], d_out)
                for t in range(len(IOU_THRS)):
                    mm[:, a] |= (dtm[t] >= 0).astype(np.int64) << t
                    mm[:, a] |= dig[t].astype(np.int64) << (16 + t)
                    if stats is None:
                        continue
                    thr = min(float(IOU_THRS[t]), 1 - 1e-10)
                    taken = np.zeros(len(gs), dtype=bool)
                    for r in range(len(ds)):
                        g = dtm[t, r]
                        if g < 0:
                            st["unmatched_outside"] += int(dig[t, r])
                            continue
                        st["to_ignored"] += int(dig[t, r])
                        taken[g] = True
                        if not dig[t, r]:                    # the other free GTs that qualified for this detection
                            free = ~taken & (sub[:, r] >= thr)
                            st["tie_non_ignored"] += int((free & ~g_out[gs, a] & (sub[:, r] == sub[g, r])).any())
                            st["ignored_larger_iou"] += int((free & g_out[gs, a] & (sub[:, r] > sub[g, r])).any())
            for r, p in enumerate(ds):
                rows.append((c, np.float32(img["det_score"][p]), seq, p, r, mm[r], float(img["det_area"][p]), float(img["det_zone"][p])))
    idx = sorted(range(len(rows)), key=lambda i: (rows[i][0], -float(rows[i][1]), rows[i][2], rows[i][4]))
    rows = [rows[i] for i in idx]
    n = len(rows)
    return {"cls": np.array([r[0] for r in rows], dtype=np.int64), "score": np.array([r[1] for r in rows], dtype=np.float32),
            "seq": np.array([r[2] for r in rows], dtype=np.int64), "p": np.array([r[3] for r in rows], dtype=np.int64),
            "rank": np.array([r[4] for r in rows], dtype=np.int64),
            "m": (np.stack([r[5] for r in rows]) if n else np.zeros((0, NA), dtype=np.int64)).astype(np.int32).reshape(n, NA),
            "area": np.array([r[6] for r in rows], dtype=np.float64), "zone": np.array([r[7] for r in rows], dtype=np.float64),
            "npig": npig}


def accumulate(rec, num_classes, max_dets):
    """-> (precision [10, 101, C, NA, NM], recall [10, C, NA, NM]): pycocotools' accumulate over the records."""
    r = dict(rec, score=np.asarray(rec["score"], dtype=np.float64))
    return S.accumulate(r, num_classes, tuple(max_dets))


def evaluate(images, num_classes, strata, max_dets=(100,), stats=None):
    rec = records(images, num_classes, strata, max(max_dets), stats)
    precision, recall = accumulate(rec, num_classes, max_dets)
    return {"records": rec, "precision": precision, "recall": recall, "npig": rec["npig"]}
