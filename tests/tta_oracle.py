"""Numpy restatement of the test-time augmentation contract (include/ep24.h ``ep24_tta_unmap`` / ``ep24_post_vote_poly24``,
DESIGN.md section 7), written from the contract and independently of csrc/tta.hip.

* ``unmap``: float32, one rounded operation per step, in the contract's order: bit-equal to the kernel.
* ``vote``: float64 from the same rules; candidates, order and greedy NMS are ``polynms_oracle``'s.  ``iou=`` replaces the
  oracle's own IoU matrix, as in ``polynms_oracle.nms_rows``.
"""
import numpy as np

import poly24_oracle as P
import polynms_oracle as N

F = np.float32


def unmap(view, w_v, s, mirror):
    """view [..., ncols >= 27] fp32 of a view of width ``w_v`` -> the rows in the canonical frame; ``s`` = W0 / w_v (rounded to
    fp32 here, once)."""
    v = np.asarray(view, dtype=np.float32)
    s = F(s)
    out = v.copy()
    if s == F(1.0) and not mirror:
        return out
    if mirror:
        out[..., 0] = ((F(w_v) - v[..., 0]).astype(np.float32) * s).astype(np.float32)
        r = v[..., 2:26][..., (12 - np.arange(24)) % 24]
    else:
        out[..., 0] = (v[..., 0] * s).astype(np.float32)
        r = v[..., 2:26]
    out[..., 1] = (v[..., 1] * s).astype(np.float32)
    out[..., 2:26] = (r * s).astype(np.float32)
    return out


def ray_hit(poly, cx, cy, dx, dy):
    """Nearest crossing t >= 0 of the ray (cx, cy) + t (dx, dy) with the closed polygon [24, 2] (inf: none), by the side-of-line
    rule: an edge meets the ray's line iff the side values of its ends have opposite signs or are zero; a vertex has ONE side
    value; an edge that lies on the line contributes its ends."""
    p = np.asarray(poly, dtype=np.float64)
    q = np.roll(p, -1, 0)
    sp = dx * (p[:, 1] - cy) - dy * (p[:, 0] - cx)
    sq = np.roll(sp, -1)
    meet = ((sp <= 0) & (sq >= 0)) | ((sp >= 0) & (sq <= 0))
    on = meet & (sp == sq)
    cross = meet & ~on
    ts = []
    with np.errstate(all="ignore"):
        u = sp / (sp - sq)
        ix, iy = p[:, 0] + u * (q[:, 0] - p[:, 0]), p[:, 1] + u * (q[:, 1] - p[:, 1])
        t = dx * (ix - cx) + dy * (iy - cy)
        ts.extend(t[cross & (t >= 0)])
        tp = dx * (p[:, 0] - cx) + dy * (p[:, 1] - cy)
        tq = dx * (q[:, 0] - cx) + dy * (q[:, 1] - cy)
        ts.extend(tp[on & (tp >= 0)])
        ts.extend(tq[on & (tq >= 0)])
    return min(ts) if ts else np.inf


def rays64():
    """(cos, sin)(15 deg k) in float64: the directions the vote casts its rays in."""
    th = np.arange(24, dtype=np.float64) * (15.0 * np.pi / 180.0)
    return np.cos(th), np.sin(th)


def polygon64(cx, cy, r):
    """c + r_k * (cos, sin)(15 deg k) in float64 [24, 2]: the rays the vote casts from c hit these vertices, so closed forms hold
    to rounding."""
    cs, sn = rays64()
    r = np.broadcast_to(np.asarray(r, dtype=np.float64), (24,))
    return np.stack([cx + r * cs, cy + r * sn], -1)


def consensus64(centres, polys, weights, kept_radii):
    """float64 (cx, cy, r[24]) of the voters ``centres [v, 2]`` / ``polys [v, 24, 2]`` / ``weights [v]`` with a positive weight
    sum, and per ray how many voters abstained.  ``kept_radii``: what a ray nobody crosses falls back to."""
    w = np.asarray(weights, dtype=np.float64)
    W = w.sum()
    c = np.asarray(centres, dtype=np.float64)
    cx, cy = (w * c[:, 0]).sum() / W, (w * c[:, 1]).sum() / W
    cs, sn = rays64()
    out = np.empty(26, dtype=np.float64)
    out[0], out[1] = cx, cy
    abst = np.zeros(24, dtype=np.int64)
    for k in range(24):
        t = np.array([ray_hit(pl, cx, cy, float(cs[k]), float(sn[k])) for pl in polys])
        ok = np.isfinite(t)
        abst[k] = int((~ok).sum())
        wk = w[ok].sum()
        out[2 + k] = (w[ok] * t[ok]).sum() / wk if wk > 0 else kept_radii[k]
    return out, abst


def consensus(rows26, polys, weights, kept):
    """The voted 26 values (fp32) of one kept row: ``rows26 [v, >= 26]`` / ``polys [v, 24, 2]`` / ``weights [v]`` of its voters,
    ``kept`` the kept row itself, returned as it is when it is the only voter or the weights sum to 0.  Also returns, per ray,
    how many voters abstained."""
    kept = np.asarray(kept, dtype=np.float32)[:26]
    w = np.asarray(weights, dtype=np.float64)
    if len(w) <= 1 or not w.sum() > 0:
        return kept.copy(), np.zeros(24, dtype=np.int64)
    out, abst = consensus64(np.asarray(rows26, dtype=np.float64)[:, :2], polys, w, kept[2:].astype(np.float64))
    return out.astype(np.float32), abst


def vote(pred, num_classes, conf_thre, nms_thre, vote_thre, agnostic=False, max_candidates=None, iou=None, detail=False):
    """One image ``pred [A, 27 + C]`` -> (keep rows in NMS order, voted [n, 26] fp32, n_voters [n]).  Voters of the kept sorted
    row i: the candidates j (of the ``max_candidates`` best), before or after i, of its class unless ``agnostic``, with
    ``iou[i, j] > (double)(float)vote_thre`` (a NaN never votes), and i itself.  ``detail``: also the kept rows' sorted positions,
    their voters' sorted positions and the abstentions per ray."""
    p = np.asarray(pred, dtype=np.float32)
    order, conf, cls = N.score_order(p, num_classes, conf_thre, max_candidates)
    if len(order) == 0:
        res = (order, np.zeros((0, 26), np.float32), np.zeros(0, np.int64))
        return res + ([], [], []) if detail else res
    M = N.iou_matrix(p[order]) if iou is None else iou(order)
    c = cls[order]
    kept = N.greedy(M, c, nms_thre, agnostic)
    score = (p[:, 26] * conf).astype(np.float32)
    polys = P.det_polygons(p[order])
    t = np.float64(np.float32(vote_thre))
    voted, nv, who, abst = [], [], [], []
    for i in kept:
        with np.errstate(invalid="ignore"):
            hit = np.asarray(M[i]) > t
        if not agnostic:
            hit &= c == c[i]
        hit[i] = True
        v = np.nonzero(hit)[0]
        row, ab = consensus(p[order[v]], polys[v], score[order[v]].astype(np.float64), p[order[i]])
        voted.append(row)
        nv.append(len(v))
        who.append(v)
        abst.append(ab)
    res = (order[kept], np.stack(voted), np.array(nv, dtype=np.int64))
    return res + (kept, who, abst) if detail else res


def vote_margin(pred, num_classes, conf_thre, vote_thre, agnostic=False, max_candidates=None):
    """min |iou[i, j] - vote_thre| over the ordered candidate pairs i != j the class rule lets vote (inf: none)."""
    p = np.asarray(pred, dtype=np.float32)
    order, _, cls = N.score_order(p, num_classes, conf_thre, max_candidates)
    if len(order) < 2:
        return np.inf
    M = N.iou_matrix(p[order])
    c = cls[order]
    pair = ~np.eye(len(order), dtype=bool)
    if not agnostic:
        pair &= c[:, None] == c[None, :]
    pair &= ~np.isnan(M)
    if not pair.any():
        return np.inf
    return float(np.abs(M[pair] - np.float64(np.float32(vote_thre))).min())
