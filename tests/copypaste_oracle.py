"""Numpy restatement of the copy-paste post-pass (csrc/paste.hip: ``ep24_paste_labels`` / ``ep24_paste_u8``), written from the
contract in include/ep24.h and DESIGN.md section 7 and independently of the kernels.

* ``paste_labels``: the sequential walk over the partner's rows, with every decision it takes and that decision's distance to its
  threshold (the GPU tests demand EQUALITY, so tests/test_copypaste_oracle.py asserts that no decision of their cases is a close call).
* ``paste_u8``: the pixel rule, pixel centre by pixel centre.
* the polygon intersection is ``poly24_oracle.poly24_iou``'s: ``inter = iou * (area_a + area_b) / (1 + iou)``.
"""
import numpy as np

import poly24_oracle as P

F = np.float32


def polygon_row(cls, cx, cy, r):
    """A label row (class, cx, cy, 24 vertices c + r_k (cos, sin)(15 deg k)) as fp32 [51]; ``r`` a scalar or [24]."""
    row = np.zeros(51, dtype=np.float32)
    row[0], row[1], row[2] = cls, cx, cy
    row[3:] = P.regular64(float(cx), float(cy), r).reshape(48)
    return row


def areas(polys):
    """Absolute shoelace areas of [..., 24, 2] polygons in float64."""
    return np.abs(P._shoelace(np.asarray(polys, dtype=np.float64)))


def inter_over_area(cand, rows):
    """cand [24,2], rows [D,24,2] (fp32 values) -> (inter [D], area(rows) [D]) in float64."""
    cand = np.asarray(cand, dtype=np.float32).astype(np.float64)
    rows = np.asarray(rows, dtype=np.float32).astype(np.float64).reshape(-1, 24, 2)
    if len(rows) == 0:
        return np.zeros(0), np.zeros(0)
    iou = P.poly24_iou(cand[None], rows)[0]
    ac, aq = areas(cand), areas(rows)
    return iou * (ac + aq) / (1.0 + iou), aq


def transform_points(x, y, flip, dx, dy, S_w):
    """fp32 coordinates through the rigid map, in double as written, rounded once to fp32."""
    X = np.asarray(x, dtype=np.float32).astype(np.float64)
    Y = np.asarray(y, dtype=np.float32).astype(np.float64)
    X = (float(S_w) - X) if flip else X
    return (X + float(dx)).astype(np.float32), (Y + float(dy)).astype(np.float32)


def paste_labels(pre_labels, pre_count, paste, S, min_margin, thr, max_labels):
    """pre_labels [n,max_labels,51] fp32, pre_count [n] int, paste [n,8] int64, S = (S_h, S_w).
    Returns (rows [n,max_labels,51] fp32, counts [n] int32, ranges [n,2] int32, decisions): ``decisions`` is a list of dicts
    {image, cand, kind, value, distance, passed}; kind is "select", "cap" or "overflow" (no quantity: distance None), "margin"
    (value = how far the centre is inside the margin rectangle, negative outside), "inside" (value = how far the nearest vertex is
    inside the closed image rectangle) or "ioa" (value = inter / area(q) against ``row`` q; passed = below thr); a candidate is
    accepted iff every one of its decisions passed."""
    pre_labels = np.asarray(pre_labels, dtype=np.float32)
    n = len(pre_labels)
    S_h, S_w = int(S[0]), int(S[1])
    W, H, m = float(S_w), float(S_h), float(min_margin)
    out = np.zeros((n, max_labels, 51), dtype=np.float32)
    counts = np.zeros(n, dtype=np.int32)
    ranges = np.zeros((n, 2), dtype=np.int32)
    decisions = []
    for i in range(n):
        pc = int(pre_count[i])
        E = max(0, min(pc, max_labels))
        out[i, :E] = pre_labels[i, :E]
        cur = E
        on, j, flip, dx, dy = (int(v) for v in paste[i][:5])
        select = int(np.asarray(paste[i][5], dtype=np.int64).astype(np.uint64))
        if on and 0 <= j < n:
            if pc > max_labels:
                decisions.append(dict(image=i, cand=None, kind="overflow", value=None, distance=None, passed=False))
            else:
                nc = max(0, min(int(pre_count[j]), max_labels))
                for k in range(nc):
                    if cur >= max_labels:
                        decisions.append(dict(image=i, cand=k, kind="cap", value=None, distance=None, passed=False))
                        break
                    if k >= 64 or not (select >> k) & 1:
                        decisions.append(dict(image=i, cand=k, kind="select", value=None, distance=None, passed=False))
                        continue
                    src = pre_labels[j, k]
                    tx, ty = transform_points(src[1::2], src[2::2], flip, dx, dy, S_w)          # centre first, then the 24 vertices
                    x64, y64 = tx.astype(np.float64), ty.astype(np.float64)
                    d = min(x64[0] - m, (W - m) - x64[0], y64[0] - m, (H - m) - y64[0])
                    ok = bool(x64[0] >= m and x64[0] <= W - m and y64[0] >= m and y64[0] <= H - m)
                    decisions.append(dict(image=i, cand=k, kind="margin", value=float(d), distance=abs(float(d)), passed=ok))
                    if not ok:
                        continue
                    d = float(np.min([x64[1:], W - x64[1:], y64[1:], H - y64[1:]]))
                    ok = bool(np.all((x64[1:] >= 0) & (x64[1:] <= W) & (y64[1:] >= 0) & (y64[1:] <= H)))
                    decisions.append(dict(image=i, cand=k, kind="inside", value=d, distance=abs(d), passed=ok))
                    if not ok:
                        continue
                    idx = (12 - np.arange(24)) % 24 if flip else np.arange(24)
                    row = np.zeros(51, dtype=np.float32)
                    row[0], row[1], row[2] = src[0], tx[0], ty[0]
                    row[3 + 2 * idx], row[4 + 2 * idx] = tx[1:], ty[1:]                         # source vertex k -> vertex (12 - k) mod 24
                    inter, aq = inter_over_area(row[3:].reshape(24, 2), out[i, :cur, 3:].reshape(-1, 24, 2))
                    veto = False
                    for q in range(cur):
                        if not aq[q] > 0.0:
                            continue
                        ioa = float(inter[q] / aq[q])
                        decisions.append(dict(image=i, cand=k, kind="ioa", row=q, value=ioa, distance=abs(ioa - thr), passed=ioa < thr))
                        veto = veto or ioa >= thr
                    if veto:
                        continue
                    out[i, cur] = row
                    cur += 1
        counts[i] = pc + (cur - E)
        ranges[i] = (E, cur)
    return out, counts, ranges, decisions


def accepted(decisions):
    """{(image, cand)} of the candidates that every decision let through."""
    state = {}
    for d in decisions:
        if d["cand"] is None:
            continue
        key = (d["image"], d["cand"])
        state[key] = state.get(key, True) and d["passed"]
    return {k for k, v in state.items() if v}


def centres_inside(poly, H, W):
    """bool [H, W]: the pixel centres (x + 0.5, y + 0.5) inside the 24-gon by the crossing rule of csrc/raster_rule.h: the edge
    (x0, y0) -> (x1, y1) counts for the row yc iff (y0 <= yc) != (y1 <= yc), its crossing is x0 + ((yc - y0) * (x1 - x0)) / (y1 - y0)
    in double as written, and a point is inside iff an odd number of counting edges cross to the right of it (px < crossing)."""
    V = np.asarray(poly, dtype=np.float32).astype(np.float64).reshape(24, 2)
    x0, y0 = V[:, 0][None], V[:, 1][None]
    x1, y1 = np.roll(V[:, 0], -1)[None], np.roll(V[:, 1], -1)[None]
    yc = (np.arange(H, dtype=np.float64) + 0.5)[:, None]
    with np.errstate(all="ignore"):
        counts = (y0 <= yc) != (y1 <= yc)
        xc = x0 + ((yc - y0) * (x1 - x0)) / (y1 - y0)
        px = (np.arange(W, dtype=np.float64) + 0.5)[None, :, None]
        right = counts[:, None, :] & (px < xc[:, None, :])
    return (right.sum(-1) & 1).astype(bool)


def paste_u8(pre_images, out_labels, paste_range, paste):
    """pre_images [n,3,S_h,S_w] fp32, out_labels [n,max_labels,51] fp32, paste_range [n,2], paste [n,8] int64.
    Returns (images [n,3,S_h,S_w] fp32, pasted [n,S_h,S_w] bool = the pixels taken from the partner)."""
    pre = np.asarray(pre_images, dtype=np.float32)
    n, _, S_h, S_w = pre.shape
    out = pre.copy()
    pasted = np.zeros((n, S_h, S_w), dtype=bool)
    for i in range(n):
        on, j, flip, dx, dy = (int(v) for v in paste[i][:5])
        if not on or not 0 <= j < n:
            continue
        mask = np.zeros((S_h, S_w), dtype=bool)
        for r in range(int(paste_range[i][0]), int(paste_range[i][1])):
            mask |= centres_inside(out_labels[i][r][3:], S_h, S_w)
        xu = np.arange(S_w, dtype=np.int64) - dx
        xs = (S_w - 1 - xu) if flip else xu
        ys = np.arange(S_h, dtype=np.int64) - dy
        valid = ((ys >= 0) & (ys < S_h))[:, None] & ((xs >= 0) & (xs < S_w))[None, :]
        take = mask & valid
        yy, xx = np.nonzero(take)
        out[i][:, yy, xx] = pre[j][:, ys[yy], xs[xx]]
        pasted[i] = take
    return out, pasted
