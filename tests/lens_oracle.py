"""Numpy float64 restatement of the fisheye lens model (``ep24_lens_points`` / ``ep24_lens_warp_u8`` / ``ep24_lens_preproc_u8`` /
``ep24_lens_labels``), written from their contract in include/ep24.h and DESIGN.md section 7, independently of csrc/lens.hip.  Test
infrastructure only.

A model is a dict: ``pin`` and ``fish`` (fx, fy, cx, cy), ``k`` (k1..k4), ``theta_max`` (radians).  thetad is inverted by BISECTION
(to below 1e-15), not by the kernels' Newton iteration.

Besides their results, ``warp_image`` and ``warp_labels`` return the distance of every decision from its threshold, so that a test can
assert that a case does not sit on a knife edge before it demands equality from the GPU.
"""
import math

import numpy as np

import fisheye_oracle as F

RAY = F.RAY


def model(pin, fish, k=(0.0, 0.0, 0.0, 0.0), fov_deg=170.0):
    return dict(pin=tuple(map(float, pin)), fish=tuple(map(float, fish)), k=tuple(map(float, k)), theta_max=math.radians(fov_deg / 2.0))


def thetad(th, k):
    t2 = th * th
    return th * (1.0 + t2 * (k[0] + t2 * (k[1] + t2 * (k[2] + t2 * k[3]))))


def invert(td, m):
    """theta in [0, theta_max] with thetad(theta) = td, by bisection: 64 halvings of an interval below pi / 2 end under 1e-19."""
    td = np.asarray(td, dtype=np.float64)
    lo, hi = np.zeros_like(td), np.full_like(td, m["theta_max"])
    for _ in range(64):
        mid = (lo + hi) / 2.0
        below = thetad(mid, m["k"]) < td
        lo, hi = np.where(below, mid, lo), np.where(below, hi, mid)
    return (lo + hi) / 2.0


def to_fisheye(u, v, m):
    """-> (X, Y, rim): rim = tan(theta_max) - r, the distance of the point from the field's rim in normalised pinhole units (>= 0
    inside the field)."""
    u, v = np.asarray(u, dtype=np.float64), np.asarray(v, dtype=np.float64)
    (fx, fy, cx, cy), (gx, gy, dx, dy) = m["pin"], m["fish"]
    a, b = (u - cx) / fx, (v - cy) / fy
    r = np.hypot(a, b)
    th = np.minimum(np.arctan(r), m["theta_max"])
    td = thetad(th, m["k"])
    with np.errstate(all="ignore"):
        s = np.where(r > 0, td / np.where(r > 0, r, 1.0), 1.0)
    return gx * a * s + dx, gy * b * s + dy, math.tan(m["theta_max"]) - r


def to_pinhole(X, Y, m):
    """-> (u, v, rim): rim = thetad(theta_max) - hypot(x, y) in normalised fisheye units (>= 0 inside the field)."""
    X, Y = np.asarray(X, dtype=np.float64), np.asarray(Y, dtype=np.float64)
    (fx, fy, cx, cy), (gx, gy, dx, dy) = m["pin"], m["fish"]
    x, y = (X - dx) / gx, (Y - dy) / gy
    rd = np.hypot(x, y)
    tdm = thetad(m["theta_max"], m["k"])
    td = np.minimum(rd, tdm)
    th = invert(td, m)
    with np.errstate(all="ignore"):
        s = np.where(rd > 0, np.tan(th) / np.where(rd > 0, rd, 1.0), 1.0)
    return fx * x * s + cx, fy * y * s + cy, tdm - rd


def map_points(pts, m, direction):
    f = to_fisheye if direction == "distort" else to_pinhole
    X, Y, _ = f(pts[:, 0], pts[:, 1], m)
    return np.stack([X, Y], 1)


def warp_image(src, m, direction, out_h, out_w, fill=114):
    """-> (uint8 [out_h,out_w,3], sampled [out_h,out_w] bool, margin [out_h,out_w] in pixels: the smallest distance of the pixel's
    decisions from their thresholds - the field rim, then (inside the field) the four source borders, then (sampled) the 1/32
    quantisation steps of both axes)."""
    h, w = src.shape[:2]
    oy, ox = np.mgrid[0:out_h, 0:out_w].astype(np.float64)
    if direction == "distort":                      # the destination is the fisheye frame
        sx, sy, rim = to_pinhole(ox, oy, m)
        rim_px = np.abs(rim) * min(m["fish"][0], m["fish"][1])
    else:
        sx, sy, rim = to_fisheye(ox, oy, m)
        rim_px = np.abs(rim) * min(m["pin"][0], m["pin"][1])
    field = rim >= 0
    border = np.minimum(np.minimum(np.abs(sx), np.abs(sx - (w - 1))), np.minimum(np.abs(sy), np.abs(sy - (h - 1))))
    sampled = field & (sx >= 0) & (sx <= w - 1) & (sy >= 0) & (sy <= h - 1)
    fx, fy = sx * 32.0 + 0.5, sy * 32.0 + 0.5
    step = np.minimum(np.abs(fx - np.round(fx)), np.abs(fy - np.round(fy))) / 32.0
    margin = rim_px.copy()
    margin[field] = np.minimum(margin, border)[field]
    margin[sampled] = np.minimum(margin, step)[sampled]
    out = np.full((out_h, out_w, 3), fill, dtype=np.uint8)
    qx, qy = np.floor(fx[sampled]).astype(np.int64), np.floor(fy[sampled]).astype(np.int64)
    xa, ya, wx, wy = qx >> 5, qy >> 5, (qx & 31)[:, None], (qy & 31)[:, None]
    xb, yb = np.minimum(xa + 1, w - 1), np.minimum(ya + 1, h - 1)
    s = src.astype(np.int64)
    v = ((32 - wx) * (32 - wy) * s[ya, xa] + wx * (32 - wy) * s[ya, xb] + (32 - wx) * wy * s[yb, xa] + wx * wy * s[yb, xb] + 512) >> 10
    out[sampled] = v.astype(np.uint8)
    return out, sampled, margin


def outline(row, h, w, sub=8):
    return F.outline(row, dict(h=h, w=w), sub)


def warp_row(row, m, direction, h, w, oh, ow, scale, sub=8):
    """One label row -> (output row [51] float64 or None when dropped, flag word, margins dict).  ``rim``: the smallest distance of
    an outline point from the field's rim in normalised units - it is no decision (a point beyond is pulled onto the rim,
    continuously), but tells whether an object straddles the rim."""
    row = np.asarray(row, dtype=np.float64)
    f = to_fisheye if direction == "distort" else to_pinhole
    P = outline(row, h, w, sub)
    X, Y, rim = f(P[:, 0], P[:, 1], m)
    M = np.stack([X, Y], 1)
    c = np.array([(M[:, 0].min() + M[:, 0].max()) / 2, (M[:, 1].min() + M[:, 1].max()) / 2])
    ok, m_inside = F.inside(c, M)
    flag = 0
    if not ok:
        cx, cy, _ = f(row[1] * w, row[2] * h, m)
        c = np.array([float(cx), float(cy)])
        flag = 1
    t, m_side = F.recast(c, M)
    pts = c[None, :] + t[:, None] * RAY
    lim = np.array([float(ow), float(oh)])
    m_clamp = float(min(np.abs(pts).min(), np.abs(pts - lim).min()))
    new = np.clip(pts, 0.0, lim) * scale
    ext = min(new[:, 0].max() - new[:, 0].min(), new[:, 1].max() - new[:, 1].min())
    margins = dict(inside=m_inside, side=m_side, clamp=m_clamp, extent=abs(ext - 1.0))
    info = dict(rim_min=float(rim.min()), rim_max=float(rim.max()), clamped=bool((new != pts * scale).any()), dropped=not ext > 1.0)
    if not ext > 1.0:
        return None, flag, margins, info
    out = np.zeros(51)
    out[0], out[1], out[2] = row[0], c[0] * scale, c[1] * scale
    out[3::2], out[4::2] = new[:, 0], new[:, 1]
    return out, flag, margins, info


def warp_labels(targets, sizes, models, direction, out_sizes, max_labels=50, scales=None, sub=8):
    """-> (table [n,max_labels,51] float32, counts [n], flags [n,max_labels], margins: the smallest of each kind over the batch,
    infos: per image the list of its rows' info dicts)."""
    n = len(targets)
    table = np.zeros((n, max_labels, 51), dtype=np.float32)
    counts = np.zeros(n, dtype=np.int32)
    flags = np.zeros((n, max_labels), dtype=np.int32)
    margins = dict(inside=np.inf, side=np.inf, clamp=np.inf, extent=np.inf)
    infos = []
    for i in range(n):
        rows = np.asarray(targets[i], dtype=np.float64)
        rows = rows.reshape(-1, 51) if rows.size else np.zeros((0, 51))
        (h, w), (oh, ow) = sizes[i], out_sizes[i]
        infos.append([])
        for row in rows[:max_labels]:
            out, flag, mg, info = warp_row(row, models[i], direction, h, w, oh, ow, 1.0 if scales is None else scales[i], sub)
            infos[-1].append(info)
            for key in margins:
                margins[key] = min(margins[key], mg[key])
            if out is None:
                continue
            table[i, counts[i]] = out.astype(np.float32)
            flags[i, counts[i]] = flag
            counts[i] += 1
    return table, counts, flags, margins, infos
