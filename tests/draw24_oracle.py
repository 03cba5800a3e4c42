"""numpy restatement of the drawing contract (include/ep24.h E3), written from the contract: float32 for the
row geometry (every operation separate), int64 for every coverage test, float64 for the fill's crossing.  It reads ``ep24.draw``'s
``FONT`` and ``palette``; it shares no code with csrc/draw.hip.  One row at a time, vectorised over the pixels of the row's reach.
"""
from fractions import Fraction

import numpy as np

from ep24.draw import FONT, palette
from ep24.evaluate import ray_cos_sin

F32 = np.float32
LIM = F32(1048576.0)            # 2^20


def default_colors(C):
    return palette(C).numpy()


def label_bytes(cls, class_names=None):
    """The class's label: its decimal index, or its name cut to 21 bytes."""
    return (str(cls) if class_names is None else str(class_names[cls])).encode("utf-8")[:21]


def row_geometry(row, ratio, conf, H, W, C):
    """One ``[29]`` row -> None (skipped) or a dict: xc, yc, vx[24], vy[24] (int64), cls, score (float32), fx / fy (the float32
    vertex values before clamp and truncation: what the margins are taken from) and r (the truncated radii)."""
    row = np.asarray(row, dtype=F32)
    ratio, conf = F32(ratio), F32(conf)
    cs = ray_cos_sin()
    with np.errstate(all="ignore"):
        score = F32(row[26] * row[27])
        if not (score >= conf):
            return None
        q = (row[:26] / ratio).astype(F32)
        if not np.all(np.isfinite(q)) or not np.all(np.abs(q) < LIM):
            return None
        fc = row[28]
        if not (fc > F32(-1.0) and fc < F32(C)):            # (int)col28 in [0, C): truncation toward zero
            return None
    cls = int(fc)
    xc, yc = int(q[0]), int(q[1])                           # int() truncates toward zero
    r = np.trunc(q[2:26]).astype(F32)
    fx = (F32(xc) + (r * cs[:24]).astype(F32)).astype(F32)
    fy = (F32(yc) + (r * cs[24:]).astype(F32)).astype(F32)
    vx = np.trunc(np.minimum(np.maximum(fx, F32(0)), F32(W))).astype(np.int64)
    vy = np.trunc(np.minimum(np.maximum(fy, F32(0)), F32(H))).astype(np.int64)
    return dict(xc=xc, yc=yc, vx=vx, vy=vy, cls=cls, score=score, fx=fx, fy=fy, r=r.astype(np.int64))


def vertex_margin(geo):
    """Smallest distance to an integer over the row's float32 vertex values in which a float decides: those whose float32
    evaluation ROUNDED (the same expression in float64 - exact there: a 20-bit integer times a 24-bit factor plus a 21-bit integer -
    gives another number).  Left out, because no rounding can move them across an integer:
      - values that float32 forms exactly (factors 1, -1 and 0.5 of the rays at 0, 60, 90, ... degrees; zero radii): every
        implementation returns the same number;
      - the four near-zero factors (cos 90 = 6.1e-17, cos 270 = -1.8e-16, sin 180 = 1.2e-16, sin 0 = 0): with |r| < 2^20 the product
        is below 2^-32, far less than half an ulp of any non-zero integer centre, so separate operations and a fused multiply-add
        both return the centre itself; for a centre of 0 the value is that product, and max(v, 0) followed by truncation is 0.
    For every other value the truncation (int) flips only if a rounding carried it across an integer."""
    cs = ray_cos_sin().astype(np.float64)
    r = geo["r"].astype(np.float64)
    m = np.inf
    for f32, c, tab in ((geo["fx"], geo["xc"], cs[:24]), (geo["fy"], geo["yc"], cs[24:])):
        exact = float(c) + r * tab
        rounded = (f32.astype(np.float64) != exact) & (np.abs(tab) > 2.0 ** -40)
        if rounded.any():
            v = f32.astype(np.float64)[rounded]
            m = min(m, float(np.min(np.abs(v - np.rint(v)))))
    return m


def cover_disc(X, Y, cx, cy, r2):
    return (X - cx) ** 2 + (Y - cy) ** 2 <= r2


def cover_edge(X, Y, P, Q):
    """Squared distance of the pixel to the segment P -> Q is <= 1, in int64."""
    dx, dy = int(Q[0]) - int(P[0]), int(Q[1]) - int(P[1])
    wx, wy = X - int(P[0]), Y - int(P[1])
    L2 = dx * dx + dy * dy
    t = wx * dx + wy * dy
    at_p = wx * wx + wy * wy <= 1
    at_q = (X - int(Q[0])) ** 2 + (Y - int(Q[1])) ** 2 <= 1
    cross = dx * wy - dy * wx
    mid = cross * cross <= L2
    return np.where(t <= 0, at_p, np.where(t >= L2, at_q, mid))


def segment_dist2_exact(x, y, P, Q):
    """Exact squared distance of the point to the segment, as a Fraction."""
    px, py, qx, qy = (int(v) for v in (P[0], P[1], Q[0], Q[1]))
    dx, dy = qx - px, qy - py
    wx, wy = x - px, y - py
    L2 = dx * dx + dy * dy
    if L2 == 0:
        return Fraction(wx * wx + wy * wy)
    t = min(max(Fraction(wx * dx + wy * dy, L2), Fraction(0)), Fraction(1))
    ex, ey = Fraction(wx) - t * dx, Fraction(wy) - t * dy
    return ex * ex + ey * ey


def cover_text(X, Y, xc, yc, data, s, font=FONT):
    out = np.zeros(X.shape, dtype=bool)
    m = len(data)
    if m == 0:
        return out
    u, v = X - (xc + 3), Y - (yc - 3 - 7 * s)
    ok = (v >= 0) & (v < 7 * s) & (u >= 0) & (u < 6 * s * m)
    if not ok.any():
        return out
    glyphs = np.array([font[(b if 32 <= b <= 126 else ord("?")) - 32] for b in data], dtype=np.int64)      # [m, 7]
    uu, vv = np.where(ok, u, 0), np.where(ok, v, 0)
    j = uu // (6 * s)
    cu = (uu % (6 * s)) // s
    bits = glyphs[j, vv // s]
    return ok & (cu < 5) & (((bits >> (4 - np.minimum(cu, 4))) & 1) == 1)


def fill_inside(X, Y, vx, vy):
    """The rasteriser's rule on the integer vertices, in float64."""
    xd, yd = X.astype(np.float64), Y.astype(np.float64)
    par = np.zeros(X.shape, dtype=bool)
    for k in range(24):
        x0, y0 = float(vx[k]), float(vy[k])
        x1, y1 = float(vx[(k + 1) % 24]), float(vy[(k + 1) % 24])
        counts = (y0 <= yd) != (y1 <= yd)
        if y1 == y0 or not counts.any():
            continue
        xcross = x0 + ((yd - y0) * (x1 - x0)) / (y1 - y0)
        par ^= counts & (xd < xcross)
    return par


def blend(pix, color, a):
    """Per channel (pix * (256 - a) + color * a + 128) >> 8, integers."""
    return ((pix.astype(np.int64) * (256 - a) + np.asarray(color, dtype=np.int64) * a + 128) >> 8).astype(np.uint8)


def score_digits(score):
    pct = min(99, max(0, int(F32(F32(score) * F32(100.0)))))
    return b" %d%d" % (pct // 10, pct % 10)


def draw(image, dets, ratio=1.0, conf=0.0, num_classes=80, class_names=None, colors=None, fill_alpha=0, font_scale=2,
         show_scores=False, margins=None):
    """The contract, row by row.  ``margins``: a list that receives ``vertex_margin`` of every row that draws."""
    img = np.array(image, dtype=np.uint8, copy=True)
    H, W = img.shape[:2]
    colors = default_colors(num_classes) if colors is None else np.asarray(colors, dtype=np.uint8)
    s = int(font_scale)
    if dets is None:
        return img
    for row in np.asarray(dets, dtype=np.float32).reshape(-1, 29):
        geo = row_geometry(row, ratio, conf, H, W, num_classes)
        if geo is None:
            continue
        if margins is not None:
            margins.append(vertex_margin(geo))
        xc, yc, vx, vy = geo["xc"], geo["yc"], geo["vx"], geo["vy"]
        data = label_bytes(geo["cls"], class_names)
        if show_scores:
            data = (data + score_digits(geo["score"]))[:24]
        # the row's reach: discs of radius 4 / 2, edges within 1 of the vertices' hull, the text cell block; the fill lies inside the hull
        x0 = min(xc - 4, int(vx.min()) - 2, xc + 3)
        x1 = max(xc + 4, int(vx.max()) + 2, xc + 3 + 6 * s * len(data))
        y0 = min(yc - 4, int(vy.min()) - 2, yc - 3 - 7 * s)
        y1 = max(yc + 4, int(vy.max()) + 2, yc - 3)
        x0, y0, x1, y1 = max(x0, 0), max(y0, 0), min(x1, W - 1), min(y1, H - 1)
        if x0 > x1 or y0 > y1:
            continue
        Y, X = np.meshgrid(np.arange(y0, y1 + 1, dtype=np.int64), np.arange(x0, x1 + 1, dtype=np.int64), indexing="ij")
        solid = cover_disc(X, Y, xc, yc, 16)
        for k in range(24):
            solid |= cover_disc(X, Y, int(vx[k]), int(vy[k]), 4)
            solid |= cover_edge(X, Y, (vx[k], vy[k]), (vx[(k + 1) % 24], vy[(k + 1) % 24]))
        solid |= cover_text(X, Y, xc, yc, data, s)
        region = img[y0:y1 + 1, x0:x1 + 1]
        color = colors[geo["cls"]]
        if fill_alpha > 0:
            inside = fill_inside(X, Y, vx, vy) & ~solid
            region[inside] = blend(region[inside], color, int(fill_alpha))
        region[solid] = color
    return img
