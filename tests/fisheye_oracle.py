"""Numpy float64 restatement of the continuous sector map and the label warp (``ep24_sector_points`` / ``ep24_sector_labels``),
written from their contract in include/ep24.h and DESIGN.md section 7, independently of csrc/sector.hip.  Test infrastructure only.

A geometry is a dict: ``theta`` (degrees), ``T`` (rows), ``h``, ``w`` (source image), ``cw`` (canvas width), ``x0``, ``y0`` (crop
origin), ``oh``, ``ow`` (size of the warped image).  ``geometry`` fills one from the reference's 1-D tables.

Besides its results, ``warp_labels`` returns the distance of every decision from its threshold, so that a test can assert that a case
does not sit on a knife edge before it demands equality from the GPU.
"""
import numpy as np

N = 13200
CANVAS = 1000
RAY = np.stack([np.cos(np.arange(24) * 15 * np.pi / 180), np.sin(np.arange(24) * 15 * np.pi / 180)], 1)


def geometry(theta, h, w, custom_rows=None):
    """Row count, canvas width and crop box of ``sector_distort`` (demo_featuremap.py:245-306) from its 1-D tables alone: rho > 0, so
    rho*cos and rho*sin are extreme where both factors are, and truncation and clipping keep the order."""
    cw = int(CANVAS * np.sin(theta / 2 * np.pi / 180) * 2)
    start = (180 - theta) / 2
    ang = np.linspace(start, start + theta, N, True) * np.pi / 180
    c, s = np.cos(ang), np.sin(ang)
    if custom_rows is None:
        ends = (c * CANVAS).astype(np.int16) + (s * CANVAS).astype(np.int16) * 1j
        T = int(np.clip(int(np.unique(ends).shape[0] * (h / w)), 0, CANVAS - 100))
    else:
        T = int(custom_rows)
    rho = np.linspace(CANVAS - T, CANVAS, T)

    def lo(v):                                    # the extreme products of a table value with a radius
        return min(v * rho.min(), v * rho.max())

    def hi(v):
        return max(v * rho.min(), v * rho.max())

    def dest_x(v):
        return int(np.int16(np.clip(np.int16(v) + cw / 2 - 1, 0, cw)))

    def dest_y(v):
        return int(np.clip((CANVAS - int(np.int16(v))) - 1, 0, CANVAS))

    x0, x1 = dest_x(lo(c.min())), dest_x(hi(c.max()))
    y0, y1 = dest_y(hi(s.max())), dest_y(lo(s.min()))
    return dict(theta=float(theta), T=T, h=int(h), w=int(w), cw=cw, x0=x0, y0=y0, oh=y1 - y0, ow=x1 - x0)


def sector_map(u, v, g):
    """Source point (u, v) in pixel-index coordinates -> (X, Y) in the warped image, contract section 1."""
    u, v = np.asarray(u, dtype=np.float64), np.asarray(v, dtype=np.float64)
    T, th = float(g["T"]), float(g["theta"])
    dx = (u + 0.5) * (N / g["w"]) - 0.5
    dy = (v + 0.5) * (T / g["h"]) - 0.5
    a = (N - 1) - dx
    r = (T - 1) - dy
    ang = ((180 - th) / 2 + th * a / (N - 1)) * np.pi / 180
    rho = (CANVAS - T) + T * r / (T - 1)
    c, s = rho * np.cos(ang), rho * np.sin(ang)
    X = c + g["cw"] / 2 - 1 - g["x0"] - 0.5 * np.sign(c)
    Y = CANVAS - s - 1 - g["y0"] + 0.5
    return X, Y


def texel_centre(flat, g):
    """Source point whose resized-image coordinates are exactly the texel ``flat`` = row * N + column of the [T, N] resized image."""
    row, col = flat // N, flat % N
    return (col + 0.5) / (N / g["w"]) - 0.5, (row + 0.5) / (g["T"] / g["h"]) - 0.5


def outline(row, g, sub=8):
    """The 24 * sub outline points of a label row, in order, in source pixel coordinates."""
    P = np.stack([row[3::2] * g["w"], row[4::2] * g["h"]], 1)
    Q = np.roll(P, -1, axis=0)
    f = (np.arange(sub) / sub)[None, :, None]
    return (P[:, None, :] + f * (Q - P)[:, None, :]).reshape(-1, 2)


def inside(c, poly):
    """Even-odd rule -> (inside?, the smallest distance of a decision from its threshold)."""
    P, Q = poly, np.roll(poly, -1, axis=0)
    margin = float(np.abs(poly[:, 1] - c[1]).min())
    cross = (P[:, 1] > c[1]) != (Q[:, 1] > c[1])
    xc = P[cross, 0] + (c[1] - P[cross, 1]) * (Q[cross, 0] - P[cross, 0]) / (Q[cross, 1] - P[cross, 1])
    if xc.size:
        margin = min(margin, float(np.abs(xc - c[0]).min()))
    return int((xc > c[0]).sum()) % 2 == 1, margin


def recast(c, poly):
    """Nearest intersection of each of the 24 rays from ``c`` with the closed outline -> (t [24], 0 where a ray meets no edge;
    the smallest |side value| of a vertex and the smallest |t| of a crossing, i.e. how far any decision is from flipping)."""
    P, Q = poly, np.roll(poly, -1, axis=0)
    t_out, margin = np.zeros(24), np.inf
    for k in range(24):
        d = RAY[k]
        sp = d[0] * (P[:, 1] - c[1]) - d[1] * (P[:, 0] - c[0])
        sq = np.roll(sp, -1)
        margin = min(margin, float(np.abs(sp).min()))
        hit = (sp < 0) != (sq < 0)
        u = sp[hit] / (sp[hit] - sq[hit])
        I = P[hit] + u[:, None] * (Q[hit] - P[hit])
        t = (I - c) @ d
        if t.size:
            margin = min(margin, float(np.abs(t).min()))
        t = t[t >= 0]
        t_out[k] = t.min() if t.size else 0.0
    return t_out, margin


def warp_row(row, g, r, sub=8):
    """One label row -> (output row [51] float64 or None when dropped, flag word, margins dict, radii [24] in warped pixels)."""
    row = np.asarray(row, dtype=np.float64)
    M = np.stack(sector_map(*outline(row, g, sub).T, g), 1)
    c = np.array([(M[:, 0].min() + M[:, 0].max()) / 2, (M[:, 1].min() + M[:, 1].max()) / 2])
    ok, m_inside = inside(c, M)
    flag = 0
    if not ok:
        c = np.array([float(v) for v in sector_map(row[1] * g["w"], row[2] * g["h"], g)])
        flag = 1
    t, m_side = recast(c, M)
    pts = c[None, :] + t[:, None] * RAY
    lim = np.array([float(g["ow"]), float(g["oh"])])
    m_clamp = float(min(np.abs(pts).min(), np.abs(pts - lim).min()))
    new = np.clip(pts, 0.0, lim) * r
    ext = min(new[:, 0].max() - new[:, 0].min(), new[:, 1].max() - new[:, 1].min())
    margins = dict(inside=m_inside, side=m_side, clamp=m_clamp, extent=abs(ext - 1.0))
    if not ext > 1.0:
        return None, flag, margins, t
    out = np.zeros(51)
    out[0], out[1], out[2] = row[0], c[0] * r, c[1] * r
    out[3::2], out[4::2] = new[:, 0], new[:, 1]
    return out, flag, margins, t


def warp_labels(targets, geoms, input_size, max_labels=50, sub=8):
    """-> (table [n,max_labels,51] float32, counts [n], flags [n,max_labels], margins: the smallest of each kind over the batch)."""
    S_h, S_w = int(input_size[0]), int(input_size[1])
    n = len(targets)
    table = np.zeros((n, max_labels, 51), dtype=np.float32)
    counts = np.zeros(n, dtype=np.int32)
    flags = np.zeros((n, max_labels), dtype=np.int32)
    margins = dict(inside=np.inf, side=np.inf, clamp=np.inf, extent=np.inf)
    for i, g in enumerate(geoms):
        rows = np.asarray(targets[i], dtype=np.float64)
        rows = rows.reshape(-1, 51) if rows.size else np.zeros((0, 51))
        r = min(S_h / g["oh"], S_w / g["ow"])
        for row in rows[:max_labels]:
            out, flag, m, _ = warp_row(row, g, r, sub)
            for key in margins:
                margins[key] = min(margins[key], m[key])
            if out is None:
                continue
            table[i, counts[i]] = out.astype(np.float32)
            flags[i, counts[i]] = flag
            counts[i] += 1
    return table, counts, flags, margins


def blob_rows(rng, k, h, w, rmin, rmax, wobble=0.25):
    """k label rows [k,51] (normalised): smooth closed outlines r(phi) = R * (1 + wobble * sin(m * phi + p)) with R in [rmin, rmax]
    around centres that keep the whole outline inside the h x w image; ``rng`` is a ``np.random.RandomState``."""
    phi = np.arange(24) * 15 * np.pi / 180
    rows = np.zeros((k, 51))
    for i in range(k):
        R = rng.uniform(rmin, rmax)
        reach = R * (1 + abs(wobble)) + 1
        cx, cy = rng.uniform(reach, w - reach), rng.uniform(reach, h - reach)
        rad = R * (1 + wobble * np.sin(rng.randint(2, 4) * phi + rng.uniform(0, 2 * np.pi)))
        rows[i, 0] = rng.randint(0, 80)
        rows[i, 1], rows[i, 2] = cx / w, cy / h
        rows[i, 3::2] = (cx + rad * np.cos(phi)) / w
        rows[i, 4::2] = (cy + rad * np.sin(phi)) / h
    return rows
