"""Numpy float64 restatement of the two augmentation kernels (``ep24_augment_u8`` / ``ep24_augment_labels``), written from
their contract in include/ep24.h and DESIGN.md section 7, independently of csrc/augment.hip.  Test infrastructure only.

Parameters are duck-typed (``ep24.augment.AugParams``): ``mosaic`` [n], ``centre`` [n,2] (xc, yc), ``partners`` [n,4],
``M`` [n,2,3], ``Minv`` [n,2,3] (a kernel INPUT: the host computes it), ``mirror`` [n], ``hsv_on`` [n], ``hsv`` [n,3].

Besides the outputs, every function returns the distance of its decisions from their thresholds, so that a test can
assert that a case does not sit on a knife edge before it demands equality from the GPU.
"""
import numpy as np

F = np.float32


def letterbox(h, w, S_h, S_w):
    s = min(S_h / h, S_w / w)
    return s, int(w * s), int(h * s)


def tiles_of(params, i, sizes, S_h, S_w):
    """-> list of dicts: src, s, rw, rh, lx1, ly1, lx2, ly2, padw, padh.  A mosaic pins the inner corner of quadrant q at the
    mosaic centre and crops the outer side at the 2S canvas; without mosaic the image is its own tile at the top left."""
    if not params.mosaic[i]:
        h, w = sizes[i]
        s, rw, rh = letterbox(h, w, S_h, S_w)
        return [dict(src=i, s=s, rw=rw, rh=rh, lx1=0, ly1=0, lx2=rw, ly2=rh, padw=0, padh=0)]
    xc, yc = int(params.centre[i][0]), int(params.centre[i][1])
    out = []
    for q in range(4):
        j = int(params.partners[i][q])
        h, w = sizes[j]
        s, rw, rh = letterbox(h, w, S_h, S_w)
        right, bottom = q % 2 == 1, q // 2 == 1
        lx1, lx2 = (xc, min(xc + rw, 2 * S_w)) if right else (max(xc - rw, 0), xc)
        ly1, ly2 = (yc, min(yc + rh, 2 * S_h)) if bottom else (max(yc - rh, 0), yc)
        sx1 = 0 if right else rw - (lx2 - lx1)          # first column / row of the resized image that is visible
        sy1 = 0 if bottom else rh - (ly2 - ly1)
        out.append(dict(src=j, s=s, rw=rw, rh=rh, lx1=lx1, ly1=ly1, lx2=lx2, ly2=ly2, padw=lx1 - sx1, padh=ly1 - sy1))
    return out


def _coef(f, ssize):
    """resize.h's lin_coef from the float32 source coordinate."""
    f = f.astype(F)
    s = np.floor(f).astype(np.int64)
    f = f - s.astype(F)
    lo = s < 0
    f[lo], s[lo] = 0, 0
    hi = s >= ssize - 1
    f[hi], s[hi] = 0, ssize - 1
    s1 = np.minimum(s + 1, ssize - 1)
    return s, s1, np.rint((F(1) - f) * F(2048)).astype(np.int64), np.rint(f * F(2048)).astype(np.int64)


def hsv_shift(b, g, r, dh, ds, dv, dtype=np.float64):
    """BGR 0..255 -> HSV (H [0,180), S, V [0,255]) -> gains -> BGR in ``dtype``, nothing rounded in between."""
    T = dtype
    b, g, r = (np.asarray(x).astype(T) for x in (b, g, r))
    dh, ds, dv = T(dh), T(ds), T(dv)
    with np.errstate(all="ignore"):
        v = np.maximum(np.maximum(b, g), r)
        mn = np.minimum(np.minimum(b, g), r)
        diff = v - mn
        s = np.where(v > 0, (diff * T(255)) / v, T(0)).astype(T)
        hr = (T(60) * (g - b)) / diff
        hg = T(120) + (T(60) * (b - r)) / diff
        hb = T(240) + (T(60) * (r - g)) / diff
        h = np.where(diff > 0, np.where(v == r, hr, np.where(v == g, hg, hb)), T(0)).astype(T)
    h = np.where(h < 0, h + T(360), h).astype(T)
    H = h * T(0.5) + dh
    H = (H - T(180) * np.floor(H / T(180))).astype(T)
    S = np.clip(s + ds, T(0), T(255)).astype(T)
    V = np.clip(v + dv, T(0), T(255)).astype(T)
    hh = (H / T(30)).astype(T)
    i = np.clip(np.floor(hh).astype(np.int64), 0, 5)
    f = (hh - i.astype(T)).astype(T)
    sn = (S / T(255)).astype(T)
    p = V * (T(1) - sn)
    q = V * (T(1) - sn * f)
    t = V * (T(1) - sn * (T(1) - f))
    r2 = np.choose(i, [V, q, p, p, t, V])
    g2 = np.choose(i, [t, V, V, q, p, p])
    b2 = np.choose(i, [p, p, t, V, V, q])
    return b2.astype(T), g2.astype(T), r2.astype(T)


def sample_u8(images, params, input_size):
    """The image half WITHOUT HSV: -> (uint8-valued array [n,3,S_h,S_w] float32, owner [n,S_h,S_w] int (-1 = padding), the
    smallest distance of any canvas coordinate from a region boundary)."""
    S_h, S_w = int(input_size[0]), int(input_size[1])
    n = len(images)
    sizes = [im.shape[:2] for im in images]
    out = np.full((n, 3, S_h, S_w), 114, dtype=np.float32)
    owner = np.full((n, S_h, S_w), -1, dtype=np.int64)
    margin = np.inf
    ys, xs = np.mgrid[0:S_h, 0:S_w].astype(np.float64)
    for i in range(n):
        (i00, i01, i02), (i10, i11, i12) = params.Minv[i]
        xm = (S_w - 1 - xs) if params.mirror[i] else xs
        u = (i00 * xm + i01 * ys) + i02
        v = (i10 * xm + i11 * ys) + i12
        tiles = tiles_of(params, i, sizes, S_h, S_w)
        for t in reversed(range(len(tiles))):
            d = tiles[t]
            if d["lx2"] <= d["lx1"] or d["ly2"] <= d["ly1"] or d["rw"] <= 0 or d["rh"] <= 0:
                continue
            m = (u >= d["lx1"] - 0.5) & (u < d["lx2"] - 0.5) & (v >= d["ly1"] - 0.5) & (v < d["ly2"] - 0.5)
            owner[i][m] = t
            for val, b in ((u, d["lx1"]), (u, d["lx2"]), (v, d["ly1"]), (v, d["ly2"])):
                margin = min(margin, float(np.abs(val - (b - 0.5)).min()))
        for t, d in enumerate(tiles):
            m = owner[i] == t
            if not m.any():
                continue
            src = images[d["src"]].astype(np.int64)
            h, w = src.shape[:2]
            fx = ((u[m] - d["padw"]) + 0.5) * (1.0 / (d["rw"] / w)) - 0.5
            fy = ((v[m] - d["padh"]) + 0.5) * (1.0 / (d["rh"] / h)) - 0.5
            x0, x1, ax0, ax1 = _coef(fx, w)
            y0, y1, by0, by1 = _coef(fy, h)
            for c in range(3):
                ch = src[:, :, c]
                h0 = ch[y0, x0] * ax0 + ch[y0, x1] * ax1
                h1 = ch[y1, x0] * ax0 + ch[y1, x1] * ax1
                val = (((by0 * (h0 >> 4)) >> 16) + ((by1 * (h1 >> 4)) >> 16) + 2) >> 2
                out[i, c][m] = np.clip(val, 0, 255).astype(np.float32)
    return out, owner, margin


def augment_images(images, params, input_size, dtype=np.float64):
    """The whole image half: sampling, then HSV (in ``dtype``) on sampled pixels of images whose switch is on."""
    base, owner, margin = sample_u8(images, params, input_size)
    out = base.astype(dtype)
    for i in range(len(images)):
        if not params.hsv_on[i]:
            continue
        m = owner[i] >= 0
        b, g, r = hsv_shift(base[i, 0][m], base[i, 1][m], base[i, 2][m], *params.hsv[i], dtype=dtype)
        out[i, 0][m], out[i, 1][m], out[i, 2][m] = b, g, r
    return out, owner, margin


RAY = np.stack([np.cos(np.arange(24) * 15 * np.pi / 180), np.sin(np.arange(24) * 15 * np.pi / 180)], 1)


def _box_exit(p, d, x1, y1, x2, y2):
    with np.errstate(divide="ignore"):
        tx = (x2 - p[0]) / d[0] if d[0] > 0 else ((x1 - p[0]) / d[0] if d[0] < 0 else np.inf)
        ty = (y2 - p[1]) / d[1] if d[1] > 0 else ((y1 - p[1]) / d[1] if d[1] < 0 else np.inf)
    return min(tx, ty)


def recast(centre, poly, eps=1e-9):
    """r_k of the 24 rays from ``centre`` through the closed polygon ``poly`` [24,2]: the smallest t >= 0 with the ray point on an
    edge, edge parameter in [0,1] (ends included; ``eps`` keeps a ray through a vertex from slipping between its two edges).
    -> (r [24] with inf where no edge is met, number of edges met per ray)."""
    P, Q = poly, np.roll(poly, -1, axis=0)
    e = Q - P
    w = P - centre
    r, hits = np.full(24, np.inf), np.zeros(24, dtype=int)
    for k in range(24):
        d = RAY[k]
        den = d[0] * e[:, 1] - d[1] * e[:, 0]
        with np.errstate(all="ignore"):
            t = (w[:, 0] * e[:, 1] - w[:, 1] * e[:, 0]) / den
            u = (w[:, 0] * d[1] - w[:, 1] * d[0]) / den
        ok = (den != 0) & (u >= -eps) & (u <= 1 + eps) & (t >= -eps)
        if ok.any():
            r[k] = max(float(t[ok].min()), 0.0)
            hits[k] = int((ok & (u > eps) & (u < 1 - eps)).sum()) or 1
    return r, hits


def augment_labels(targets, sizes, params, input_size, max_labels=50, min_margin=2.0):
    """The label half -> (table [n,max_labels,51] float32, survivors per image, info).  ``info``: ``centre_margin`` /
    ``extent_margin`` = the smallest distance of a keep / drop decision from its threshold, ``kept`` = per image the list of
    (tile, row) of the survivors in output order, ``hits`` = edges met per ray over all survivors."""
    S_h, S_w = int(input_size[0]), int(input_size[1])
    n = len(targets)
    table = np.zeros((n, max_labels, 51), dtype=np.float32)
    counts = np.zeros(n, dtype=np.int64)
    info = dict(centre_margin=np.inf, extent_margin=np.inf, kept=[], hits=[])
    for i in range(n):
        A, t = params.M[i][:, :2], params.M[i][:, 2]
        Ai = params.Minv[i][:, :2]
        kept_rows, kept_ids = [], []
        for q, d in enumerate(tiles_of(params, i, sizes, S_h, S_w)):
            if d["lx2"] <= d["lx1"] or d["ly2"] <= d["ly1"] or d["rw"] <= 0 or d["rh"] <= 0:
                continue
            h, w = sizes[d["src"]]
            rows = np.asarray(targets[d["src"]], dtype=np.float64)
            rows = rows.reshape(-1, 51) if rows.size else np.zeros((0, 51))
            for ri, row in enumerate(rows[:max_labels]):
                X = (row[1::2] * w) * d["s"] + d["padw"]
                Y = (row[2::2] * h) * d["s"] + d["padh"]
                ox = (A[0, 0] * X + A[0, 1] * Y) + t[0]
                oy = (A[1, 0] * X + A[1, 1] * Y) + t[1]
                if params.mirror[i]:
                    ox = S_w - ox
                slack = [ox[0] - min_margin, (S_w - min_margin) - ox[0], oy[0] - min_margin, (S_h - min_margin) - oy[0],
                         X[0] - (d["lx1"] + min_margin), (d["lx2"] - min_margin) - X[0],
                         Y[0] - (d["ly1"] + min_margin), (d["ly2"] - min_margin) - Y[0]]
                info["centre_margin"] = min(info["centre_margin"], abs(min(slack)))
                if min(slack) < 0:
                    continue
                c = np.array([ox[0], oy[0]])
                r, hits = recast(c, np.stack([ox[1:], oy[1:]], 1))
                new = np.zeros((24, 2))
                for k in range(24):
                    dk = RAY[k]
                    rk = min(r[k], _box_exit(c, dk, 0.0, 0.0, float(S_w), float(S_h)))
                    dm = np.array([-dk[0] if params.mirror[i] else dk[0], dk[1]])
                    rk = min(rk, _box_exit((X[0], Y[0]), Ai @ dm, d["lx1"], d["ly1"], d["lx2"], d["ly2"]))
                    new[k] = c + rk * dk
                ext = min(new[:, 0].max() - new[:, 0].min(), new[:, 1].max() - new[:, 1].min())
                info["extent_margin"] = min(info["extent_margin"], abs(ext - 1.0))
                if not ext > 1.0:
                    continue
                out = np.zeros(51)
                out[0], out[1], out[2] = row[0], c[0], c[1]
                out[3::2], out[4::2] = new[:, 0], new[:, 1]
                kept_rows.append(out)
                kept_ids.append((q, ri))
                info["hits"].append(hits)
        counts[i] = len(kept_rows)
        info["kept"].append(kept_ids)
        for j, row in enumerate(kept_rows[:max_labels]):
            table[i, j] = row.astype(np.float32)
    return table, counts, info
