"""Numpy float64 restatement of the polygon geometry of ep24 (csrc/poly24.h, csrc/mask.hip), written from the contract in
DESIGN.md section 7 and independently of the kernels.

* ``poly24_iou(A, B)``: exact area IoU of 24-gons by the signed trapezoid decomposition, vectorised over the [G, D] pairs.
* ``raster_pixels``: the pixel rule as it is stated, pixel by pixel; ``raster_words``: the packed prefix-XOR form.
* packing, boxes, areas and mask IoU in integers.
"""
import numpy as np

import eval24_oracle as O

F = np.float32


def det_polygons(det, ratio=None):
    """[n, >= 26] rows (cx, cy, 24 radii) -> [n, 24, 2] fp32: c + r_k * (cos, sin)(15 deg k), product and sum rounded to fp32
    separately; with ``ratio`` the centre and the radii are first divided by it in fp32."""
    q = np.asarray(det, dtype=np.float32)[:, :26]
    if ratio is not None:
        q = (q / F(ratio)).astype(np.float32)
    c, s = O.ray_cos_sin()
    xs = (q[:, 0:1] + (q[:, 2:26] * c[None]).astype(np.float32)).astype(np.float32)
    ys = (q[:, 1:2] + (q[:, 2:26] * s[None]).astype(np.float32)).astype(np.float32)
    return np.stack([xs, ys], -1)


def gt_polygons(gt50):
    """[G, 50] label columns 1..50 (centre, 24 vertices) -> [G, 24, 2] fp32."""
    return np.asarray(gt50, dtype=np.float32)[:, 2:].reshape(-1, 24, 2)


def regular(cx, cy, r):
    """A 24-gon with radii r (scalar or [24]) around (cx, cy) as fp32 vertices (through ``det_polygons``)."""
    row = np.concatenate([[cx, cy], np.broadcast_to(np.asarray(r, dtype=np.float64), (24,))]).astype(np.float32)
    return det_polygons(row[None])[0]


def square_radii(h):
    """Radii that put the 24 vertices on the axis-aligned square of half side h (the corners are the 45 degree rays)."""
    th = np.arange(24, dtype=np.float64) * (15.0 * np.pi / 180.0)
    return h / np.maximum(np.abs(np.cos(th)), np.abs(np.sin(th)))


def _rays():
    th = np.arange(24, dtype=np.float64) * (15.0 * np.pi / 180.0)
    return np.cos(th), np.sin(th)


def regular64(cx, cy, r):
    """c + r_k * (cos, sin)(15 deg k) in float64 [24, 2]: analytic cases without the fp32 rounding of the detection path."""
    c, s = _rays()
    r = np.broadcast_to(np.asarray(r, dtype=np.float64), (24,))
    return np.stack([cx + r * c, cy + r * s], -1)


def square64(cx, cy, h):
    """The 24-gon with radii h / max(|cos|, |sin|): every vertex on the axis-aligned square of half side h.  Evaluated as
    c + h * ((cos, sin) / max), so that a side's coordinate is exactly c +- h."""
    c, s = _rays()
    m = np.maximum(np.abs(c), np.abs(s))
    return np.stack([cx + h * (c / m), cy + h * (s / m)], -1)


def _shoelace(P):
    x, y = P[..., 0], P[..., 1]
    x1, y1 = np.roll(x, -1, -1), np.roll(y, -1, -1)
    acc = np.zeros(P.shape[:-2])
    for k in range(24):
        acc = acc + (x[..., k] * y1[..., k] - x1[..., k] * y[..., k])
    return 0.5 * acc


def poly24_iou(A, B):
    """A [G, 24, 2], B [D, 24, 2] -> [G, D] float64.  NaN for a pair with a NaN coordinate, exactly 0 when the vertex boxes do
    not overlap with positive width and height."""
    A = np.asarray(A, dtype=np.float64)
    B = np.asarray(B, dtype=np.float64)
    G, D = len(A), len(B)
    if G == 0 or D == 0:
        return np.zeros((G, D))
    with np.errstate(all="ignore"):
        nan = np.isnan(A).any((1, 2))[:, None] | np.isnan(B).any((1, 2))[None, :]
        alo, ahi = np.nanmin(A, 1), np.nanmax(A, 1)
        blo, bhi = np.nanmin(B, 1), np.nanmax(B, 1)
        w = np.minimum(ahi[:, None, 0], bhi[None, :, 0]) - np.maximum(alo[:, None, 0], blo[None, :, 0])
        h = np.minimum(ahi[:, None, 1], bhi[None, :, 1]) - np.maximum(alo[:, None, 1], blo[None, :, 1])
        overlap = (w > 0) & (h > 0)
        yb = np.minimum(alo[:, None, 1], blo[None, :, 1])                         # [G, D]
        S = np.zeros((G, D))
        for i in range(24):
            i1 = (i + 1) % 24
            ex0, ey0, ex1, ey1 = A[:, i, 0], A[:, i, 1], A[:, i1, 0], A[:, i1, 1]
            er = ex1 > ex0
            exa, exb = np.where(er, ex0, ex1)[:, None], np.where(er, ex1, ex0)[:, None]
            eya, eyb = np.where(er, ey0, ey1)[:, None] - yb, np.where(er, ey1, ey0)[:, None] - yb
            se = np.where(ex0 == ex1, 0.0, np.where(er, 1.0, -1.0))[:, None]
            for j in range(24):
                j1 = (j + 1) % 24
                fx0, fy0, fx1, fy1 = B[:, j, 0], B[:, j, 1], B[:, j1, 0], B[:, j1, 1]
                fr = fx1 > fx0
                fxa, fxb = np.where(fr, fx0, fx1)[None, :], np.where(fr, fx1, fx0)[None, :]
                fya, fyb = np.where(fr, fy0, fy1)[None, :] - yb, np.where(fr, fy1, fy0)[None, :] - yb
                sf = np.where(fx0 == fx1, 0.0, np.where(fr, 1.0, -1.0))[None, :]
                xl, xr = np.maximum(exa, fxa), np.minimum(exb, fxb)
                live = (xl < xr) & (se != 0) & (sf != 0)
                al = eya + (xl - exa) * (eyb - eya) / (exb - exa)
                ar = eya + (xr - exa) * (eyb - eya) / (exb - exa)
                bl = fya + (xl - fxa) * (fyb - fya) / (fxb - fxa)
                br = fya + (xr - fxa) * (fyb - fya) / (fxb - fxa)
                dl, dr = al - bl, ar - br
                ml, mr = np.minimum(al, bl), np.minimum(ar, br)
                cross = ((dl < 0) & (dr > 0)) | ((dl > 0) & (dr < 0))
                t = dl / (dl - dr)
                xm, hm = xl + t * (xr - xl), al + t * (ar - al)
                split = 0.5 * (ml + hm) * (xm - xl) + 0.5 * (hm + mr) * (xr - xm)
                plain = 0.5 * (ml + mr) * (xr - xl)
                term = np.where(cross, split, plain)
                S = S + np.where(live, se * sf * term, 0.0)
        sa, sb = _shoelace(A)[:, None], _shoelace(B)[None, :]
        aa, ab = np.abs(sa), np.abs(sb)
        inter = np.clip(np.sign(sa) * np.sign(sb) * S, 0.0, np.minimum(aa, ab))
        uni = aa + ab - inter
        iou = np.where(uni > 0, inter / np.where(uni > 0, uni, 1.0), 0.0)
        iou = np.where(overlap, iou, 0.0)
        return np.where(nan, np.nan, iou)


def iou_poly24(gt50, det26):
    """The evaluator's "poly24" matrix [G, D]: GT rows' vertices against the detections' 24 points."""
    return poly24_iou(gt_polygons(gt50), det_polygons(det26))


def rect_iou(a, b):
    """IoU of two boxes (x0, y0, x1, y1) in float64."""
    w = max(0.0, min(a[2], b[2]) - max(a[0], b[0]))
    h = max(0.0, min(a[3], b[3]) - max(a[1], b[1]))
    i = w * h
    return i / ((a[2] - a[0]) * (a[3] - a[1]) + (b[2] - b[0]) * (b[3] - b[1]) - i)


# ---------------------------------------------------------------------------------------------------- raster
def _crossings(poly, H):
    """-> counts [H, 24] bool, xc [H, 24] float64 of the pixel rule for the rows yc = 0 .. H - 1."""
    P = np.asarray(poly, dtype=np.float32).astype(np.float64)
    x0, y0 = P[:, 0][None], P[:, 1][None]
    x1, y1 = np.roll(P[:, 0], -1)[None], np.roll(P[:, 1], -1)[None]
    yc = np.arange(H, dtype=np.float64)[:, None]
    with np.errstate(all="ignore"):
        counts = (y0 <= yc) != (y1 <= yc)
        xc = x0 + ((yc - y0) * (x1 - x0)) / (y1 - y0)
    return counts, xc


def raster_pixels(poly, H, W):
    """The pixel rule as stated: pixel (x, y) is set iff an odd number of counting edges have (double)x < xc.  bool [H, W]."""
    counts, xc = _crossings(poly, H)
    x = np.arange(W, dtype=np.float64)[None, :, None]
    with np.errstate(all="ignore"):
        left = counts[:, None, :] & (x < xc[:, None, :])
    return (left.sum(-1) & 1).astype(bool)


def raster_words(poly, H, W):
    """The packed form: word w of a row = XOR over the counting edges of prefix(clamp(ceil(xc) - 32 w, 0, 32)).
    uint32 [H, ceil(W / 32)]."""
    counts, xc = _crossings(poly, H)
    with np.errstate(all="ignore"):
        c = np.ceil(xc)
        c = np.where(c > 0, np.where(c < W, c, W), 0).astype(np.int64)            # a NaN crossing has no pixel left of it
    c = np.where(counts, c, 0)
    WW = (W + 31) // 32
    k = np.clip(c[:, None, :] - 32 * np.arange(WW, dtype=np.int64)[None, :, None], 0, 32)
    pre = ((np.uint64(1) << k.astype(np.uint64)) - np.uint64(1)).astype(np.uint32)
    return np.bitwise_xor.reduce(pre, axis=-1)


def pack_bits(masks):
    """bool / uint8 [N, H, W] -> uint32 [N, H, ceil(W / 32)]: pixel x is bit x & 31 of word x >> 5."""
    m = np.asarray(masks) != 0
    N, H, W = m.shape
    WW = (W + 31) // 32
    pad = np.zeros((N, H, WW * 32), dtype=np.uint64)
    pad[:, :, :W] = m
    sh = np.arange(32, dtype=np.uint64)
    return (pad.reshape(N, H, WW, 32) << sh).sum(-1).astype(np.uint32)


def unpack_bits(words, W):
    w = np.asarray(words, dtype=np.uint32)
    bits = (w[..., None] >> np.arange(32, dtype=np.uint32)) & np.uint32(1)
    return bits.reshape(w.shape[:-1] + (-1,))[..., :W].astype(bool)


def boxes_areas(masks):
    """bool [N, H, W] -> bbox int32 [N, 4] (x0, y0, x1, y1 of the set pixels, (W, H, -1, -1) when empty), area int32 [N]."""
    m = np.asarray(masks) != 0
    N, H, W = m.shape
    bbox = np.zeros((N, 4), dtype=np.int32)
    area = m.reshape(N, -1).sum(1).astype(np.int32)
    for n in range(N):
        ys, xs = np.nonzero(m[n])
        bbox[n] = (xs.min(), ys.min(), xs.max(), ys.max()) if len(xs) else (W, H, -1, -1)
    return bbox, area


def rasterize(polys, H, W):
    """[N, 24, 2] -> (words uint32 [N, H, WW], bbox, area) by the packed form."""
    polys = np.asarray(polys, dtype=np.float32).reshape(-1, 24, 2)
    words = np.zeros((len(polys), H, (W + 31) // 32), dtype=np.uint32)
    for n, p in enumerate(polys):
        words[n] = raster_words(p, H, W)
    bbox, area = boxes_areas(unpack_bits(words, W))
    return words, bbox, area


def mask_iou(a, b):
    """bool [G, H, W], [D, H, W] -> (inter int64 [G, D], iou float64 [G, D]); 0 where the union is empty."""
    a = (np.asarray(a) != 0).reshape(len(a), -1).astype(np.int64)
    b = (np.asarray(b) != 0).reshape(len(b), -1).astype(np.int64)
    inter = a @ b.T
    uni = a.sum(1)[:, None] + b.sum(1)[None, :] - inter
    iou = np.where(uni != 0, inter.astype(np.float64) / np.where(uni != 0, uni, 1).astype(np.float64), 0.0)
    return inter, iou


def generator_pairs(n=40, seed=0):
    """The consistency generator: n pairs of detection rows [n, 2, 26] fp32, centres U(20, 44)^2, radii U(3, 20) - they fit a
    64 x 64 canvas."""
    rng = np.random.default_rng(seed)
    c = rng.uniform(20.0, 44.0, (n, 2, 2))
    r = rng.uniform(3.0, 20.0, (n, 2, 24))
    return np.concatenate([c, r], -1).astype(np.float32)
