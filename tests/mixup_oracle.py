"""Numpy float64 restatement of the mixup variants of the augmentation kernels (``ep24_augment_mix_u8`` /
``ep24_augment_mix_labels``), written from their contract in include/ep24.h and DESIGN.md section 7, independently of
csrc/augment.hip.  Test infrastructure only; the mosaic / affine half is tests/augment_oracle.py's.

Parameters are duck-typed (``ep24.augment.AugParams``): what ``augment_oracle`` reads, plus ``mixup`` [n], ``mix_partner`` [n],
``mix_jit`` [n], ``mix_flip`` [n], ``mix_off`` [n,2] = (x_off, y_off).

Like its sibling, every function returns the distance of its decisions from their thresholds beside the outputs.
"""
import numpy as np

import augment_oracle as ao

# per-pixel class
TILE, PARTNER, PARTNER_PAD, BLACK, PLAIN_PAD = 0, 1, 2, 3, 4
# TILE:        a tile owns the pixel and the partner image does not (this includes every sampled pixel of an image without mixup)
# PARTNER:     the partner image owns the pixel (a tile may own it too)
# PARTNER_PAD: no owner; inside the jittered canvas, on the partner's letterbox padding: (114 + 114) >> 1 = 114
# BLACK:       no owner; outside the jittered canvas: (114 + 0) >> 1 = 57
# PLAIN_PAD:   no owner, image without mixup: 114


def geometry(params, i, sizes, S_h, S_w):
    """The partner of output image i -> dict(src, s, rw, rh, Wj, Hj, x_off, y_off, flip)."""
    j = int(params.mix_partner[i])
    h, w = sizes[j]
    s, rw, rh = ao.letterbox(h, w, S_h, S_w)
    jit = float(params.mix_jit[i])
    Wj, Hj = int(S_w * jit), int(S_h * jit)
    if Wj < 1 or Hj < 1:
        raise ValueError("empty jittered canvas")
    return dict(src=j, s=s, rw=rw, rh=rh, Wj=Wj, Hj=Hj, x_off=int(params.mix_off[i][0]), y_off=int(params.mix_off[i][1]),
                flip=bool(params.mix_flip[i]))


def sample_u8(images, params, input_size):
    """The image half WITHOUT HSV -> (uint8-valued array [n,3,S_h,S_w] float32, class [n,S_h,S_w], tile owner [n,S_h,S_w] as
    ``augment_oracle.sample_u8`` returns it, pixel margin of the tile map, pixel margin of the partner map)."""
    S_h, S_w = int(input_size[0]), int(input_size[1])
    n = len(images)
    sizes = [im.shape[:2] for im in images]
    a, owner, tile_margin = ao.sample_u8(images, params, input_size)
    out = a.copy()
    cls = np.where(owner >= 0, TILE, PLAIN_PAD)
    mix_margin = np.inf
    ys, xs = np.mgrid[0:S_h, 0:S_w]
    for i in range(n):
        if not params.mixup[i]:
            continue
        g = geometry(params, i, sizes, S_h, S_w)
        xm = (S_w - 1 - xs) if params.mirror[i] else xs           # the frame before the final mirror
        px, py = xm + g["x_off"], ys + g["y_off"]
        inside = (px < g["Wj"]) & (py < g["Hj"])
        pxf = np.where(g["flip"], g["Wj"] - 1 - px, px)
        u = (pxf + 0.5) * (S_w / g["Wj"]) - 0.5
        v = (py + 0.5) * (S_h / g["Hj"]) - 0.5
        owned = inside & (u >= -0.5) & (u < g["rw"] - 0.5) & (v >= -0.5) & (v < g["rh"] - 0.5)
        for val, b in ((u, 0), (u, g["rw"]), (v, 0), (v, g["rh"])):
            mix_margin = min(mix_margin, float(np.abs(val[inside] - (b - 0.5)).min()))
        b = np.zeros((3, S_h, S_w), dtype=np.int64)                # the zero canvas
        b[:, inside] = 114                                         # the letterbox padding
        src = images[g["src"]].astype(np.int64)
        h, w = src.shape[:2]
        fx = (u[owned] + 0.5) * (1.0 / (g["rw"] / w)) - 0.5
        fy = (v[owned] + 0.5) * (1.0 / (g["rh"] / h)) - 0.5
        x0, x1, ax0, ax1 = ao._coef(fx, w)
        y0, y1, by0, by1 = ao._coef(fy, h)
        for c in range(3):
            ch = src[:, :, c]
            h0 = ch[y0, x0] * ax0 + ch[y0, x1] * ax1
            h1 = ch[y1, x0] * ax0 + ch[y1, x1] * ax1
            val = (((by0 * (h0 >> 4)) >> 16) + ((by1 * (h1 >> 4)) >> 16) + 2) >> 2
            b[c][owned] = np.clip(val, 0, 255)
        out[i] = ((a[i].astype(np.int64) + b) >> 1).astype(np.float32)
        free = owner[i] < 0
        cls[i][free & inside] = PARTNER_PAD
        cls[i][free & ~inside] = BLACK
        cls[i][owned] = PARTNER
    return out, cls, owner, tile_margin, mix_margin


def augment_images(images, params, input_size, dtype=np.float64):
    """The whole image half: sampling and blend, then HSV (in ``dtype``) on the pixels that a tile or the partner image owns."""
    base, cls, owner, tile_margin, mix_margin = sample_u8(images, params, input_size)
    out = base.astype(dtype)
    for i in range(len(images)):
        if not params.hsv_on[i]:
            continue
        m = (cls[i] == TILE) | (cls[i] == PARTNER)
        b, g, r = ao.hsv_shift(base[i, 0][m], base[i, 1][m], base[i, 2][m], *params.hsv[i], dtype=dtype)
        out[i, 0][m], out[i, 1][m], out[i, 2][m] = b, g, r
    return out, cls, owner, tile_margin, mix_margin


def augment_labels(targets, sizes, params, input_size, max_labels=50, min_margin=2.0):
    """The label half -> (table [n,max_labels,51] float32, survivors per image, info).  The four tiles' survivors are
    ``augment_oracle.augment_labels``'s; the partner's follow them.  ``info`` as the sibling's, with the partner's survivors as
    tile 4 in ``kept``, and ``partner_kept`` = per image the number of partner survivors."""
    S_h, S_w = int(input_size[0]), int(input_size[1])
    table, counts, info = ao.augment_labels(targets, sizes, params, input_size, max_labels, min_margin)
    table, counts = table.copy(), counts.copy()
    info["partner_kept"] = [0] * len(targets)
    for i in range(len(targets)):
        if not params.mixup[i]:
            continue
        g = geometry(params, i, sizes, S_h, S_w)
        h, w = sizes[g["src"]]
        rows = np.asarray(targets[g["src"]], dtype=np.float64)
        rows = rows.reshape(-1, 51) if rows.size else np.zeros((0, 51))
        jx, jy = g["Wj"] / S_w, g["Hj"] / S_h
        kept_rows = []
        for ri, row in enumerate(rows[:max_labels]):
            X = (row[1::2] * w) * g["s"]                           # the letterbox canvas
            Y = (row[2::2] * h) * g["s"]
            PX, PY = X * jx, Y * jy                                # the jittered frame
            if g["flip"]:
                PX = g["Wj"] - PX
            ox, oy = PX - g["x_off"], PY - g["y_off"]              # the crop
            if params.mirror[i]:
                ox = S_w - ox
            slack = [ox[0] - min_margin, (S_w - min_margin) - ox[0], oy[0] - min_margin, (S_h - min_margin) - oy[0],
                     X[0] - min_margin, (g["rw"] - min_margin) - X[0], Y[0] - min_margin, (g["rh"] - min_margin) - Y[0]]
            info["centre_margin"] = min(info["centre_margin"], abs(min(slack)))
            if min(slack) < 0:
                continue
            c = np.array([ox[0], oy[0]])
            r, hits = ao.recast(c, np.stack([ox[1:], oy[1:]], 1))
            new = np.zeros((24, 2))
            for k in range(24):
                dk = ao.RAY[k]
                rk = min(r[k], ao._box_exit(c, dk, 0.0, 0.0, float(S_w), float(S_h)))
                dx = -dk[0] if params.mirror[i] else dk[0]         # undo the final mirror, then the partner's map
                back = np.array([dx / (-jx if g["flip"] else jx), dk[1] / jy])
                rk = min(rk, ao._box_exit((X[0], Y[0]), back, 0.0, 0.0, float(g["rw"]), float(g["rh"])))
                new[k] = c + rk * dk
            ext = min(new[:, 0].max() - new[:, 0].min(), new[:, 1].max() - new[:, 1].min())
            info["extent_margin"] = min(info["extent_margin"], abs(ext - 1.0))
            if not ext > 1.0:
                continue
            out = np.zeros(51)
            out[0], out[1], out[2] = row[0], c[0], c[1]
            out[3::2], out[4::2] = new[:, 0], new[:, 1]
            kept_rows.append(out)
            info["kept"][i].append((4, ri))
            info["hits"].append(hits)
        first = int(min(counts[i], max_labels))
        for j, row in enumerate(kept_rows[:max_labels - first]):
            table[i, first + j] = row.astype(np.float32)
        counts[i] += len(kept_rows)
        info["partner_kept"][i] = len(kept_rows)
    return table, counts, info
