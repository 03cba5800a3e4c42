"""Baseline JPEG forward path in numpy: the arithmetic of libjpeg's default compress path, restated ("JPEG encode").

``rgb_ycc_convert`` (16-bit fixed point), edge extension, ``h2v1`` / ``h2v2`` downsampling with their alternating bias,
``jpeg_fdct_islow`` on samples - 128 (rows first, then columns), quantisation by ``8 * qt`` with round-half-away, and the dummy blocks
that pad the luma grid of a subsampled file to whole MCUs.  All of it integer, so equality with libjpeg is equality in every
coefficient.  The result has the layout of ``ep24.jpeg``: component-major, block row-major over the MCU-padded grid, 64 int16 per
block in natural order.  Test infrastructure, not a product path.
"""
import numpy as np

MODES = {"grey": 0, "4:4:4": 1, "4:2:2": 2, "4:2:0": 3}
FACTORS = {0: (1, 1), 1: (1, 1), 2: (2, 1), 3: (2, 2)}          # luma (h, v) of every mode

# Annex K, natural order
LUMA_Q = np.array([16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87,
                   80, 62, 18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72, 92,
                   95, 98, 112, 100, 103, 99])
CHROMA_Q = np.array([17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99,
                     99, 99, 99] + [99] * 32)


def _fix(x):
    return int(x * 65536 + 0.5)


def quality_tables(q):
    """jpeg_set_quality: -> uint16 [2, 64] (luma, chroma), natural order."""
    q = min(max(int(q), 1), 100)
    scale = 5000 // q if q < 50 else 200 - 2 * q
    return np.stack([np.clip((b * scale + 50) // 100, 1, 255) for b in (LUMA_Q, CHROMA_Q)]).astype(np.uint16)


def ycc(rgb):
    """uint8 [h, w, 3] RGB -> three int64 [h, w] planes."""
    r, g, b = [rgb[:, :, i].astype(np.int64) for i in range(3)]
    y = (_fix(.299) * r + _fix(.587) * g + _fix(.114) * b + 32768) >> 16
    cb = (-_fix(.16874) * r - _fix(.33126) * g + _fix(.5) * b + (128 << 16) + 32767) >> 16
    cr = (_fix(.5) * r - _fix(.41869) * g - _fix(.08131) * b + (128 << 16) + 32767) >> 16
    return y, cb, cr


def grid(h, w, mode):
    """-> per component (fx, fy, wb, hb, blocks_w, blocks_h): the downsampling factors, the real and the MCU-padded block grid."""
    hmax, vmax = FACTORS[mode]
    ncomp = 1 if mode == 0 else 3
    mx, my = -(-w // (8 * hmax)), -(-h // (8 * vmax))
    out = []
    for c in range(ncomp):
        hc, vc = (hmax, vmax) if c == 0 else (1, 1)
        cw, ch = -(-w * hc // hmax), -(-h * vc // vmax)
        out.append((hmax // hc, vmax // vc, -(-cw // 8), -(-ch // 8), mx * hc, my * vc))
    return out


def sample_plane(p, fx, fy, wb, hb):
    """One full-resolution component -> its uint8-valued sample plane [hb * 8, wb * 8] (the edge rules in libjpeg's order)."""
    h, w = p.shape
    cols = np.minimum(np.arange(wb * 8 * fx), w - 1)
    rows = np.minimum(np.arange(-(-h // fy) * fy), h - 1)
    p = p[rows][:, cols]
    if (fx, fy) == (2, 1):
        p = (p[:, 0::2] + p[:, 1::2] + (np.arange(wb * 8) & 1)) >> 1
    elif (fx, fy) == (2, 2):
        p = (p[0::2, 0::2] + p[0::2, 1::2] + p[1::2, 0::2] + p[1::2, 1::2] + 1 + (np.arange(wb * 8) & 1)) >> 2
    return p[np.minimum(np.arange(hb * 8), p.shape[0] - 1)]              # the DOWNSAMPLED rows repeated down


def _descale(v, n):
    return (v + (1 << (n - 1))) >> n


def _fdct_pass(d, first):
    """d: int64 [..., 8] along the transformed axis."""
    d0, d1, d2, d3, d4, d5, d6, d7 = [d[..., i] for i in range(8)]
    t0, t7, t1, t6, t2, t5, t3, t4 = d0 + d7, d0 - d7, d1 + d6, d1 - d6, d2 + d5, d2 - d5, d3 + d4, d3 - d4
    t10, t13, t11, t12 = t0 + t3, t0 - t3, t1 + t2, t1 - t2
    n = 11 if first else 15
    o0 = (t10 + t11) << 2 if first else _descale(t10 + t11, 2)
    o4 = (t10 - t11) << 2 if first else _descale(t10 - t11, 2)
    z1 = (t12 + t13) * 4433
    o2 = _descale(z1 + t13 * 6270, n)
    o6 = _descale(z1 - t12 * 15137, n)
    z1, z2, z3, z4 = t4 + t7, t5 + t6, t4 + t6, t5 + t7
    z5 = (z3 + z4) * 9633
    t4, t5, t6, t7 = t4 * 2446, t5 * 16819, t6 * 25172, t7 * 12299
    z1, z2, z3, z4 = z1 * -7373, z2 * -20995, z3 * -16069 + z5, z4 * -3196 + z5
    o7, o5, o3, o1 = _descale(t4 + z1 + z3, n), _descale(t5 + z2 + z4, n), _descale(t6 + z2 + z3, n), _descale(t7 + z1 + z4, n)
    return np.stack([o0, o1, o2, o3, o4, o5, o6, o7], -1)


def fdct_quant(plane, qt):
    """uint8-valued [hb * 8, wb * 8] -> int16 [hb, wb, 64] quantised coefficients, natural order."""
    hb, wb = plane.shape[0] // 8, plane.shape[1] // 8
    x = plane.astype(np.int64).reshape(hb, 8, wb, 8).transpose(0, 2, 1, 3) - 128          # [hb, wb, row, col]
    x = _fdct_pass(x, True)                                                              # along the rows
    x = np.swapaxes(_fdct_pass(np.swapaxes(x, -1, -2), False), -1, -2)                    # down the columns
    t = x.reshape(hb, wb, 64)
    q8 = 8 * qt.astype(np.int64)
    return (np.sign(t) * ((np.abs(t) + (q8 >> 1)) // q8)).astype(np.int16)


def pad_dummy(c, blocks_w, blocks_h, hc):
    """[hb, wb, 64] -> [blocks_h, blocks_w, 64]: the dummy blocks hold a DC only.  hc: blocks of this component per MCU row."""
    hb, wb = c.shape[:2]
    out = np.zeros((blocks_h, blocks_w, 64), np.int16)
    out[:hb, :wb] = c
    for bx in range(wb, blocks_w):                         # right of the last real block: the DC of the block to the left
        out[:hb, bx, 0] = out[:hb, bx - 1, 0]
    for by in range(hb, blocks_h):                         # a dummy row: the DC of the last block of the row above in the same MCU
        for bx in range(blocks_w):
            out[by, bx, 0] = out[by - 1, bx // hc * hc + hc - 1, 0]
    return out


def forward(img, qt, mode, bgr=False):
    """img: uint8 [h, w, 3] ([h, w] for mode 0), qt: [ncomp or 2, 64] -> list of int16 [blocks_h, blocks_w, 64] per component."""
    mode = MODES.get(mode, mode)
    img = np.asarray(img)
    if mode == 0:
        comps = [img.reshape(img.shape[0], img.shape[1]).astype(np.int64)]
    else:
        comps = ycc(img[:, :, ::-1] if bgr else img)
    out = []
    for c, (fx, fy, wb, hb, bw, bh) in enumerate(grid(img.shape[0], img.shape[1], mode)):
        q = np.asarray(qt)[min(c, len(qt) - 1)]
        co = fdct_quant(sample_plane(comps[c], fx, fy, wb, hb), q)
        out.append(pad_dummy(co, bw, bh, bw // (-(-img.shape[1] // (8 * FACTORS[mode][0])))))
    return out


def flat(coef):
    return np.concatenate([c.reshape(-1) for c in coef])
