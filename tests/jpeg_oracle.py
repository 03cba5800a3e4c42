"""Baseline JPEG decoder in numpy: the arithmetic of libjpeg's default decode path, restated ("JPEG decode").

Bit stream: baseline Huffman, DC differences per component (reset at every restart marker), AC run/size codes, byte stuffing;
coefficients de-zigzagged into natural order.  Arithmetic: dequantise, the ``islow`` integer IDCT (columns first, descale 11,
then rows, descale 18, + 128, clamp), "fancy" triangle upsampling of 2:1 chroma (replication when the chroma row has at most two
samples), 16-bit fixed-point YCbCr -> RGB.  All of it integer, so equality with libjpeg is bit equality.

The layout of ``entropy_decode``'s result is the layout of ``ep24.jpeg``: component-major, block row-major within a component
over the MCU-padded grid, 64 int16 per block.  Slow (pure Python bit reader): test infrastructure, not a product path.
"""
import numpy as np

ZIGZAG = np.array([0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28,
                   35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55,
                   62, 63])


class Unsupported(ValueError):
    pass


class Header:
    pass


def _u16(d, p):
    return (d[p] << 8) | d[p + 1]


def parse(data):
    """Markers up to and including SOS.  -> Header (width, height, ncomp, h, v, qt [ncomp,64] natural order, restart_interval,
    blocks_w, blocks_h (MCU-padded grid per component), dc / ac Huffman tables of each component, scan_pos)."""
    d = bytes(data)
    if len(d) < 4 or d[0] != 0xFF or d[1] != 0xD8:
        raise ValueError("not a JPEG: no SOI")
    qts, huff, hd = {}, {}, Header()
    hd.restart_interval, frame, p = 0, None, 2
    while True:
        if p + 4 > len(d):
            raise ValueError("truncated before SOS")
        if d[p] != 0xFF:
            raise ValueError("marker expected at %d" % p)
        while p < len(d) and d[p] == 0xFF:
            p += 1
        m = d[p]
        p += 1
        if m == 0xD8 or 0xD0 <= m <= 0xD7 or m == 0x01:
            continue
        if p + 2 > len(d):
            raise ValueError("truncated")
        L = _u16(d, p)
        seg, end = d[p + 2:p + L], p + L
        if L < 2 or end > len(d):
            raise ValueError("truncated segment")
        if m == 0xDB:
            q = 0
            while q < len(seg):
                pq, tq = seg[q] >> 4, seg[q] & 15
                if pq:
                    vals = [_u16(seg, q + 1 + 2 * k) for k in range(64)]
                    q += 129
                else:
                    vals = list(seg[q + 1:q + 65])
                    q += 65
                t = np.zeros(64, np.uint16)
                t[ZIGZAG] = vals
                qts[tq] = t
        elif m == 0xC4:
            q = 0
            while q < len(seg):
                tc, th = seg[q] >> 4, seg[q] & 15
                bits = list(seg[q + 1:q + 17])
                n = sum(bits)
                huff[(tc, th)] = (bits, list(seg[q + 17:q + 17 + n]))
                q += 17 + n
        elif m in (0xC0, 0xC1):
            if seg[0] != 8:
                raise Unsupported("%d-bit precision" % seg[0])
            hd.height, hd.width, hd.ncomp = _u16(seg, 1), _u16(seg, 3), seg[5]
            if hd.ncomp not in (1, 3):
                raise Unsupported("%d components" % hd.ncomp)
            frame = [(seg[6 + 3 * i], seg[7 + 3 * i] >> 4, seg[7 + 3 * i] & 15, seg[8 + 3 * i]) for i in range(hd.ncomp)]
        elif m in (0xC2, 0xC3, 0xC5, 0xC6, 0xC7, 0xC9, 0xCA, 0xCB, 0xCD, 0xCE, 0xCF):
            raise Unsupported("SOF%d (progressive, lossless or arithmetic coding)" % (m - 0xC0))
        elif m == 0xDD:
            hd.restart_interval = _u16(seg, 0)
        elif m == 0xDA:
            if frame is None:
                raise ValueError("SOS before SOF")
            if seg[0] != hd.ncomp:
                raise Unsupported("more than one scan")
            sel = {seg[1 + 2 * i]: (seg[2 + 2 * i] >> 4, seg[2 + 2 * i] & 15) for i in range(hd.ncomp)}
            hd.scan_pos = end
            break
        elif m == 0xD9:
            raise ValueError("EOI before SOS")
        p = end
    hd.h = [1] if hd.ncomp == 1 else [f[1] for f in frame]
    hd.v = [1] if hd.ncomp == 1 else [f[2] for f in frame]
    if hd.ncomp == 3 and ((hd.h[0], hd.v[0]) not in ((1, 1), (2, 1), (2, 2)) or hd.h[1:] != [1, 1] or hd.v[1:] != [1, 1]):
        raise Unsupported("sampling %s x %s" % (hd.h, hd.v))
    hmax, vmax = max(hd.h), max(hd.v)
    mx, my = -(-hd.width // (8 * hmax)), -(-hd.height // (8 * vmax))
    hd.mcus_x, hd.mcus_y = mx, my
    hd.blocks_w = [mx * h for h in hd.h]
    hd.blocks_h = [my * v for v in hd.v]
    hd.qt = np.stack([qts[f[3]] for f in frame])
    hd.dc = [huff[(0, sel[f[0]][0])] for f in frame]
    hd.ac = [huff[(1, sel[f[0]][1])] for f in frame]
    return hd


def _lut(bits, vals):
    """16-bit look-up: code length and symbol for every 16-bit window (length 0: no code)."""
    ln, sy = np.zeros(65536, np.uint8), np.zeros(65536, np.uint8)
    code, k = 0, 0
    for l in range(1, 17):
        for _ in range(bits[l - 1]):
            lo = code << (16 - l)
            ln[lo:lo + (1 << (16 - l))] = l
            sy[lo:lo + (1 << (16 - l))] = vals[k]
            code, k = code + 1, k + 1
        code <<= 1
    return ln.tolist(), sy.tolist()


class _Bits:
    def __init__(self, d, p):
        self.d, self.p, self.acc, self.n, self.pad = d, p, 0, 0, 0

    def fill(self):
        d = self.d
        while self.n < 32:
            b = 0
            if self.p < len(d):
                b = d[self.p]
                if b == 0xFF:
                    if self.p + 1 < len(d) and d[self.p + 1] == 0:
                        self.p += 2
                    else:
                        b = None                      # a marker: the segment ends here
                else:
                    self.p += 1
            else:
                b = None
            if b is None:
                self.pad += 8
                b = 0
            self.acc = ((self.acc << 8) | b) & 0xFFFFFFFFFFFF
            self.n += 8

    def peek16(self):
        if self.n < 16:
            self.fill()
        return (self.acc >> (self.n - 16)) & 0xFFFF

    def skip(self, k):
        self.n -= k
        if self.pad > self.n:
            raise ValueError("entropy-coded data ends early")

    def get(self, k):
        if k == 0:
            return 0
        if self.n < k:
            self.fill()
        v = (self.acc >> (self.n - k)) & ((1 << k) - 1)
        self.skip(k)
        return v


def entropy_decode(data):
    """-> (Header, [int16 [blocks_h, blocks_w, 64] per component])."""
    d = bytes(data)
    hd = parse(d)
    dc = [_lut(*t) for t in hd.dc]
    ac = [_lut(*t) for t in hd.ac]
    coef = [np.zeros((hd.blocks_h[c], hd.blocks_w[c], 64), np.int16) for c in range(hd.ncomp)]
    zz = ZIGZAG.tolist()
    br = _Bits(d, hd.scan_pos)
    pred = [0] * hd.ncomp
    nmcu, ri, rst = hd.mcus_x * hd.mcus_y, hd.restart_interval, 0
    for mcu in range(nmcu):
        if ri and mcu and mcu % ri == 0:
            p = br.p                                      # the reader stopped in front of the marker
            while p < len(d) and d[p] == 0xFF and p + 1 < len(d) and d[p + 1] == 0xFF:
                p += 1
            if p + 1 >= len(d) or d[p] != 0xFF or d[p + 1] != 0xD0 + rst:
                raise ValueError("RST%d expected at MCU %d" % (rst, mcu))
            rst = (rst + 1) & 7
            br = _Bits(d, p + 2)
            pred = [0] * hd.ncomp
        my, mx = divmod(mcu, hd.mcus_x)
        for c in range(hd.ncomp):
            for by in range(hd.v[c]):
                for bx in range(hd.h[c]):
                    blk = [0] * 64
                    w = br.peek16()
                    l = dc[c][0][w]
                    if not l:
                        raise ValueError("bad DC code")
                    br.skip(l)
                    t = dc[c][1][w]
                    if t > 11:
                        raise ValueError("bad DC size")
                    v = br.get(t)
                    if t and v < (1 << (t - 1)):
                        v -= (1 << t) - 1
                    pred[c] += v
                    blk[0] = pred[c]
                    k = 1
                    while k < 64:
                        w = br.peek16()
                        l = ac[c][0][w]
                        if not l:
                            raise ValueError("bad AC code")
                        br.skip(l)
                        rs = ac[c][1][w]
                        r, s = rs >> 4, rs & 15
                        if s == 0:
                            if r != 15:
                                break
                            k += 16
                            continue
                        k += r
                        if k > 63:
                            raise ValueError("AC run past the block")
                        v = br.get(s)
                        if v < (1 << (s - 1)):
                            v -= (1 << s) - 1
                        blk[zz[k]] = v
                        k += 1
                    coef[c][my * hd.v[c] + by, mx * hd.h[c] + bx] = np.asarray(blk, np.int64).astype(np.int16)
    return hd, coef


def _descale(v, n):
    v = (v + (1 << (n - 1))).astype(np.int32)            # wrapping 32-bit, arithmetic shift
    return v >> n


def _idct_pass(x, n):
    """x: int64 [..., 8] along the transformed axis -> int32 [..., 8]."""
    x0, x1, x2, x3, x4, x5, x6, x7 = [x[..., i] for i in range(8)]
    z1 = (x2 + x6) * 4433
    t2 = z1 - x6 * 15137
    t3 = z1 + x2 * 6270
    t0 = (x0 + x4) << 13
    t1 = (x0 - x4) << 13
    t10, t13, t11, t12 = t0 + t3, t0 - t3, t1 + t2, t1 - t2
    a0, a1, a2, a3 = x7, x5, x3, x1
    z1, z2, z3, z4 = a0 + a3, a1 + a2, a0 + a2, a1 + a3
    z5 = (z3 + z4) * 9633
    a0, a1, a2, a3 = a0 * 2446, a1 * 16819, a2 * 25172, a3 * 12299
    z1, z2 = z1 * -7373, z2 * -20995
    z3, z4 = z3 * -16069 + z5, z4 * -3196 + z5
    a0, a1, a2, a3 = a0 + z1 + z3, a1 + z2 + z4, a2 + z2 + z3, a3 + z1 + z4
    out = [t10 + a3, t11 + a2, t12 + a1, t13 + a0, t13 - a0, t12 - a1, t11 - a2, t10 - a3]
    return np.stack([_descale(o, n) for o in out], -1).astype(np.int64)


def idct(coef, qt):
    """coef int16 [..., 64] natural order, qt [64] -> uint8 [..., 8, 8]."""
    x = (coef.astype(np.int64) * qt.astype(np.int64)).reshape(coef.shape[:-1] + (8, 8))
    ws = np.swapaxes(_idct_pass(np.swapaxes(x, -1, -2), 11), -1, -2)        # pass 1: down the columns
    out = _idct_pass(ws, 18)                                                 # pass 2: along the rows
    return np.clip(out + 128, 0, 255).astype(np.uint8)


def planes(hd, coef):
    """MCU-padded uint8 sample plane [blocks_h * 8, blocks_w * 8] of every component."""
    out = []
    for c in range(hd.ncomp):
        px = idct(coef[c], hd.qt[c])                                         # [bh, bw, 8, 8]
        out.append(px.transpose(0, 2, 1, 3).reshape(hd.blocks_h[c] * 8, hd.blocks_w[c] * 8))
    return out


def _h2v1(p):
    p = p.astype(np.int32)
    dw = p.shape[1]
    if dw <= 2:
        return np.repeat(p, 2, 1)
    i = np.arange(dw)
    left, right = p[:, np.maximum(i - 1, 0)], p[:, np.minimum(i + 1, dw - 1)]
    out = np.empty((p.shape[0], 2 * dw), np.int32)
    out[:, 0::2] = (3 * p + left + 1) >> 2
    out[:, 1::2] = (3 * p + right + 2) >> 2
    return out


def _h2v2(p):
    p = p.astype(np.int32)
    dh, dw = p.shape
    if dw <= 2:
        return np.repeat(np.repeat(p, 2, 0), 2, 1)
    out = np.empty((2 * dh, 2 * dw), np.int32)
    r, i = np.arange(dh), np.arange(dw)
    for half, nb in ((0, np.maximum(r - 1, 0)), (1, np.minimum(r + 1, dh - 1))):
        cs = 3 * p + p[nb]
        left, right = cs[:, np.maximum(i - 1, 0)], cs[:, np.minimum(i + 1, dw - 1)]
        out[half::2, 0::2] = (3 * cs + left + 8) >> 4
        out[half::2, 1::2] = (3 * cs + right + 7) >> 4
    return out


def color(hd, pl, bgr=False):
    """Crop, upsample, convert: planes -> uint8 [H, W, 3]."""
    H, W = hd.height, hd.width
    y = pl[0][:H, :W].astype(np.int32)
    if hd.ncomp == 1:
        return np.repeat(y[:, :, None], 3, 2).astype(np.uint8)
    hmax, vmax = max(hd.h), max(hd.v)
    ch = []
    for c in (1, 2):
        dw, dh = -(-W * hd.h[c] // hmax), -(-H * hd.v[c] // vmax)
        p = pl[c][:dh, :dw]
        if (hmax, vmax) == (2, 1):
            p = _h2v1(p)
        elif (hmax, vmax) == (2, 2):
            p = _h2v2(p)
        ch.append(p[:H, :W].astype(np.int32) - 128)
    cb, cr = ch
    r = y + ((91881 * cr + 32768) >> 16)
    b = y + ((116130 * cb + 32768) >> 16)
    g = y + ((-22554 * cb - 46802 * cr + 32768) >> 16)
    order = (b, g, r) if bgr else (r, g, b)
    return np.clip(np.stack(order, -1), 0, 255).astype(np.uint8)


def flat_coefficients(coef):
    """The component-major int16 vector that ``ep24.jpeg.entropy_decode`` returns."""
    return np.concatenate([c.reshape(-1) for c in coef])


def decode(data, bgr=False):
    hd, coef = entropy_decode(data)
    return color(hd, planes(hd, coef), bgr)
