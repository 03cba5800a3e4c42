"""Sequential restatement of the COCO mask API's polygon and RLE decoding (rleFrPoly, rleMerge as a union, rleDecode,
rleFrString / rleToString), the specification of ep24.cocomask.  Plain Python lists, ints and floats, one statement per
step of the C code, so that it can be read against it; Python's float is the C double and every operation rounds on its
own.  ``int()`` truncates toward zero like a C cast.
"""
import math


def dense_points(xy, h, w):
    """Steps 1 and 2: integer vertices at 5x scale, every edge walked into max(dx, dy) + 1 points (u, v)."""
    k = len(xy) // 2
    X = [int(5 * xy[2 * j] + .5) for j in range(k)]
    Y = [int(5 * xy[2 * j + 1] + .5) for j in range(k)]
    X.append(X[0])
    Y.append(Y[0])
    u, v = [], []
    for j in range(k):
        xs, xe, ys, ye = X[j], X[j + 1], Y[j], Y[j + 1]
        dx, dy = abs(xe - xs), abs(ye - ys)
        flip = (dx >= dy and xs > xe) or (dx < dy and ys > ye)
        if flip:
            xs, xe = xe, xs
            ys, ye = ye, ys
        if dx == 0 and dy == 0:                       # s = 0 / 0; the point's v is never read
            u.append(xs)
            v.append(ys)
            continue
        s = float(ye - ys) / dx if dx >= dy else float(xe - xs) / dy
        if dx >= dy:
            for d in range(dx + 1):
                t = dx - d if flip else d
                u.append(t + xs)
                v.append(int(ys + s * t + .5))
        else:
            for d in range(dy + 1):
                t = dy - d if flip else d
                v.append(t + ys)
                u.append(int(xs + s * t + .5))
    return u, v


def boundary_points(xy, h, w):
    """Step 3: the (x, y) points at which a column's runs change, y in 0..h."""
    u, v = dense_points(xy, h, w)
    out = []
    for j in range(1, len(u)):
        if u[j] == u[j - 1]:
            continue
        xd = float(u[j] if u[j] < u[j - 1] else u[j] - 1)
        xd = (xd + .5) / 5 - .5
        if math.floor(xd) != xd or xd < 0 or xd > w - 1:
            continue
        yd = float(v[j] if v[j] < v[j - 1] else v[j - 1])
        yd = (yd + .5) / 5 - .5
        if yd < 0:
            yd = 0.0
        elif yd > h:
            yd = float(h)
        yd = math.ceil(yd)
        out.append((int(xd), int(yd)))
    return out


def rle_from_poly(xy, h, w):
    """Steps 1 - 4: column-major run lengths of one polygon, starting with a run of zeros."""
    a = [x * h + y for x, y in boundary_points(xy, h, w)]
    a.append(h * w)
    a.sort()
    p = 0
    for j in range(len(a)):
        t = a[j]
        a[j] -= p
        p = t
    k = len(a)
    b = [a[0]]
    j = 1
    while j < k:
        if a[j] > 0:
            b.append(a[j])
            j += 1
        else:
            j += 1
            if j < k:
                b[-1] += a[j]
                j += 1
    return b


def rle_decode(counts, h, w):
    """rleDecode: rows of 0 / 1, mask[y][x]; the runs are column-major and alternate from 0."""
    assert sum(counts) == h * w and min(counts) >= 0
    flat, val = [], 0
    for c in counts:
        flat.extend([val] * c)
        val = 1 - val
    return [[flat[x * h + y] for x in range(w)] for y in range(h)]


def mask_from_parity(xy, h, w):
    """The per-pixel form: mask[y][x] = parity of the boundary points (x, y') with y' <= y."""
    cnt = [[0] * w for _ in range(h + 1)]
    for x, y in boundary_points(xy, h, w):
        cnt[y][x] += 1
    out = [[0] * w for _ in range(h)]
    for x in range(w):
        run = 0
        for y in range(h):
            run += cnt[y][x]
            out[y][x] = run & 1
    return out


def rle_from_string(s):
    """rleFrString: the compressed ``counts`` of the COCO json -> run lengths."""
    if isinstance(s, bytes):
        s = s.decode("ascii")
    cnts, p = [], 0
    while p < len(s):
        x, k, more = 0, 0, 1
        while more:
            c = ord(s[p]) - 48
            x |= (c & 0x1f) << (5 * k)
            more = c & 0x20
            p += 1
            k += 1
            if not more and (c & 0x10):
                x |= -1 << (5 * k)
        if len(cnts) > 2:
            x += cnts[len(cnts) - 2]
        cnts.append(x)
    return cnts


def rle_to_string(cnts):
    """rleToString, the inverse of rle_from_string."""
    s = []
    for i in range(len(cnts)):
        x = cnts[i]
        if i > 2:
            x -= cnts[i - 2]
        more = True
        while more:
            c = x & 0x1f
            x >>= 5
            more = (x != -1) if (c & 0x10) else (x != 0)
            if more:
                c |= 0x20
            s.append(chr(c + 48))
    return "".join(s)


def ann_to_mask(segmentation, h, w):
    """annToMask: a list of polygons (their union) or an RLE dict -> rows of 0 / 1."""
    if isinstance(segmentation, dict):
        counts = segmentation["counts"]
        if isinstance(counts, (str, bytes)):
            counts = rle_from_string(counts)
        return rle_decode(list(counts), h, w)
    out = [[0] * w for _ in range(h)]
    for xy in segmentation:
        m = rle_decode(rle_from_poly(xy, h, w), h, w)
        for y in range(h):
            for x in range(w):
                out[y][x] |= m[y][x]
    return out
