"""NumPy oracle of the feature-map response kernels, written from the contract in include/ep24.h (E4), not from the kernels.
fp32 steps are np.float32 operations one by one; double steps are float64.  Slow and plain on purpose."""
import numpy as np

F = np.float32
LIM = F(1048576.0)                                             # 2^20


def bf16_round(x):
    """float32 array -> the nearest bfloat16 values (round to nearest even), as float32."""
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32).astype(np.uint64)
    u = (u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFF0000
    return u.astype(np.uint32).view(np.float32)


def bf16_bits(x):
    """float32 array holding bf16-representable values -> their uint16 bit patterns (as int16 for torch.from_numpy)."""
    return (np.ascontiguousarray(x, dtype=np.float32).view(np.uint32) >> 16).astype(np.uint16).view(np.int16)


def mean_exact(rows):
    """rows [M, C] of integer-valued operands: np.float32(sum) / np.float32(C) - every order gives the same fp32 sum."""
    rows = np.asarray(rows, dtype=np.float64)
    s = rows.sum(1)
    assert np.all(s == np.round(s)) and np.all(np.abs(rows).sum(1) < 2 ** 24)
    return (s.astype(np.float32) / F(rows.shape[1])).astype(np.float32)


def mean_f64(rows):
    return np.asarray(rows, dtype=np.float64).mean(1)


def mean_bound(rows):
    """A-priori bound of an fp32 sum of C terms in any order plus one division, against the float64 mean."""
    rows = np.asarray(rows, dtype=np.float64)
    C = rows.shape[1]
    return 1.001 * (C + 1) * 2.0 ** -24 * np.abs(rows).mean(1)


def value_range(maps):
    """[N, cells] -> float32 [N, 2]: fmin / fmax from (+inf, -inf): NaNs are ignored."""
    maps = np.asarray(maps, dtype=np.float32).reshape(len(maps), -1)
    out = np.empty((len(maps), 2), dtype=np.float32)
    for n, m in enumerate(maps):
        lo, hi = F(np.inf), F(-np.inf)
        for v in m:
            lo, hi = np.fmin(lo, v), np.fmax(hi, v)
        out[n] = (lo, hi)
    return out


def color_index(v, lo, hi):
    v, lo, hi = F(v), F(lo), F(hi)
    with np.errstate(all="ignore"):
        t = F(F(v - lo) / F(hi - lo))
        q = F(t * F(256.0))
    if not (hi > lo) or not (q >= F(0.0)):
        return 0
    if q >= F(255.0):
        return 255
    return int(q)


def base_byte(b):
    b = F(b)
    if not (b >= F(0.0)):
        return 0
    if b >= F(255.0):
        return 255
    return int(b)


def render(maps, scale, rng, lut, base=None, alpha=128):
    """maps [N, H, W] fp32, rng [N, 2], lut uint8 [256, 3], base fp32 [N, 3, H * scale, W * scale] or None -> uint8 [N, HS, WS, 3]."""
    maps = np.asarray(maps, dtype=np.float32)
    N, H, W = maps.shape
    out = np.zeros((N, H * scale, W * scale, 3), dtype=np.uint8)
    a = int(alpha)
    for n in range(N):
        idx = np.array([[color_index(maps[n, i, j], rng[n][0], rng[n][1]) for j in range(W)] for i in range(H)])
        col = np.asarray(lut)[idx].astype(np.int64)                                           # [H, W, 3]
        col = np.repeat(np.repeat(col, scale, axis=0), scale, axis=1)
        if base is None:
            out[n] = col
            continue
        b = np.asarray(base[n], dtype=np.float32)
        with np.errstate(invalid="ignore"):
            byte = np.where(~(b >= F(0.0)), 0, np.where(b >= F(255.0), 255, np.nan_to_num(b, nan=0.0, posinf=255.0, neginf=0.0).astype(np.int64)))
        byte = np.transpose(byte, (1, 2, 0)).astype(np.int64)
        out[n] = (byte * (256 - a) + col * a + 128) >> 8
    return out


def _is_padding(row):
    tot = F(0.0)
    with np.errstate(all="ignore"):
        for v in np.asarray(row, dtype=np.float32):
            tot = F(tot + v)
    return not (tot > F(0.0))


def _usable(row):
    v = np.asarray(row[3:51], dtype=np.float32)
    return bool(np.all(np.abs(v) < LIM))                        # False for NaN and infinities too


def _trunc_div(a, s):
    return int(F(F(a) / F(s)))                                  # int() truncates toward zero


def inside(verts, px, py):
    """The rasteriser's crossing rule in float64: verts [24, 2]."""
    n, odd = len(verts), False
    for k in range(n):
        x0, y0 = float(verts[k][0]), float(verts[k][1])
        x1, y1 = float(verts[(k + 1) % n][0]), float(verts[(k + 1) % n][1])
        if (y0 <= py) != (y1 <= py):
            xc = x0 + ((py - y0) * (x1 - x0)) / (y1 - y0)
            if px < xc:
                odd = not odd
    return odd


def region_cells(row, H, W, stride, mode):
    """-> list of (i, j) members of the region of one label row [51]."""
    if _is_padding(row) or not _usable(row):
        return []
    xs, ys = np.asarray(row[3:51:2], dtype=np.float32), np.asarray(row[4:51:2], dtype=np.float32)
    if mode == "rect":
        s = F(stride)
        x0, x1 = _trunc_div(xs.min(), s), _trunc_div(xs.max(), s)
        y0, y1 = _trunc_div(ys.min(), s), _trunc_div(ys.max(), s)
        x0, x1 = min(max(x0, 0), W), min(max(x1, 0), W)
        y0, y1 = min(max(y0, 0), H), min(max(y1, 0), H)
        return [(i, j) for i in range(y0, y1) for j in range(x0, x1)]
    verts = np.stack([xs, ys], 1).astype(np.float64)
    sd = float(stride)
    px, py = (np.arange(W, dtype=np.float64) + 0.5) * sd, (np.arange(H, dtype=np.float64) + 0.5) * sd
    odd = np.zeros((H, W), dtype=bool)                          # inside() for every cell centre at once: the same float64 operations
    for k in range(24):
        (x0, y0), (x1, y1) = verts[k], verts[(k + 1) % 24]
        counts = (y0 <= py) != (y1 <= py)
        if not counts.any():
            continue
        with np.errstate(all="ignore"):
            xc = x0 + ((py - y0) * (x1 - x0)) / (y1 - y0)
        odd ^= counts[:, None] & (px[None, :] < xc[:, None])
    return [(int(i), int(j)) for i, j in zip(*np.nonzero(odd))]


def response(maps, stride, labels, mode):
    """maps [B, H, W] fp32, labels [B, L, 51] fp32 -> (sum float64 [B, L], count int32 [B, L], mean float64 [B, L], sum of |v| [B, L])."""
    maps = np.asarray(maps, dtype=np.float32)
    B, H, W = maps.shape
    L = labels.shape[1]
    tot, cnt, mean, mag = np.zeros((B, L)), np.zeros((B, L), dtype=np.int32), np.zeros((B, L)), np.zeros((B, L))
    for b in range(B):
        for l in range(L):
            cells = region_cells(labels[b, l], H, W, stride, mode)
            if cells:
                v = np.array([maps[b, i, j] for i, j in cells], dtype=np.float64)
                tot[b, l], cnt[b, l], mag[b, l] = v.sum(), len(cells), np.abs(v).sum()
                mean[b, l] = tot[b, l] / len(cells)
    return tot, cnt, mean, mag
