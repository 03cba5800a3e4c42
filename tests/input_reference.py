"""References and case tables of the input pipeline kernels - csrc/preproc.hip, csrc/augment.hip, csrc/sector.hip, csrc/paste.hip -
shared by tests/test_input_reference.py (no GPU) and tests/test_gpu_input_exact.py.  Plain numpy, float64 and integers.

The arithmetic is the repository's existing restatements: ``oracle.sector.resize_linear_u8`` / ``augment_oracle._coef`` (the fixed-point
bilinear sample), ``augment_oracle`` / ``mixup_oracle`` (ownership, blend, HSV, the keep rules and the re-cast), ``fisheye_oracle``
(the label warp), ``copypaste_oracle`` (the paste walk and the pixel rule), ``resize_oracle`` (the multiscale rule).  What is new here
is the form of the ARGUMENTS: these references take what the C ABI takes - one byte buffer with offsets and row strides, descriptor
tables, row ranges, any ``max_labels`` - so that a test can hand the kernels inputs the Python wrappers never build.

Every reference takes ``mutant``: the name of one deliberate mistake (MUTANTS below).  tests/test_input_reference.py shows that each of
them changes the expected output of at least one case, i.e. that the cases would notice a kernel making that mistake.

The sizes of the cases come from the constants of the .hip files, restated here under the names they have there.
"""
import functools

import numpy as np

import augment_oracle as ao
import copypaste_oracle as co
import fisheye_oracle as fo
import resize_oracle as ro
from oracle import sector as osec

F = np.float32

# ---------------------------------------------------------------------------------------------------------------------------
# (a) the kernels' constants
PRE_WG, PRE_THREADS, PRE_QUAD = 4096, 256, 4            # preproc_u8 and augment_u8<MIX>: at most 4096 workgroups of 256 quads of 4 pixels
PRE_CAP = PRE_WG * PRE_THREADS * PRE_QUAD               # 4 194 304 pixels of one plane in the first trip
LABEL_THREADS, ROW = 256, 51                            # preproc_labels: one workgroup per image walks max_labels * 51 elements
SCALE_WG, SCALE_THREADS = 2048, 256                     # scale_labels: 524 288 elements = 10 280.2 rows in the first trip
SCALE_CAP_ROWS = SCALE_WG * SCALE_THREADS // ROW + 1    # 10 281: the first row count with a second trip
RESIZE_WG, RESIZE_TOTAL_WG = 2048, 8192                 # resize_bilinear_f32: grid.x <= 2048, grid.y = min(8192 / grid.x, planes)
CHUNK = 10                                              # augment_labels: candidates per pass
ROWS_PER_WG, COMPACT_PASS = 4, 256                      # sector_labels: one wave per row; sector_compact: row slots per pass
GATHER_WG, WARP_WG, RESIZE_U8_WG, BBOX_WG = 2048, 4096, 4096, 256     # x 256 pixels each
TW, TH, MAX_ROWS = 64, 16, 256                          # paste_u8: pixels per workgroup; rows both paste kernels keep in LDS
TILE_I, TILE_D, PAR_D, MIX_I, MIX_D, GEO_D, PASTE_I = 16, 3, 16, 16, 12, 12, 8

MUTANTS = ("last_quad", "x1_clamp", "pixel_mirror", "label_mirror", "tile_cap", "slot_chunk", "overflow_written", "tail",
           "compact_carry", "stride", "xy_swap", "edge_column")
# last_quad         preproc_u8 / augment_u8: the last, partial quad of a row of the resized area (of the output row) is skipped
# x1_clamp          resize_bilinear_f32: i1 = i0 + 1 without the clamp at the right border (it reads the next element in memory)
# pixel_mirror      augment_u8: xm = S_w - x instead of S_w - 1 - x
# label_mirror      augment_labels: ox = S_w - 1 - ox instead of S_w - ox
# tile_cap          augment_labels: a tile hands over all its rows, not at most max_labels
# slot_chunk        augment_labels: the running survivor count forgets the last candidate of a chunk
# overflow_written  augment_labels: survivors beyond max_labels are written (into the next image's rows)
# tail              preproc_labels / augment_labels / sector_compact: the rows behind the count are left as they were
# compact_carry     sector_compact: the second pass of 256 row slots starts at slot 0 again
# stride            preproc_u8 / augment_u8: rows are taken to be 3 * w bytes apart whatever the descriptor says
# xy_swap           preproc_labels / scale_labels: the x factor on the y columns and the other way round
# edge_column       paste_u8: a source column one beyond the image counts as existing (it reads the next row's first pixel)


def f64bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def f32bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


# ---------------------------------------------------------------------------------------------------------------------------
# (b) the fixed-point sample of a raw HWC source that lives in a byte buffer
def sample_bgr(buf, off, sh, sw, ld, fx, fy):
    """buf int64 [bytes]; fx, fy float64 arrays of one shape (rounded to float32 as the kernels do) -> int64 [3, ...]"""
    x0, x1, ax0, ax1 = ao._coef(np.asarray(fx, dtype=np.float64), sw)
    y0, y1, by0, by1 = ao._coef(np.asarray(fy, dtype=np.float64), sh)
    out = []
    for c in range(3):
        p00, p01 = buf[off + y0 * ld + x0 * 3 + c], buf[off + y0 * ld + x1 * 3 + c]
        p10, p11 = buf[off + y1 * ld + x0 * 3 + c], buf[off + y1 * ld + x1 * 3 + c]
        h0, h1 = p00 * ax0 + p01 * ax1, p10 * ax0 + p11 * ax1
        out.append(np.clip((((by0 * (h0 >> 4)) >> 16) + ((by1 * (h1 >> 4)) >> 16) + 2) >> 2, 0, 255))
    return np.stack(out)


def preproc_u8_ref(buf, desc, scales, S_h, S_w, mutant=None):
    """buf uint8 [bytes]; desc int64 [n,6] = (offset, h, w, ld, rh, rw); scales float64 [n,2] = (scale_x, scale_y)
    -> float32 [n,3,S_h,S_w]: the resized area top left, 114 elsewhere."""
    b = np.asarray(buf).astype(np.int64)
    out = np.full((len(desc), 3, S_h, S_w), 114, dtype=np.float32)
    for i, (off, sh, sw, ld, rh, rw) in enumerate(np.asarray(desc, dtype=np.int64).tolist()):
        rh, rw = min(rh, S_h), min(rw, S_w)
        if rh <= 0 or rw <= 0:
            continue
        if mutant == "stride":
            ld = 3 * sw
        if mutant == "last_quad":
            rw = rw // 4 * 4
            if rw == 0:
                continue
        fx = (np.arange(rw) + 0.5) * scales[i][0] - 0.5
        fy = (np.arange(rh) + 0.5) * scales[i][1] - 0.5
        out[i, :, :rh, :rw] = sample_bgr(b, off, sh, sw, ld, np.broadcast_to(fx[None, :], (rh, rw)), np.broadcast_to(fy[:, None], (rh, rw)))
    return out


def preproc_labels_ref(rows, row_off, whr, max_labels, mutant=None):
    """rows float64 [R,51] normalised; row_off int64 [n+1]; whr float64 [n,3] = (w, h, r) -> float32 [n,max_labels,51]:
    (float)((t * w) * r) on the x columns, h on the y columns, the class copied, zero behind the count."""
    n = len(row_off) - 1
    out = np.zeros((n, max_labels, ROW), dtype=np.float32)
    for i in range(n):
        lo = int(row_off[i])
        cnt = max(0, min(max_labels, int(row_off[i + 1]) - lo))
        w, h, r = (float(v) for v in whr[i])
        if mutant == "xy_swap":
            w, h = h, w
        t = np.asarray(rows, dtype=np.float64).reshape(-1, ROW)[lo:lo + cnt]
        v = t.copy()
        v[:, 1::2] = (t[:, 1::2] * w) * r
        v[:, 2::2] = (t[:, 2::2] * h) * r
        out[i, :cnt] = v.astype(np.float32)
        if mutant == "tail":
            out[i, cnt:] = np.nan
    return out


def scale_labels_ref(labels, scale_x, scale_y, mutant=None):
    if mutant == "xy_swap":
        scale_x, scale_y = scale_y, scale_x
    return ro.scale_labels(labels, scale_x, scale_y)


def resize_bilinear_ref(x, oh, ow, mutant=None):
    """``resize_oracle.resize``; the mutant reads x1 = x0 + 1 beyond a row's end, i.e. the next element of the flat source."""
    if mutant != "x1_clamp":
        return ro.resize(x, oh, ow)
    x = np.asarray(x)
    P, H, W = x.shape
    y0, y1, wy0, wy1 = ro.axis(H, oh)
    x0, _, wx0, wx1 = ro.axis(W, ow)
    flat = np.concatenate([x.reshape(-1), np.zeros(1, dtype=np.float32)])
    base = (np.arange(P) * H * W)[:, None, None]
    a, b = flat[base + (y0 * W)[None, :, None] + x0[None, None, :]], flat[base + (y0 * W)[None, :, None] + x0[None, None, :] + 1]
    c, d = flat[base + (y1 * W)[None, :, None] + x0[None, None, :]], flat[base + (y1 * W)[None, :, None] + x0[None, None, :] + 1]
    top, bot = a * wx0 + b * wx1, c * wx0 + d * wx1
    return top * wy0[:, None] + bot * wy1[:, None]


def resize_grid(n, dh, dw):
    """-> (grid.x, grid.y) of ep24_resize_bilinear_f32"""
    bx = min(-(-(dh * dw) // 256), RESIZE_WG)
    return bx, max(1, min(RESIZE_TOTAL_WG // bx, n))


# ---------------------------------------------------------------------------------------------------------------------------
# (c) the image half of the augmentation, from the descriptor tables
def augment_u8_ref(buf, tiles, tscale, params, flags, mixi, mixd, S_h, S_w, hsv_dtype=None, mutant=None):
    """tiles int64 [n,4,16], tscale float64 [n,4,3], params float64 [n,16], flags int32 [n,2]; mixi int64 [n,16] / mixd float64 [n,12]
    or None.  -> (float [n,3,S_h,S_w], owned bool [n,S_h,S_w]).  ``hsv_dtype`` None: HSV is not applied (the exact part); else the
    HSV of ``augment_oracle.hsv_shift`` in that type on the owned pixels of images whose switch is on."""
    b = np.asarray(buf).astype(np.int64)
    n = len(tiles)
    out = np.zeros((n, 3, S_h, S_w), dtype=np.float64)
    owned_all = np.zeros((n, S_h, S_w), dtype=bool)
    ys, xs = np.mgrid[0:S_h, 0:S_w]
    for i in range(n):
        P = params[i]
        mirror = flags[i][0] != 0
        xm = ((S_w - xs) if mutant == "pixel_mirror" else (S_w - 1 - xs)) if mirror else xs
        u = (P[6] * xm.astype(np.float64) + P[7] * ys.astype(np.float64)) + P[8]
        v = (P[9] * xm.astype(np.float64) + P[10] * ys.astype(np.float64)) + P[11]
        own = np.full((S_h, S_w), -1, dtype=np.int64)
        for t in (3, 2, 1, 0):
            d = tiles[i][t]
            own[(u >= d[6] - 0.5) & (u < d[8] - 0.5) & (v >= d[7] - 0.5) & (v < d[9] - 0.5)] = t
        a = np.full((3, S_h, S_w), 114, dtype=np.int64)
        for t in range(4):
            m = own == t
            if not m.any():
                continue
            d = [int(k) for k in tiles[i][t]]
            fx = ((u[m] - d[10]) + 0.5) * tscale[i][t][0] - 0.5
            fy = ((v[m] - d[11]) + 0.5) * tscale[i][t][1] - 0.5
            a[:, m] = sample_bgr(b, d[0], d[1], d[2], 3 * d[2] if mutant == "stride" else d[3], fx, fy)
        owned = own >= 0
        if mixi is not None and mixi[i][0] != 0:
            X, XD = [int(k) for k in mixi[i]], mixd[i]
            px, py = xm + X[9], ys + X[10]
            inside = (px >= 0) & (px < X[7]) & (py >= 0) & (py < X[8])
            pxf = (X[7] - 1 - px) if X[11] else px
            pu = (pxf + 0.5) * XD[0] - 0.5
            pv = (py + 0.5) * XD[1] - 0.5
            m = inside & (pu >= -0.5) & (pu < X[5] - 0.5) & (pv >= -0.5) & (pv < X[6] - 0.5)
            bb = np.zeros((3, S_h, S_w), dtype=np.int64)
            bb[:, inside] = 114
            if m.any():
                bb[:, m] = sample_bgr(b, X[1], X[2], X[3], 3 * X[3] if mutant == "stride" else X[4], (pu[m] + 0.5) * XD[2] - 0.5,
                                      (pv[m] + 0.5) * XD[3] - 0.5)
            a = (a + bb) >> 1
            owned = owned | m
        res = a.astype(np.float64)
        if hsv_dtype is not None and flags[i][1] != 0 and owned.any():
            base = a.astype(np.float32)
            bgr = ao.hsv_shift(base[0][owned], base[1][owned], base[2][owned], F(P[12]), F(P[13]), F(P[14]), dtype=hsv_dtype)
            for c in range(3):
                res[c][owned] = bgr[c]
        if mutant == "last_quad":
            res[:, :, S_w - 4:] = np.nan
        out[i], owned_all[i] = res, owned
    return out, owned_all


# ---------------------------------------------------------------------------------------------------------------------------
# (d) the label half of the augmentation, from the descriptor tables
def augment_labels_ref(rows, tiles, tscale, params, flags, mixi, mixd, S_h, S_w, margin, max_labels, mutant=None):
    """-> (table float64 [n,max_labels,51], unrounded; counts int [n]; info).  ``info``: ``kept`` per image the candidate indices that
    survive, ``cands`` per image the number of candidates, ``centre_margin`` / ``extent_margin`` the smallest distance of a decision
    from its threshold, ``hits`` the edges each re-cast ray met.  Candidates: the rows of tile 0, 1, 2, 3 (at most max_labels each),
    then the partner's; survivors are appended in that order; those beyond max_labels are dropped and still counted."""
    rows = np.asarray(rows, dtype=np.float64).reshape(-1, ROW)
    n = len(tiles)
    W, H = float(S_w), float(S_h)
    flat = np.zeros(n * max_labels * ROW + ROW * 64, dtype=np.float64)
    late = []
    counts = np.zeros(n, dtype=np.int64)
    info = dict(kept=[], cands=[], centre_margin=np.inf, extent_margin=np.inf, hits=[])
    for i in range(n):
        P = params[i]
        mirror = flags[i][0] != 0
        cands = []                                                   # (source t, row index)
        for t in range(4):
            d = tiles[i][t]
            c = max(0, int(d[13] - d[12]))
            if mutant != "tile_cap":
                c = min(c, max_labels)
            cands += [(t, int(d[12]) + k) for k in range(c)]
        if mixi is not None and mixi[i][0] != 0:
            X = mixi[i]
            cands += [(4, int(X[12]) + k) for k in range(max(0, min(int(X[13] - X[12]), max_labels)))]
        keep, out_rows = [], []
        for t, ri in cands:
            row = rows[ri]
            if t == 4:
                X, XD = [int(k) for k in mixi[i]], mixd[i]
                cx, cy = (row[1::2] * X[3]) * XD[4], (row[2::2] * X[2]) * XD[4]
                ox, oy = XD[5] * cx + XD[7], XD[6] * cy + XD[8]
                reg = (0.0, 0.0, float(X[5]), float(X[6]))
                back = lambda dxy: np.array([XD[9] * dxy[0], XD[10] * dxy[1]])
            else:
                d = [int(k) for k in tiles[i][t]]
                s = tscale[i][t][2]
                cx, cy = (row[1::2] * d[2]) * s + d[10], (row[2::2] * d[1]) * s + d[11]
                ox, oy = (P[0] * cx + P[1] * cy) + P[2], (P[3] * cx + P[4] * cy) + P[5]
                reg = (float(d[6]), float(d[7]), float(d[8]), float(d[9]))
                back = lambda dxy: np.array([P[6] * dxy[0] + P[7] * dxy[1], P[9] * dxy[0] + P[10] * dxy[1]])
            if mirror:
                ox = (W - 1 - ox) if mutant == "label_mirror" else (W - ox)
            slack = [ox[0] - margin, (W - margin) - ox[0], oy[0] - margin, (H - margin) - oy[0], cx[0] - (reg[0] + margin),
                     (reg[2] - margin) - cx[0], cy[0] - (reg[1] + margin), (reg[3] - margin) - cy[0]]
            info["centre_margin"] = min(info["centre_margin"], abs(min(slack)))
            if min(slack) < 0:
                keep.append(False)
                continue
            c = np.array([ox[0], oy[0]])
            r, hits = ao.recast(c, np.stack([ox[1:], oy[1:]], 1))
            new = np.zeros((24, 2))
            for k in range(24):
                dk = ao.RAY[k]
                rk = min(r[k], ao._box_exit(c, dk, 0.0, 0.0, W, H))
                rk = min(rk, ao._box_exit((cx[0], cy[0]), back((-dk[0] if mirror else dk[0], dk[1])), *reg))
                new[k] = c + rk * dk
            ext = min(new[:, 0].max() - new[:, 0].min(), new[:, 1].max() - new[:, 1].min())
            info["extent_margin"] = min(info["extent_margin"], abs(ext - 1.0))
            if not ext > 1.0:
                keep.append(False)
                continue
            o = np.zeros(ROW)
            o[0], o[1], o[2] = row[0], c[0], c[1]
            o[3::2], o[4::2] = new[:, 0], new[:, 1]
            keep.append(True)
            out_rows.append(o)
            info["hits"].append(hits)
        # the append, chunk by chunk as the kernel numbers the slots
        kept0, it = 0, iter(out_rows)
        for base in range(0, len(cands), CHUNK):
            ks = keep[base:base + CHUNK]
            for c, k in enumerate(ks):
                if not k:
                    continue
                slot, o = kept0 + sum(ks[:c]), next(it)
                at = (i * max_labels + slot) * ROW
                if slot < max_labels:
                    flat[at:at + ROW] = o
                elif mutant == "overflow_written":
                    late.append((at, o))
            kept0 += sum(ks[:-1]) if mutant == "slot_chunk" and len(ks) == CHUNK else sum(ks)
        tail = slice((i * max_labels + min(kept0, max_labels)) * ROW, (i + 1) * max_labels * ROW)
        flat[tail] = np.nan if mutant == "tail" else 0.0
        counts[i] = kept0
        info["kept"].append([j for j, k in enumerate(keep) if k])
        info["cands"].append(len(cands))
    for at, o in late:
        flat[at:at + ROW] = o
    return flat[:n * max_labels * ROW].reshape(n, max_labels, ROW), counts, info


# ---------------------------------------------------------------------------------------------------------------------------
# (e) the sector kernels
def sector_gather_ref(src, winner, canvas_w, y0, x0, oh, ow, T, n_ang, fill):
    """winner int32 [rows * canvas_w]; src uint8 [T * n_ang * 3] or None -> (dst uint8 [oh,ow,3] or None, src_index int32 [oh,ow])"""
    key = np.asarray(winner).reshape(-1, canvas_w)[y0:y0 + oh, x0:x0 + ow].astype(np.int64)
    a, r = key // T, key % T
    flat = np.where(key >= 0, (T - 1 - r) * n_ang + (n_ang - 1 - a), -1)
    if src is None:
        return None, flat.astype(np.int32)
    dst = np.full((oh, ow, 3), fill, dtype=np.uint8)
    dst[key >= 0] = np.asarray(src).reshape(-1, 3)[flat[key >= 0]]
    return dst, flat.astype(np.int32)


def sector_warp_ref(img, winner, canvas_w, y0, x0, oh, ow, T, n_ang, fill):
    """the fused form: the [T, n_ang] resize of ``img`` is never stored; the result is the gather from it"""
    return sector_gather_ref(osec.resize_linear_u8(img, n_ang, T).reshape(-1), winner, canvas_w, y0, x0, oh, ow, T, n_ang, fill)[0]


def mask_bbox_ref(mask3, init):
    """-> [xmin, ymin, xmax, ymax]; an empty mask leaves ``init``"""
    ys, xs = np.nonzero(np.asarray(mask3)[..., 0])
    if len(xs) == 0:
        return list(init)
    return [min(init[0], int(xs.min())), min(init[1], int(ys.min())), max(init[2], int(xs.max())), max(init[3], int(ys.max()))]


def geo_dict(G):
    return dict(theta=float(G[0]), T=int(G[1]), h=int(G[2]), w=int(G[3]), cw=int(G[4]), x0=int(G[5]), y0=int(G[6]), oh=int(G[7]), ow=int(G[8]))


_WARP_CACHE = {}


def warp_row_cached(row, G):
    key = (np.asarray(row, dtype=np.float64).tobytes(), tuple(float(v) for v in G[:10]))
    if key not in _WARP_CACHE:
        out, flag, margins, _ = fo.warp_row(row, geo_dict(G), float(G[9]))
        _WARP_CACHE[key] = (out, flag, margins)
    return _WARP_CACHE[key]


def sector_labels_ref(rows, geo, max_labels, mutant=None):
    """rows float64 [R,51]; geo float64 [n,12] -> (cand float64 [n,max_labels,51] with NaN where the kernel writes nothing, keep int32
    [n,max_labels], out float64 [n,max_labels,51], counts int32 [n], flags int32 [n,max_labels], margins)"""
    rows = np.asarray(rows, dtype=np.float64).reshape(-1, ROW)
    n = len(geo)
    cand = np.full((n, max_labels, ROW), np.nan)
    keep = np.zeros((n, max_labels), dtype=np.int32)
    margins = dict(inside=np.inf, side=np.inf, clamp=np.inf, extent=np.inf)
    for i, G in enumerate(geo):
        cnt = max(0, min(int(G[11]), max_labels))
        for j in range(cnt):
            out, flag, m = warp_row_cached(rows[int(G[10]) + j], G)
            for k in margins:
                margins[k] = min(margins[k], m[k])
            keep[i, j] = (1 if out is not None else 0) | (flag << 1)
            if out is not None:
                cand[i, j] = out
    out, counts, flags = sector_compact_ref(cand, keep, mutant)
    return cand, keep, out, counts, flags, margins


def sector_compact_ref(cand, keep, mutant=None):
    n, max_labels = keep.shape
    out = np.full((n, max_labels, ROW), np.nan)
    flags = np.full((n, max_labels), -1, dtype=np.int32)
    counts = np.zeros(n, dtype=np.int32)
    for i in range(n):
        kept0 = 0
        for base in range(0, max_labels, COMPACT_PASS):
            if mutant == "compact_carry":
                kept0 = 0
            for j in range(base, min(base + COMPACT_PASS, max_labels)):
                if keep[i, j] & 1:
                    out[i, kept0], flags[i, kept0] = cand[i, j], keep[i, j] >> 1
                    kept0 += 1
        if mutant != "tail":
            out[i, kept0:], flags[i, kept0:] = 0.0, 0
        counts[i] = kept0
    return out, counts, flags


# ---------------------------------------------------------------------------------------------------------------------------
# (f) the pixel half of copy-paste with the one mutant the CPU file wants; the label half is copypaste_oracle.paste_labels as it is
def paste_u8_ref(pre_images, out_labels, paste_range, paste, mutant=None):
    if mutant != "edge_column":
        return co.paste_u8(pre_images, out_labels, paste_range, paste)
    pre = np.asarray(pre_images, dtype=np.float32)
    n, _, S_h, S_w = pre.shape
    out = pre.copy()
    pasted = np.zeros((n, S_h, S_w), dtype=bool)
    for i in range(n):
        on, j, flip, dx, dy = (int(v) for v in paste[i][:5])
        if not on or not 0 <= j < n:
            continue
        mask = np.zeros((S_h, S_w), dtype=bool)
        for r in range(int(paste_range[i][0]), int(paste_range[i][1])):
            mask |= co.centres_inside(out_labels[i][r][3:], S_h, S_w)
        xu = np.arange(S_w, dtype=np.int64) - dx
        xs = (S_w - 1 - xu) if flip else xu
        ys = np.arange(S_h, dtype=np.int64) - dy
        take = mask & ((ys >= 0) & (ys < S_h))[:, None] & ((xs >= 0) & (xs <= S_w))[None, :]
        yy, xx = np.nonzero(take)
        src = np.concatenate([pre[j].reshape(3, -1), np.zeros((3, 1), dtype=np.float32)], 1)
        out[i][:, yy, xx] = src[:, ys[yy] * S_w + xs[xx]]
        pasted[i] = take
    return out, pasted


def paste_vec(S_w, pre_ptr, out_ptr):
    """the launcher's choice of the VEC = true instantiation"""
    return S_w % 4 == 0 and pre_ptr % 16 == 0 and out_ptr % 16 == 0


# ===========================================================================================================================
# CASES
# ===========================================================================================================================
def letterbox(h, w, S_h, S_w):
    r = min(S_h / h, S_w / w)
    return r, int(h * r), int(w * r)


def pack_images(specs, seed):
    """specs: (h, w, pad, gap) per image: rows of 3 * w + pad bytes, ``gap`` bytes before the image.  Everything, gaps and row pads
    included, is random.  -> (buf uint8, [(offset, ld)], [image uint8 [h,w,3]])"""
    rng = np.random.RandomState(seed)
    total = sum(gap + h * (3 * w + pad) for h, w, pad, gap in specs)
    buf = rng.randint(0, 256, total).astype(np.uint8)
    place, images, off = [], [], 0
    for h, w, pad, gap in specs:
        off += gap
        ld = 3 * w + pad
        images.append(np.lib.stride_tricks.as_strided(buf[off:], (h, w, 3), (ld, 3, 1)).copy())
        place.append((off, ld))
        off += h * ld
    return buf, place, images


# ---- preproc_u8: name -> (S_h, S_w, [(h, w, pad, gap, rh, rw)]); rh / rw None: the letterbox's own
PREPROC_CASES = {
    "1x1": (8, 8, [(1, 1, 0, 0, None, None)]),                                       # resized area = the whole input: no padding
    "1xN": (8, 12, [(1, 9, 0, 0, None, None)]),                                      # rh = 1: padding below only
    "Nx1": (12, 8, [(9, 1, 0, 0, None, None)]),                                      # rw = 1: padding on the right only, one pixel of a quad
    "odd": (40, 64, [(37, 53, 0, 0, None, None), (53, 37, 0, 3, None, None), (23, 31, 0, 1, 25, 33)]),   # rw = 57, 27, 33: quads cut at 1, 3, 1
    "equal": (16, 24, [(16, 24, 0, 0, None, None)]),                                 # scale 1: the input itself
    "stride": (32, 40, [(13, 17, 5, 7, None, None), (11, 19, 1, 2, 20, 30), (17, 13, 64, 11, None, None)]),   # padded ld, unequal offsets
    "flat": (32, 32, [(1, 4000, 0, 0, None, None), (5, 7, 0, 0, None, None)]),       # rh = 0: the whole plane stays 114
    "narrow": (5, 4, [(3, 2, 0, 0, None, None), (2, 3, 3, 1, 3, 3)]),                # S_w = 4, the minimum: one quad per row
    "cap": (2048, 2052, [(5, 7, 2, 0, None, None)]),                                 # 1 050 624 quads > 4096 x 256
}


@functools.lru_cache(maxsize=None)
def preproc_case(name):
    S_h, S_w, specs = PREPROC_CASES[name]
    buf, place, images = pack_images([s[:4] for s in specs], 1000 + sorted(PREPROC_CASES).index(name))
    desc, scales = [], []
    for (h, w, pad, gap, rh, rw), (off, ld) in zip(specs, place):
        if rh is None:
            _, rh, rw = letterbox(h, w, S_h, S_w)
        desc.append([off, h, w, ld, rh, rw])
        scales.append([1.0 / (rw / w) if rw else 1.0, 1.0 / (rh / h) if rh else 1.0])
    buf.setflags(write=False)
    return dict(S_h=S_h, S_w=S_w, buf=buf, desc=np.array(desc, dtype=np.int64), scales=np.array(scales, dtype=np.float64), images=images)


# ---- preproc_labels
LABEL_MAX = (1, 5, 6, 50)                                # 51, 255, 306 and 2550 elements on 256 threads


@functools.lru_cache(maxsize=None)
def labels_case(max_labels):
    """four images: max_labels rows, none, max_labels + 3 (truncated), min(2, max_labels)"""
    counts = [max_labels, 0, max_labels + 3, min(2, max_labels)]
    rng = np.random.RandomState(50 + max_labels)
    R = sum(counts)
    rows = np.concatenate([rng.randint(0, 80, (R, 1)).astype(np.float64), rng.rand(R, 50)], 1)
    whr = np.array([[640.0, 480.0, 640 / 640], [333.0, 517.0, min(416 / 517, 320 / 333)], [97.0, 131.0, 160 / 131], [1.0, 4000.0, 0.008]])
    rows.setflags(write=False)
    return dict(rows=rows, row_off=np.concatenate([[0], np.cumsum(counts)]).astype(np.int64), whr=whr, counts=counts)


SCALE_ROWS = (1, SCALE_CAP_ROWS)
SCALES = (1.3, 0.7)                                      # neither is a power of two: every product rounds

# ---- resize_bilinear_f32: the one shape beyond resize_oracle.SHAPES (planes, source, output)
RESIZE_CAP = (5, (5, 7), (725, 724))                     # 524 900 items > 2048 x 256, grid.y = 4 < 5 planes


# ---- augment_u8: hand-built descriptors
def _tile(off, h, w, ld, rw, rh, lx1, ly1, lx2, ly2, padw, padh, r0=0, r1=0):
    d = np.zeros(TILE_I, dtype=np.int64)
    d[:14] = (off, h, w, ld, rw, rh, lx1, ly1, lx2, ly2, padw, padh, r0, r1)
    return d, (1.0 / (rw / w), 1.0 / (rh / h), 1.0)


def _quadrants(place, sizes, resized, xc, yc, cw, ch):
    """the mosaic placement of ``ep24.augment.tile_layout`` on a cw x ch canvas, with the resized sizes given"""
    tiles, ts = [], []
    for q, ((off, ld), (h, w), (rw, rh)) in enumerate(zip(place, sizes, resized)):
        lx1, lx2, padw = (xc, min(xc + rw, cw), xc) if q & 1 else (max(xc - rw, 0), xc, xc - rw)
        ly1, ly2, padh = (yc, min(yc + rh, ch), yc) if q & 2 else (max(yc - rh, 0), yc, yc - rh)
        d, s = _tile(off, h, w, ld, rw, rh, lx1, ly1, lx2, ly2, padw, padh)
        tiles.append(d)
        ts.append(s)
    return np.stack(tiles), np.array(ts)


def _params(M, hsv=(0.0, 0.0, 0.0)):
    from ep24.augment import affine_inverse
    P = np.zeros(PAR_D)
    P[0:6] = np.asarray(M, dtype=np.float64).reshape(6)
    P[6:12] = affine_inverse(M).reshape(6)
    P[12:15] = hsv
    return P


def _mix(place, h, w, S_h, S_w, jit, x_off, y_off, flip, r0=0, r1=0):
    s, rh, rw = letterbox(h, w, S_h, S_w)
    Wj, Hj = int(S_w * jit), int(S_h * jit)
    X = np.zeros(MIX_I, dtype=np.int64)
    X[:14] = (1, place[0], h, w, place[1], rw, rh, Wj, Hj, x_off, y_off, int(flip), r0, r1)
    a00, a11 = (-(Wj / S_w) if flip else Wj / S_w), Hj / S_h
    XD = np.zeros(MIX_D)
    XD[:11] = (S_w / Wj, S_h / Hj, 1.0 / (rw / w), 1.0 / (rh / h), s, a00, a11, float(Wj - x_off if flip else -x_off), float(-y_off),
               1.0 / a00, 1.0 / a11)
    return X, XD


AUG_S = (24, 32)


@functools.lru_cache(maxsize=None)
def augment_case(name):
    """"meet": four tiles around the canvas point (16, 12); the inverse map is u = x + 7.5, v = y + 5.5, so the output pixel (8, 6) sits
    EXACTLY on u = 16 - 0.5 and v = 12 - 0.5, where the right / lower tile begins (>=).  Tile 0 is wider than what is left of the canvas
    on its side (padw = 16 - 21 < 0).  Every source has a padded row stride and lies at an odd offset.  Image 0 plain, image 1 mirrored.
    "mix": the same tiles; image 0 has a flipped partner whose jittered canvas (24 x 18) lies inside the window, so that the zero
    region, the 114 region and the partner's image are all there; image 1 has no partner; image 2 has one without flip at an offset.
    "cap" / "cap_mix": 2048 x 2052 from small sources through a rotation, one image."""
    specs = [(10, 14, 3, 5), (12, 9, 1, 2), (7, 11, 6, 1), (13, 13, 2, 9), (9, 15, 4, 3)]
    buf, place, images = pack_images(specs, 77)
    sizes = [s[:2] for s in specs]
    if name in ("meet", "mix"):
        S_h, S_w = AUG_S
        tl, ts = _quadrants(place[:4], sizes[:4], [(21, 15), (13, 10), (11, 7), (14, 14)], 16, 12, 2 * S_w, 2 * S_h)
        n = 2 if name == "meet" else 3
        tiles, tscale = np.stack([tl] * n), np.stack([ts] * n)
        params = np.stack([_params([[1.0, 0.0, -7.5], [0.0, 1.0, -5.5]])] * n)
        flags = np.zeros((n, 2), dtype=np.int32)
        flags[1, 0] = 1
        mixi = mixd = None
        if name == "mix":
            mixi, mixd = np.zeros((n, MIX_I), dtype=np.int64), np.zeros((n, MIX_D))
            mixi[0], mixd[0] = _mix(place[4], 9, 15, S_h, S_w, 0.75, 0, 0, True)
            mixi[2], mixd[2] = _mix(place[4], 9, 15, S_h, S_w, 1.25, 5, 3, False)
            flags[2, 0] = 1
    else:
        S_h, S_w = 2048, 2052
        rw, rh = 1400, 1000
        d, s = _tile(place[0][0], 10, 14, place[0][1], rw, rh, 300, 200, 300 + rw, 200 + rh, 300, 200)
        tiles, tscale = np.zeros((1, 4, TILE_I), dtype=np.int64), np.ones((1, 4, TILE_D))
        tiles[0, 0], tscale[0, 0] = d, s
        c, sn = np.cos(np.deg2rad(9.0)), np.sin(np.deg2rad(9.0))
        params = np.stack([_params([[1.1 * c, 1.1 * sn, 40.25], [-1.1 * sn, 1.1 * c, 300.5]])])
        flags = np.array([[1, 0]], dtype=np.int32)
        mixi = mixd = None
        if name == "cap_mix":
            X, XD = _mix(place[4], 9, 15, S_h, S_w, 0.8, 0, 0, True)
            mixi, mixd = X[None], XD[None]
    buf.setflags(write=False)
    return dict(S_h=S_h, S_w=S_w, buf=buf, tiles=tiles, tscale=tscale, params=params, flags=flags, mixi=mixi, mixd=mixd)


@functools.lru_cache(maxsize=None)
def hsv_case():
    """One 8 x 8 source shown 1 : 1 (scale 1, so the crafted pixels arrive unchanged) in three images with different gains: greys, black
    (v == 0), the six hue sectors at full and at weak saturation, and values that the gains push beyond both clamps of S and V."""
    px = [(0, 0, 0), (128, 128, 128), (255, 255, 255), (1, 1, 1), (7, 7, 7), (200, 200, 200),
          (0, 0, 255), (0, 255, 255), (0, 255, 0), (255, 255, 0), (255, 0, 0), (255, 0, 255),          # BGR: the six sector starts
          (10, 60, 250), (10, 250, 200), (60, 250, 10), (250, 200, 10), (250, 10, 60), (200, 10, 250),  # one inside each sector
          (120, 125, 130), (130, 120, 125), (125, 130, 120), (3, 2, 1), (254, 255, 253), (0, 0, 1),     # weak saturation, near-black, near-white
          (20, 20, 21), (240, 10, 10), (10, 240, 10), (10, 10, 240), (255, 254, 0), (0, 1, 255), (90, 180, 45), (45, 90, 180)]
    rng = np.random.RandomState(5)
    img = rng.randint(0, 256, (8, 8, 3)).astype(np.uint8)
    img.reshape(-1, 3)[:len(px)] = np.array(px, dtype=np.uint8)
    buf = img.reshape(-1).copy()
    gains = [(7.5, 40.0, 40.0), (-7.5, -40.0, -40.0), (179.0, 300.0, -300.0)]
    n = len(gains)
    d, s = _tile(0, 8, 8, 24, 8, 8, 0, 0, 8, 8, 0, 0)
    tiles, tscale = np.zeros((n, 4, TILE_I), dtype=np.int64), np.ones((n, 4, TILE_D))
    tiles[:, 0], tscale[:, 0] = d, s
    params = np.stack([_params([[1.0, 0.0, 0.0], [0.0, 1.0, 0.0]], g) for g in gains])
    flags = np.ones((n, 2), dtype=np.int32)
    flags[:, 0] = (0, 1, 0)
    buf.setflags(write=False)
    return dict(S_h=8, S_w=12, buf=buf, tiles=tiles, tscale=tscale, params=params, flags=flags, mixi=None, mixd=None, image=img)


# ---- augment_labels: per max_labels a batch of images, each a list of four tile patterns and a partner pattern.
# K: an object that survives; d: one that the extent filter drops (0.2 px wide); D: one whose centre lies outside its tile's region.
LAB_S = (120, 160)
LAB_SOURCES = [(90, 120), (100, 100), (120, 160), (75, 130), (110, 140)]       # the four tiles' sources and the partner's
LAB_CENTRE = (150, 110)
LAB_MARGIN = 2.0
LAB_BATCH = {
    50: [("", "", "", "", None),                                                # 0 candidates
         ("KdKKDKKdK", "", "", "", None),                                       # 9: one short of a chunk
         ("KKdKDKKKdK", "", "", "", None),                                      # 10: a chunk exactly, its last candidate survives
         ("KKdKDKKKdKK", "", "", "", None),                                     # 11: one into the second chunk
         ("KKKKKKKKKK" "KKKKKKKKKK", "", "", "", None),                         # 20
         ("KKKKKKKKKK" "KKKKKKKKKK" "K", "", "", "", None),                     # 21: every chunk boundary carries a survivor
         ("KdK", "", "DKKK", "", "KKdKDKKK"),                                   # the partner's rows start at candidate 7, mid-chunk
         ("K" * 53, "KKKKK", "", "", None)],                                    # 53 rows in a tile of 50; 55 survivors for 50 rows
    6: [("", "", "", "", None),
        ("KdKKDK", "KdK", "", "", None),                                        # 6 + 3 = 9
        ("KKdKDK", "KKdK", "", "", None),                                       # 10
        ("KKdKDK", "KKdKK", "", "", None),                                      # 11
        ("KdKDdD", "DdKdDD", "dDdDKd", "KD", None),                             # 20, four survivors
        ("KdKDdD", "DdKdDD", "dDdDKd", "KDK", None),                            # 21, the fifth survivor is candidate 20
        ("KKKKKD", "DDKKKK", "", "", None),                                     # survivor 6 at candidate 8, 7 at 9, 8 and 9 at 10, 11: the overflow straddles a chunk
        ("KKKKKKKKK", "KK", "", "", None),                                      # 9 rows in a tile of 6: candidates 6 + 2
        ("Kd", "", "K", "", "dKKDKKK")],                                        # partner from candidate 3; survivors 2 + 5 > 6
    1: [("", "", "", "", None), ("K", "", "", "", None), ("KKK", "", "", "", None), ("D", "K", "", "", None), ("K", "", "K", "", None),
        ("d", "", "", "", "K"), ("K", "", "", "", "KK")],
}


def _lab_geometry():
    S_h, S_w = LAB_S
    resized = []
    for h, w in LAB_SOURCES:
        s, rh, rw = letterbox(h, w, S_h, S_w)
        resized.append((rw, rh, s))
    xc, yc = LAB_CENTRE
    place = [(0, 3 * w) for _, w in LAB_SOURCES]                               # the label kernel reads no pixels
    tl, ts = _quadrants(place[:4], LAB_SOURCES[:4], [r[:2] for r in resized[:4]], xc, yc, 2 * S_w, 2 * S_h)
    for q in range(4):
        ts[q][2] = resized[q][2]
    c, sn = 0.6 * np.cos(np.deg2rad(5.0)), 0.6 * np.sin(np.deg2rad(5.0))
    A = np.array([[c, sn], [-sn, c]])
    t = np.array([S_w / 2.0, S_h / 2.0]) - A @ np.array([xc, yc], dtype=np.float64)
    M = np.concatenate([A, t[:, None]], 1)
    return tl, ts, M


def _polygon_row(rng, cls, X, Y, radius, padw, padh, s, h, w):
    """a 24-gon around the canvas point (X, Y) as a normalised row of the source (h, w) that a tile shows at scale s, offset pad"""
    phi = np.arange(24) * 15 * np.pi / 180 + 0.1
    rad = radius * (1 + 0.2 * np.sin(3 * phi + rng.uniform(0, 6.28)))
    row = np.zeros(ROW)
    row[0] = cls
    row[1], row[2] = (X - padw) / (s * w), (Y - padh) / (s * h)
    row[3::2] = (X + rad * np.cos(phi) - padw) / (s * w)
    row[4::2] = (Y + rad * np.sin(phi) - padh) / (s * h)
    return row


@functools.lru_cache(maxsize=None)
def label_case(max_labels):
    """-> dict(rows, tiles, tscale, params, flags, mixi, mixd, S_h, S_w, patterns).  Image i is mirrored iff i is odd.  The objects'
    positions are drawn inside the part of a tile's region that the affine map shows 14 px inside the output, radius 6 .. 9 px there."""
    S_h, S_w = LAB_S
    tl, ts, M = _lab_geometry()
    A, t = M[:, :2], M[:, 2]
    batch = LAB_BATCH[max_labels]
    n = len(batch)
    rng = np.random.RandomState(300 + max_labels)
    rows = [np.full(ROW, 0.5)]                                                  # row 0 belongs to nobody
    tiles, tscale = np.stack([tl] * n).copy(), np.stack([ts] * n).copy()
    mixi, mixd = np.zeros((n, MIX_I), dtype=np.int64), np.zeros((n, MIX_D))
    flags = np.zeros((n, 2), dtype=np.int32)
    flags[1::2, 0] = 1
    ph, pw = LAB_SOURCES[4]
    for i, spec in enumerate(batch):
        if spec[4] is not None:
            mixi[i], mixd[i] = _mix((0, 3 * pw), ph, pw, S_h, S_w, 1.25, 20, 10, i % 3 == 0)
        for src, pattern in enumerate(spec):
            if pattern is None:
                continue
            first = len(rows)
            for k, kind in enumerate(pattern):
                if src < 4:
                    d, (h, w) = tiles[i, src], LAB_SOURCES[src]
                    reg, pad, s = (d[6], d[7], d[8], d[9]), (d[10], d[11]), ts[src][2]
                    fwd = lambda X, Y: A @ np.array([X, Y]) + t
                    zoom = 0.6
                else:
                    X_, XD = mixi[i], mixd[i]
                    h, w, reg, pad, s = ph, pw, (0, 0, X_[5], X_[6]), (0, 0), XD[4]
                    fwd = lambda X, Y: np.array([XD[5] * X + XD[7], XD[6] * Y + XD[8]])
                    zoom = 1.25
                if kind == "D":
                    X, Y = reg[0] - 6.0 - k, reg[1] - 6.0                      # outside the region on both axes
                else:
                    for _ in range(10000):
                        X, Y = rng.uniform(reg[0] + 24, reg[2] - 24), rng.uniform(reg[1] + 24, reg[3] - 24)
                        o = fwd(X, Y)
                        if 14 <= o[0] <= S_w - 14 and 14 <= o[1] <= S_h - 14:
                            break
                    else:
                        raise AssertionError("no room for an object of image %d source %d" % (i, src))
                radius = (0.2 if kind == "d" else rng.uniform(6.0, 9.0)) / zoom
                rows.append(_polygon_row(rng, (7 * len(rows)) % 80, X, Y, radius, pad[0], pad[1], s, h, w))
            if src < 4:
                tiles[i, src, 12], tiles[i, src, 13] = first, len(rows)
            else:
                mixi[i, 12], mixi[i, 13] = first, len(rows)
    rows = np.stack(rows)
    rows.setflags(write=False)
    params = np.stack([_params(M)] * n)
    return dict(rows=rows, tiles=tiles, tscale=tscale, params=params, flags=flags, mixi=mixi, mixd=mixd, S_h=S_h, S_w=S_w, patterns=batch)


def label_expectation(max_labels):
    """from the patterns alone -> (candidates, survivor candidate indices) per image"""
    out = []
    for spec in LAB_BATCH[max_labels]:
        seq = "".join(p[:max_labels] for p in spec[:4]) + (spec[4] or "")[:max_labels]
        out.append((len(seq), [j for j, k in enumerate(seq) if k == "K"]))
    return out


# ---- sector_labels
SECTOR_MAX = (1, 2, 3, 5, 50, 256, 257, 300)
SECTOR_S = (256, 320)
SECTOR_GEOMS = ((60, 240, 320), (120, 300, 200))
SECTOR_POOL = 306


def arc_band(h, w, cx, cy, r_out, r_in):
    """a half ring open towards -y: the middle of its box lies in the hollow, the row's own centre on the band (``fell_back``)"""
    a = np.linspace(0.0, np.pi, 12)
    row = np.zeros(ROW)
    row[0], row[1], row[2] = 7, (cx + 3.0) / w, (cy + (r_out + r_in) / 2) / h
    row[3::2] = np.concatenate([cx + r_out * np.cos(a), cx + r_in * np.cos(a[::-1])]) / w
    row[4::2] = np.concatenate([cy + r_out * np.sin(a), cy + r_in * np.sin(a[::-1])]) / h
    return row


@functools.lru_cache(maxsize=None)
def sector_pool():
    """Per geometry 306 rows: blobs that survive, every third one 0.04 .. 0.05 px small (dropped), and a half ring at 4, 5, 260 and 299
    (the one at 5 directly behind one at 4 and in front of a plain row; 260 and 299 are slots of the second compact pass)."""
    pools = []
    for gi, (theta, h, w) in enumerate(SECTOR_GEOMS):
        rng = np.random.RandomState(55 + gi)
        big = min(h, w) / 8.0
        rows = fo.blob_rows(rng, SECTOR_POOL, h, w, big / 3.0, big)
        tiny = fo.blob_rows(rng, SECTOR_POOL, h, w, 0.04, 0.05)
        rows[2::3] = tiny[2::3]
        for j in (4, 5, 260, 299):
            rows[j] = arc_band(h, w, 0.45 * w, 0.3 * h, 0.2 * min(h, w), 0.15 * min(h, w))
        rows.setflags(write=False)
        pools.append(rows)
    return pools


@functools.lru_cache(maxsize=None)
def sector_case(max_labels):
    """four images: 0 rows, 1 row, max_labels rows, max_labels + 3 rows (G[11] above max_labels), alternating between the two geometries;
    each image's rows start at its own offset into its geometry's pool"""
    pools = sector_pool()
    rows = np.concatenate(pools)
    counts = [0, 1, max_labels, max_labels + 3]
    first = [5, 4, 0, 3]                                  # the single row is a half ring; image 3 starts on a blob
    geo = np.zeros((4, GEO_D))
    for i, (cnt, f) in enumerate(zip(counts, first)):
        gi = i % 2
        theta, h, w = SECTOR_GEOMS[gi]
        g = fo.geometry(theta, h, w)
        geo[i] = (theta, g["T"], h, w, g["cw"], g["x0"], g["y0"], g["oh"], g["ow"], min(SECTOR_S[0] / g["oh"], SECTOR_S[1] / g["ow"]),
                  gi * SECTOR_POOL + f, cnt)
    return dict(rows=rows, geo=geo, counts=counts)


# ---- sector_gather / sector_warp_u8 / resize_linear_u8 / mask_bbox
@functools.lru_cache(maxsize=None)
def gather_case():
    """an 11 x 23 canvas, T = 5, n_ang = 9; the crop is 7 x 17 at (2, 3).  -1 at the crop's first and last pixel and at a few more;
    the canvas around the crop holds keys too, so a wrong origin or width shows."""
    rng = np.random.RandomState(8)
    T, n_ang, cw, ch = 5, 9, 23, 11
    y0, x0, oh, ow = 2, 3, 7, 17
    winner = rng.randint(0, T * n_ang, (ch, cw)).astype(np.int32)
    winner[rng.rand(ch, cw) < 0.15] = -1
    winner[y0, x0] = winner[y0 + oh - 1, x0 + ow - 1] = -1
    winner[y0, x0 + 1], winner[y0 + oh - 1, x0 + ow - 2] = T * n_ang - 1, 0
    src = rng.randint(0, 256, (T, n_ang, 3)).astype(np.uint8)
    img = rng.randint(0, 256, (6, 8, 3)).astype(np.uint8)
    return dict(T=T, n_ang=n_ang, cw=cw, ch=ch, y0=y0, x0=x0, oh=oh, ow=ow, winner=winner, src=src, img=img)


RESIZE_U8_SHAPES = [((6, 8), (5, 9)), ((1, 1), (3, 5)), ((7, 5), (3, 2)), ((9, 1), (4, 7)), ((3, 11), (17, 1))]
# existing full warps (tests/test_gpu_sector.py): (theta, h, w) -> the CPU file shows that they cross every cap of this family
SECTOR_FULL = [(60, 640, 640), (90, 427, 640), (30, 1280, 1280)]


# ---- paste
PASTE_MARGIN, PASTE_THR = 2.0, 0.30
PASTE_NEW = ("cut", "shifted", "rows256", "nosource")


def _paste_images(n, S_h, S_w, seed):
    return np.random.RandomState(seed).randint(0, 256, (n, 3, S_h, S_w)).astype(np.float32)


def _table(rows_per_image, max_labels, counts=None):
    n = len(rows_per_image)
    lab = np.zeros((n, max_labels, ROW), dtype=np.float32)
    for i, rows in enumerate(rows_per_image):
        for r, row in enumerate(rows[:max_labels]):
            lab[i, r] = row
    cnt = np.array([len(r) for r in rows_per_image] if counts is None else counts, dtype=np.int32)
    return lab, cnt


def _desc(items):
    d = np.zeros((len(items), PASTE_I), dtype=np.int64)
    for i, (on, j, flip, dx, dy, select) in enumerate(items):
        d[i, :5] = (on, j, flip, dx, dy)
        d[i, 5] = np.array([select], dtype=np.uint64).view(np.int64)[0]
    return d


ALL = 2 ** 64 - 1


@functools.lru_cache(maxsize=None)
def paste_case(name):
    """"cut":      S = 17 x 65 (one column in the second tile of 64, one row in the second of 16), max_labels 6: an object pasted over the
                   column 64 and the row 16, a second image that pastes it mirrored.  S_w % 4 = 1: VEC = false.
    "shifted":  S = 16 x 64, both image buffers 4 bytes off a 16-byte boundary: VEC = false although S_w % 4 == 0.
    "rows256":  S = 96 x 128, max_labels = 256 (52 floats of LDS per row: 53 248 bytes).  Image 0 pastes from image 1, which has 70 rows
                on a grid: those of the first 64 that its own three rows do not hide arrive, 64 .. 69 have no select bit.  Image 1 is
                full (256 rows): nothing fits.  Image 2 pastes image 0's three rows into an empty table.
    "nosource": S = 48 x 80: the partner's object hangs 5 px over its right edge; shifted by -9 it lies inside, but the columns whose
                source would be column 80 .. 84 keep the image's own pixels."""
    if name in ("cut", "shifted"):
        S_h, S_w, ml = (17, 65, 6) if name == "cut" else (16, 64, 6)
        obj = [co.polygon_row(3, S_w - 9.2, S_h - 9.2, 6.0), co.polygon_row(4, 9.0, 7.5, 4.0)]     # shifted by (3, 3) it ends at S_w - 0.2, S_h - 0.2
        lab, cnt = _table([[], obj, []], ml)
        paste = _desc([(1, 1, 0, 3, 3, ALL), (0, 0, 0, 0, 0, 0), (1, 1, 1, -3, 1, ALL)])
        n = 3
    elif name == "rows256":
        S_h, S_w, ml = 96, 128, 256
        grid = [co.polygon_row(k % 80, 8.0 + 12.0 * (k % 10), 8.0 + 12.0 * (k // 10), 3.0 + 0.1 * (k % 7)) for k in range(70)]
        own = [co.polygon_row(1, 20.0, 20.0, 9.0), co.polygon_row(2, 32.0, 20.0, 2.5), co.polygon_row(3, 92.3, 44.2, 2.0)]    # candidates 12 and 37 would hide the small ones
        full = [co.polygon_row(k % 80, 10.0 + (k % 16) * 7.0, 10.0 + (k // 16) * 5.0, 2.2) for k in range(256)]
        lab, cnt = _table([own, grid, full, []], ml)
        paste = _desc([(1, 1, 0, 0, 0, ALL), (0, 0, 0, 0, 0, 0), (1, 1, 0, 0, 0, ALL), (1, 0, 1, 4, 3, ALL)])
        n = 4
    else:
        S_h, S_w, ml = 48, 80, 6
        over = co.polygon_row(5, 76.0, 24.0, 9.0)                 # vertices up to x = 85
        lab, cnt = _table([[], [over]], ml)
        paste = _desc([(1, 1, 0, -9, 0, ALL), (1, 1, 1, 14, 2, ALL)])
        n = 2
    pre = _paste_images(n, S_h, S_w, 900 + PASTE_NEW.index(name))
    return dict(S=(S_h, S_w), max_labels=ml, pre_images=pre, pre_labels=lab, pre_count=cnt, paste=paste, n=n)
