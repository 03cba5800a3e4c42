"""References, draws and shape lists of the glue kernels of csrc/elementwise.hip: the SPP pools (ep24_spp_fwd, ep24_spp_bwd), the
nearest x2 upsample (ep24_upsample2_fwd, _bwd), ep24_rows_copy, the head decode (ep24_head_decode_fwd, _bwd), the bias column sums
(ep24_colsum, ep24_colsum_slab, ep24_colsum_splits) and the two stem packers (ep24_focus_pack, ep24_stem_pack).  A helper, not a test
module: tests/test_glue_reference.py checks it on the CPU (against torch's max_pool2d, autograd, interpolate and unfold, the direct
against the separable pool, and that every mutant of MUTANTS is rejected by an input of the GPU test), tests/test_gpu_glue_exact.py
runs the kernels against it.  It never imports the package under test.

The operations are written from the modules of the model (SPPBottleneck: three MaxPool2d(k, 1, k // 2) of the same map; Upsample(2,
"nearest"); Focus.forward: cat(top-left, bottom-left, top-right, bottom-right); the head's get_output_and_grid: grid = (x, y) of
meshgrid(arange(H), arange(W)), xy = (t + grid) * stride, radii = exp(t) * stride) and from include/ep24.h, not from the kernels.

Maps are numpy float32 arrays [B, H, W, C] whose values are bf16 numbers; what is compared bit for bit travels as bit patterns
(update_reference.bf16_rne, bits32), NaN equal to NaN.
"""
import functools
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from update_reference import bf16_rne, bf16_widen, bits32, from_bits32, random_bits  # noqa: E402

NEG = np.float32(-np.inf)
RADII = (2, 4, 6)                 # windows 5, 9, 13
CENTRE = 0x88
MAX_ITEMS = 2048 * 256            # MAX_BLOCKS workgroups of 256 lanes: one trip of a grid-stride loop


def bf(a):
    """float -> the nearest bf16 numbers, as float32"""
    return from_bits32(bf16_widen(bf16_rne(bits32(np.asarray(a, dtype=np.float32))))).reshape(np.shape(a))


def b16(a):
    """bf16-valued float32 array -> its bf16 bit patterns (flat)"""
    return bf16_rne(bits32(np.asarray(a, dtype=np.float32))).reshape(-1)


def bf16_from_f64(x):
    """float64 -> bf16 bit patterns, rounded to nearest even ONCE (no float32 in between); normal range only"""
    x = np.asarray(x, dtype=np.float64)
    _, e = np.frexp(x)                                   # |x| = m 2^e, 0.5 <= m < 1: 8 significant bits end at 2^(e - 8)
    ulp = np.ldexp(1.0, e - 8)
    q = np.rint(x / ulp) * ulp                           # rint: halves to even; the sign of a zero is kept
    out = (bits32(q.astype(np.float32)).reshape(-1) >> np.uint32(16)).astype(np.uint16)
    out[np.isnan(x).reshape(-1)] = 0x7FC0
    return out.reshape(-1)


def bf16_ulp(v):
    """the spacing of bf16 numbers at |v| (float64)"""
    _, e = np.frexp(np.asarray(v, dtype=np.float64))
    return np.ldexp(1.0, e - 8)


# ---------------------------------------------------------------------------------------------------------------------------
# (a) draws
def integer_draw(shape, seed):
    """bf16 integers in [-8, 8]: every sum of up to 2^20 of them is an fp32 number, whatever the order"""
    return np.random.default_rng(seed).integers(-8, 9, shape).astype(np.float32)


def ties_draw(shape, seed):
    """5 levels: most windows hold their maximum more than once"""
    return (np.random.default_rng(seed).integers(0, 5, shape).astype(np.float32) - np.float32(2.0)) * np.float32(0.5)


def special_draw(shape, seed):
    """the ties draw with a handful of NaN and -inf cells; in image 0 the channels 0 and C - 1 hold -inf over the whole 13-window of
    the pixel (H // 2, W // 2), so that window (and the 5- and 9-windows inside it) has no element above -inf"""
    B, H, W, C = shape
    rng = np.random.default_rng(seed)
    x = ties_draw(shape, seed + 1)
    n = x.size
    k = min(n, max(3, n // 40))
    flat = x.reshape(-1)
    flat[rng.choice(n, k, replace=False)] = NEG
    flat[rng.choice(n, k, replace=False)] = np.float32(np.nan)
    cy, cx = H // 2, W // 2
    for c in (0, C - 1):
        x[0, max(0, cy - 6):cy + 7, max(0, cx - 6):cx + 7, c] = NEG
    if W > 1:                                            # two NaN in one row of one window: the last one must win
        x[B - 1, H - 1, W - 2:, 1 % C] = np.float32(np.nan)
    return x


def general_draw(shape, seed, scale=1.0):
    return bf(np.random.default_rng(seed).standard_normal(shape).astype(np.float32) * np.float32(scale))


def dyadic4_draw(shape, seed):
    """m 2^e, |m| <= 15, -3 <= e <= 3: at most 4 significant bits"""
    rng = np.random.default_rng(seed)
    return (rng.integers(-15, 16, shape) * np.exp2(rng.integers(-3, 4, shape))).astype(np.float32)


# ---------------------------------------------------------------------------------------------------------------------------
# (b) SPP forward
def _code(dy, dx):
    return ((dy + 8) << 4) | (dx + 8)


def _spp_direct_one(x, r, tie="first"):
    B, H, W, C = x.shape
    k = 2 * r + 1
    xp = np.pad(x, ((0, 0), (r, r), (r, r), (0, 0)), constant_values=NEG)
    st = np.stack([xp[:, r + dy:r + dy + H, r + dx:r + dx + W] for dy in range(-r, r + 1) for dx in range(-r, r + 1)])
    nan = np.isnan(st)
    mx = np.where(nan, NEG, st).max(0)
    hit = st == mx
    first = hit.argmax(0) if tie == "first" else k * k - 1 - hit[::-1].argmax(0)
    first = np.where(mx == NEG, r * k + r, first)         # nothing above -inf: the centre
    has_nan = nan.any(0)
    last_nan = k * k - 1 - nan[::-1].argmax(0)
    win = np.where(has_nan, last_nan, first)
    val = np.where(has_nan, np.float32(np.nan), mx).astype(np.float32)
    code = (((win // k - r + 8) << 4) | (win % k - r + 8)).astype(np.uint8)
    return val, code


def spp_ref(x, radii=RADII, tie="first", cross=False, swap=False):
    """x [B, H, W, C] -> (vals float32 [3, B, H, W, C], codes uint8 [3, B, H, W, C]); all k^2 positions of every window.
    The keyword arguments make the mutants of MUTANTS."""
    shape = x.shape
    if cross:
        x = x.reshape(1, shape[0] * shape[1], shape[2], shape[3])
    vals, codes = zip(*[_spp_direct_one(x, r, tie) for r in radii])
    vals, codes = np.stack(vals).reshape((3,) + shape), np.stack(codes).reshape((3,) + shape)
    if swap:
        codes = ((codes & 15) << 4) | (codes >> 4)
    return vals, codes


def _pool1d(a, r, axis, carry=None):
    """One pass of the separable form along `axis`: -> (maximum, offset of the winner, carry at the winner).  A later element
    replaces the winner if it is greater or a NaN: the first maximum, the last NaN."""
    n = a.shape[axis]
    m = np.full(a.shape, NEG, dtype=np.float32)
    off = np.zeros(a.shape, dtype=np.int8)
    c = None if carry is None else carry.copy()
    for d in range(-r, r + 1):
        lo, hi = max(0, -d), min(n, n - d)
        if lo >= hi:
            continue
        dst, src = [slice(None)] * a.ndim, [slice(None)] * a.ndim
        dst[axis], src[axis] = slice(lo, hi), slice(lo + d, hi + d)
        dst, src = tuple(dst), tuple(src)
        v, cur = a[src], m[dst]
        take = (v > cur) | np.isnan(v)
        m[dst] = np.where(take, v, cur)
        off[dst] = np.where(take, np.int8(d), off[dst])
        if c is not None:
            c[dst] = np.where(take, carry[src], c[dst])
    return m, off, c


def spp_ref_separable(x):
    """The same through row maxima: the first row-major maximum is in the first row whose maximum is the window's, at that row's
    first maximum; the last NaN in the last row that has one, at that row's last NaN."""
    vals, codes = [], []
    for r in RADII:
        rm, rdx, _ = _pool1d(x, r, 2)
        m, dy, dx = _pool1d(rm, r, 1, carry=rdx)
        vals.append(m)
        codes.append((((dy.astype(np.int32) + 8) << 4) | (dx.astype(np.int32) + 8)).astype(np.uint8))
    return np.stack(vals), np.stack(codes)


def decode_codes(codes):
    """-> (dy, dx) int arrays"""
    c = codes.astype(np.int32)
    return (c >> 4) - 8, (c & 15) - 8


# (c) SPP backward
def _targets(codes_p):
    B, H, W, C = codes_p.shape
    dy, dx = decode_codes(codes_p)
    b, y, x, c = np.meshgrid(np.arange(B), np.arange(H), np.arange(W), np.arange(C), indexing="ij")
    ty, tx = y + dy, x + dx
    assert ty.min() >= 0 and ty.max() < H and tx.min() >= 0 and tx.max() < W, "a winner outside its image"
    return (((b * H + ty) * W + tx) * C + c).reshape(-1)


def spp_bwd_ref(dy5, dy9, dy13, codes, old, accumulate, round_first=False):
    """Every output sends its gradient to its winner; (+ old).  -> (sum float64, sum of |terms| float64, number of terms), each
    [B, H, W, C].  The bf16 result is bf16_from_f64(sum): rounded once."""
    shape = dy5.shape
    n = dy5.size
    tot, mag, cnt = np.zeros(n), np.zeros(n), np.zeros(n, dtype=np.int64)
    for g, cp in zip((dy5, dy9, dy13), codes):
        t = _targets(cp)
        g64 = g.astype(np.float64).reshape(-1)
        tot += np.bincount(t, weights=g64, minlength=n)
        mag += np.bincount(t, weights=np.abs(g64), minlength=n)
        cnt += np.bincount(t, minlength=n)
    if round_first:                                       # mutant: the routed sum is rounded to bf16 before old is added
        tot = from_bits32(bf16_widen(bf16_from_f64(tot))).astype(np.float64)
    if accumulate:
        o = old.astype(np.float64).reshape(-1)
        tot, mag, cnt = tot + o, mag + np.abs(o), cnt + 1
    return tot.reshape(shape), mag.reshape(shape), cnt.reshape(shape)


def spp_bwd_ordered_ref(dy5, dy9, dy13, codes, old, accumulate, round_first=False):
    """The fp32 order of the gather form: for an input pixel p, over dy (outer) and dx (inner) in -6 .. 6, the outputs o = p - (dy, dx)
    whose winner is p, the 13-pool first, then 9, then 5; old is added last.  -> bf16 bit patterns (flat)"""
    B, H, W, C = dy5.shape
    gs = (dy5, dy9, dy13)
    acc = np.zeros((B, H, W, C), dtype=np.float32)
    for dy in range(-6, 7):
        p_y, o_y = slice(max(0, dy), min(H, H + dy)), slice(max(0, dy) - dy, min(H, H + dy) - dy)
        if p_y.start >= p_y.stop:
            continue
        for dx in range(-6, 7):
            p_x, o_x = slice(max(0, dx), min(W, W + dx)), slice(max(0, dx) - dx, min(W, W + dx) - dx)
            if p_x.start >= p_x.stop:
                continue
            for pool in (2, 1, 0):
                if max(abs(dy), abs(dx)) > RADII[pool]:
                    continue
                hit = codes[pool][:, o_y, o_x] == _code(dy, dx)
                acc[:, p_y, p_x] += np.where(hit, gs[pool][:, o_y, o_x], np.float32(0.0))
    if round_first:
        acc = bf(acc)
    if accumulate:
        acc = acc + old.astype(np.float32)
    return b16(acc)


def lds_bound(mag, cnt, got):
    """|bf16 result - float64 sum| of an fp32 summation of cnt terms in any order: (cnt - 1) 2^-24 sum|terms| for the additions plus
    half a bf16 ulp of the result for the final rounding"""
    return np.maximum(cnt - 1, 0) * 2.0 ** -24 * mag + 0.5 * bf16_ulp(got)


# ---------------------------------------------------------------------------------------------------------------------------
# (d) upsample, rows_copy
def upsample2_ref(x, transposed=False):
    """nearest x2: y[b, 2h + a, 2w + c] = x[b, h, w].  transposed (mutant): rows and columns exchanged in the pixel index"""
    if transposed:
        B, H, W, C = x.shape
        return upsample2_ref(x.reshape(B, W, H, C)).reshape(B, 2 * H, 2 * W, C)
    return np.repeat(np.repeat(x, 2, axis=1), 2, axis=2)


def upsample2_bwd_ref(dy, old, accumulate, order="row", round_first=False):
    """dx = ((a00 + a01) + a10) + a11 of each 2x2 block in fp32 (a[row parity][column parity]), + old, one bf16 rounding.
    -> bf16 bit patterns (flat).  order 'col' (mutant): the parities exchanged, (a00 + a10) + a01."""
    B, H2, W2, C = dy.shape
    a = dy.astype(np.float32).reshape(B, H2 // 2, 2, W2 // 2, 2, C)
    first, second = (a[:, :, 0, :, 1], a[:, :, 1, :, 0]) if order == "row" else (a[:, :, 1, :, 0], a[:, :, 0, :, 1])
    acc = ((a[:, :, 0, :, 0] + first) + second) + a[:, :, 1, :, 1]
    if round_first:
        acc = bf(acc)
    if accumulate:
        acc = acc + old.astype(np.float32)
    return b16(acc)


def rows_copy_ref(src_bits, old_bits, accumulate):
    """dst[m, 0:C] = src, or bf16(dst + src) in fp32: bit patterns in, bit patterns out; the plain copy passes every pattern"""
    src_bits = np.asarray(src_bits, dtype=np.uint16)
    if not accumulate:
        return src_bits.copy()
    with np.errstate(all="ignore"):
        s = from_bits32(bf16_widen(src_bits)) + from_bits32(bf16_widen(np.asarray(old_bits, dtype=np.uint16)))
    return bf16_rne(bits32(s)).reshape(src_bits.shape)


# ---------------------------------------------------------------------------------------------------------------------------
# (e) head decode.  raw / dout / out are float32 [B, A, ncols]; the level holds the rows a0 .. a0 + H W of every image.
def decode_fwd_ref(raw, a0, H, W, s, origin=None, x_mod=None):
    """-> (out float32 [B, A, ncols]: columns 0, 1 of the level's rows decoded in fp32 (exact for dyadic raw values), everything else
    as in raw; radii float64 [B, H W, 24] = s exp(t) for columns 2 .. 25; origin with the level's raw columns 0 .. 25 written).
    x_mod (mutant): the modulus that gives x, W when right."""
    x_mod = W if x_mod is None else x_mod
    out = raw.copy()
    hw = np.arange(H * W)
    gx, gy = (hw % x_mod).astype(np.float32), (hw // x_mod).astype(np.float32)
    lvl = raw[:, a0:a0 + H * W]
    out[:, a0:a0 + H * W, 0] = (lvl[..., 0] + gx) * np.float32(s)
    out[:, a0:a0 + H * W, 1] = (lvl[..., 1] + gy) * np.float32(s)
    radii = float(s) * np.exp(lvl[..., 2:26].astype(np.float64))
    if origin is not None:
        origin = origin.copy()
        origin[:, a0:a0 + H * W, :] = lvl[..., :26]
    return out, radii, origin


def decode_bwd_ref(dout, out, a0, H, W, s, d_origin=None, zero_pad=True, pad_fill=0):
    """-> (d_regobj uint16 [B H W, 32], d_cls uint16 [B H W, (C + 7) & ~7]): float64, one bf16 rounding; columns 27 .. 31 and the
    class pad +0.  zero_pad False (mutant): the class pad keeps pad_fill."""
    B, A, ncols = dout.shape
    C = ncols - 27
    ld = (C + 7) & ~7
    d = dout[:, a0:a0 + H * W].astype(np.float64)
    o = out[:, a0:a0 + H * W].astype(np.float64)
    reg = np.zeros((B, H * W, 32))
    reg[..., 0:2] = d[..., 0:2] * float(s)
    reg[..., 2:26] = d[..., 2:26] * o[..., 2:26]
    if d_origin is not None:
        reg[..., :26] = reg[..., :26] + d_origin[:, a0:a0 + H * W].astype(np.float64)
    reg[..., 26] = d[..., 26]
    cls = np.zeros((B, H * W, ld))
    cls[..., :C] = d[..., 27:]
    cb = bf16_from_f64(cls).reshape(B * H * W, ld)
    if not zero_pad:
        cb[:, C:] = pad_fill
    return bf16_from_f64(reg).reshape(B * H * W, 32), cb


# ---------------------------------------------------------------------------------------------------------------------------
# (f) column sums.  g is an integer matrix [M, >= N] (the integer draw before it becomes bf16).
def colsum_splits_ref(M):
    """include/ep24.h leaves the count to the library; the kernel's comment: one split per 4 rows, at most 64"""
    return int(min(64, max(1, (M + 3) // 4)))


def colsum_ref(g, M, N):
    return g[:M, :N].sum(0, dtype=np.float64)


def colsum_owner(M, N, splits):
    """Block b sums the rows b rpp + r + k splits rpp (r < rpp = 256 // chunks row lanes, chunks = ceil(N / 8), k = 0, 1, ...), so row m
    belongs to block (m // rpp) % splits and to sweep k = m // (splits rpp).  -> (owner [M], k [M])"""
    rpp = 256 // ((N + 7) // 8)
    m = np.arange(M)
    return (m // rpp) % splits, m // (splits * rpp)


def colsum_slab_ref(g, M, N, splits, drop_last_group=False):
    """-> float64 [splits, N]: the partial of every block.  drop_last_group (mutant): the rows of the last sweep are left out."""
    owner, k = colsum_owner(M, N, splits)
    keep = k < k.max() if drop_last_group else np.ones(M, dtype=bool)
    out = np.zeros((splits, N))
    for b in range(splits):
        out[b] = g[:M][(owner == b) & keep][:, :N].sum(0, dtype=np.float64)
    return out


# ---------------------------------------------------------------------------------------------------------------------------
# (g) stem packers.  img: uint32 bit patterns [B, 3, H, W].
def focus_ref(img):
    """Focus.forward: cat(top-left, bottom-left, top-right, bottom-right) on the channel axis, as NHWC bf16 with 16 channels:
    -> uint16 [B, H / 2, W / 2, 16], channels 12 .. 15 zero"""
    B, _, H, W = img.shape
    r = bf16_rne(img).reshape(img.shape)
    cat = np.concatenate([r[:, :, 0::2, 0::2], r[:, :, 1::2, 0::2], r[:, :, 0::2, 1::2], r[:, :, 1::2, 1::2]], axis=1)
    out = np.zeros((B, H // 2, W // 2, 16), dtype=np.uint16)
    out[..., :12] = cat.transpose(0, 2, 3, 1)
    return out


def stem_rows_ref(img, ld, dx_major=False):
    """The 3x3, pad 1 patches of the Focus map: -> uint16 [B FH FW, ld], column (ky * 3 + kx) * 12 + channel; taps outside the map and
    the columns 108 .. ld are +0.  dx_major (mutant): tap kx * 3 + ky."""
    f = focus_ref(img)[..., :12]
    B, FH, FW, _ = f.shape
    fp = np.zeros((B, FH + 2, FW + 2, 12), dtype=np.uint16)
    fp[:, 1:-1, 1:-1] = f
    rows = np.zeros((B, FH, FW, ld), dtype=np.uint16)
    for ky in range(3):
        for kx in range(3):
            tap = kx * 3 + ky if dx_major else ky * 3 + kx
            rows[..., tap * 12:tap * 12 + 12] = fp[:, ky:ky + FH, kx:kx + FW]
    return rows.reshape(B * FH * FW, ld)


def image_bits(B, H, W, seed):
    """random fp32 patterns with the SPECIAL32 patterns at the front, in the middle and at the end"""
    return random_bits(B * 3 * H * W, seed).reshape(B, 3, H, W)


# ---------------------------------------------------------------------------------------------------------------------------
# (h) the shapes of tests/test_gpu_glue_exact.py, (B, H, W, C).  Every family has a non-square map.
SPP_FWD_SHAPES = [(1, 1, 1, 8), (2, 3, 7, 8), (2, 5, 13, 16), (1, 13, 12, 24), (3, 14, 6, 8), (2, 20, 20, 16)]
SPP_FWD_BIG = (2, 9, 8, 29136)                         # 144 pixels x 3642 channel groups = 524 448 items > MAX_ITEMS
SPP_BWD_LDS = [(2, 3, 7, 8), (1, 13, 45, 8), (2, 20, 20, 16)]
SPP_BWD_GATHER = [(1, 14, 42, 8), (1, 2, 293, 8), (2, 25, 25, 16)]
SPP_BWD_BIG = (1, 18, 33, 7072)                        # 594 pixels (gather form) x 884 channel groups = 525 096 items
UP_SHAPES = [(1, 1, 1, 8), (2, 3, 5, 24), (2, 5, 5, 16)]
UP_BIG = (1, 3, 5, 279624)                             # 15 x 34 953 = 524 295 items of the backward; the forward has 4 x as many
COPY_SHAPES = [(1, 8), (255, 24), (257, 16), (30, 24)]            # (M, C)
COPY_BIG = (2049, 2048)                                # 2049 x 256 items
DECODE_MAPS = [(3, 5), (4, 4)]
DECODE_STRIDES = [8.0, 16.0, 32.0]
COLSUM_N = [1, 8, 27, 80, 85, 256, 2048]
COLSUM_M = [1, 3, 4, 5, 255, 257, 40000]
STEM_IMAGES = [(1, 2, 2), (2, 6, 10), (3, 16, 12), (1, 34, 66)]    # (B, H, W); 17 x 33 = 561 pixels, not a multiple of 32
STEM_LD = [112, 120, 128, 136]
STEM_BIG = (1, 1450, 1450)                             # 525 625 pixels > 16 384 workgroups x 32


def items(shape):
    B, H, W, C = shape
    return B * H * W * (C // 8)


@functools.lru_cache(maxsize=None)
def spp_case(shape, draw):
    """-> (x, vals, codes) of a forward shape, shared by the tests that use it (read-only)"""
    x = {"ties": ties_draw, "special": special_draw}[draw](shape, 100 + sum(shape))
    vals, codes = spp_ref(x) if items(shape) <= 4096 else spp_ref_separable(x)
    return x, vals, codes


@functools.lru_cache(maxsize=None)
def colsum_draw(ld):
    """int8 [40 000, ld]: the integer draw, shared by every M of one ld (its first M rows)"""
    return np.random.default_rng(7000 + ld).integers(-8, 9, (max(COLSUM_M), ld), dtype=np.int8)


def int_bits(g8):
    """the bf16 bit patterns of an array of integers in [-8, 8]"""
    lut = b16(np.arange(-8, 9, dtype=np.float32))
    return lut[g8.astype(np.int16) + 8]


@functools.lru_cache(maxsize=None)
def spp_bwd_case(shape, draw):
    """-> (dy5, dy9, dy13, codes, old): incoming gradients and the old dx of `draw` ('integer' or 'general'), the winner codes of the
    special forward draw of the shape (NaN winners and windows without a maximum included)"""
    f = {"integer": integer_draw, "general": general_draw}[draw]
    seed = 200 + sum(shape)
    return tuple(f(shape, seed + i) for i in range(3)) + (spp_case(shape, "special")[2], f(shape, seed + 3))


def up_case(shape, draw):
    """-> (dy [B, 2H, 2W, C], old [B, H, W, C])"""
    B, H, W, C = shape
    f = {"integer": integer_draw, "general": general_draw}[draw]
    return f((B, 2 * H, 2 * W, C), 300 + sum(shape)), f(shape, 301 + sum(shape))


def bits16_draw(n, seed):
    """random bf16 patterns of every class: numbers, NaN with payloads of both signs, infinities, both zeros, denormals"""
    b = np.random.default_rng(seed).integers(0, 1 << 16, n, dtype=np.uint32).astype(np.uint16)
    edge = np.array([0x0000, 0x8000, 0x7F80, 0xFF80, 0x7FC0, 0xFFC0, 0x7F81, 0xFFA5, 0x7FFF, 0x0001, 0x8001, 0x3F80], dtype=np.uint16)
    k = min(n, edge.size)
    b[:k] = edge[:k]
    b[n - k:] = edge[:k][::-1]
    return b


DECODE_A0, DECODE_TAIL = 5, 4


def decode_fwd_case(H, W, ncols, seed=0):
    """raw float32 [2, A, ncols]: random patterns everywhere, k / 1024 (|k| <= 4096) in columns 0 .. 25 of the level's rows"""
    A = DECODE_A0 + H * W + DECODE_TAIL
    raw = from_bits32(random_bits(2 * A * ncols, 400 + seed + ncols)).reshape(2, A, ncols).copy()
    k = np.random.default_rng(401 + seed + ncols).integers(-4096, 4097, (2, H * W, 26))
    raw[:, DECODE_A0:DECODE_A0 + H * W, :26] = (k / 1024.0).astype(np.float32)
    return raw


def decode_bwd_case(H, W, ncols, seed=0):
    """-> (dout, out float32 [2, A, ncols], d_origin float32 [2, A, 26]), all of dyadic4_draw: every product and sum of the backward
    has at most 21 significant bits"""
    A = DECODE_A0 + H * W + DECODE_TAIL
    return (dyadic4_draw((2, A, ncols), 500 + seed + ncols), dyadic4_draw((2, A, ncols), 501 + seed + ncols),
            dyadic4_draw((2, A, 26), 502 + seed + ncols))
