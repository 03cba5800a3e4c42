"""References, draws and shape lists of the kernels of csrc/backbone_ops.hip (ep24_im2col_bf16, ep24_relu_fwd / _bwd, ep24_maxpool3s2_fwd /
_bwd, ep24_maxpool2_fwd / _bwd, ep24_avgpool2_fwd / _bwd, ep24_chanscale, ep24_colstats, ep24_stats_gather, ep24_incr_i64) and of
csrc/dwconv.hip (ep24_dwconv_fwd_bf16, _dgrad_bf16, _wgrad_slab_bf16, _wgrad_splits).  A helper, not a test module:
tests/test_backbone_reference.py checks it on the CPU (against torch's max_pool2d with indices and autograd through it, avg_pool2d, unfold,
relu and its autograd, conv2d(groups=C) with autograd in float64; the conditions on the draws; every mutant of MUTANTS rejected by an
input of the GPU test), tests/test_gpu_backbone_exact.py runs the kernels against it.  It never imports the package under test.

Maps are numpy float32 arrays [B, H, W, C] whose values are bf16 numbers, or uint16 bit patterns of the same shape; what is compared
bit for bit travels as bit patterns (update_reference.bf16_rne, bits32), NaN equal to NaN.

The bounds of the general class (normal draws through bf16, w = 0.3 N(0, 1) in fp32; u = 2^-24, the unit roundoff of fp32):
  z, dx        nine fused multiply-adds from a = 0: the first is one rounding of one product, every later one rounds a sum that holds the
               earlier errors, so |a - a64| <= ((1 + u)^9 - 1) sum|x w| =: e9 (Higham, Accuracy and Stability, (3.4) with fused products);
               the accumulate form adds one more rounded addition ((1 + u)^10 - 1, old among the terms); the bf16 rounding adds at most
               half a bf16 ulp of the result.
  sums         a sum of N fp32 terms t_i in ANY tree of rounded additions is within ((1 + u)^(N - 1) - 1) sum|t_i| of the sum of the t_i
               (each term passes through at most N - 1 additions).  The terms' own errors come on top:
                 colstats sum x:     the terms are exact;       sum x^2:  each product is rounded once: ((1 + u)^N - 1) sum x^2
                 slab sums:          x dz of two bf16 numbers is exact in fp32 and enters through an fma: ((1 + u)^(N - 1) - 1) sum|x dz|
                                     (a thread's chain of fused multiply-adds followed by the fold over row slots is such a tree)
                 depthwise sum a:    ((1 + u)^(N - 1) - 1) sum(|a64| + e9) + sum e9
                 depthwise sum a^2:  t = fl(a a), |t - a64^2| <= d := 2 |a64| e9 + e9^2 + u (|a64| + e9)^2, so
                                     ((1 + u)^(N - 1) - 1) sum(a64^2 + d) + sum d
               and every workgroup rounds its partial to 2^-20 fixed point once per word: 2^-21 per workgroup.
"""
import functools
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from update_reference import bf16_rne, bf16_widen, bits32, from_bits32, random_bits, is_nan16  # noqa: E402
from glue_reference import bf, b16, bf16_from_f64, bf16_ulp  # noqa: E402

NEG = np.float32(-np.inf)
NAN = np.float32(np.nan)
UR = 2.0 ** -24
FIX = 2 ** 20
MAX_BLOCKS = 16384                                # cap_grid of backbone_ops.hip
MAX_ITEMS = MAX_BLOCKS * 256                      # one trip of its grid-stride loops: 4 194 304 eight-channel items
COLSTATS_BLOCKS = 1024                            # ep24_colstats: one workgroup per 16 rows, at most 1024
DW_GRID_CAP = 4096                                # forward and input gradient of dwconv.hip: ~4 pixels per thread
DW_SPLIT_CAP = 256                                # weight gradient: >= 16 pixels per thread


def widen(bits):
    """bf16 bit patterns -> float32"""
    return from_bits32(bf16_widen(np.asarray(bits, dtype=np.uint16).reshape(-1))).reshape(np.shape(bits))


def bits_of(a):
    """bf16-valued float32 array -> bit patterns of the same shape"""
    return b16(a).reshape(np.shape(a))


def rounds(a):
    """float32 array -> bf16 bit patterns (one rounding to nearest even), same shape"""
    return bf16_rne(bits32(np.asarray(a, dtype=np.float32)).reshape(-1)).reshape(np.shape(a))


# ---------------------------------------------------------------------------------------------------------------------------
# (a) draws
def ties_draw(shape, seed):
    """(a) integers in [-2, 2]: ties everywhere"""
    return np.random.default_rng(seed).integers(-2, 3, shape).astype(np.float32)


def negative_draw(shape, seed):
    """(b) all negative: a pool that pads with zeros gives 0 in every border window"""
    return -(np.random.default_rng(seed).integers(1, 6, shape).astype(np.float32)) * np.float32(0.5)


def special_draw(shape, seed):
    """(c) the ties draw with NaN and -inf in the interior and at a border; two NaN in one window (the last one wins); in image 0,
    channel 0 the first 3x3 window holds -inf only"""
    B, H, W, C = shape
    rng = np.random.default_rng(seed)
    x = ties_draw(shape, seed + 1)
    flat = x.reshape(-1)
    k = min(flat.size, max(2, flat.size // 30))
    flat[rng.choice(flat.size, k, replace=False)] = NEG
    flat[rng.choice(flat.size, k, replace=False)] = NAN
    x[0, :2, :2, 0] = NEG
    x[B - 1, H - 1, W - 1, C - 1] = NAN
    x[B - 1, H // 2, W // 2, 1] = NAN
    if W > 1:
        x[B - 1, H - 1, W - 2, C - 1] = NAN
    x[0, 0, 0, 2] = np.float32(-0.0)
    return x


def bits_draw(shape, seed):
    """random bf16 patterns (update_reference.random_bits rounded to bf16: numbers, infinities, NaN, both zeros; no denormals)"""
    n = int(np.prod(shape))
    return widen(bf16_rne(random_bits(n, seed))).reshape(shape)


def general_draw(shape, seed, scale=1.0):
    return bf(np.random.default_rng(seed).standard_normal(shape).astype(np.float32) * np.float32(scale))


def planted_draw(shape, seed):
    """normal draws with NaN, +inf, -inf and -0 planted by hand at the front, in the middle and at the end"""
    x = general_draw(shape, seed)
    flat = x.reshape(-1)
    sp = np.array([np.nan, np.inf, -np.inf, -0.0], dtype=np.float32)
    n = flat.size
    for at in (0, n // 2, n - 4):
        if 0 <= at and at + 4 <= n:
            flat[at:at + 4] = sp
    return x


def integer_draw(shape, seed, lim=8):
    return np.random.default_rng(seed).integers(-lim, lim + 1, shape).astype(np.float32)


POOL_DRAWS = {"ties": ties_draw, "negative": negative_draw, "special": special_draw, "bits": bits_draw}


# ---------------------------------------------------------------------------------------------------------------------------
# (b) max pools.  A later tap replaces the winner if it is greater or a NaN (ATen's update): the first maximum, the last NaN.
def _update(best, code, v, t, tie="first", nan_wins=True):
    """one tap of the scan, in place on (a view of) best / code"""
    with np.errstate(invalid="ignore"):
        take = (code == 0xFF) | ((v >= best) if tie == "last" else (v > best))
        if nan_wins:
            take |= np.isnan(v)
    np.copyto(best, v, where=take)
    np.copyto(code, np.uint8(t), where=take)


def pool3_out(n, oh="ceil"):
    return (n - 1) // 2 + 1 if oh == "ceil" else max(n // 2, 1)


def _span(n, on, k):
    """the outputs o0 .. o1 - 1 whose tap k lies inside 0 .. n - 1, and that tap's first position: 0 <= 2 o - 1 + k < n"""
    o0 = 0 if k >= 1 else 1
    o1 = min(on, (n - k) // 2 + 1)
    return o0, o1, 2 * o0 - 1 + k


def maxpool3s2_ref(x, tie="first", nan_wins=True, pad="skip", oh="ceil"):
    """nn.MaxPool2d(3, 2, 1): window 3, stride 2, pad 1, OH = (H - 1) // 2 + 1; padding taps do not take part; code = kh * 3 + kw.
    The keyword arguments make the mutants (pad 'zero': padding taps hold 0 and take part; oh 'floor': OH = H // 2)."""
    B, H, W, C = x.shape
    OH, OW = pool3_out(H, oh), pool3_out(W, oh)
    best = np.full((B, OH, OW, C), NEG, dtype=np.float32)
    code = np.full((B, OH, OW, C), 0xFF, dtype=np.uint8)
    if pad == "zero":
        xp = np.zeros((B, 2 * OH + 2, 2 * OW + 2, C), dtype=np.float32)
        hh, ww = min(H, 2 * OH + 1), min(W, 2 * OW + 1)
        xp[:, 1:hh + 1, 1:ww + 1] = x[:, :hh, :ww]
        for t in range(9):
            _update(best, code, xp[:, t // 3:t // 3 + 2 * OH:2, t % 3:t % 3 + 2 * OW:2], t, tie, nan_wins)
        return best, code
    for kh in range(3):
        y0, y1, py = _span(H, OH, kh)
        for kw in range(3):
            x0, x1, px = _span(W, OW, kw)
            if y0 < y1 and x0 < x1:
                v = x[:, py:py + 2 * (y1 - y0):2, px:px + 2 * (x1 - x0):2]
                _update(best[:, y0:y1, x0:x1], code[:, y0:y1, x0:x1], v, kh * 3 + kw, tie, nan_wins)
    return best, code


def maxpool2_ref(x, tie="first", nan_wins=True):
    """nn.MaxPool2d(2, 2): code = dy * 2 + dx"""
    B, H, W, C = x.shape
    best = np.full((B, H // 2, W // 2, C), NEG, dtype=np.float32)
    code = np.full((B, H // 2, W // 2, C), 0xFF, dtype=np.uint8)
    for t in range(4):
        _update(best, code, x[:, t // 2::2, t % 2::2], t, tie, nan_wins)
    return best, code


def maxpool3s2_bwd_ref(dy, codes, old, accumulate, H, W):
    """Per input pixel the fp32 sum over the windows that chose it, kh outer and kw inner (py = 2 oy - 1 + kh), then the old value,
    one rounding.  -> bf16 bit patterns [B, H, W, C]"""
    B, OH, OW, C = dy.shape
    acc = np.zeros((B, H, W, C), dtype=np.float32)
    with np.errstate(all="ignore"):
        for kh in range(3):
            y0, y1, py = _span(H, OH, kh)
            for kw in range(3):
                x0, x1, px = _span(W, OW, kw)
                if y0 >= y1 or x0 >= x1:
                    continue
                dst = acc[:, py:py + 2 * (y1 - y0):2, px:px + 2 * (x1 - x0):2]
                np.add(dst, dy[:, y0:y1, x0:x1], out=dst, where=codes[:, y0:y1, x0:x1] == kh * 3 + kw)
        if accumulate:
            acc = old.astype(np.float32) + acc
    return rounds(acc)


def maxpool2_bwd_ref(dy, codes, old, accumulate):
    """bf16(old + (hit ? g : 0)); without accumulate old is +0"""
    B, OH, OW, C = dy.shape
    g = np.repeat(np.repeat(dy, 2, axis=1), 2, axis=2)
    c = np.repeat(np.repeat(codes, 2, axis=1), 2, axis=2)
    want = ((np.arange(2 * OH) & 1)[:, None] * 2 + (np.arange(2 * OW) & 1)[None, :]).astype(np.uint8)
    o = old.astype(np.float32) if accumulate else np.zeros(g.shape, dtype=np.float32)
    with np.errstate(all="ignore"):
        return rounds(o + np.where(c == want[None, :, :, None], g, np.float32(0.0)))


# (c) avgpool2, chanscale
def avgpool2_ref(x, order="row", round_pairs=False):
    """bf16((((0 + x00) + x01) + x10) + x11) * 0.25) in fp32 (the sum starts from +0: four -0 give +0).  order 'col' (mutant):
    x10 before x01; round_pairs (mutant): bf16(x00 + x01) + bf16(x10 + x11), a rounding in between."""
    a, b, c, d = x[:, 0::2, 0::2], x[:, 0::2, 1::2], x[:, 1::2, 0::2], x[:, 1::2, 1::2]
    if order == "col":
        b, c = c, b
    with np.errstate(all="ignore"):
        s = (((np.float32(0.0) + a) + b) + c) + d
        if round_pairs:
            s = widen(rounds(a + b)) + widen(rounds(c + d))
        return rounds(s * np.float32(0.25))


def avgpool2_bwd_ref(dy, old, accumulate):
    """bf16(old + g * 0.25), or bf16(g * 0.25)"""
    g = np.repeat(np.repeat(dy, 2, axis=1), 2, axis=2)
    with np.errstate(all="ignore"):
        q = g * np.float32(0.25)
        return rounds(old.astype(np.float32) + q if accumulate else q)


def chanscale_ref(x, keep):
    """bf16(fl32(x * keep[n * C + c])): x [B, HW, C], keep float32 [B, C]"""
    with np.errstate(all="ignore"):
        return rounds(x * keep[:, None, :].astype(np.float32))


# (d) im2col, relu
def im2col_out(n, k, s, p):
    return (n + 2 * p - k) // s + 1


def im2col_ref(img_bits, k, s, p, ld, channel_major=False):
    """img_bits uint32 [B, C, H, W] (fp32 patterns) -> uint16 [B OH OW, ld]: column (kh k + kw) C + c, +0 in the padding and in the
    columns >= k k C, one rounding fp32 -> bf16.  channel_major (mutant): column c k k + kh k + kw."""
    B, C, H, W = img_bits.shape
    OH, OW = im2col_out(H, k, s, p), im2col_out(W, k, s, p)
    r = bf16_rne(img_bits.reshape(-1)).reshape(B, C, H, W).transpose(0, 2, 3, 1)
    rp = np.zeros((B, H + 2 * p + s, W + 2 * p + s, C), dtype=np.uint16)
    rp[:, p:p + H, p:p + W] = r
    rows = np.zeros((B, OH, OW, ld), dtype=np.uint16)
    for kh in range(k):
        for kw in range(k):
            v = rp[:, kh:kh + s * OH:s, kw:kw + s * OW:s][:, :OH, :OW]
            if channel_major:
                rows[..., kh * k + kw:k * k * C:k * k] = v
            else:
                rows[..., (kh * k + kw) * C:(kh * k + kw + 1) * C] = v
    return rows.reshape(B * OH * OW, ld)


def relu_fwd_ref(bits, zero_nan=False):
    """ATen's relu on bf16 patterns: x < 0 -> +0, everything else - NaN and -0 included - as it is.  zero_nan (mutant): NaN -> +0."""
    bits = np.asarray(bits, dtype=np.uint16)
    with np.errstate(invalid="ignore"):
        neg = widen(bits) < 0
    if zero_nan:
        neg = neg | is_nan16(bits)
    return np.where(neg, np.uint16(0), bits)


def relu_bwd_ref(dy_bits, y_bits, zero_nan=False):
    """ATen's threshold_backward: y <= 0 -> +0, else the gradient as it is; a NaN y passes it.  zero_nan (mutant): a NaN y zeroes."""
    dy_bits, y_bits = np.asarray(dy_bits, dtype=np.uint16), np.asarray(y_bits, dtype=np.uint16)
    with np.errstate(invalid="ignore"):
        off = widen(y_bits) <= 0
    if zero_nan:
        off = off | is_nan16(y_bits)
    return np.where(off, np.uint16(0), dy_bits)


# (e) statistics in 2^-20 fixed point
def colstats_blocks(M):
    return int(min(COLSTATS_BLOCKS, (M + 15) // 16))


def colstats_ref(x):
    """x float32 [M, C] -> (sum x, sum x^2) float64 [2, C].  On the integer draw sum * 2^20 is the exact fixed-point word."""
    x64 = x.astype(np.float64)
    return np.stack([x64.sum(0), (x64 * x64).sum(0)])


def colstats_bound(x, blocks):
    """-> float64 [2, C], see the module docstring"""
    M = x.shape[0]
    x64 = np.abs(x.astype(np.float64))
    g1, g2 = (1 + UR) ** (M - 1) - 1, (1 + UR) ** M - 1
    return np.stack([g1 * x64.sum(0), g2 * (x64 * x64).sum(0)]) + blocks * 2.0 ** -21


def fix_words(sums):
    """exact integer-valued sums float64 -> int64 fixed-point words"""
    w = np.asarray(sums, dtype=np.float64) * FIX
    assert np.array_equal(w, np.rint(w)) and float(np.abs(w).max(initial=0)) < 2.0 ** 62
    return w.astype(np.int64)


def stats_gather_ref(src, C):
    """src int64 [reps, 2, ld_src] -> [reps, 2, C]"""
    return src[:, :, :C].copy()


# ---------------------------------------------------------------------------------------------------------------------------
# (f) depthwise 3x3, pad 1, stride 1 or 2, OH = (H - 1) // stride + 1.  x [B, H, W, C], w [C, 3, 3], float64 sums.
def dw_out(n, s):
    return (n - 1) // s + 1


def dw_rpb(C):
    tpr = C // 8
    return 1 if tpr >= 256 else 256 // tpr


def dw_grid(M, C, cap=DW_GRID_CAP):
    return int(min(cap, max(1, -(-M // (dw_rpb(C) * 4)))))


def dw_splits_ref(B, H, W, C, stride):
    """ep24_dwconv_wgrad_splits: one workgroup per 16 rpb output pixels (rpb = 256 // (C / 8) row slots, 1 from C = 2048), 1 .. 256;
    -1 for an empty shape, C % 8 != 0 or a stride other than 1 and 2"""
    if B <= 0 or H <= 0 or W <= 0 or C <= 0 or C % 8 or stride not in (1, 2):
        return -1
    M = B * dw_out(H, stride) * dw_out(W, stride)
    return int(min(DW_SPLIT_CAP, max(1, -(-M // (16 * dw_rpb(C))))))


def _dw_taps(x, s):
    B, H, W, C = x.shape
    OH, OW = dw_out(H, s), dw_out(W, s)
    xp = np.zeros((B, H + 2, W + 2, C), dtype=np.float64)
    xp[:, 1:-1, 1:-1] = x
    return [(kh, kw, xp[:, kh:kh + s * (OH - 1) + 1:s, kw:kw + s * (OW - 1) + 1:s]) for kh in range(3) for kw in range(3)]


def dw_fwd_ref(x, w, s):
    """-> (acc float64 [B, OH, OW, C], sum|terms|)"""
    w64 = w.astype(np.float64)
    acc, mag = 0.0, 0.0
    for kh, kw, v in _dw_taps(x, s):
        t = v * w64[:, kh, kw]
        acc, mag = acc + t, mag + np.abs(t)
    return acc, mag


def dw_dgrad_ref(dz, w, s, H, W, parity=True):
    """dx[y, x] = sum over the taps (kh, kw) with (y + 1 - kh, x + 1 - kw) = s (oy, ox) inside the output of dz[oy, ox] w[kh, kw].
    -> (sum float64 [B, H, W, C], sum|terms|).  parity False (mutant): stride 2 takes odd (y + 1 - kh) as well, halved."""
    B, OH, OW, C = dz.shape
    w64, dz64 = w.astype(np.float64), dz.astype(np.float64)
    acc, mag = np.zeros((B, H, W, C)), np.zeros((B, H, W, C))
    for kh in range(3):
        ny = np.arange(H) + 1 - kh
        oky = (ny >= 0) & ((ny % s == 0) | (not parity)) & (ny // s < OH)
        for kw in range(3):
            nx = np.arange(W) + 1 - kw
            okx = (nx >= 0) & ((nx % s == 0) | (not parity)) & (nx // s < OW)
            g = dz64[:, np.clip(ny // s, 0, OH - 1)][:, :, np.clip(nx // s, 0, OW - 1)]
            t = g * w64[:, kh, kw] * (oky[:, None] & okx[None, :])[None, :, :, None]
            acc, mag = acc + t, mag + np.abs(t)
    return acc, mag


def dw_wgrad_ref(x, dz, s):
    """-> (dw float64 [C, 3, 3], sum|terms| [C, 3, 3])"""
    C = x.shape[-1]
    dw, mag = np.zeros((C, 3, 3)), np.zeros((C, 3, 3))
    dz64 = dz.astype(np.float64)
    for kh, kw, v in _dw_taps(x, s):
        t = v * dz64
        dw[:, kh, kw], mag[:, kh, kw] = t.sum((0, 1, 2)), np.abs(t).sum((0, 1, 2))
    return dw, mag


def dw_stats_ref(acc, of="acc"):
    """(sum a, sum a^2) float64 [2, C] of the fp32 accumulator; of 'z' (mutant): of the stored bf16 z"""
    a = acc if of == "acc" else widen(bf16_from_f64(acc)).astype(np.float64).reshape(acc.shape)
    return np.stack([a.sum((0, 1, 2)), (a * a).sum((0, 1, 2))])


def dw_z_bound(mag, got, terms=9):
    return ((1 + UR) ** terms - 1) * mag + 0.5 * bf16_ulp(got)


def dw_stats_bound(acc, mag, grid):
    """-> float64 [2, C], see the module docstring"""
    N = acc.shape[0] * acc.shape[1] * acc.shape[2]
    e9 = ((1 + UR) ** 9 - 1) * mag
    a = np.abs(acc)
    g = (1 + UR) ** (N - 1) - 1
    d = 2 * a * e9 + e9 * e9 + UR * (a + e9) ** 2
    b1 = g * (a + e9).sum((0, 1, 2)) + e9.sum((0, 1, 2))
    b2 = g * (a * a + d).sum((0, 1, 2)) + d.sum((0, 1, 2))
    return np.stack([b1, b2]) + grid * 2.0 ** -21


def dw_sum_bound(mag, N):
    return ((1 + UR) ** (N - 1) - 1) * mag


def dw_exact_draw(shape, seed, ternary=False):
    """-> (x, w [C, 3, 3], dz per stride {1: , 2: }, old dx): integers, x and dz in [-8, 8], w in [-32, 32]; ternary: all in {-1, 0, 1}"""
    B, H, W, C = shape
    rng = np.random.default_rng(seed)
    lx, lw = (1, 1) if ternary else (8, 32)
    x = rng.integers(-lx, lx + 1, shape).astype(np.float32)
    w = rng.integers(-lw, lw + 1, (C, 3, 3)).astype(np.float32)
    dz = {s: rng.integers(-lx, lx + 1, (B, dw_out(H, s), dw_out(W, s), C)).astype(np.float32) for s in (1, 2)}
    old = rng.integers(-lx, lx + 1, shape).astype(np.float32)
    return x, w, dz, old


def dw_general_draw(shape, seed):
    B, H, W, C = shape
    rng = np.random.default_rng(seed)
    x = bf(rng.standard_normal(shape).astype(np.float32))
    w = (rng.standard_normal((C, 3, 3)) * 0.3).astype(np.float32)
    dz = {s: bf(rng.standard_normal((B, dw_out(H, s), dw_out(W, s), C)).astype(np.float32)) for s in (1, 2)}
    old = bf(rng.standard_normal(shape).astype(np.float32))
    return x, w, dz, old


@functools.lru_cache(maxsize=None)
def dw_case(shape, stride, draw):
    """Everything the depthwise tests of one (shape, stride, draw) need, computed once (read-only).  draw: 'integer', 'ternary',
    'general'."""
    B, H, W, C = shape
    x, w, dzs, old = dw_general_draw(shape, 900 + sum(shape)) if draw == "general" else dw_exact_draw(shape, 800 + sum(shape), draw == "ternary")
    dz = dzs[stride]
    acc, mag = dw_fwd_ref(x, w, stride)
    dx, dmag = dw_dgrad_ref(dz, w, stride, H, W)
    dw, wmag = dw_wgrad_ref(x, dz, stride)
    return dict(x=x, w=w, dz=dz, old=old, acc=acc, mag=mag, dx=dx, dmag=dmag, dw=dw, wmag=wmag, stats=dw_stats_ref(acc),
                stats_z=dw_stats_ref(acc, "z"), M=acc.shape[0] * acc.shape[1] * acc.shape[2])


def dw_exact_conditions(case, main):
    """The conditions that make the integer class exact and discriminating, on the reference alone.  Every case: per-channel sum|a|
    and sum a^2 over the whole case below 2^24 (every partial sum of any partition is then an exact integer in fp32), the values
    integers.  main: >= 10 % of the outputs need a real rounding to bf16 and the statistics of the accumulator differ from those of
    bf16(z) in at least half the channels."""
    acc = case["acc"]
    assert np.array_equal(acc, np.rint(acc))
    assert float(np.abs(acc).sum((0, 1, 2)).max()) < 2 ** 24 and float((acc * acc).sum((0, 1, 2)).max()) < 2 ** 24
    assert float(np.abs(case["dx"]).max()) + 8 < 2 ** 24 and float(case["wmag"].max()) < 2 ** 24
    if main:
        z = widen(bf16_from_f64(acc)).astype(np.float64).reshape(acc.shape)
        assert float((z != acc).mean()) >= 0.10, float((z != acc).mean())
        differ = np.any(case["stats"] != case["stats_z"], axis=0)
        assert int(differ.sum()) * 2 >= differ.size, int(differ.sum())


# ---------------------------------------------------------------------------------------------------------------------------
# (g) the shapes of tests/test_gpu_backbone_exact.py, (B, H, W, C).  Every family has a non-square map.
POOL3_MAPS = [(1, 1), (1, 6), (7, 9), (8, 5), (14, 18)]
POOL2_MAPS = [(2, 2), (2, 10), (6, 8)]
BC = [(1, 8), (3, 24), (3, 8), (1, 24)]


def _pool_shapes(maps):
    return [(BC[i % 2][0], h, w, BC[i % 2][1]) for i, (h, w) in enumerate(maps)] + [(BC[2 + i % 2][0], h, w, BC[2 + i % 2][1]) for i, (h, w) in enumerate(maps[1:])]


POOL3_SHAPES = _pool_shapes(POOL3_MAPS)
POOL2_SHAPES = _pool_shapes(POOL2_MAPS)
LAYOUTS = {"tight": (0, 0), "slice8": (8, 16), "slice16": (16, 8)}        # (column offset of the slice, columns behind it): ld = off + C + behind

ROWS_SHAPES = [(1, 8), (15, 24), (17, 8), (300, 24)]                      # (M, C) of relu and chanscale
IM2COL_CASES = [                                                           # (B, C, H, W, k, s, p, ld)
    (2, 3, 15, 12, 7, 2, 3, 152), (1, 3, 16, 13, 7, 2, 3, 152), (1, 3, 7, 7, 7, 2, 3, 152), (2, 3, 7, 7, 3, 1, 1, 32),
    (1, 3, 6, 9, 3, 1, 1, 32), (2, 3, 5, 8, 3, 1, 1, 32), (1, 3, 3, 3, 7, 2, 3, 152)]
IM2COL_BIG = (1, 8, 683, 683, 3, 1, 1, 72)                                 # 466 489 rows x 9 chunks = 4 198 401 items
COLSTATS_C = [8, 24, 200, 2048]
COLSTATS_M = [1, 15, 17, 300]
COLSTATS_BIG = (16400, 8)                                                  # 1025 groups of 16 rows: past the 1024-workgroup cap
GATHER_CASES = [(8, 8, 1), (24, 40, 3), (200, 256, 8), (2048, 2056, 2)]    # (C, ld_src, reps)

DW_MAIN = [(2, 9, 7, 16), (1, 9, 7, 24), (3, 5, 6, 8)]                     # integer draw, all conditions
DW_BORDER = [(1, 1, 1, 8), (1, 1, 5, 8), (1, 5, 1, 24), (1, 2, 2, 8), (2, 6, 5, 16), (3, 9, 7, 8), (1, 9, 7, 200)]     # integer draw
DW_TERNARY = [(1, 3, 3, 2048), (1, 5, 6, 2048), (1, 3, 4, 2056), (2, 5, 6, 2056)]
DW_GENERAL = [(2, 9, 7, 16), (1, 6, 5, 24), (1, 9, 7, 200), (1, 3, 4, 2056)]
DW_WGRAD_CAP = (1, 17, 241, 2048)                                          # 4097 pixels, one row slot: 257 groups of 16 -> the cap of 256
DW_STATS_FORMS = ["null", "r1", "r8"]

# one case per kernel with a cap_grid loop: (B, H, W, C) just above MAX_ITEMS items, few pixels and many channels
CAP = {
    "relu_fwd": (1, 1, 3, 8 * 1398102), "relu_bwd": (1, 1, 3, 8 * 1398102), "chanscale": (1, 1, 3, 8 * 1398102),
    "maxpool3s2_fwd": (1, 1, 3, 8 * 2097153), "maxpool3s2_bwd": (1, 1, 3, 8 * 1398102),
    "maxpool2_fwd": (1, 2, 2, 8 * 4194305), "maxpool2_bwd": (1, 2, 2, 8 * 1048577),
    "avgpool2_fwd": (1, 2, 2, 8 * 4194305), "avgpool2_bwd": (1, 2, 2, 8 * 1048577),
}


def cap_items(name):
    B, H, W, C = CAP[name]
    if name == "maxpool3s2_fwd":
        H, W = pool3_out(H), pool3_out(W)
    elif name in ("maxpool2_fwd", "avgpool2_fwd"):
        H, W = H // 2, W // 2
    return B * H * W * (C // 8)


def im2col_items(case):
    B, C, H, W, k, s, p, ld = case
    return B * im2col_out(H, k, s, p) * im2col_out(W, k, s, p) * (ld // 8)


@functools.lru_cache(maxsize=None)
def pool_case(kind, shape, draw):
    """-> (x, vals, codes) of a max-pool forward case, shared by the tests that use it (read-only)"""
    x = POOL_DRAWS[draw](shape, 100 + sum(shape))
    vals, codes = (maxpool3s2_ref if kind == 3 else maxpool2_ref)(x)
    return x, vals, codes


def pool_conditions(kind, shape, draw):
    """What makes a max-pool case discriminating, on the reference alone.  (a) ties: at least 25 % of the windows hold their maximum
    more than once (maps of 12 pixels and more: a 1 x 1 map has one-tap windows) and every legal code occurs (48 outputs and more);
    (b) negative: every window's maximum - the border windows' included - is negative, so a pool that pads with zeros differs there;
    (c) special: a NaN wins somewhere and, on maps of 12 pixels and more, a window holds nothing above -inf."""
    B, H, W, C = shape
    x, vals, codes = pool_case(kind, shape, draw)
    if draw == "ties":
        assert H * W < 12 or tied_fraction(kind, x, vals) >= 0.25, tied_fraction(kind, x, vals)
        assert vals.size < 48 or set(np.unique(codes)) == legal_codes(kind, H, W)
    elif draw == "negative":
        assert float(x.max()) < 0 and float(vals.max()) < 0
    elif draw == "special":
        assert np.isnan(vals).any() and (H * W < 12 or bool((vals == NEG).any()))
    assert set(np.unique(codes)) <= legal_codes(kind, H, W)


def tied_fraction(kind, x, vals):
    """the share of windows that hold their maximum more than once"""
    if kind == 2:
        cnt = sum((x[:, dy::2, dx::2] == vals) for dy in range(2) for dx in range(2))
    else:
        B, H, W, C = x.shape
        OH, OW = vals.shape[1:3]
        xp = np.full((B, 2 * OH + 2, 2 * OW + 2, C), np.float32(np.nan))
        xp[:, 1:H + 1, 1:W + 1] = x
        cnt = sum((xp[:, kh:kh + 2 * OH:2, kw:kw + 2 * OW:2] == vals) for kh in range(3) for kw in range(3))
    return float((cnt > 1).mean())


def legal_codes(kind, H, W):
    """the codes some window of an H x W map can take"""
    if kind == 2:
        return set(range(4))
    OH, OW = pool3_out(H), pool3_out(W)
    ys = {kh for oy in range(OH) for kh in range(3) if 0 <= 2 * oy - 1 + kh < H}
    xs = {kw for ox in range(OW) for kw in range(3) if 0 <= 2 * ox - 1 + kw < W}
    return {kh * 3 + kw for kh in ys for kw in xs}


# ---------------------------------------------------------------------------------------------------------------------------
# (h) the inputs the GPU test feeds, shared with the CPU module (read-only)
def cancel_draw(shape, seed):
    """normal draws with planted specials; the first 2x2 window of every image and channel holds (big, -big, small, x11): the row
    order gives small + x11, an order that adds x10 before x01 loses `small` in the rounding of big + small"""
    x = planted_draw(shape, seed)
    x[:, 0, 0, :], x[:, 0, 1, :], x[:, 1, 0, :] = np.float32(2.0 ** 20), np.float32(-2.0 ** 20), np.float32(0.0078125)
    return x


AVG_DRAWS = {"cancel": cancel_draw, "bits": bits_draw, "integer": integer_draw}


@functools.lru_cache(maxsize=None)
def avg_case(shape, draw):
    """-> (x [B, H, W, C], dy [B, H / 2, W / 2, C], old [B, H, W, C])"""
    B, H, W, C = shape
    f = AVG_DRAWS[draw]
    g = planted_draw if draw == "cancel" else f
    return f(shape, 300 + sum(shape)), g((B, H // 2, W // 2, C), 301 + sum(shape)), g(shape, 302 + sum(shape))


@functools.lru_cache(maxsize=None)
def pool_bwd_case(kind, shape):
    """-> (dy [B, OH, OW, C], old [B, H, W, C]) of planted normal draws for the codes of the forward cases of `shape`"""
    B, H, W, C = shape
    OH, OW = (pool3_out(H), pool3_out(W)) if kind == 3 else (H // 2, W // 2)
    return planted_draw((B, OH, OW, C), 400 + sum(shape)), planted_draw(shape, 401 + sum(shape))


@functools.lru_cache(maxsize=None)
def relu_case(M, C):
    """-> (y bits [M, C], dy bits [M, C]): random patterns; by hand y = NaN, -0, +inf, -inf, +0, a negative NaN at the front and at
    the end of the buffer, against gradients that are ordinary numbers there (a NaN y must pass them)"""
    n = M * C
    y, dy = bf16_rne(random_bits(n, 500 + n)), bf16_rne(random_bits(n, 501 + n))
    hand = np.array([0x7FC0, 0x8000, 0x7F80, 0xFF80, 0x0000, 0xFFC1], dtype=np.uint16)
    grad = bits_of(np.array([1.5, 2.5, -3.0, 4.0, 5.0, -6.0], dtype=np.float32))
    for at in ((0, n - 6) if n >= 12 else (0,)):
        y[at:at + 6], dy[at:at + 6] = hand, grad
    return y.reshape(M, C), dy.reshape(M, C)


@functools.lru_cache(maxsize=None)
def chanscale_case(B, HW, C):
    """-> (x [B, HW, C] planted normal draws, keep float32 [B, C]: 0, 1 / (1 - p) for p = 0.2 and other factors)"""
    rng = np.random.default_rng(600 + B * HW * C)
    keep = rng.choice(np.array([0.0, 1.25, 1.0, 2.0, 0.3, -1.7], dtype=np.float32), (B, C)).astype(np.float32)
    keep[0, :2] = (0.0, 1.25)
    return planted_draw((B, HW, C), 601 + B * HW * C), keep


@functools.lru_cache(maxsize=None)
def im2col_image(case):
    """random fp32 patterns [B, C, H, W] with the special patterns of update_reference"""
    B, C, H, W = case[:4]
    return random_bits(B * C * H * W, 700 + sum(case)).reshape(B, C, H, W)


def quarter_bits(q):
    """integer array q (|q| <= 64) -> the bf16 patterns of q / 4, through a table: the cap cases hold up to 2^27 elements"""
    lut = b16(np.arange(-64, 65, dtype=np.float32) * np.float32(0.25))
    return lut[np.asarray(q).astype(np.int16) + 64]


def small_int_draw(shape, seed, lim):
    """-> int8 integers in [-lim, lim]"""
    return np.random.default_rng(seed).integers(-lim, lim + 1, shape, dtype=np.int8)


def stats_prefill(n, seed):
    """non-zero int64 words: the kernels ADD to what the buffer holds"""
    v = np.random.default_rng(seed).integers(1, 1 << 30, n, dtype=np.int64)
    return v * np.where(np.arange(n) & 1, -1, 1)


@functools.lru_cache(maxsize=None)
def colstats_case(C, draw):
    """float32 [300, C]: the rows of every M; 'integer' in [-8, 8] (the words are exact), 'general' normal through bf16"""
    f = integer_draw if draw == "integer" else general_draw
    return f((max(COLSTATS_M), C), 1000 + C)
