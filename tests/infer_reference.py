"""References, draws and case tables of the inference kernels of csrc/infer.hip: ep24_bn_act_infer, ep24_fold_bn, ep24_head_decode_eval,
ep24_post_prepare, ep24_post_nms (with nms_compact_sort of csrc/nms_sort.h) and ep24_post_gather.  A helper, not a test module:
tests/test_infer_reference.py checks it on the CPU (against torch's batch_norm and conv2d, the oracle's eval decode and postprocess,
the conditions on every draw, the float32 emulations against the bounds, and that every mutant is rejected),
tests/test_gpu_infer_exact.py runs the kernels against it.  It never imports the package under test.

Every kernel but the decode's expf and the SiLU is a chain of separate IEEE fp32 operations (the library is built without
contraction and without fast-math), so each reference is a float32 numpy emulation in the kernel's own operation order that the
device must match bit for bit; float64 forms stand beside it where a bound is used.  What is compared bit for bit travels as bit
patterns (update_reference.bits32, bf16_rne), NaN equal to NaN.
"""
import fractions
import functools
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bn_reference as BN  # noqa: E402
from glue_reference import b16, bf  # noqa: E402
from update_reference import SENT16, SENT32, bits32, from_bits32, random_bits  # noqa: E402

f32 = np.float32
TWO128 = 2.0 ** 128               # what rounds to +inf in fp32 (the largest number is 2^128 - 2^104)


# ---------------------------------------------------------------------------------------------------------------------------
# (a) fp32 helpers
def _fraction_to_f32(q):
    """an exact rational -> the nearest fp32 number, ties to even"""
    x = f32(float(q))
    cands = [np.nextafter(x, f32(-np.inf)), x, np.nextafter(x, f32(np.inf))]
    return min(cands, key=lambda c: (abs(fractions.Fraction(float(c)) - q), int(np.array([c], dtype=f32).view(np.uint32)[0]) & 1))


def fma32(a, b, c):
    """fmaf(a, b, c) for a with at most 8 significant bits (a bf16 number): the product is exact in float64 (8 + 24 bits), the sum is
    rounded to float64 and then to fp32.  The two roundings differ from one only where the float64 sum is inexact AND sits exactly
    between two fp32 numbers; those elements are redone in rational arithmetic.  -> (fp32 array, number of elements redone)"""
    a64, b64, c64 = np.broadcast_arrays(np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64), np.asarray(c, dtype=np.float64))
    with np.errstate(all="ignore"):
        p = a64 * b64
        s = p + c64
        bb = s - p
        err = (p - (s - bb)) + (c64 - bb)                              # TwoSum: p + c = s + err exactly
        r = s.astype(f32)
        r64 = r.astype(np.float64)
        nb = np.nextafter(r, np.where(s > r64, f32(np.inf), f32(-np.inf)).astype(f32)).astype(np.float64)
        tie = np.isfinite(s) & (err != 0) & (s != r64) & (s == 0.5 * (r64 + nb))
    idx = np.flatnonzero(tie.reshape(-1))
    if idx.size:
        r = r.copy()
        flat = r.reshape(-1)
        for i in idx:
            q = fractions.Fraction(float(a64.reshape(-1)[i])) * fractions.Fraction(float(b64.reshape(-1)[i])) + fractions.Fraction(float(c64.reshape(-1)[i]))
            flat[i] = _fraction_to_f32(q)
    return r, int(idx.size)


def ulp32(x):
    """the spacing of fp32 numbers at |x| (float64 in and out), 2^-149 in the denormal range"""
    _, e = np.frexp(np.abs(np.asarray(x, dtype=np.float64)))
    with np.errstate(all="ignore"):
        return np.maximum(np.ldexp(1.0, np.maximum(e, -2000) - 24), 2.0 ** -149)


def exact_class(want):
    """where a float64 reference value leaves no room: NaN, an infinity, 0, 1, or beyond the fp32 range (the fp32 answer is inf)"""
    want = np.asarray(want, dtype=np.float64)
    with np.errstate(all="ignore"):
        return np.isnan(want) | np.isinf(want) | (want == 0) | (want == 1) | (np.abs(want) >= TWO128)


def err_in_units(got, want, unit):
    """got fp32, want / unit float64 -> (largest |got - want| / unit over the elements outside exact_class, the number of elements
    inside exact_class whose fp32 pattern is not the one of want rounded to fp32; NaN for NaN)"""
    got = np.asarray(got, dtype=f32)
    want = np.asarray(want, dtype=np.float64)
    ex = exact_class(want)
    with np.errstate(all="ignore"):
        w32 = want.astype(f32)
        ratio = np.abs(got.astype(np.float64) - want) / unit
    ratio = np.where(np.isfinite(got), ratio, np.inf)
    worst = float(ratio[~ex].max()) if (~ex).any() else 0.0
    gb, wb = bits32(got).reshape(-1)[ex.reshape(-1)], bits32(w32).reshape(-1)[ex.reshape(-1)]
    nan = np.isnan(got).reshape(-1)[ex.reshape(-1)] & np.isnan(w32).reshape(-1)[ex.reshape(-1)]
    return worst, int(((gb != wb) & ~nan).sum())


# ---------------------------------------------------------------------------------------------------------------------------
# (b) ep24_bn_act_infer: y = bf16(act(fma(z, scale, shift)) + residual)
BN_SHAPES = [(1, 8), (33, 8), (130, 40), (70, 1024), (3, 8192)]       # one row; one thread per row; C no power of two; 128 groups per
#                                                                        row, more than one row per workgroup pass; the LDS limit (64 KiB)
BN_CAP = (2049, 4096)                                                 # 2049 x 512 = 1 049 088 items > 2048 workgroups x 512
BN_MAX_BLOCKS, BN_ITEMS_PER_BLOCK = 2048, 512
BN_MAX_C = 8192
BN_LAYOUTS = {"dense": (0, 0, 0), "strided": (8, 24, 16)}              # ld - C of z, y, residual
BN_EPS = {(1, 8): 1e-3, (33, 8): 1e-5, (130, 40): 1e-3, (70, 1024): 1e-5, (3, 8192): 1e-3, BN_CAP: 1e-5}


def bn_grid(M, C):
    """workgroups of 256 lanes, one 8-channel item per lane and trip: the host asks for half as many lanes as items"""
    return min(BN_MAX_BLOCKS, (M * (C // 8) + BN_ITEMS_PER_BLOCK - 1) // BN_ITEMS_PER_BLOCK)


@functools.lru_cache(maxsize=2)
def bn_draw(M, C):
    """-> dict(z, res: bf16-valued float32 [M, C]; gamma, beta, mean, var: float32 [C]; eps).  Both signs of gamma; var = 0 in the
    channels 3, 11, ...; a NaN, a +inf and a -inf element in z (in three different channels of the first and last row)."""
    rng = np.random.default_rng(9000 + M * 31 + C)
    z = bf(rng.standard_normal((M, C), dtype=f32) * f32(1.5) + f32(0.25))
    res = bf(rng.standard_normal((M, C), dtype=f32))
    gamma = ((rng.random(C, dtype=f32) + f32(0.5)) * np.where(rng.integers(0, 2, C) > 0, f32(1), f32(-1))).astype(f32)
    gamma[:2] = (f32(0.75), f32(-1.25))
    beta = (rng.random(C, dtype=f32) - f32(0.5)).astype(f32)
    mean = (rng.standard_normal(C, dtype=f32) * f32(0.5)).astype(f32)
    var = (rng.random(C, dtype=f32) + f32(0.5)).astype(f32)
    var[3::8] = 0
    z[0, 1], z[M - 1, 5], z[M - 1, 6] = np.nan, np.inf, -np.inf
    return dict(z=z, res=res, gamma=gamma, beta=beta, mean=mean, var=var, eps=float(f32(BN_EPS[(M, C)])))


def bn_consts32(gamma, beta, mean, var, eps):
    """scale = fl(gamma / fl(sqrt(fl(var + eps)))), shift = fl(beta - fl(mean * scale))"""
    with np.errstate(all="ignore"):
        scale = (gamma / np.sqrt((var + f32(eps)).astype(f32)).astype(f32)).astype(f32)
        shift = (beta - (mean * scale).astype(f32)).astype(f32)
    return scale, shift


@functools.lru_cache(maxsize=1)
def bn_case(M, C):
    """-> (draw, scale, shift, u = fmaf(z, scale, shift)) of a shape, shared by its layouts and forms (read-only)"""
    d = bn_draw(M, C)
    sc, sh = bn_consts32(d["gamma"], d["beta"], d["mean"], d["var"], d["eps"])
    return d, sc, sh, fma32(d["z"], sc[None, :], sh[None, :])[0]


def bn_consts64(gamma, beta, mean, var, eps):
    g, b, m, v = (np.asarray(a, dtype=np.float64) for a in (gamma, beta, mean, var))
    scale = g / np.sqrt(v + float(eps))
    return scale, b - m * scale


def act32(u, act):
    """The activation in fp32.  ReLU as ATen writes it (u < 0 -> +0: NaN stays NaN, -0 stays -0); SiLU through bn_reference's
    exp2 / reciprocal emulation, which is compared under a bound only."""
    with np.errstate(all="ignore"):
        if act == 1:
            return BN._act32(u, 1)
        if act == 2:
            return np.where(u < 0, f32(0), u).astype(f32)
        if act == 3:
            return np.where(u > 0, u, (f32(0.1) * u).astype(f32)).astype(f32)
    return u


def act64(u, act):
    with np.errstate(all="ignore"):
        if act == 1:
            return u / (1.0 + np.exp(-u))
        if act == 2:
            return np.where(u < 0, 0.0, u)
        if act == 3:
            return np.where(u > 0, u, 0.1 * u)
    return u


def bn_act_infer_ref(u, act, res=None, res_first=False):
    """u = fma32(z, scale, shift)[0] (shared by the forms of one shape) -> bf16 bit patterns, shape of u.  Without a residual the
    kernel still adds +0: a -0 becomes +0.  res_first (mutant): the residual goes through the activation."""
    with np.errstate(all="ignore"):
        r = f32(0) if res is None else res.astype(f32)
        a = act32((u + r).astype(f32), act) if res_first else (act32(u, act) + r).astype(f32)
    return b16(a).reshape(u.shape)


def bn_act_infer_ref64(z, scale, shift, act, res=None):
    """float64: act(z * scale + shift) + residual, scale / shift as given (float64 of bn_consts64, or the fp32 emulation's)"""
    with np.errstate(all="ignore"):
        u = z.astype(np.float64) * np.asarray(scale, dtype=np.float64)[None, :] + np.asarray(shift, dtype=np.float64)[None, :]
        a = act64(u, act)
        return u, a, (a if res is None else a + res.astype(np.float64))


def bn_tol(z, scale, shift, mean, beta, a64, y64, act):
    """bn_reference.tol_y for the eval form: scale and shift are the emulation's own numbers, so invstd carries no error of its own
    (E[z^2] = 0 in eps_c leaves its 2^-22); what remains is the fma's rounding, the SiLU's exp / rcp (S_SILU), the fp32 addition of the
    residual and the bf16 rounding."""
    t = lambda a: torch.from_numpy(np.ascontiguousarray(np.asarray(a, dtype=np.float64)))
    sc = t(scale)
    with np.errstate(all="ignore"):
        mean_eff = np.where(np.asarray(scale) != 0, (np.asarray(beta, dtype=np.float64) - np.asarray(shift, dtype=np.float64)) / np.asarray(scale, dtype=np.float64), 0.0)
    r = dict(sc=sc, y=t(np.nan_to_num(y64, nan=0.0, posinf=0.0, neginf=0.0)), a=t(np.nan_to_num(a64, nan=0.0, posinf=0.0, neginf=0.0)),
             mean=t(mean_eff), ez2=torch.zeros_like(sc), var=torch.ones_like(sc))
    zz = t(np.nan_to_num(z.astype(np.float64), nan=0.0, posinf=0.0, neginf=0.0))
    return BN.tol_y(r, zz, t(beta), act).numpy()


def strided(img_rows, ld, C, pad=SENT16):
    """uint16 [M, C] -> the flat image of [M, ld] rows whose pad columns hold `pad`"""
    M = img_rows.shape[0]
    img = np.full((M, ld), pad, dtype=np.uint16)
    img[:, :C] = img_rows
    return img.reshape(-1)


# ---------------------------------------------------------------------------------------------------------------------------
# (c) ep24_fold_bn.  desc[s] = {master offset, packed offset, Cout, T, Cin, Cin_pad, gamma offset, beta offset (flat), running-mean
# offset, running-var offset (bstat), bias offset, 0} (include/ep24.h); prefix / cprefix = running sums of Cout T Cin / Cout.
FOLD_CHUNK = 1024                                                     # elements per workgroup and trip
FOLD_CAP = 8192 * FOLD_CHUNK                                          # 8 388 608: one trip of the weights kernel
# (Cout, T, Cin, Cin_pad).  Elements 24, 96, 1000, 928, 1024, 1048, 108, 216, 1152, 120, 24, 1008: the segments start at 0, 24, 120, 1120,
# 2048 (a chunk base), 3072 (another), 4120, 4228, 4444, 5596, 5716, 5740 and end at 6748 = 6 x 1024 + 604 (a partial last chunk).  Chunk
# 0 holds three segments, chunk 4 = [4096, 5120) four.  Cin = 3 / 12 / 116 are padded to 8 / 16 / 120; T = 9 with and without a pad.
# 445 channels: two workgroups of the bias kernel, the second partial.
FOLD_SMALL = [(8, 1, 3, 8), (8, 1, 12, 16), (125, 1, 8, 8), (8, 1, 116, 120), (128, 1, 8, 8), (131, 1, 8, 8), (4, 9, 3, 8), (2, 9, 12, 16),
              (16, 9, 8, 8), (5, 1, 24, 24), (3, 1, 8, 8), (7, 9, 16, 16)]
FOLD_SMALL_EPS = [1e-3, 1e-5, 0.5, 0.0, 1e-2, 2e-3, 1e-4, 0.25, 3e-3, 1e-6, 0.125, 5e-3]
# 8 384 512 elements in two segments, then (9, 1, 512) across the cap (512 of its elements beyond it), then two short segments: the second
# trip's only chunk [8 388 608, 8 389 244) holds three segments, one of them padded
FOLD_BIG = [(1024, 1, 4096, 4096), (1023, 1, 4096, 4096), (9, 1, 512, 512), (5, 1, 12, 16), (8, 1, 8, 8)]
FOLD_BIG_EPS = [1e-3, 1e-5, 0.5, 0.0, 1e-2]
FOLD_ONE = [(8, 1, 12, 16)]
FOLD_ONE_EPS = [1e-3]
FOLD_LAYOUTS = {"small": (FOLD_SMALL, FOLD_SMALL_EPS), "big": (FOLD_BIG, FOLD_BIG_EPS), "one": (FOLD_ONE, FOLD_ONE_EPS)}


class FoldLayout:
    pass


def _place(sizes, order, gap, start=0):
    """offsets of the blocks `sizes`, laid out one behind the other in `order` with `gap` unused elements between them"""
    off, at = [0] * len(sizes), start
    for s in order:
        off[s] = at
        at += sizes[s] + gap
    return off, at


@functools.lru_cache(maxsize=None)
def fold_layout(name):
    """The seven tables (masters, gamma, beta in flat; mean, var in bstat; the packed weights; the bias) each in an order of its own,
    so a wrong d[k] lands on another segment's data; 8 / 1 sentinel elements between the packed segments / the bias vectors."""
    segs, eps = FOLD_LAYOUTS[name]
    n = len(segs)
    rng = np.random.default_rng(77 + n)
    orders = []
    while len(orders) < 7:
        p = tuple(rng.permutation(n))
        if n == 1 or p not in orders:
            orders.append(p)
    numel = [co * t * ci for co, t, ci, _ in segs]
    packed = [co * t * cp for co, t, _, cp in segs]
    chans = [co for co, _, _, _ in segs]
    L = FoldLayout()
    m_off, at = _place(numel, orders[0], 3)
    g_off, at = _place(chans, orders[1], 1, at)
    b_off, L.flat_n = _place(chans, orders[2], 1, at)
    mu_off, at = _place(chans, orders[3], 1)
    v_off, L.bstat_n = _place(chans, orders[4], 1, at)
    p_off, L.wf_n = _place(packed, orders[5], 8, 8)
    bi_off, L.bias_n = _place(chans, orders[6], 1, 1)
    L.segs, L.n_seg, L.orders = segs, n, orders
    L.desc = np.array([[m_off[s], p_off[s], segs[s][0], segs[s][1], segs[s][2], segs[s][3], g_off[s], b_off[s], mu_off[s], v_off[s], bi_off[s], 0]
                       for s in range(n)], dtype=np.int64)
    L.prefix = np.concatenate([[0], np.cumsum(numel)]).astype(np.int64)
    L.cprefix = np.concatenate([[0], np.cumsum(chans)]).astype(np.int64)
    L.total, L.total_channels = int(L.prefix[-1]), int(L.cprefix[-1])
    L.eps = np.array(eps, dtype=f32)
    return L


@functools.lru_cache(maxsize=2)
def fold_draw(name):
    """-> (flat, bstat) float32: normal masters and means, |gamma| in [0.5, 1.5) with both signs, var in [0.5, 1.5) (eps = 0 is among
    the eps), everything outside a table NaN"""
    L = fold_layout(name)
    rng = np.random.default_rng(78 + L.n_seg)
    flat = np.full(L.flat_n, np.nan, dtype=f32)
    bstat = np.full(L.bstat_n, np.nan, dtype=f32)
    for d in L.desc:
        mo, _, co, t, ci, _, go, bo, mu, vo, _, _ = (int(v) for v in d)
        flat[mo:mo + co * t * ci] = rng.standard_normal(co * t * ci, dtype=f32)
        flat[go:go + co] = (rng.random(co, dtype=f32) + f32(0.5)) * np.where(rng.integers(0, 2, co) > 0, f32(1), f32(-1))
        flat[bo:bo + co] = rng.random(co, dtype=f32) - f32(0.5)
        bstat[mu:mu + co] = rng.standard_normal(co, dtype=f32)
        bstat[vo:vo + co] = rng.random(co, dtype=f32) + f32(0.5)
    return flat, bstat


def fold_bn_ref(L, flat, bstat, mutant=None):
    """-> (packed weights uint16 [wf_n], bias uint32 [bias_n]) as bit images that hold the sentinel wherever the call must not write:
    the Cin_pad - Cin pad columns, the gaps between the segments.  w' = bf16(fl(w * scale[co])), bias = fl(beta - fl(mean * scale)).
    mutant: 'eps0', 'stride_cin', 'co_cin_pad', 'bias_var_for_mean', 'one_trip'."""
    wf = np.full(L.wf_n, SENT16, dtype=np.uint16)
    bias = np.full(L.bias_n, SENT32, dtype=np.uint32)
    for s, d in enumerate(L.desc):
        mo, po, co, t, ci, cp, go, bo, mu, vo, bi, _ = (int(v) for v in d)
        eps = L.eps[0 if mutant == "eps0" else s]
        with np.errstate(all="ignore"):
            scale = (flat[go:go + co] / np.sqrt((bstat[vo:vo + co] + eps).astype(f32)).astype(f32)).astype(f32)
            mean = bstat[vo:vo + co] if mutant == "bias_var_for_mean" else bstat[mu:mu + co]
            bias[bi:bi + co] = bits32((flat[bo:bo + co] - (mean * scale).astype(f32)).astype(f32))
            e = np.arange(co * t * ci, dtype=np.int64)
            ch = e // (t * (cp if mutant == "co_cin_pad" else ci))
            vals = b16((flat[mo:mo + co * t * ci] * scale[ch]).astype(f32))
        dst = po + (e // ci) * (ci if mutant == "stride_cin" else cp) + e % ci
        if mutant == "one_trip":
            keep = (L.prefix[s] + e) < FOLD_CAP
            dst, vals = dst[keep], vals[keep]
        wf[dst] = vals
    return wf, bias


# ---------------------------------------------------------------------------------------------------------------------------
# (d) ep24_head_decode_eval, in place on the rows [a0, a0 + H W) of every image of out [B, A, ncols]
DECODE_MAPS = [(3, 5), (4, 4), (1, 7)]
DECODE_STRIDES = [8.0, 16.0, 32.0]
DECODE_NCOLS = [27, 28, 107]
DECODE_A0, DECODE_TAIL = 5, 4
DECODE_CAP = (1, 99, 100, 107)                                        # (B, H, W, ncols): 1 059 300 elements > 4096 workgroups x 256
DECODE_MAX_ITEMS = 4096 * 256
PLANTED = [100.0, -100.0, 88.8, -88.8, 0.0, -0.0, np.nan, np.inf, -np.inf]


@functools.lru_cache(maxsize=None)
def decode_case(B, H, W, ncols):
    """raw float32 [B, A, ncols], A = 5 + H W + 4: random bit patterns in the rows outside the map, t = k / 1024 (|t| <= 4) in every
    column of the map's rows, and each PLANTED logit in radii columns and in score columns (first, last and one in between) of a
    cell of its own, counted from the first cell of the last image"""
    A = DECODE_A0 + H * W + DECODE_TAIL
    raw = from_bits32(random_bits(B * A * ncols, 600 + ncols + H * W)).reshape(B, A, ncols).copy()
    k = np.random.default_rng(601 + ncols + H * W).integers(-4096, 4097, (B, H * W, ncols))
    raw[:, DECODE_A0:DECODE_A0 + H * W] = (k / 1024.0).astype(f32)
    cols = sorted({2, 13, 25, 26, 27 if ncols > 27 else 26, ncols - 1})
    assert B * H * W >= len(PLANTED)
    for i, v in enumerate(PLANTED):                                      # one cell per planted value, in every chosen column
        raw[B - 1 - i // (H * W), DECODE_A0 + i % (H * W), cols] = v
    return raw


def decode_eval_ref(raw, a0, H, W, s, swap_xy=False, sig_from=26):
    """-> (out float32 [B, A, ncols]: the fp32 emulation - columns 0 and 1 are what the device must give bit for bit, the radii and
    scores numpy's expf stands in for the device's; radii float64 [B, H W, 24] = s exp(t); scores float64 [B, H W, ncols - 26] =
    1 / (1 + exp(-t))).  A sigmoid whose expf(-t) overflows is expf(t): the quotient 1 / (1 + inf) would be 0 where the answer is a
    denormal number.  swap_xy / sig_from (mutants): x from hw / W, the sigmoid one column late."""
    out = raw.copy()
    hw = np.arange(H * W)
    gx, gy = (hw % W).astype(f32), (hw // W).astype(f32)
    if swap_xy:
        gx, gy = gy, gx
    lvl = raw[:, a0:a0 + H * W]
    s32 = f32(s)
    with np.errstate(all="ignore"):
        out[:, a0:a0 + H * W, 0] = (lvl[..., 0] + gx).astype(f32) * s32
        out[:, a0:a0 + H * W, 1] = (lvl[..., 1] + gy).astype(f32) * s32
        out[:, a0:a0 + H * W, 2:sig_from] = np.exp(lvl[..., 2:sig_from]).astype(f32) * s32
        t = lvl[..., sig_from:]
        e = np.exp(-t).astype(f32)
        out[:, a0:a0 + H * W, sig_from:] = np.where(np.isinf(e), np.exp(t).astype(f32), f32(1) / (f32(1) + e)).astype(f32)
        radii = float(s) * np.exp(lvl[..., 2:26].astype(np.float64))
        scores = 1.0 / (1.0 + np.exp(-lvl[..., 26:].astype(np.float64)))
    return out, radii, scores


def decode_errors(got_lvl, raw_lvl, s, radii, scores):
    """got_lvl / raw_lvl: the map's rows [B, H W, ncols].  -> (radii err in units of s ulp(exp t), wrong exact radii, score err in ulp,
    wrong exact scores).  The radii's unit is the issue's `2 ulp of s exp(t)` wherever exp(t) is a normal fp32 number (s is a power of two);
    below, the product cannot be closer than expf's own denormal spacing times s."""
    with np.errstate(all="ignore"):
        unit_r = float(s) * ulp32(np.exp(raw_lvl[..., 2:26].astype(np.float64)))
    er, br = err_in_units(got_lvl[..., 2:26], radii, unit_r)
    es, bs = err_in_units(got_lvl[..., 26:], scores, ulp32(scores))
    return er, br, es, bs


RADII_ULP, SCORE_ULP = 2.0, 3.0


# ---------------------------------------------------------------------------------------------------------------------------
# (e) postprocess: prepare, NMS, gather
def ray_factors():
    """theta_k cos(theta_k), theta_k sin(theta_k) as the product's host code and the oracle form them (fp32 torch)"""
    theta = torch.arange(24) * torch.tensor(15 * 3.141592653589793 / 180)
    return torch.cat((theta * torch.cos(theta), theta * torch.sin(theta))).float().numpy()


PREP_C = [1, 2, 80]
PREP_N = [1, 255, 257, 1000]
PREP_CAP = (1048576 + 300, 1)                                          # rows beyond 4096 workgroups x 256
PREP_MAX_ROWS = 4096 * 256
CONF_THRE = 0.25


@functools.lru_cache(maxsize=2)
def prepare_draw(N, C):
    """pred float32 [N, 27 + C]: centres in [0, 640), radii in [1, 50), objectness and class scores in [0, 1).  Row i with i % 16 =
    1: all classes equal; 2: the maximum at two places; 3: obj * conf = 0.25 in bits; 4: one ulp below; 5: NaN in class column 0; 6:
    NaN in the last class column; 7: NaN objectness; 8: negative radii among the 24; 9: all radii zero; 10: NaN in class column 0 and
    a larger number behind it."""
    rng = np.random.default_rng(8000 + N + C)
    p = rng.random((N, 27 + C), dtype=f32)
    p[:, 0:2] *= f32(640)
    p[:, 2:26] = p[:, 2:26] * f32(49) + f32(1)
    i = np.arange(N) % 16
    cls = p[:, 27:]
    cls[i == 1] = f32(0.625)
    if C >= 2:
        top = cls[i == 2].max(1)
        cls[i == 2, 0] = top
        cls[i == 2, C - 1] = top
    for k, obj in ((3, f32(0.5)), (4, np.nextafter(f32(0.5), f32(0)))):
        cls[i == k] = np.minimum(cls[i == k], f32(0.5))
        cls[i == k, C - 1] = f32(0.5)
        p[i == k, 26] = obj
    cls[i == 5, 0] = np.nan
    cls[i == 6, C - 1] = np.nan
    p[i == 7, 26] = np.nan
    p[i == 8, 2:26:3] *= f32(-1)
    p[i == 9, 2:26] = 0
    cls[i == 10, 0] = np.nan
    if C >= 2:
        cls[i == 10, 1] = f32(0.99)
    return p


def post_prepare_ref(pred, C, conf_thre, ray, last_max=False, strict=False):
    """-> (score, conf float32 [N], cls int32 [N], rect float32 [N, 4]) as the kernel forms them: the scan over the classes starts at
    column 27 and moves on only to a GREATER number (the first maximum; a NaN is never greater, a leading NaN stays); score = fl(obj *
    conf) where >= conf_thre, else -1 (NaN: -1); the rectangle is fminf / fmaxf over fl(fl(r_k * ray_k) + c).  last_max / strict
    (mutants): >= in the scan / > at conf_thre."""
    pred = np.asarray(pred, dtype=f32)
    best = pred[:, 27].copy()
    bi = np.zeros(pred.shape[0], dtype=np.int32)
    with np.errstate(all="ignore"):
        for c in range(1, C):
            col = pred[:, 27 + c]
            take = (col >= best) if last_max else (col > best)
            best = np.where(take, col, best)
            bi = np.where(take, np.int32(c), bi)
        sc = (pred[:, 26] * best).astype(f32)
        ok = (sc > f32(conf_thre)) if strict else (sc >= f32(conf_thre))
        score = np.where(ok, sc, f32(-1)).astype(f32)
        px = ((pred[:, 2:26] * ray[None, :24]).astype(f32) + pred[:, 0:1]).astype(f32)
        py = ((pred[:, 2:26] * ray[None, 24:]).astype(f32) + pred[:, 1:2]).astype(f32)
        inf = f32(np.inf)
        rect = np.stack([np.fmin.reduce(px, axis=1, initial=inf), np.fmin.reduce(py, axis=1, initial=inf),
                         np.fmax.reduce(px, axis=1, initial=-inf), np.fmax.reduce(py, axis=1, initial=-inf)], axis=1).astype(f32)
    return score, best.astype(f32), bi, rect


def iou32(a, b):
    """the IoU of nms_kernel, a [4] against b [n, 4], every operation in fp32"""
    a, b = np.asarray(a, dtype=f32), np.asarray(b, dtype=f32).reshape(-1, 4)
    with np.errstate(all="ignore"):
        aarea = (a[2] - a[0]) * (a[3] - a[1])
        iw = np.fmax(np.fmin(a[2], b[:, 2]) - np.fmax(a[0], b[:, 0]), f32(0))
        ih = np.fmax(np.fmin(a[3], b[:, 3]) - np.fmax(a[1], b[:, 1]), f32(0))
        inter = iw * ih
        return inter / ((aarea + (b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1])) - inter)


def nms_ref(score, cls, rect, thr, agnostic, ge=False, non_greedy=False, tie_desc=False, drop_class=False):
    """One image: the rows with score >= 0 (NaN is none, -0.0 is one and equals 0.0) by (score descending, row ascending); a row that is
    alive is kept and kills every later row of its class (of any class: agnostic) with iou32 > thr; a dead row kills nobody.  -> kept
    rows int32.  Mutants: ge (>= thr), non_greedy (a dead row kills too), tie_desc (ties by descending row), drop_class."""
    s = np.asarray(score, dtype=f32)
    with np.errstate(all="ignore"):
        cand = np.flatnonzero(s >= 0)
    key = s[cand] + f32(0)
    order = cand[np.lexsort(((-cand if tie_desc else cand), -key))]
    r, c = np.asarray(rect, dtype=f32).reshape(-1, 4)[order], np.asarray(cls)[order]
    n = order.size
    dead = np.zeros(n, dtype=bool)
    keep = []
    thr = f32(thr)
    for i in range(n):
        if dead[i] and not non_greedy:
            continue
        if not dead[i]:
            keep.append(order[i])
        iou = iou32(r[i], r[i + 1:])
        with np.errstate(all="ignore"):
            hit = (iou >= thr) if ge else (iou > thr)
        if not (agnostic or drop_class):
            hit &= c[i + 1:] == c[i]
        dead[i + 1:] |= hit
    return np.array(keep, dtype=np.int32)


def gather_ref(pred, conf, cls, keep, swap=False):
    """-> det float32 [n, 29] = (pred[keep, :27], conf[keep], float(cls[keep]));  swap (mutant): the last two exchanged"""
    keep = np.asarray(keep, dtype=np.int64)
    a, b = conf[keep].astype(f32), cls[keep].astype(f32)
    if swap:
        a, b = b, a
    return np.concatenate([pred[keep, :27], a[:, None], b[:, None]], axis=1).astype(f32)


def postprocess_ref(pred, C, conf_thre, nms_thre, agnostic):
    """pred float32 [B, A, 27 + C] -> list of B entries, None or det [n, 29]: the three stages one after the other"""
    B, A, ncols = pred.shape
    ray = ray_factors()
    score, conf, cls, rect = post_prepare_ref(pred.reshape(B * A, ncols), C, conf_thre, ray)
    out = []
    for b in range(B):
        sl = slice(b * A, (b + 1) * A)
        keep = nms_ref(score[sl], cls[sl], rect[sl], nms_thre, agnostic)
        out.append(gather_ref(pred[b], conf[sl], cls[sl], keep) if keep.size else None)
    return out


# the NMS cases: (name, A, P, candidates per image, draw).  1024 lanes stride over the rows and the candidates: 1023 / 1024 / 1025 and
# 2049 = two strides + 1; the bitonic network pads n to the next power of two (1025 -> 2048, 2049 -> 4096 = P); A = 1024 with P = A, and
# P > A for A = 7 (8), 1024 (2048) and 2100 (4096); an image without candidates between two full ones.
NMS_CASES = [
    ("one-row", 1, 1, [0, 1], "general"),
    ("seven", 7, 8, [2, 0, 7, 1], "general"),
    ("full-empty-full", 1024, 1024, [1024, 0, 1023], "general"),
    ("two-strides", 2100, 4096, [2049, 1025], "general"),
    ("all-equal", 1024, 2048, [1024, 1023, 2], "equal"),
    ("zeros", 2100, 4096, [1025, 7], "zeros"),
]
NMS_THRE = 0.5
NMS_THRE_BELOW = float(np.nextafter(f32(0.5), f32(0)))
# hand-made images, A = 3, P = 4 (row: score, class, rectangle)
EDGE_IMAGES = {
    "threshold pair": [(0.9, 0, (0, 0, 2, 2)), (0.8, 0, (0, 0, 2, 1)), (-1.0, 0, (0, 0, 2, 2))],          # IoU = 2 / 4 exactly
    "degenerate pair": [(0.9, 1, (3, 3, 3, 3)), (np.nan, 1, (3, 3, 3, 3)), (0.9, 1, (3, 3, 3, 3))],         # 0 / 0: both kept
    "chain": [(0.8, 2, (3, 0, 13, 10)), (0.7, 2, (6, 0, 16, 10)), (0.9, 2, (0, 0, 10, 10))],                # rows 2, 0, 1 = A, B, C
    "cross-class pair": [(0.6, 0, (0, 0, 8, 8)), (0.7, 1, (0, 0, 8, 8)), (-0.0, 0, (100, 100, 101, 101))],
}


def edge_images():
    """-> score [4, 3], cls [4, 3], rect [4, 3, 4]"""
    rows = [EDGE_IMAGES[k] for k in EDGE_IMAGES]
    score = np.array([[r[0] for r in im] for im in rows], dtype=f32)
    cls = np.array([[r[1] for r in im] for im in rows], dtype=np.int32)
    rect = np.array([[r[2] for r in im] for im in rows], dtype=f32)
    return score, cls, rect


def nms_image(A, n, draw, seed):
    """-> score [A], cls [A], rect [A, 4].  n candidates at random rows; the other rows hold -1 or NaN alternately.  Boxes in clusters:
    about four candidates share a 100-pixel cell, 40 +- 6 pixels wide, centres within +-8 - most pairs of a cell overlap beyond 0.5.
    general: scores k / 64 (many ties); equal: all 0.5; zeros: 0.0 and -0.0 mixed."""
    rng = np.random.default_rng(seed)
    score = np.where(np.arange(A) % 2 == 0, f32(-1), f32(np.nan)).astype(f32)
    rows = rng.permutation(A)[:n]
    if draw == "general":
        score[rows] = (rng.integers(20, 64, n) / 64.0).astype(f32)
    elif draw == "equal":
        score[rows] = f32(0.5)
    else:
        score[rows] = np.where(rng.integers(0, 2, n) > 0, f32(0.0), f32(-0.0))
    cells = max(1, n // 4)
    cell = rng.integers(0, cells, A)
    cx = (cell % 64) * 100.0 + rng.uniform(-8, 8, A)
    cy = (cell // 64) * 100.0 + rng.uniform(-8, 8, A)
    w, h = 40.0 + rng.uniform(-6, 6, A), 40.0 + rng.uniform(-6, 6, A)
    rect = np.stack([cx - w / 2, cy - h / 2, cx + w / 2, cy + h / 2], axis=1).astype(f32)
    return score, rng.integers(0, 3, A).astype(np.int32), rect


@functools.lru_cache(maxsize=None)
def nms_case(name):
    """-> (A, P, score [B, A], cls [B, A], rect [B, A, 4]) of a case of NMS_CASES"""
    _, A, P, ns, draw = [c for c in NMS_CASES if c[0] == name][0]
    imgs = [nms_image(A, n, draw, 5000 + 17 * b + A + n) for b, n in enumerate(ns)]
    return A, P, np.stack([i[0] for i in imgs]), np.stack([i[1] for i in imgs]), np.stack([i[2] for i in imgs])


def nms_want(score, cls, rect, thr, agnostic, sentinel, **mutant):
    """-> (keep image int32 [B, A]: the kept rows at the front of every image's row, the sentinel behind them; counts int32 [B])"""
    B, A = score.shape
    keep = np.full((B, A), sentinel, dtype=np.int32)
    count = np.zeros(B, dtype=np.int32)
    for b in range(B):
        k = nms_ref(score[b], cls[b], rect[b], thr, agnostic, **mutant)
        keep[b, :k.size] = k
        count[b] = k.size
    return keep, count


GATHER_N = [0, 1, 300, 9040]                                           # 9040 x 29 = 262 160 elements > 1024 workgroups x 256
GATHER_A, GATHER_NCOLS = 9100, 30
GATHER_MAX_ITEMS = 1024 * 256


@functools.lru_cache(maxsize=1)
def gather_draw():
    """-> (pred [A, 30] float32 random patterns, conf [A], cls int32 [A], perm: a permutation of the rows)"""
    rng = np.random.default_rng(31)
    pred = from_bits32(random_bits(GATHER_A * GATHER_NCOLS, 32)).reshape(GATHER_A, GATHER_NCOLS).copy()
    return pred, rng.random(GATHER_A, dtype=f32), rng.integers(0, 3, GATHER_A).astype(np.int32), rng.permutation(GATHER_A).astype(np.int32)


def entry_draw(second):
    """The two predictions [2, 64, 29] of the Python-entry case: clustered detections in both images; in the second call image 1 has
    nothing above the threshold."""
    rng = np.random.default_rng(41 + int(second))
    p = rng.random((2, 64, 29), dtype=f32)
    cell = rng.integers(0, 12, (2, 64))
    p[..., 0] = (cell % 4) * 100.0 + 50 + rng.uniform(-4, 4, (2, 64))
    p[..., 1] = (cell // 4) * 100.0 + 50 + rng.uniform(-4, 4, (2, 64))
    p[..., 2:26] = 20 + rng.uniform(-2, 2, (2, 64, 24))
    p[..., 26] = (rng.integers(32, 64, (2, 64)) / 64.0)
    if second:
        p[1, :, 26] = f32(0.01)
    return p.astype(f32)
