"""References, draws and cases of the fp32 parity kernels of csrc/f32path.hip, one per entry point: ep24_f32_conv (forward and
transposed), ep24_f32_conv_wgrad, ep24_f32_bn_act_fwd, _bwd, ep24_f32_spp_fwd, _bwd, ep24_f32_upsample2_fwd, _bwd, ep24_f32_rows_copy,
ep24_f32_stem_pack, ep24_f32_head_decode_bwd, ep24_f32_colsum.  A helper, not a test module: tests/test_f32_reference.py checks it on
the CPU (against torch's conv2d, batch_norm, max_pool2d, interpolate, unfold and their autograd in float64, and that every mutant of
its list is rejected by a case of the GPU test), tests/test_gpu_f32_exact.py runs the kernels against it.  It never imports the package
under test; the operations are written from include/ep24.h and the modules of the model.

Every reference computes in float64 and gives three things per output element: the float64 value, the expected fp32 bit pattern where
the rounding sequence is fixed, and the error bound of the case where it is not.  A case (`Case`) is the whole call: the bit image of
every buffer before the call, the argument list, and a `Want` per buffer - the image after the call, with the positions that are held
under a bound marked `soft`.

The bounds (class V: a float64 value v with a bound e on |computed - v|).  The kernels sum in double and round to fp32 once, so a
sum of n terms is within (n - 1) 2^-53 sum|terms| of the float64 sum before the rounding (dsum_err) and V.r() adds the rounding: half
an fp32 ulp at |v| + e.  Every further fp32 operation of the kernel's expression is one more V.r(); products and quotients carry the
errors of their operands (V.__mul__, V.__truediv__).  The library is built without FMA contraction and without fast-math, so where the
operands make every fp32 result exact - or leave one sequence of separately rounded IEEE operations on identical inputs - the bits are
fixed and numpy's float32 arithmetic gives them.  expf has no documented error figure in ROCm: as in tests/test_gpu_glue_exact.py it
is taken as within 2 ulp of its fp32 result (a relative 2^-22).

Roundings counted from the source, per case (written again beside each builder):
  conv                1 (the double sum -> fp32) + 1 with a bias in the forward form + 1 with accumulate
  conv_wgrad          2 (the double sum -> fp32, the add to dw)
  bn save             1 each;  running statistics: the statistic -> fp32, two products, one sum = 4 (1.f - momentum is a constant)
  bn y                4 for u = ((z - mean) inv) gamma + beta; + 1 for act 3 below zero; SiLU: expf, 1 + e, the quotient; + 1 with a residual
  bn dz               1 (the double expression -> fp32) on top of zh (2), u (2), the activation's gradient and du (1)
  bn sums             double: the terms' own errors + (M - 1) 2^-53 sum|terms|;  gamma_grad, beta_grad: 2 (sum -> fp32, the add)
  spp_bwd             1 + 1 with accumulate;  colsum 2;  upsample2_bwd 3 + 1 with accumulate, in the fixed order (s0 + s1) + (s2 + s3), + old
"""
import collections
import functools
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import update_reference as U  # noqa: E402
from update_reference import SENT32, bits32, from_bits32  # noqa: E402

_NP = {"f32": np.uint32, "i32": np.int32, "i64": np.int64, "f64": np.uint64}
_SENT = {"f32": SENT32, "i32": 0x5A5A5A5A, "i64": 0x5A5A5A5A5A5A, "f64": U.SENT64}
NEG = np.float32(-np.inf)
NAN = np.float32(np.nan)
EXPF_REL = 2.0 ** -22             # 2 ulp of an fp32 result
DBL = 2.0 ** -53
SECOND = 1.0 + 2.0 ** -20         # second-order terms of the double arithmetic
EPS = float(np.float32(1e-5))
F01 = np.float32(0.1)
P = collections.namedtuple("P", "buf off", defaults=(0,))     # a pointer argument: element `off` of buffer `buf`
STREAM = "stream"


def f32(a):
    return np.asarray(a, dtype=np.float32)


def f64(a):
    return np.asarray(a, dtype=np.float64)


def ulp32(v):
    """the spacing of fp32 numbers at |v| (float64); 2^-149 at zero and among the denormals"""
    v = np.abs(f64(v))
    _, e = np.frexp(v)
    return np.where(v == 0, 2.0 ** -149, np.ldexp(1.0, np.maximum(e - 24, -149)))


def dsum_err(n, mag):
    """a double sum of n terms in any order against the float64 sum"""
    return np.maximum(f64(n) - 1, 0) * DBL * f64(mag) * SECOND


class V:
    """a float64 value and a bound on |what the kernel holds - value|"""

    def __init__(self, v, e=0.0):
        self.v, self.e = [a.copy() for a in np.broadcast_arrays(f64(v), f64(e))]

    @staticmethod
    def of(x):
        return x if isinstance(x, V) else V(x)

    def __add__(self, o):
        o = V.of(o)
        return V(self.v + o.v, self.e + o.e)

    __radd__ = __add__

    def __sub__(self, o):
        o = V.of(o)
        return V(self.v - o.v, self.e + o.e)

    def __rsub__(self, o):
        return V.of(o) - self

    def __mul__(self, o):
        o = V.of(o)
        return V(self.v * o.v, np.abs(self.v) * o.e + np.abs(o.v) * self.e + self.e * o.e)

    __rmul__ = __mul__

    def __truediv__(self, o):
        o = V.of(o)
        den = np.abs(o.v) - o.e
        assert bool(np.all(den > 0) | np.any(np.isnan(den)))
        with np.errstate(all="ignore"):
            q = self.v / o.v
            return V(q, (self.e + np.abs(q) * o.e) / den)

    def __rtruediv__(self, o):
        return V.of(o) / self

    def r(self):
        """one fp32 rounding"""
        return V(self.v, self.e + 0.5 * ulp32(np.abs(self.v) + self.e))

    def d(self, ops=1):
        """`ops` double roundings"""
        return V(self.v, self.e + ops * DBL * (np.abs(self.v) + self.e))

    def sum(self, axis):
        n = self.v.shape[axis]
        return V(self.v.sum(axis), self.e.sum(axis) + dsum_err(n, (np.abs(self.v) + self.e).sum(axis)))


# ---------------------------------------------------------------------------------------------------------------------------
# (a) cases
class Want:
    """The image of one buffer after the call: `bits` everywhere, but where `soft` the float64 `val` within `bound`."""

    def __init__(self, kind, bits, val=None, bound=None, soft=None):
        self.kind = kind
        self.bits = np.ascontiguousarray(bits, dtype=_NP[kind]).reshape(-1)
        n = self.bits.size
        self.soft = np.zeros(n, dtype=bool) if soft is None else np.asarray(soft, dtype=bool).reshape(-1)
        self.val = None if val is None else f64(val).reshape(-1)
        self.bound = None if bound is None else f64(bound).reshape(-1)

    def floats(self, bits=None):
        b = self.bits if bits is None else np.ascontiguousarray(bits, dtype=_NP[self.kind])
        with np.errstate(invalid="ignore"):               # the sentinel is a signalling NaN
            return b.view(np.float32 if self.kind == "f32" else np.float64).astype(np.float64)

    def ratio(self, bits):
        """largest err / bound of an image over the soft positions (inf where it is not finite); 0 without soft positions"""
        if not self.soft.any():
            return 0.0
        g = self.floats(bits)[self.soft]
        with np.errstate(all="ignore"):
            r = np.abs(g - self.val[self.soft]) / np.maximum(self.bound[self.soft], 1e-300)
        r[~np.isfinite(g)] = np.inf
        return float(r.max())

    def hard_bits(self, got):
        """the expected image with the soft positions taken from `got`"""
        return np.where(self.soft, np.asarray(got, dtype=self.bits.dtype), self.bits)


Case = collections.namedtuple("Case", "calls bufs want exact")     # calls [(name, [args])], bufs {name: (kind, bits)}, want {name: Want}


def make_case(calls, bufs, want, exact):
    bufs = {k: (kind, np.ascontiguousarray(b, dtype=_NP[kind]).reshape(-1)) for k, (kind, b) in bufs.items()}
    for k, (kind, b) in bufs.items():                     # a buffer without a Want must come back as it went
        if k not in want:
            want[k] = Want(kind, b)
    return Case(calls, bufs, want, exact)


def rejects(true, other):
    """Does the outcome `other` (a mutant's Case) fail the comparison against `true` that the GPU test makes?"""
    for k, t in true.want.items():
        o = other.want[k]
        hard = ~t.soft
        if U.mismatches(t.bits[hard], o.bits[hard]).size or t.ratio(o.bits) > 1.0:
            return True
    return False


def sent(n, kind="f32"):
    return np.full(n, _SENT[kind], dtype=_NP[kind])


def rows(n, ld, parts, kind="f32"):
    """[n, ld] bit image: parts = [(column offset, [n, C] bits)], everything else the sentinel"""
    img = sent(n * ld, kind).reshape(n, ld)
    for off, a in parts:
        a = np.asarray(a, dtype=_NP[kind]).reshape(n, -1)
        img[:, off:off + a.shape[1]] = a
    return img


def vwant(v, exact, n, ld, off=0, bits=None):
    """Want of an f32 [n, ld] buffer whose columns off .. off + C hold V `v`: bit for bit (float32(v.v), or `bits`) if exact"""
    C = v.v.reshape(n, -1).shape[1]
    b = bits32(v.v.astype(np.float32)) if bits is None else bits
    img = rows(n, ld, [(off, b)])
    if exact:
        return Want("f32", img)
    soft = np.zeros((n, ld), dtype=bool)
    soft[:, off:off + C] = True
    val, bound = np.zeros((n, ld)), np.zeros((n, ld))
    val[:, off:off + C], bound[:, off:off + C] = v.v.reshape(n, C), v.e.reshape(n, C)
    return Want("f32", img, val, bound, soft)


# (b) draws: float64 arrays whose values are fp32 numbers
def ints(shape, seed, lo=-8, hi=8):
    return np.random.default_rng(seed).integers(lo, hi + 1, shape).astype(np.float64)


def normal(shape, seed, scale=1.0):
    return (np.random.default_rng(seed).standard_normal(shape).astype(np.float32) * np.float32(scale)).astype(np.float64)


def dyadic4(shape, seed):
    """m 2^e, |m| <= 15, -3 <= e <= 3"""
    rng = np.random.default_rng(seed)
    return rng.integers(-15, 16, shape) * np.exp2(rng.integers(-3, 4, shape))


def pick(vals, shape, seed):
    return np.random.default_rng(seed).choice(f64(vals), shape)


def draw(kind, shape, seed, scale=1.0):
    return ints(shape, seed) if kind == "int" else normal(shape, seed, scale)


def b32(a):
    return bits32(f64(a).astype(np.float32)).reshape(np.shape(a))


# ---------------------------------------------------------------------------------------------------------------------------
# (c) convolution.  Forward: y[n, oh, ow, co] = bias[co] + sum x[n, oh s + kh - p, ow s + kw - p, ci] w[co, kh k + kw, ci];
# transposed: dx[n, h, w, ci] = sum dy[n, (h + p - kh) / s, (w + p - kw) / s, co] w[co, t, ci] over the taps where both quotients are
# whole and inside the output map.  B, H, W, Cin, Cout, k, s describe the forward convolution in both forms.
def out_size(H, W, k, s):
    p = (k - 1) // 2
    return (H + 2 * p - k) // s + 1, (W + 2 * p - k) // s + 1


def read_w(wbuf, wco, wt, Cout, T, Cin, swap=False):
    """[Cout, T, Cin] of the flat weight buffer: element (co, t, ci) at co wco + t wt + ci.  swap (mutant): the strides exchanged"""
    if swap:
        wco, wt = wt, wco
    idx = np.arange(Cout)[:, None, None] * wco + np.arange(T)[None, :, None] * wt + np.arange(Cin)[None, None, :]
    return np.take(wbuf, idx, mode="wrap")


def conv_ref(x, w, H, W, k, s, transposed, mut=None):
    """x [B, SH, SW, K] (the map, or dy of the transposed form), w [Cout, T, Cin] -> (sum, sum|terms|, terms), [B, GH, GW, N].
    Rows past the end of x read as zero (only a mutant goes there)."""
    p = (k - 1) // 2
    OH, OW = out_size(H, W, k, s)
    B, SH, SW, K = x.shape
    GH, GW = (H, W) if transposed else (OH, OW)
    assert (SH, SW) == ((OH, OW) if transposed else (H, W))
    N = w.shape[2] if transposed else w.shape[0]
    flat = np.concatenate([x.reshape(-1, K), np.zeros((1, K))])
    zero_row = flat.shape[0] - 1
    gy, gx = np.meshgrid(np.arange(GH), np.arange(GW), indexing="ij")
    n = np.arange(B)[:, None, None]
    tot, mag, cnt = np.zeros((B, GH, GW, N)), np.zeros((B, GH, GW, N)), np.zeros((B, GH, GW, 1))
    for kh in range(k):
        for kw in range(k):
            t = kh * k + kw
            if not transposed:
                sy, sx = gy * s + kh - p + (1 if mut == "tap" else 0), gx * s + kw - p
                ok = (sy >= 0) & (sy < H) & (sx >= 0) & (sx < W)
                wm = w[:, t, :].T
            else:
                ny, nx = gy + p - kh, gx + p - kw
                ok = (ny >= 0) & (nx >= 0)
                if mut != "no_mod":
                    ok &= (ny % s == 0) & (nx % s == 0)
                sy, sx = ny // s, nx // s
                if mut != "no_oh":
                    ok &= (sy < OH) & (sx < OW)
                wm = w[:, t, :]
            row = np.where(ok[None], (n * SH + sy[None]) * SW + sx[None], zero_row)
            v = flat[np.clip(row, 0, zero_row)]
            tot += v @ wm
            mag += np.abs(v) @ np.abs(wm)
            cnt += ok[None, :, :, None] * K
    return tot, mag, cnt


ConvCall = collections.namedtuple("ConvCall", "B H W Cin Cout k s tr acc ld_x ld_y wco wt ybr yr0 yoff")


def conv_into(c, x, wbuf, bias, Y, mut=None):
    """One call on the y buffer Y = (V [R, ld_y], written [R, ld_y]).  Roundings: 1 + bias (forward only) + accumulate."""
    w = read_w(wbuf, c.wco, c.wt, c.Cout, c.k * c.k, c.Cin, swap=mut == "swap_w")
    tot, mag, cnt = conv_ref(x, w, c.H, c.W, c.k, c.s, c.tr, mut)
    r = V(tot, dsum_err(cnt, mag)).r()
    if bias is not None and (not c.tr or mut == "bias_t"):
        r = (r + V(np.resize(bias, tot.shape[-1]))).r()   # (the mutant indexes the bias by input channel)
    B, GH, GW, N = tot.shape
    dbs = c.ybr if c.ybr > 0 else GH * GW
    rws = (np.arange(B)[:, None] * dbs + (0 if mut == "row0" else c.yr0) + np.arange(GH * GW)[None, :]).reshape(-1)
    r = V(r.v.reshape(-1, N), r.e.reshape(-1, N))
    cols = slice(c.yoff, c.yoff + N)
    yv, written = Y
    if c.acc and mut != "no_acc":
        r = (V(yv.v[rws, cols], yv.e[rws, cols]) + r).r()
    yv.v[rws, cols], yv.e[rws, cols], written[rws, cols] = r.v, r.e, True


def conv_args(c, bias):
    return ("f32_conv", [P("x"), c.ld_x, P("w"), c.wco, c.wt, P("y", c.yoff), c.ld_y, c.ybr, c.yr0, P("bias") if bias else None, c.acc,
                         c.B, c.H, c.W, c.Cin, c.Cout, c.k, c.s, c.tr, STREAM])


def y_want(Y, init_bits, exact):
    yv, written = Y
    bits = np.where(written, b32(yv.v), init_bits.reshape(yv.v.shape))
    if exact:
        assert U.exact32(yv.v[written])
        return Want("f32", bits)
    return Want("f32", bits, yv.v, yv.e, written)


CONV_K, CONV_S = (1, 3, 7), (1, 2)
CONV_SHAPES = [(1, 1, 1), (2, 5, 7), (1, 6, 4)]
CONV_CH = [(3, 4), (5, 1), (1, 4)]                       # (Cin, Cout)
CONV_PARAMS = [(k, s, sh, tr, acc, dr) for k in CONV_K for s in CONV_S for sh in CONV_SHAPES for tr in (0, 1) for acc in (0, 1)
               for dr in ("int", "normal")]


def conv_channels(k, s, shape, tr):
    """every (k, s) meets every channel pair; (2, 5, 7) forward stride 1 has Cout = 4: 280 outputs, more than one workgroup and no
    multiple of 256"""
    if shape == (2, 5, 7) and s == 1 and not tr:
        return 3, 4
    return CONV_CH[(CONV_SHAPES.index(shape) + CONV_K.index(k) + s + tr) % 3]


@functools.lru_cache(maxsize=None)
def conv_case(k, s, shape, tr, acc, dr, mut=None):
    """x in the first K of K + 3 columns, y in the first N of N + 2, weights with a gap behind every tap and every output channel
    (wt = Cin + 1, wco = T wt + 2).  A bias is always passed: the transposed form must ignore it."""
    B, H, W = shape
    Cin, Cout = conv_channels(k, s, shape, tr)
    T = k * k
    OH, OW = out_size(H, W, k, s)
    K, N = (Cout, Cin) if tr else (Cin, Cout)
    c = ConvCall(B, H, W, Cin, Cout, k, s, tr, acc, K + 3, N + 2, T * (Cin + 1) + 2, Cin + 1, 0, 0, 0)
    seed = 1000 + 97 * k + 31 * s + 7 * sum(shape) + 3 * tr + acc
    xs = (B, OH, OW, K) if tr else (B, H, W, K)
    x = draw(dr, xs, seed)
    wbuf = draw(dr, Cout * c.wco, seed + 1, 0.5) if dr == "normal" else ints(Cout * c.wco, seed + 1, -4, 4)
    bias, old = draw(dr, Cout, seed + 2), draw(dr, (B * (H * W if tr else OH * OW), N), seed + 3)
    R = old.shape[0]
    y0 = rows(R, c.ld_y, [(0, b32(old))] if acc else [])
    Y = (V(np.zeros((R, c.ld_y))), np.zeros((R, c.ld_y), dtype=bool))
    Y[0].v[:, :N] = old
    conv_into(c, x, wbuf, bias, Y, mut)
    bufs = dict(x=("f32", rows(x.size // K, c.ld_x, [(0, b32(x).reshape(-1, K))])), w=("f32", b32(wbuf)), bias=("f32", b32(bias)), y=("f32", y0))
    return make_case([conv_args(c, True)], bufs, dict(y=y_want(Y, y0, dr == "int")), dr == "int")


@functools.lru_cache(maxsize=None)
def conv_stem_case(dr, mut=None):
    """The stem: Cin = 108 of 112-wide rows, one tap, weights flat (wco = wt = 108), no bias"""
    B, H, W, Cin, Cout = 2, 2, 3, 108, 4
    c = ConvCall(B, H, W, Cin, Cout, 1, 1, 0, 0, 112, Cout + 2, 108, 108, 0, 0, 0)
    x, wbuf = draw(dr, (B, H, W, Cin), 41), (ints(Cout * 108, 42, -4, 4) if dr == "int" else normal(Cout * 108, 42, 0.2))
    y0 = rows(B * H * W, c.ld_y, [])
    Y = (V(np.zeros((B * H * W, c.ld_y))), np.zeros((B * H * W, c.ld_y), dtype=bool))
    conv_into(c, x, wbuf, None, Y, mut)
    bufs = dict(x=("f32", rows(B * H * W, 112, [(0, b32(x).reshape(-1, Cin))])), w=("f32", b32(wbuf)), y=("f32", y0))
    return make_case([conv_args(c, False)], bufs, dict(y=y_want(Y, y0, dr == "int")), dr == "int")


HEAD_LEVELS = [(2, 3, 1), (1, 2, 7)]                     # (H, W, a0): rows 0 and 9 of each image belong to no level
HEAD_A, HEAD_C, HEAD_CH = 10, 3, 5


@functools.lru_cache(maxsize=None)
def conv_head_case(dr, mut=None):
    """The head: the outputs [B, A, 27 + C] of a B = 2 call, written by two 1x1 convs per level (27 columns at the row's start, C
    columns at offset 27, both with a bias, ld_y = ncols, y_batch_rows = A, y_row0 = a0).  The two levels interleave in the buffer;
    the rows of no level keep the sentinel."""
    B, ncols = 2, 27 + HEAD_C
    y0 = rows(B * HEAD_A, ncols, [])
    Y = (V(np.zeros((B * HEAD_A, ncols))), np.zeros((B * HEAD_A, ncols), dtype=bool))
    bufs, calls = dict(y=("f32", y0)), []
    for lv, (H, W, a0) in enumerate(HEAD_LEVELS):
        for part, (cout, off) in enumerate([(27, 0), (HEAD_C, 27)]):
            tag = "%d%d" % (lv, part)
            c = ConvCall(B, H, W, HEAD_CH, cout, 1, 1, 0, 0, HEAD_CH + 1, ncols, HEAD_CH, HEAD_CH, HEAD_A, a0, off)
            seed = 50 + 10 * lv + part
            x, wbuf, bias = draw(dr, (B, H, W, HEAD_CH), seed), (ints(cout * HEAD_CH, seed + 3, -4, 4) if dr == "int" else normal(cout * HEAD_CH, seed + 3)), draw(dr, cout, seed + 6)
            conv_into(c, x, wbuf, bias, Y, mut)
            bufs.update({"x" + tag: ("f32", rows(B * H * W, c.ld_x, [(0, b32(x).reshape(-1, HEAD_CH))])), "w" + tag: ("f32", b32(wbuf)),
                         "b" + tag: ("f32", b32(bias))})
            name, args = conv_args(c, True)
            calls.append((name, [P(a.buf + tag, a.off) if isinstance(a, P) and a.buf != "y" else a for a in args]))
            calls[-1][1][9] = P("b" + tag)
    return make_case(calls, bufs, dict(y=y_want(Y, y0, dr == "int")), dr == "int")


# (d) weight gradient: dw[co, t, ci] += sum over output pixels dy[n, oh, ow, co] x[n, oh s + kh - p, ow s + kw - p, ci]
def wgrad_ref(x, dy, k, s, mut=None):
    """x [B, H, W, Cin], dy [B, OH, OW, Cout] -> (sum, sum|terms|, terms) [Cout, T, Cin]"""
    B, H, W, Cin = x.shape
    _, OH, OW, Cout = dy.shape
    p = (k - 1) // 2
    xp = np.zeros((B, H + 2 * p + 1, W + 2 * p, Cin))
    ok = np.zeros((H + 2 * p + 1, W + 2 * p))
    xp[:, p:p + H, p:p + W], ok[p:p + H, p:p + W] = x, 1.0
    tot, mag, cnt = (np.zeros((Cout, k * k, Cin)) for _ in range(3))
    for kh in range(k):
        for kw in range(k):
            y0 = kh + (1 if mut == "tap" else 0)
            xs = xp[:, y0:y0 + s * OH:s, kw:kw + s * OW:s]
            tot[:, kh * k + kw] = np.einsum("bhwo,bhwc->oc", dy, xs)
            mag[:, kh * k + kw] = np.einsum("bhwo,bhwc->oc", np.abs(dy), np.abs(xs))
            cnt[:, kh * k + kw] = B * ok[y0:y0 + s * OH:s, kw:kw + s * OW:s].sum()
    return tot, mag, cnt


WGRAD_PARAMS = [(k, s, sh, dr) for k in CONV_K for s in CONV_S for sh in CONV_SHAPES for dr in ("int", "normal")]


@functools.lru_cache(maxsize=None)
def wgrad_case(k, s, shape, dr, mut=None):
    """dw pre-filled at its elements, the sentinel in the gaps behind every tap and every output channel; ld_dy = Cout or 32 in turn.
    Roundings: 2."""
    B, H, W = shape
    Cin, Cout = conv_channels(k, s, shape, 0)
    T = k * k
    OH, OW = out_size(H, W, k, s)
    wt, ld_x = Cin + 1, Cin + 3
    wco = T * wt + 2
    ld_dy = Cout if (CONV_K.index(k) + s + CONV_SHAPES.index(shape)) % 2 else 32
    seed = 3000 + 97 * k + 31 * s + 7 * sum(shape)
    x, dy, old = draw(dr, (B, H, W, Cin), seed), draw(dr, (B, OH, OW, Cout), seed + 1), draw(dr, (Cout, T, Cin), seed + 2)
    tot, mag, cnt = wgrad_ref(x, dy, k, s, mut)
    new = (V(old) + V(tot, dsum_err(cnt, mag)).r()).r()
    if mut == "no_acc":
        new = V(tot, dsum_err(cnt, mag)).r()
    idx = (np.arange(Cout)[:, None, None] * wco + np.arange(T)[None, :, None] * wt + np.arange(Cin)[None, None, :]).reshape(-1)
    dw0 = sent(Cout * wco)
    dw0[idx] = b32(old).reshape(-1)
    bits, soft, val, bound = dw0.copy(), np.zeros(dw0.size, dtype=bool), np.zeros(dw0.size), np.zeros(dw0.size)
    bits[idx], soft[idx], val[idx], bound[idx] = b32(new.v).reshape(-1), dr != "int", new.v.reshape(-1), new.e.reshape(-1)
    if dr == "int":
        assert U.exact32(new.v)
    bufs = dict(x=("f32", rows(B * H * W, ld_x, [(0, b32(x).reshape(-1, Cin))])), dy=("f32", rows(B * OH * OW, ld_dy, [(0, b32(dy).reshape(-1, Cout))])),
                dw=("f32", dw0))
    call = ("f32_conv_wgrad", [P("x"), ld_x, P("dy"), ld_dy, P("dw"), wco, wt, B, H, W, Cin, Cout, k, s, STREAM])
    return make_case([call], bufs, dict(dw=Want("f32", bits, val, bound, soft)), dr == "int")


# ---------------------------------------------------------------------------------------------------------------------------
# (e) BatchNorm (training mode) + activation (+ residual).  act 0 none, 1 SiLU, 2 ReLU, 3 LeakyReLU(0.1).
BN_M, BN_C, BN_ACT = (1, 2, 255, 256, 257, 1000), (1, 3, 9), (0, 1, 2, 3)
BN_PARAMS = [(M, C, act, dr) for M in BN_M for C in BN_C for act in BN_ACT for dr in ("exact", "normal")]
MOMENTUM = 0.125


def pow2(M):
    return M & (M - 1) == 0


def act_fwd_v(u, act):
    """V of act(u) as the kernel evaluates it in fp32"""
    if act == 0:
        return u
    if act == 2:
        return V(np.where(u.v < 0, 0.0, u.v), u.e)        # NaN < 0 is false: NaN stays
    if act == 3:                                          # 1-Lipschitz and continuous; one rounding below zero
        return V(np.where(u.v > 0, u.v, float(F01) * u.v), u.e).r()
    with np.errstate(all="ignore"):
        E = np.exp(-u.v)
        e = V(E, E * (np.expm1(u.e) + EXPF_REL * np.exp(u.e)))
    return (u / (1.0 + e).r()).r()


def act_fwd_32(u, act):
    """the same in numpy's float32 arithmetic (acts 0, 2, 3: separately rounded IEEE operations)"""
    if act == 2:
        return np.where(u < 0, np.float32(0), u)
    if act == 3:
        return np.where(u > 0, u, F01 * u)
    assert act == 0
    return u


def act_grad_v(u, act):
    if act == 0:
        return V(np.ones_like(u.v))
    if act in (2, 3):                                    # a step at zero: where the sign of the computed u is open, the whole step
        lo = 0.0 if act == 2 else float(F01)
        return V(np.where(u.v > 0, 1.0, lo), np.where(np.abs(u.v) <= u.e, 1.0 - lo, 0.0))
    with np.errstate(all="ignore"):
        E = np.exp(-u.v)
        e = V(E, E * (np.expm1(u.e) + EXPF_REL * np.exp(u.e)))
    s = (1.0 / (1.0 + e).r()).r()
    return (s * (1.0 + (u * (1.0 - s).r()).r()).r()).r()


def act_grad_32(u, act):
    if act == 0:
        return np.ones_like(u)
    return np.where(u > 0, np.float32(1), np.float32(0) if act == 2 else F01)


def bn_stats_ref(z, eps=EPS, mut=None):
    """z float64 [M, C] -> (mean V, biased variance V, invstd V) per channel: the two-pass form in double"""
    M = z.shape[0]
    s = z.sum(0)
    mean = V(s / M, dsum_err(M, np.abs(z).sum(0)) / M).d()
    d = (V(z) - mean).d()
    q = (d * d).d().sum(0)
    var = (q / float(M - 1 if mut == "m1_var" else M)).d()
    with np.errstate(all="ignore"):
        inv = 1.0 / np.sqrt(var.v + eps)
        lo = np.maximum(var.v - var.e + eps, eps / 2)
        inv = V(inv, 0.5 * lo ** -1.5 * var.e).d(3)
    return mean, var, inv


def bn_fwd_ref(z, gamma, beta, rmean0, rvar0, momentum, act, res, mut=None):
    """-> dict of V: save [2 C], rmean, rvar [C], y [M, C]; and of float32 arrays (the fixed rounding sequence): the same names + '32'"""
    M, C = z.shape
    mean, var, inv = bn_stats_ref(z, mut=mut)
    sm, si = mean.r(), inv.r()
    unb = var if (M == 1 or mut == "biased") else ((var * float(M)).d() / float(M if mut == "m_for_m1" else M - 1)).d()
    c1 = float(np.float32(1) - np.float32(momentum))
    out = dict(save=V(np.concatenate([sm.v, si.v]), np.concatenate([sm.e, si.e])))
    out["rmean"] = ((c1 * V(rmean0)).r() + (momentum * sm).r()).r()
    out["rvar"] = ((c1 * V(rvar0)).r() + (momentum * unb.r()).r()).r()
    u = ((((V(z) - sm).r() * si).r() * V(gamma)).r() + V(beta)).r()
    if mut == "res_first":
        y = act_fwd_v((u + V(res)).r(), act)
    else:
        y = act_fwd_v(u, act)
        if res is not None:
            y = (y + V(res)).r()
    out["y"] = y
    with np.errstate(all="ignore"):                       # the sequence of fp32 operations on float32(mean), float32(invstd)
        m32, i32, mo = sm.v.astype(np.float32), si.v.astype(np.float32), np.float32(momentum)
        out["save32"] = np.concatenate([m32, i32])
        out["rmean32"] = (np.float32(1) - mo) * f32(rmean0) + mo * m32
        out["rvar32"] = (np.float32(1) - mo) * f32(rvar0) + mo * unb.v.astype(np.float32)
        if act != 1:
            u32 = (f32(z) - m32) * i32 * f32(gamma) + f32(beta)
            if mut == "res_first":
                out["y32"] = act_fwd_32(u32 + f32(res), act)
            else:
                out["y32"] = act_fwd_32(u32, act) + (f32(res) if res is not None else np.float32(0))
    return out


def bn_variant(M, C, act):
    """(residual, running statistics, num_batches) present?  Rotated over the cases so that every form occurs with every act"""
    i = BN_M.index(M) * 3 + BN_C.index(C) + act
    return i % 2 == 1, i % 3 != 0, i % 4 != 1


def bn_fwd_draw(M, C, dr, nan=False):
    seed = 5000 + 13 * M + 5 * C
    if dr == "exact":                                    # integers, dyadic parameters: every step but 1 / sqrt is exact for M = 2^j
        z = ints((M, C), seed)
        if C >= 3:
            z[:, C - 1] = 3.0                             # a constant channel: var = 0, invstd = 1 / sqrt(eps)
        gamma, beta = pick([0.5, -0.5, 1.0, 2.0, 4.0], C, seed + 1), np.zeros(C)
        rm, rv, res = ints(C, seed + 2) / 8.0, ints(C, seed + 3, 1, 16) / 8.0, ints((M, C), seed + 4) / 4.0
    else:
        z = normal((M, C), seed, 1.5) + normal((1, C), seed + 9)
        z = z.astype(np.float32).astype(np.float64)
        gamma, beta = normal(C, seed + 1) + 1.0, normal(C, seed + 5, 0.5)
        gamma = gamma.astype(np.float32).astype(np.float64)
        rm, rv, res = normal(C, seed + 2), np.abs(normal(C, seed + 3)) + 0.5, normal((M, C), seed + 4)
        rv = rv.astype(np.float32).astype(np.float64)
    if nan:
        z[M // 2, 1 % C] = np.nan
    return z, gamma, beta, rm, rv, res


@functools.lru_cache(maxsize=None)
def bn_fwd_case(M, C, act, dr, mut=None, nan=False):
    """ld_z = C + 2, ld_y = C + 3, ld_res = C + 1.  Bit for bit: the exact draw with M a power of two (save, running statistics, and y
    for every act but SiLU); everything else under its bound.  num_batches: + 1, once."""
    z, gamma, beta, rm, rv, res = bn_fwd_draw(M, C, dr, nan)
    with_res, with_run, with_nbt = bn_variant(M, C, act)
    if mut == "res_first":
        with_res = True
    r = bn_fwd_ref(z, gamma, beta, rm, rv, MOMENTUM, act, res if with_res else None, mut)
    exact = dr == "exact" and pow2(M)
    ld_z, ld_y, ld_res = C + 2, C + 3, C + 1
    bufs = dict(z=("f32", rows(M, ld_z, [(0, b32(z))])), gamma=("f32", b32(gamma)), beta=("f32", b32(beta)), save=("f32", sent(2 * C)),
                y=("f32", sent(M * ld_y)))
    want = dict(save=vwant(r["save"], exact, 1, 2 * C, bits=bits32(r["save32"])),
                y=vwant(r["y"], exact and act != 1, M, ld_y, bits=bits32(r["y32"]) if act != 1 else None))
    if with_res:
        bufs["res"] = ("f32", rows(M, ld_res, [(0, b32(res))]))
    if with_run:
        bufs["rmean"], bufs["rvar"] = ("f32", b32(rm)), ("f32", b32(rv))
        want["rmean"] = vwant(r["rmean"], exact, 1, C, bits=bits32(r["rmean32"]))
        want["rvar"] = vwant(r["rvar"], exact, 1, C, bits=bits32(r["rvar32"]))
    if with_nbt:
        bufs["nbt"] = ("i64", np.array([41], dtype=np.int64))
        want["nbt"] = Want("i64", np.array([41 + (C if mut == "nbt_c" else 1)], dtype=np.int64))
    call = ("f32_bn_act_fwd", [P("z"), ld_z, P("gamma"), P("beta"), P("rmean") if with_run else None, P("rvar") if with_run else None,
                               P("nbt") if with_nbt else None, P("save"), P("y"), ld_y, P("res") if with_res else None, ld_res if with_res else 0,
                               M, C, EPS, MOMENTUM, act, STREAM])
    return make_case([call], bufs, want, exact and act != 1)


def bn_bwd_ref(dy, z, mean, inv, gamma, beta, gg0, bg0, act):
    """save = (mean, inv) is an input.  -> dict of V: sums [2 C] (double), dz [M, C], ggrad, bgrad [C]; float32 / float64 arrays of
    the fixed sequence under the same names + '32' (acts 0, 2, 3)"""
    M = z.shape[0]
    zh = ((V(z) - mean).r() * inv).r()
    u = ((zh * gamma).r() + beta).r()
    du = (V(dy) * act_grad_v(u, act)).r()
    sg, sb = (du * zh).sum(0), du.sum(0)
    mg, mb = (sg * (1.0 / M)).d(), (sb * (1.0 / M)).d()
    dz = ((V(gamma * inv) * (du - mb - zh * mg)).d(5)).r()
    out = dict(sums=V(np.concatenate([sg.v, sb.v]), np.concatenate([sg.e, sb.e])), dz=dz,
               ggrad=(V(gg0) + sg.r()).r(), bgrad=(V(bg0) + sb.r()).r())
    if act != 1:
        zh32 = (f32(z) - f32(mean)) * f32(inv)
        du32 = f32(dy) * act_grad_32(zh32 * f32(gamma) + f32(beta), act)
        d64, z64 = du32.astype(np.float64), zh32.astype(np.float64)
        s_g, s_b = (d64 * z64).sum(0), d64.sum(0)
        out["sums32"] = np.concatenate([s_g, s_b])
        out["dz32"] = (f64(gamma) * f64(inv) * (d64 - s_b / M - z64 * (s_g / M))).astype(np.float32)
        out["ggrad32"], out["bgrad32"] = f32(gg0) + s_g.astype(np.float32), f32(bg0) + s_b.astype(np.float32)
    return out


def bn_bwd_draw(M, C, dr):
    seed = 7000 + 13 * M + 5 * C
    if dr == "exact":           # zh, u, du and every sum are exact (act 3: du = fl(0.1f dy) is a multiple of 2^-27, the sums fit 53 bits)
        z, dy = ints((M, C), seed), ints((M, C), seed + 1)
        mean, inv = ints(C, seed + 2, -2, 2), pick([0.25, 0.5, 1.0], C, seed + 3)
        gamma, beta = pick([0.5, -0.5, 1.0, 2.0], C, seed + 4), pick([0.0, 0.25, -0.25, 0.5], C, seed + 5)
        gg0, bg0 = ints(C, seed + 6) / 4.0, ints(C, seed + 7) / 4.0
    else:
        z, dy = normal((M, C), seed, 1.5), normal((M, C), seed + 1)
        mean, inv = normal(C, seed + 2, 0.3), (np.abs(normal(C, seed + 3)) + 0.5).astype(np.float32).astype(np.float64)
        gamma, beta = (normal(C, seed + 4) + 1.0).astype(np.float32).astype(np.float64), normal(C, seed + 5, 0.5)
        gg0, bg0 = normal(C, seed + 6), normal(C, seed + 7)
    return dy, z, mean, inv, gamma, beta, gg0, bg0


@functools.lru_cache(maxsize=None)
def bn_bwd_case(M, C, act, dr, mut=None):
    """ld_dy = C + 1, ld_z = C + 2, ld_dz = C + 3; gamma_grad and beta_grad pre-filled, or both null in every fourth case.  Bit for bit:
    the exact draw with M a power of two and act 0, 2, 3 (the sums as float64 patterns too)."""
    dy, z, mean, inv, gamma, beta, gg0, bg0 = bn_bwd_draw(M, C, dr)
    r = bn_bwd_ref(dy, z, mean, inv, gamma, beta, gg0, bg0, act)
    with_grads = (BN_M.index(M) + BN_C.index(C) + act) % 4 != 3
    exact = dr == "exact" and pow2(M) and act != 1
    ld_dy, ld_z, ld_dz = C + 1, C + 2, C + 3
    bufs = dict(dy=("f32", rows(M, ld_dy, [(0, b32(dy))])), z=("f32", rows(M, ld_z, [(0, b32(z))])), save=("f32", b32(np.concatenate([mean, inv]))),
                gamma=("f32", b32(gamma)), beta=("f32", b32(beta)), sums=("f64", sent(2 * C, "f64")), dz=("f32", sent(M * ld_dz)))
    if exact:
        sums = Want("f64", r["sums32"].view(np.uint64))
    else:
        sums = Want("f64", r["sums"].v.view(np.uint64), r["sums"].v, r["sums"].e, np.ones(2 * C, dtype=bool))
    want = dict(sums=sums, dz=vwant(r["dz"], exact, M, ld_dz, bits=bits32(r["dz32"]) if act != 1 else None))
    if with_grads:
        bufs["ggrad"], bufs["bgrad"] = ("f32", b32(gg0)), ("f32", b32(bg0))
        for k in ("ggrad", "bgrad"):
            want[k] = vwant(r[k], exact, 1, C, bits=bits32(r[k + "32"]) if act != 1 else None)
    if mut == "no_acc" and with_grads:
        want["ggrad"], want["bgrad"] = vwant(V(r["sums"].v[:C]), True, 1, C), vwant(V(r["sums"].v[C:]), True, 1, C)
    call = ("f32_bn_act_bwd", [P("dy"), ld_dy, P("z"), ld_z, P("save"), P("gamma"), P("beta"), P("sums"), P("ggrad") if with_grads else None,
                               P("bgrad") if with_grads else None, P("dz"), ld_dz, M, C, act, STREAM])
    return make_case([call], bufs, want, exact)


# ---------------------------------------------------------------------------------------------------------------------------
# (f) SPP pools: three MaxPool2d(k, 1, k // 2), k = 5, 9, 13, of the same map; ATen's rule: a later element wins if it is greater or a
# NaN (the first maximum, the last NaN); a window with nothing above -inf reports its first cell.
SPP_MAPS = [(1, 1, 1), (1, 3, 3), (1, 13, 13), (1, 14, 5), (2, 6, 7)]
SPP_C = (1, 3)
NAN_MAP = [[1, np.nan, 3], [4, 5, np.nan], [0, 9, 2]]


def spp_draw(name, shape, C):
    B, H, W = shape
    seed = 900 + 11 * sum(shape) + C
    rng = np.random.default_rng(seed)
    x = ((rng.integers(0, 5, (B, H, W, C)) - 2) * 0.5).astype(np.float32)          # 5 levels: most windows hold their maximum twice
    if name == "nan33":
        assert (H, W) == (3, 3)
        x[0, :, :, 0] = np.array(NAN_MAP, dtype=np.float32)
    if name == "special":
        n = x.size
        k = max(1, n // 40)
        x.reshape(-1)[rng.choice(n, k, replace=False)] = NEG
        x.reshape(-1)[rng.choice(n, k, replace=False)] = NAN
        cy, cx = H // 2, W // 2
        x[0, max(0, cy - 2):cy + 3, max(0, cx - 2):cx + 3, 0] = NEG                # the 5-window of the centre holds nothing above -inf
        x[B - 1, H - 1, 0, C - 1] = NAN                                            # a single NaN
        x[B - 1, H - 1, max(0, W - 2):, 1 % C] = NAN                               # two NaN in one row of one window: the last one wins
    return x


def spp_fwd_ref(x, tie="first", nan=True, planes=(0, 1, 2)):
    """x float32 [B, H, W, C] -> (vals float32 [3, B, H, W, C], idx int32 [3, B, H, W, C]: y W + x of the winner in its image)"""
    B, H, W, C = x.shape
    vals, idxs = [], []
    ys, xs = np.arange(H)[None, :, None, None], np.arange(W)[None, None, :, None]
    for r in (2, 4, 6):
        k = 2 * r + 1
        xp = np.pad(x, ((0, 0), (r, r), (r, r), (0, 0)), constant_values=NEG)
        inb = np.pad(np.ones((1, H, W, 1), dtype=bool), ((0, 0), (r, r), (r, r), (0, 0)))
        st = np.stack([xp[:, a:a + H, b:b + W] for a in range(k) for b in range(k)])
        ok = np.stack([np.broadcast_to(inb[:, a:a + H, b:b + W], (B, H, W, C)) for a in range(k) for b in range(k)])
        isn = np.isnan(st)
        clean = np.where(isn, NEG, st)
        mx = clean.max(0)
        hit = (clean == mx) & ok & ~isn                   # the cells of the map that hold the maximum; all of them where that is -inf
        hit = np.where(hit.any(0), hit, ok)               # (a window of NaN alone)
        win = hit.argmax(0) if tie == "first" else k * k - 1 - hit[::-1].argmax(0)
        val = mx
        if nan:                                           # nan False (mutant): a NaN never wins
            has = isn.any(0)
            win = np.where(has, k * k - 1 - isn[::-1].argmax(0), win)
            val = np.where(has, NAN, mx)
        vals.append(val.astype(np.float32))
        idxs.append(((ys + win // k - r) * W + (xs + win % k - r)).astype(np.int32))
    return np.stack(vals), np.stack([idxs[p] for p in planes])


@functools.lru_cache(maxsize=None)
def spp_inputs(name, shape, C):
    x = spp_draw(name, shape, C)
    return (x,) + spp_fwd_ref(x)


SPP_FWD_PARAMS = [(sh, C, dr, lay) for sh in SPP_MAPS for C in SPP_C for dr in ("ties", "special") for lay in ("cat", "pad")] + \
                 [((1, 3, 3), C, "nan33", "pad") for C in SPP_C]


@functools.lru_cache(maxsize=None)
def spp_fwd_case(shape, C, dr, layout, mut=None):
    """cat: the engine's concatenation x | y5 | y9 | y13 in one buffer, ld = 4 C; pad: four buffers with 3 pad columns behind every row"""
    B, H, W = shape
    x = spp_inputs(dr, shape, C)[0]
    kw = dict(last=dict(tie="last"), no_nan=dict(nan=False), planes=dict(planes=(2, 1, 0))).get(mut, {})
    vals, idx = spp_fwd_ref(x, **kw)
    n = B * H * W
    xb = bits32(x).reshape(n, C)
    want = dict(idx=Want("i32", idx.reshape(-1)))
    bufs = dict(idx=("i32", sent(3 * n * C, "i32")))
    if layout == "cat":
        ld = 4 * C
        bufs["cat"] = ("f32", rows(n, ld, [(0, xb)]))
        want["cat"] = Want("f32", rows(n, ld, [(0, xb)] + [((p + 1) * C, bits32(vals[p])) for p in range(3)]))
        args = [P("cat"), ld, P("cat", C), P("cat", 2 * C), P("cat", 3 * C), ld]
    else:
        ld = C + 3
        bufs["x"] = ("f32", rows(n, ld, [(0, xb)]))
        for p in range(3):
            bufs["y%d" % p] = ("f32", sent(n * ld))
            want["y%d" % p] = Want("f32", rows(n, ld, [(0, bits32(vals[p]))]))
        args = [P("x"), ld, P("y0"), P("y1"), P("y2"), ld]
    return make_case([("f32_spp_fwd", args + [P("idx"), B, H, W, C, STREAM])], bufs, want, True)


def spp_bwd_ref(dys, idx, old, accumulate):
    """dys [3, B, H, W, C] float64, idx of the forward -> V [B, H, W, C]: every output sends its gradient to its winner, in double;
    one rounding, one more with the old value"""
    _, B, H, W, C = dys.shape
    n = B * H * W * C
    b, c = np.arange(B)[:, None, None, None], np.arange(C)[None, None, None, :]
    tot, mag, cnt = np.zeros(n), np.zeros(n), np.zeros(n)
    for p in range(3):
        t = ((b * H * W + idx[p]) * C + c).reshape(-1)
        g = dys[p].reshape(-1)
        tot += np.bincount(t, weights=g, minlength=n)
        mag += np.bincount(t, weights=np.abs(g), minlength=n)
        cnt += np.bincount(t, minlength=n)
    r = V(tot, dsum_err(cnt, mag)).r()
    if accumulate:
        r = (V(old.reshape(-1)) + r).r()
    return V(r.v.reshape(B, H, W, C), r.e.reshape(B, H, W, C))


SPP_BWD_PARAMS = [(sh, C, dr, acc) for sh in SPP_MAPS for C in SPP_C for dr in ("int", "normal") for acc in (0, 1)]


@functools.lru_cache(maxsize=None)
def spp_bwd_case(shape, C, dr, acc, mut=None):
    """dy5 | dy9 | dy13 | 2 pad columns in one buffer, dx in the last C of 2 C + 1 columns; the winners of the special forward draw, so
    NaN winners, ties (the whole gradient goes to the first maximum) and windows without a maximum route gradients too"""
    B, H, W = shape
    n = B * H * W
    idx = spp_inputs("special", shape, C)[2]
    seed = 1500 + 11 * sum(shape) + C
    dys, old = draw(dr, (3, B, H, W, C), seed), draw(dr, (B, H, W, C), seed + 1)
    r = spp_bwd_ref(dys, idx, old, acc and mut != "no_acc")
    ld_dy, ld_dx = 3 * C + 2, 2 * C + 1
    dy_img = rows(n, ld_dy, [(p * C, b32(dys[p]).reshape(n, C)) for p in range(3)])
    dx0 = rows(n, ld_dx, [(C + 1, b32(old).reshape(n, C))] if acc else [])
    w = vwant(V(r.v.reshape(n, C), r.e.reshape(n, C)), dr == "int", n, ld_dx, off=C + 1)
    bufs = dict(dy=("f32", dy_img), idx=("i32", idx.reshape(-1)), dx=("f32", dx0))
    call = ("f32_spp_bwd", [P("dy"), P("dy", C), P("dy", 2 * C), ld_dy, P("idx"), P("dx", C + 1), ld_dx, acc, B, H, W, C, STREAM])
    return make_case([call], bufs, dict(dx=w), dr == "int")


# ---------------------------------------------------------------------------------------------------------------------------
# (g) nearest x2 upsample, rows_copy
UP_SHAPE, UP_C = (2, 3, 5), 3


def upsample2_ref(x):
    return np.repeat(np.repeat(x, 2, axis=1), 2, axis=2)


def upsample2_bwd_ref(dy, old, accumulate, order="pairs"):
    """float32: (a00 + a01) + (a10 + a11) of each 2x2 block (a[row parity][column parity]), then old + that.  order 'chain' (mutant):
    ((a00 + a01) + a10) + a11"""
    B, H2, W2, C = dy.shape
    a = f32(dy).reshape(B, H2 // 2, 2, W2 // 2, 2, C)
    if order == "pairs":
        v = (a[:, :, 0, :, 0] + a[:, :, 0, :, 1]) + (a[:, :, 1, :, 0] + a[:, :, 1, :, 1])
    else:
        v = ((a[:, :, 0, :, 0] + a[:, :, 0, :, 1]) + a[:, :, 1, :, 0]) + a[:, :, 1, :, 1]
    return f32(old) + v if accumulate else v


@functools.lru_cache(maxsize=None)
def up_fwd_case():
    """a pure copy: random bit patterns; x in the columns 2 .. 2 + C of C + 4, y in the last C of 2 C + 1"""
    B, H, W = UP_SHAPE
    C, n = UP_C, B * H * W
    xb = U.random_bits(n * C, 77).reshape(B, H, W, C)
    ld_x, ld_y = C + 4, 2 * C + 1
    bufs = dict(x=("f32", rows(n, ld_x, [(2, xb.reshape(n, C))])), y=("f32", sent(4 * n * ld_y)))
    want = dict(y=Want("f32", rows(4 * n, ld_y, [(C + 1, upsample2_ref(xb).reshape(4 * n, C))])))
    return make_case([("f32_upsample2_fwd", [P("x", 2), ld_x, P("y", C + 1), ld_y, B, H, W, C, STREAM])], bufs, want, True)


@functools.lru_cache(maxsize=None)
def up_bwd_case(dr, acc, mut=None):
    B, H, W = UP_SHAPE
    C, n = UP_C, B * H * W
    dy, old = draw(dr, (B, 2 * H, 2 * W, C), 78), draw(dr, (B, H, W, C), 79)
    v = upsample2_bwd_ref(dy, old, acc and mut != "no_acc", "chain" if mut == "chain" else "pairs")
    ld_dy, ld_dx = C + 2, 2 * C + 1
    bufs = dict(dy=("f32", rows(4 * n, ld_dy, [(0, b32(dy).reshape(4 * n, C))])), dx=("f32", rows(n, ld_dx, [(C + 1, b32(old).reshape(n, C))] if acc else [])))
    want = dict(dx=Want("f32", rows(n, ld_dx, [(C + 1, bits32(v).reshape(n, C))])))
    return make_case([("f32_upsample2_bwd", [P("dy"), ld_dy, P("dx", C + 1), ld_dx, acc, B, H, W, C, STREAM])], bufs, want, True)


COPY_M, COPY_C = 7, 37                                    # 259 elements: one more workgroup for three of them


@functools.lru_cache(maxsize=None)
def copy_case(mode, mut=None):
    """bits: the plain copy of random patterns (NaN payloads, -0, the largest numbers); int / normal: dst += src, one fp32 add"""
    M, C = COPY_M, COPY_C
    acc = int(mode != "bits")
    if mode == "bits":
        sb, ob = U.random_bits(M * C, 5).reshape(M, C), sent(M * C).reshape(M, C)
        wb = sb
    else:
        s, o = draw(mode, (M, C), 6), draw(mode, (M, C), 7)
        sb, ob = b32(s), b32(o)
        wb = bits32(f32(o) + f32(s)) if mut != "no_acc" else sb
    ld_s, ld_d = C + 4, C + 1
    bufs = dict(src=("f32", rows(M, ld_s, [(3, sb)])), dst=("f32", rows(M, ld_d, [(1, ob)])))
    want = dict(dst=Want("f32", rows(M, ld_d, [(1, wb)])))
    return make_case([("f32_rows_copy", [P("src", 3), ld_s, P("dst", 1), ld_d, acc, M, C, STREAM])], bufs, want, True)


# ---------------------------------------------------------------------------------------------------------------------------
# (h) stem pack: the 3x3, pad 1 patches of Focus.forward = cat(top-left, bottom-left, top-right, bottom-right) of the image
STEM_IMAGES = [(2, 4, 6), (1, 2, 2)]
STEM_LD = (112, 108)


def stem_rows_ref(img, ld, order=(0, 1, 2, 3)):
    """img uint32 [B, 3, H, W] -> uint32 [B FH FW, ld]: column (ky 3 + kx) 12 + patch 3 + channel; taps outside the map and the columns
    from 108 on are +0.  order (mutant): the patches in another order"""
    B, _, H, W = img.shape
    patches = [img[:, :, 0::2, 0::2], img[:, :, 1::2, 0::2], img[:, :, 0::2, 1::2], img[:, :, 1::2, 1::2]]
    f = np.concatenate([patches[i] for i in order], axis=1).transpose(0, 2, 3, 1)          # [B, FH, FW, 12]
    FH, FW = H // 2, W // 2
    fp = np.zeros((B, FH + 2, FW + 2, 12), dtype=np.uint32)
    fp[:, 1:-1, 1:-1] = f
    out = np.zeros((B, FH, FW, ld), dtype=np.uint32)
    for ky in range(3):
        for kx in range(3):
            t = ky * 3 + kx
            out[..., t * 12:t * 12 + 12] = fp[:, ky:ky + FH, kx:kx + FW]
    return out.reshape(B * FH * FW, ld)


@functools.lru_cache(maxsize=None)
def stem_case(image, ld, mut=None):
    B, H, W = image
    img = U.random_bits(B * 3 * H * W, 12).reshape(B, 3, H, W)
    out = stem_rows_ref(img, ld, (0, 2, 1, 3) if mut == "patch" else (0, 1, 2, 3))
    bufs = dict(img=("f32", img), rows=("f32", sent(out.size)))
    return make_case([("f32_stem_pack", [P("img"), P("rows"), ld, B, H, W, STREAM])], bufs, dict(rows=Want("f32", out)), True)


# (i) the gradient of the train-mode head decode: xy = (t + grid) s, radii = exp(t) s = out, so d t = (dout s, dout out) per column,
# + d_origin [B, A, 26] (the L1 branch); column 26 passes, 27 .. 31 are +0; d_cls holds the class columns and +0 in its pad.
DEC_A0, DEC_H, DEC_W, DEC_TAIL, DEC_S = 2, 2, 3, 3, 8.0
DEC_PARAMS = [(C, org) for C in (3, 9) for org in (False, True)]


def decode_bwd_ref(dout, out, a0, H, W, s, d_origin, mut=None):
    """float32 arrays [B, A, ncols] -> (d_regobj uint32 [B H W, 32], d_cls uint32 [B H W, ldc]) in the kernel's fp32 operations"""
    B, A, ncols = dout.shape
    C = ncols - 27
    ldc = (C + 7) & ~7
    d, o = f32(dout[:, a0:a0 + H * W]), f32(out[:, a0:a0 + H * W])
    reg = np.zeros((B, H * W, 32), dtype=np.float32)
    reg[..., 0:2] = d[..., 0:2] * np.float32(s)
    reg[..., 2:26] = d[..., 2:26] if mut == "no_out" else d[..., 2:26] * o[..., 2:26]
    reg[..., 26] = d[..., 26]
    if d_origin is not None:
        cell = (np.arange(B)[:, None] * A + a0 + np.arange(H * W)[None, :])[..., None]
        flat = np.concatenate([f32(d_origin).reshape(-1), np.zeros(B * A, dtype=np.float32)])
        reg[..., :26] = reg[..., :26] + flat[cell * (27 if mut == "stride27" else 26) + np.arange(26)]
    cls = bits32(np.zeros((B, H * W, ldc), dtype=np.float32)).reshape(B, H * W, ldc)
    if mut == "pad":
        cls[:] = SENT32
    cls[..., :C] = bits32(d[..., 27:]).reshape(B, H * W, C)
    return bits32(reg).reshape(B * H * W, 32), cls.reshape(B * H * W, ldc)


@functools.lru_cache(maxsize=None)
def decode_case(C, with_origin, mut=None):
    """two images, a0 > 0, rows of other levels before and behind; dyadic draws: every product and sum is an fp32 number"""
    B, H, W, a0 = 2, DEC_H, DEC_W, DEC_A0
    A, ncols = a0 + H * W + DEC_TAIL, 27 + C
    dout, out, org = dyadic4((B, A, ncols), 500 + C), dyadic4((B, A, ncols), 501 + C), dyadic4((B, A, 26), 502 + C)
    assert U.exact32(dout[..., :26] * out[..., :26] + org) and U.exact32(dout[..., :2] * DEC_S + org[..., :2])
    reg, cls = decode_bwd_ref(dout, out, a0, H, W, DEC_S, org if with_origin else None, mut)
    bufs = dict(dout=("f32", b32(dout)), out=("f32", b32(out)), org=("f32", b32(org)), reg=("f32", sent(reg.size)), cls=("f32", sent(cls.size)))
    call = ("f32_head_decode_bwd", [P("dout"), P("out"), P("reg"), P("cls"), B, A, a0, H, W, DEC_S, ncols, P("org") if with_origin else None, STREAM])
    return make_case([call], bufs, dict(reg=Want("f32", reg), cls=Want("f32", cls)), True)


# (j) bias column sums: db[c] += sum over rows, a double sum rounded once, then the add
COLSUM_PARAMS = [(M, N, dr) for M in (1, 255, 257) for N in (1, 27) for dr in ("int", "normal")]


@functools.lru_cache(maxsize=None)
def colsum_case(M, N, dr, mut=None):
    ld = 32
    g, old = draw(dr, (M, N), 600 + M + N), draw(dr, N, 601 + M + N)
    s = V(g).sum(0).r()
    r = s if mut == "no_acc" else (V(old) + s).r()
    bufs = dict(g=("f32", rows(M, ld, [(0, b32(g))])), db=("f32", b32(old)))
    call = ("f32_colsum", [P("g"), ld, P("db"), M, N, STREAM])
    return make_case([call], bufs, dict(db=vwant(r, dr == "int", 1, N)), dr == "int")
