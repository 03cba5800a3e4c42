"""The conv kernels against an independent reference BIT FOR BIT.

bf16 x bf16 products are exact in fp32, and with small integer operands every fp32 partial sum of a conv is an integer below
2^24: exact in any order.  So every conv kernel (tiled, streaming, ring, 8-wave halo patch, weights in registers, weight gradient)
has exactly one right answer per element - float64 F.conv2d on the CPU, rounded once to the output format - and no tolerance
is needed: outputs, input gradients (plain and accumulated), the fixed-point batch statistics and the fp32 weight gradients are
compared with torch.equal.  Every destination sits inside a buffer filled with a sentinel (three guard rows before and after, for
the slice layouts also columns left and right), and the WHOLE buffer is compared: a store past Cout, past M or on a wrong row shows.

Draw D1 (values): integers in [-8, 8].  Draw D2 (statistics): {-1, 0, 1} with a density per case.  The conditions that make "exact"
true (every |partial sum| < 2^24) and the tests discriminating (>= 1 % of the outputs need a real rounding to bf16, the two accumulate
forms differ on >= 1 % of the elements) are asserted on the reference alone, before any launch.

Accumulate forms (include/ep24.h at ep24_conv_dgrad_bf16): the tiled, ring and halo-patch kernels store bf16(float(bf16(acc)) + old)
- two roundings - through both store widths of their epilogues; the streaming 1x1 kernel stores bf16(acc + old) - one rounding.
"""
import functools

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BF = torch.bfloat16
SENT = -7.0                      # finite, exact in bf16 and fp32; never the value a kernel would leave by accident (0) in a guard
GUARD = 3                        # rows before the first and after the last pixel
LIM = float(2 ** 24)

# kernel_opts bits of the _ex entry points (include/ep24.h)
NARROW, PER_CLASS, PATCH8, NO_DEEP, TILED256, NO_WREG = 2, 4, 8, 128, 256, 512
TILED, STREAM, RING, WREG, PATCH = 0, 2, 3, 6, 1


def _abi():
    from ep24._lib import call, lib, ptr, stream_ptr
    return call, ptr, stream_ptr, lib().fn


def _shape(t):
    B, H, Cin, Cout, k, s = t[:6]
    W = t[6] if len(t) > 6 else H
    pad = (k - 1) // 2
    OH, OW = (H + 2 * pad - k) // s + 1, (W + 2 * pad - k) // s + 1
    return B, H, W, Cin, Cout, k, s, OH, OW


def _ints(shape, seed):
    return torch.randint(-8, 9, shape, generator=torch.Generator().manual_seed(seed)).double()


def _tern(shape, seed, density):
    g = torch.Generator().manual_seed(seed)
    sign = torch.randint(0, 2, shape, generator=g).double() * 2 - 1
    return sign * (torch.rand(shape, generator=g) < density).double()


def rows(t_nchw):
    """[B, C, H, W] -> the kernels' [B*H*W, C] rows (NHWC)."""
    return t_nchw.permute(0, 2, 3, 1).reshape(-1, t_nchw.shape[1]).contiguous()


def two_roundings(acc, old):
    return (acc.to(BF).double() + old).to(BF)


def one_rounding(acc, old):
    return (acc + old).to(BF)


@functools.lru_cache(maxsize=None)
def ref_d1(shape):
    """Draw D1 and its float64 CPU reference, once per shape; the returned tensors are shared and never written."""
    B, H, W, Cin, Cout, k, s, OH, OW = _shape(shape)
    pad = (k - 1) // 2
    x = _ints((B, Cin, H, W), 1).requires_grad_(True)
    w = _ints((Cout, Cin, k, k), 2).requires_grad_(True)
    gy = _ints((B, Cout, OH, OW), 3)
    y = F.conv2d(x, w, None, s, pad)
    y.backward(gy)
    r = dict(x=x.detach(), w=w.detach(), gy=gy, y=y.detach(), dx=x.grad, dw=w.grad, old=_ints((B * H * W, Cin), 5))
    M = B * OH * OW
    # exactness: no fp32 partial sum of any kernel leaves the integers that fp32 holds exactly
    assert float(F.conv2d(r["x"].abs(), r["w"].abs(), None, s, pad).max()) < LIM
    assert float(F.conv_transpose2d(gy.abs(), r["w"].abs(), None, s, pad, output_padding=(H + 2 * pad - k) % s if s > 1 else 0).max()) < LIM
    assert M * 64 < 2 ** 24                                        # weight gradients: M products of at most 8 * 8
    # discriminating: a kernel that lost the last bit of a sum, or rounded at the wrong place, would be seen
    r["frac_rounded"] = float((r["y"].to(BF).double() != r["y"]).double().mean())
    assert r["frac_rounded"] >= 0.01, r["frac_rounded"]
    acc, old = rows(r["dx"]), r["old"]
    r["dx2_two"], r["dx2_one"] = two_roundings(acc, old), one_rounding(acc, old)
    r["frac_forms"] = float((r["dx2_two"] != r["dx2_one"]).double().mean())
    return r


@functools.lru_cache(maxsize=None)
def ref_d2(shape, density):
    B, H, W, Cin, Cout, k, s, OH, OW = _shape(shape)
    pad = (k - 1) // 2
    x, w = _tern((B, Cin, H, W), 11, density), _tern((Cout, Cin, k, k), 12, density)
    y = F.conv2d(x, w, None, s, pad)
    assert float(F.conv2d(x.abs(), w.abs(), None, s, pad).max()) < LIM
    s1, s2 = y.sum((0, 2, 3)), (y * y).sum((0, 2, 3))
    # every fp32 partial sum of any workgroup (the weights-in-registers kernel sums over all of its tiles) stays exact
    assert float(s2.max()) < LIM and float(y.abs().sum((0, 2, 3)).max()) < LIM
    assert float(s2.min()) > 0
    want = (torch.stack([s1, s2]) * 2 ** 20).round().long()
    return dict(x=x, w=w, y=y, stats=want)


# ---------------------------------------------------------------------------------------------------------------------------
# layouts: how a [rows, C] operand / destination sits in its buffer.  (ld - C, channel offset); every buffer has GUARD rows around
LAYOUTS = {
    "dense": dict(src=(0, 0), dst=(0, 0), ko=0),
    # channel slices of a concat buffer, as the engine calls the kernels in every CSP layer; 16-byte aligned: the wide store path
    "slice": dict(src=(24, 8), dst=(40, 16), ko=0),
    # the 8-byte store path, reached through the destination's alignment (ld % 8 == 4, channel offset 4) ...
    "narrow_off": dict(src=(24, 8), dst=(12, 4), ko=0),
    # ... and through kernel_opts bit 1
    "narrow_bit": dict(src=(0, 0), dst=(0, 0), ko=NARROW),
}


class Buf:
    """A [GUARD + M + GUARD, ld] device buffer full of the sentinel with a [M, C] window at channel offset `off`."""

    def __init__(self, M, C, extra_ld, off, dtype=BF, fill=None):
        self.M, self.C, self.ld, self.off = M, C, C + extra_ld, off
        self.host = torch.full((M + 2 * GUARD, self.ld), SENT, dtype=dtype)
        if fill is not None:
            self.window(self.host)[:] = fill.to(dtype)
        self.dev = self.host.to(DEV)

    def window(self, t):
        return t[GUARD:GUARD + self.M, self.off:self.off + self.C]

    def ptr(self):
        return self.dev.data_ptr() + (GUARD * self.ld + self.off) * self.dev.element_size()

    def check(self, want, what):
        """The whole buffer: `want` inside the window, the sentinel (or the operand it held) everywhere else - bit for bit."""
        exp = self.host.clone()
        self.window(exp)[:] = want.to(exp.dtype)
        got = self.dev.cpu()
        if not torch.equal(got, exp):
            bad = (got != exp).nonzero()
            inside = ((bad[:, 0] >= GUARD) & (bad[:, 0] < GUARD + self.M) & (bad[:, 1] >= self.off) & (bad[:, 1] < self.off + self.C)).sum().item()
            i, j = bad[0].tolist()
            raise AssertionError("%s: %d of %d elements differ (%d inside the window, %d outside); first at buffer row %d col %d (window row %d, "
                                 "channel %d): got %s, want %s" % (what, len(bad), got.numel(), inside, len(bad) - inside, i, j, i - GUARD, j - self.off,
                                                                   got[i, j].item(), exp[i, j].item()))


def pad_cols(t2d, C):
    """[M, c] -> [M, C] with zero columns (the kernels' Cout_k: a multiple of 8, zero padded)."""
    if t2d.shape[1] == C:
        return t2d.contiguous()
    out = torch.zeros(t2d.shape[0], C, dtype=t2d.dtype)
    out[:, :t2d.shape[1]] = t2d
    return out


def c8(c):
    return (c + 7) // 8 * 8


# ---------------------------------------------------------------------------------------------------------------------------
# The cases: (B, H, Cin, Cout, k, s[, W]), kernel_opts, kernel ids (forward, stride-1 input gradient) the dry-run query must give.
# acc = False: the accumulated input gradient is left out, with the reason.
class Case:
    def __init__(self, name, shape, ko, kid_f, kid_d, acc=True, density=0.5):
        self.name, self.shape, self.ko, self.kid_f, self.kid_d, self.acc, self.density = name, shape, ko, kid_f, kid_d, acc, density


S2_128 = (9, 128, 72, 72, 3, 2)
CASES = [
    # tiled kernel, 64-wide two-stage tiles
    Case("tiled64-3x3", (2, 12, 16, 24, 3, 1), 0, TILED, TILED),
    Case("tiled64-s2", (1, 24, 8, 16, 3, 2), 0, TILED, TILED),
    # (its input gradient is a 1x1 layer with K = 64: the streaming kernel)
    Case("tiled64-1x1-k512", (2, 8, 512, 64, 1, 1), 0, TILED, STREAM),
    # M, N and K tails; N > 64 with 18 K steps: the default is the three-stage form, bit 7 the 64-wide two-stage tiles
    Case("tiled-deep-tails", (5, 9, 72, 200, 3, 1), 0, TILED, TILED),
    Case("tiled64-tails", (5, 9, 72, 200, 3, 1), NO_DEEP, TILED, TILED),
    # three-stage form: too few tiles for 128-wide two-stage tiles, N > 64, 9 K steps; and the same shape without it
    Case("tiled-deep", (1, 16, 64, 128, 3, 1), 0, TILED, TILED),
    Case("tiled-deep-off", (1, 16, 64, 128, 3, 1), NO_DEEP, TILED, TILED),
    # 128-wide tiles: 288 of them, K > 256 (its input gradient: K = 128, the streaming kernel)
    Case("tiled128-1x1-k264", (9, 64, 264, 128, 1, 1), 0, TILED, STREAM),
    # ... and a stride-2 3x3 layer of the same size class (288 tiles of 128 x 128 forward and per parity class), K and N tails
    Case("tiled128-s2", S2_128, 0, TILED, TILED, density=0.4),
    Case("tiled128-s2-per-class", S2_128, PER_CLASS, TILED, TILED, density=0.4),
    # streaming 1x1 kernel: K <= 64 / 64 < K <= 128 / 128 < K <= 256, both N tile widths, rows past M, N % 8 == 4, K tails
    # acc = False: its input gradient sums 16 products (Cout_k = 16), |sum| < 256 on 99 % of the elements - bf16 holds them exactly, the
    # two accumulate forms cannot differ on 1 %; the plain input gradient is checked
    Case("stream-k64-n12", (3, 13, 64, 12, 1, 1), 0, STREAM, STREAM, acc=False),
    Case("stream-k120-n68", (2, 19, 120, 68, 1, 1), 0, STREAM, STREAM),
    Case("stream-k200-n132", (3, 17, 200, 132, 1, 1), 0, STREAM, STREAM),
    Case("stream-k256-n128", (2, 24, 256, 128, 1, 1), 0, STREAM, STREAM),
    # bit 8 sends the 128 < K <= 256 layers to the tiled kernel
    Case("tiled-k200-n132", (3, 17, 200, 132, 1, 1), TILED256, TILED, TILED),
    # ring (default) and 8-wave halo patch (bit 3): exactly 200 tiles, one patch buffer (the input gradient has N = 64: tiled)
    Case("ring-200-tiles", (8, 80, 64, 128, 3, 1), 0, RING, TILED),
    Case("patch-200-tiles", (8, 80, 64, 128, 3, 1), PATCH8, PATCH, TILED),
    # two patch buffers (K = 72 > 64 forward, 136 backward) with K and N tails, non-square, 51 030 pixels = 199 * 256 + 86: a last tile
    # with rows past M; 400 tiles forward, exactly 200 in the input gradient (W = 90 is the widest image two patch buffers take)
    Case("ring-tails", (9, 63, 72, 136, 3, 1, 90), 0, RING, RING, density=0.4),
    Case("patch-tails", (9, 63, 72, 136, 3, 1, 90), PATCH8, PATCH, PATCH, density=0.4),
    # weights in registers: the minimum of 65 536 pixels; a last tile past M with K and N tails; bit 9 = the tiled kernel instead.
    # (The kernel takes plain first-writer 16-byte destinations only: the accumulated input gradient and the narrow layouts run in
    # what the dispatcher falls back to, the tiled kernel.)
    Case("wreg-min", (1, 256, 16, 24, 3, 1, 256), 0, WREG, WREG),
    Case("wreg-tails", (3, 150, 48, 40, 3, 1, 160), 0, WREG, WREG, density=0.4),
    Case("wreg-off-tails", (3, 150, 48, 40, 3, 1, 160), NO_WREG, TILED, TILED, density=0.4),
]
CASE_IDS = [c.name for c in CASES]


def _kernel_ids(fn, c, ko):
    B, H, W, Cin, Cout, k, s, OH, OW = _shape(c.shape)
    f = fn["ep24_conv_kernel_for_ex"](0, B, H, W, Cin, Cout, k, s, 0, 0, ko)
    d = fn["ep24_conv_kernel_for_ex"](1, B, H, W, Cin, Cout, k, s, 0, 0, ko)
    return f, d


def _assert_dispatch(fn, c, layout):
    """The case runs where it is meant to (the library's own dry-run query, dense operands).  Returns the accumulate form of the
    input gradient's kernel."""
    f, d = _kernel_ids(fn, c, c.ko)
    assert (f, d) == (c.kid_f, c.kid_d), "dispatch of %s: forward %d, input gradient %d" % (c.name, f, d)
    ko = c.ko | LAYOUTS[layout]["ko"]
    fb, db = _kernel_ids(fn, c, ko)
    if WREG in (c.kid_f, c.kid_d) and layout in ("narrow_off", "narrow_bit"):
        # the weights-in-registers kernel refuses an 8-byte destination: the fallback (its shapes have N <= 64: the tiled kernel)
        fn_ = _kernel_ids(fn, c, c.ko | NARROW)
        assert fn_ == (TILED, TILED), fn_
    else:
        assert (fb, db) == (c.kid_f, c.kid_d)
    return "one" if d == STREAM else "two"


@pytest.mark.parametrize("layout", list(LAYOUTS))
@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_conv_fwd_dgrad_exact(case, layout):
    call, ptr, sp, fn = _abi()
    B, H, W, Cin, Cout, k, s, OH, OW = _shape(case.shape)
    form = _assert_dispatch(fn, case, layout)
    r = ref_d1(case.shape)
    L = LAYOUTS[layout]
    ko = case.ko | L["ko"]
    M_out, M_in, Ck = B * OH * OW, B * H * W, c8(Cout)
    wf = r["w"].permute(0, 2, 3, 1).contiguous().to(BF).to(DEV)                                   # [Cout][kh][kw][Cin]
    wd = pad_cols(r["w"].permute(1, 2, 3, 0).reshape(-1, Cout), Ck).to(BF).to(DEV)                # [Cin][kh][kw][Cout_k]

    # forward
    xb = Buf(M_in, Cin, *L["src"], fill=rows(r["x"]))
    yb = Buf(M_out, Cout, *L["dst"])
    call("conv_fwd_bf16_ex", xb.ptr(), xb.ld, ptr(wf), yb.ptr(), yb.ld, 0, 0, 0, None, None, 1, B, H, W, Cin, Cout, k, s, ko, sp())
    yb.check(rows(r["y"]).to(BF), "forward y")

    # input gradient: first writer (the window held the sentinel) ...
    gb = Buf(M_out, Ck, *L["src"], fill=pad_cols(rows(r["gy"]), Ck))
    want_dx = rows(r["dx"]).to(BF)
    if not (k == 1 and s == 2):
        db = Buf(M_in, Cin, *L["dst"])
        call("conv_dgrad_bf16_ex", gb.ptr(), gb.ld, ptr(wd), db.ptr(), db.ld, 0, B, H, W, Cin, Ck, k, s, ko, sp())
        db.check(want_dx, "input gradient dx")
    # ... and accumulated onto integer contents, in the form documented for the kernel that runs
    if case.acc:
        assert r["frac_forms"] >= 0.01, r["frac_forms"]
        ab = Buf(M_in, Cin, *L["dst"], fill=r["old"])
        call("conv_dgrad_bf16_ex", gb.ptr(), gb.ld, ptr(wd), ab.ptr(), ab.ld, 1, B, H, W, Cin, Ck, k, s, ko, sp())
        ab.check(r["dx2_one"] if form == "one" else r["dx2_two"], "accumulated dx (%s rounding%s)" % (form, "" if form == "one" else "s"))
    assert fn["ep24_conv_ring_timeouts"]() == 0


def test_stride2_input_gradient_merged_equals_per_class():
    """kernel_opts bit 2 runs the four parity classes of a stride-2 input gradient as four launches instead of one: the same bits
    (both also equal the reference: the two cases of this shape in test_conv_fwd_dgrad_exact)."""
    call, ptr, sp, fn = _abi()
    B, H, W, Cin, Cout, k, s, OH, OW = _shape(S2_128)
    r = ref_d1(S2_128)
    wd = r["w"].permute(1, 2, 3, 0).contiguous().to(BF).to(DEV)
    gy = rows(r["gy"]).to(BF).to(DEV)
    outs = []
    for ko in (0, PER_CLASS):
        for accumulate in (0, 1):
            dx = r["old"].to(BF).to(DEV)
            call("conv_dgrad_bf16_ex", ptr(gy), Cout, ptr(wd), ptr(dx), Cin, accumulate, B, H, W, Cin, Cout, k, s, ko, sp())
            outs.append(dx)
    assert torch.equal(outs[0], outs[2]) and torch.equal(outs[1], outs[3])
    assert torch.equal(outs[0].cpu(), rows(r["dx"]).to(BF)) and torch.equal(outs[1].cpu(), r["dx2_two"])


# (bit 2 changes the input gradient only: the forward statistics of that shape are the tiled128-s2 case)
STAT_CASES = [c for c in CASES if c.ko != PER_CLASS]


@pytest.mark.parametrize("layout", list(LAYOUTS))
@pytest.mark.parametrize("case", STAT_CASES, ids=[c.name for c in STAT_CASES])
def test_conv_batch_statistics_exact(case, layout):
    """Draw D2: the 2^-20 fixed-point sums of y and y * y per channel, as integers - through the wide epilogues' per-wave sums, the
    narrow path's fold through LDS, the streaming kernel's registers and the weights-in-registers kernel's sums over all its tiles."""
    call, ptr, sp, fn = _abi()
    B, H, W, Cin, Cout, k, s, OH, OW = _shape(case.shape)
    _assert_dispatch(fn, case, layout)
    r = ref_d2(case.shape, case.density)
    L = LAYOUTS[layout]
    ko = case.ko | L["ko"]
    M_out, M_in = B * OH * OW, B * H * W
    wf = r["w"].permute(0, 2, 3, 1).contiguous().to(BF).to(DEV)
    xb = Buf(M_in, Cin, *L["src"], fill=rows(r["x"]))
    yb = Buf(M_out, Cout, *L["dst"])
    R = 4
    stats = torch.zeros(R, 2, Cout, dtype=torch.int64, device=DEV)
    call("conv_fwd_bf16_ex", xb.ptr(), xb.ld, ptr(wf), yb.ptr(), yb.ld, 0, 0, 0, None, ptr(stats), R, B, H, W, Cin, Cout, k, s, ko, sp())
    yb.check(rows(r["y"]).to(BF), "forward y")
    got = stats.sum(0).cpu()
    assert torch.equal(got, r["stats"]), "statistics differ on channels %s" % (got != r["stats"]).any(0).nonzero().flatten().tolist()[:16]
    assert fn["ep24_conv_ring_timeouts"]() == 0


@pytest.mark.parametrize("layout", list(LAYOUTS))
def test_conv_bias_and_statistics_with_rows_past_m(layout):
    """bf16 output WITH a bias and the batch statistics (the tiled kernel: a bias keeps a 1x1 layer out of the streaming kernel), 432
    pixels = 3 tiles of 128 + 48: the rows past M of the last tile hold acc + bias = bias, not zero - only the `live` select of the wide
    epilogue (the row test of the narrow one) keeps them out of the sums."""
    call, ptr, sp, fn = _abi()
    shape = (3, 12, 64, 80, 1, 1)
    B, H, W, Cin, Cout, k, s, OH, OW = _shape(shape)
    assert fn["ep24_conv_kernel_for_ex"](0, B, H, W, Cin, Cout, k, s, 0, 1, LAYOUTS[layout]["ko"]) == TILED and (B * H * W) % 128 != 0
    r = ref_d2(shape, 0.5)
    bias = _ints((Cout,), 7)
    bias[bias == 0] = 3.0                                           # every channel's dead rows would add something
    y = rows(r["y"]) + bias
    s2 = (y * y).sum(0)
    assert float(s2.max()) + 128 * 64 < LIM                         # also with 128 rows of bias added by mistake
    want = (torch.stack([y.sum(0), s2]) * 2 ** 20).round().long()
    L = LAYOUTS[layout]
    wf = r["w"].reshape(Cout, Cin).to(BF).to(DEV)
    xb = Buf(B * H * W, Cin, *L["src"], fill=rows(r["x"]))
    yb = Buf(B * H * W, Cout, *L["dst"])
    bd = bias.float().to(DEV)
    R = 2
    stats = torch.zeros(R, 2, Cout, dtype=torch.int64, device=DEV)
    call("conv_fwd_bf16_ex", xb.ptr(), xb.ld, ptr(wf), yb.ptr(), yb.ld, 0, 0, 0, ptr(bd), ptr(stats), R, B, H, W, Cin, Cout, k, s, L["ko"], sp())
    yb.check(y.to(BF), "forward y + bias")
    assert torch.equal(stats.sum(0).cpu(), want)


# ---------------------------------------------------------------------------------------------------------------------------
# weight gradients (they do not depend on the conv kernel_opts: once per shape)
WGRAD_SHAPES = []
for _c in CASES:
    if _c.shape not in WGRAD_SHAPES:
        WGRAD_SHAPES.append(_c.shape)


def _wgrad_want(r, Cout_v=None, Cin_v=None):
    dw = r["dw"].permute(0, 2, 3, 1)                                 # [Cout][kh][kw][Cin]
    Cout, kh, kw, Cin = dw.shape
    return dw[:Cout_v or Cout, :, :, :Cin_v or Cin].reshape(Cout_v or Cout, -1).float()


@pytest.mark.parametrize("layout", ["dense", "slice"])
@pytest.mark.parametrize("shape", WGRAD_SHAPES, ids=lambda t: "x".join(str(v) for v in t))
def test_conv_wgrad_exact(shape, layout):
    """Slab + ordered reduce, the atomic form and the grouped launch: == dw_ref as fp32, == 2 * dw_ref after a second +=; strided x / dy;
    slabs pre-filled with NaN and fully overwritten."""
    call, ptr, sp, fn = _abi()
    B, H, W, Cin, Cout, k, s, OH, OW = _shape(shape)
    r = ref_d1(shape)
    L = LAYOUTS[layout]
    Ck = c8(Cout)
    xb = Buf(B * H * W, Cin, *L["src"], fill=rows(r["x"]))
    gb = Buf(B * OH * OW, Ck, *L["src"], fill=pad_cols(rows(r["gy"]), Ck))
    ld_dw = k * k * Cin
    numel = Cout * ld_dw
    want = _wgrad_want(r).reshape(-1)
    # slabs + reduce (twice: += semantics), at an odd offset of the gradient vector
    splits = fn["ep24_conv_wgrad_splits"](B, H, W, Cin, Ck, k, s)
    assert splits >= 1
    slab = torch.full((splits * numel,), float("nan"), device=DEV)
    call("conv_wgrad_slab_bf16", xb.ptr(), xb.ld, gb.ptr(), gb.ld, ptr(slab), splits * numel, ld_dw, Cout, Cin, B, H, W, Cin, Ck, k, s, sp())
    assert not torch.isnan(slab).any(), "a slab element nobody wrote"
    g = torch.zeros(8 + numel, device=DEV)
    desc = torch.tensor([[8, numel, splits, 0]], dtype=torch.int64, device=DEV)
    call("wgrad_reduce", ptr(desc), 1, numel, ptr(g), ptr(slab), sp())
    assert torch.equal(g[8:].cpu(), want) and float(g[:8].abs().max()) == 0.0
    call("wgrad_reduce", ptr(desc), 1, numel, ptr(g), ptr(slab), sp())
    assert torch.equal(g[8:].cpu(), 2 * want)
    # the atomic form
    dw = torch.zeros(numel, device=DEV)
    for rep in (1, 2):
        call("conv_wgrad_bf16", xb.ptr(), xb.ld, gb.ptr(), gb.ld, ptr(dw), ld_dw, Cout, Cin, B, H, W, Cin, Ck, k, s, sp())
        assert torch.equal(dw.cpu(), rep * want), rep
    # the grouped launch, as a group of one with the caller's split count
    gs = 2
    slab2 = torch.full((gs * numel,), float("nan"), device=DEV)
    row = torch.tensor([[xb.ptr(), xb.ld, gb.ptr(), gb.ld, slab2.data_ptr(), gs * numel, ld_dw, Cout, Cin, B, H, W, Cin, Ck, k, s, gs]], dtype=torch.int64)
    call("conv_wgrad_group_bf16", row.data_ptr(), 1, sp())
    torch.cuda.synchronize()
    assert not torch.isnan(slab2).any(), "a slab element nobody wrote (grouped)"
    assert torch.equal(slab2.view(gs, numel).sum(0).cpu(), want)
    # the operands are untouched
    xb.check(rows(r["x"]), "x after the weight gradient")
    assert fn["ep24_conv_ring_timeouts"]() == 0


@pytest.mark.parametrize("shape,cout_v,cin_v", [((2, 12, 16, 24, 3, 1), 19, 13), ((5, 9, 72, 200, 3, 1), 197, 70), ((3, 17, 200, 136, 1, 1), 132, 195)],
                         ids=["3x3-19of24-13of16", "3x3-197of200-70of72", "1x1-132of136-195of200"])
def test_conv_wgrad_valid_region_and_row_padding(shape, cout_v, cin_v):
    """ld_dw > taps * cin_valid with cout_valid / cin_valid below the padded counts: the valid region exact, the padding of every
    row left untouched (slab and atomic form), strided x / dy."""
    call, ptr, sp, fn = _abi()
    B, H, W, Cin, Cout, k, s, OH, OW = _shape(shape)
    r = ref_d1(shape)
    L = LAYOUTS["slice"]
    xb = Buf(B * H * W, Cin, *L["src"], fill=rows(r["x"]))
    gb = Buf(B * OH * OW, Cout, *L["src"], fill=rows(r["gy"]))
    valid = k * k * cin_v
    ld_dw = valid + 5
    want = _wgrad_want(r, cout_v, cin_v)                            # [cout_v][taps * cin_v]
    splits = fn["ep24_conv_wgrad_splits"](B, H, W, Cin, Cout, k, s)
    slab = torch.full((splits, cout_v, ld_dw), float("nan"), device=DEV)
    call("conv_wgrad_slab_bf16", xb.ptr(), xb.ld, gb.ptr(), gb.ld, ptr(slab), slab.numel(), ld_dw, cout_v, cin_v, B, H, W, Cin, Cout, k, s, sp())
    assert not torch.isnan(slab[:, :, :valid]).any(), "a slab element nobody wrote"
    assert torch.equal(slab[:, :, :valid].sum(0).cpu(), want)
    assert bool(torch.isnan(slab[:, :, valid:]).all()), "the row padding of a slab was written"
    dw = torch.full((cout_v, ld_dw), SENT, device=DEV)
    dw[:, :valid] = 0
    for rep in (1, 2):
        call("conv_wgrad_bf16", xb.ptr(), xb.ld, gb.ptr(), gb.ld, ptr(dw), ld_dw, cout_v, cin_v, B, H, W, Cin, Cout, k, s, sp())
        assert torch.equal(dw[:, :valid].cpu(), rep * want), rep
    assert bool((dw[:, valid:] == SENT).all()), "the row padding of dw was written"


# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("act", [0, 2], ids=["linear", "relu"])
@pytest.mark.parametrize("shape,kid", [((8, 80, 64, 128, 3, 1), RING), ((2, 12, 16, 24, 3, 1), TILED), ((2, 19, 120, 68, 1, 1), STREAM), ((2, 12, 16, 20, 3, 1), TILED),
                                       ((2, 24, 256, 128, 1, 1), STREAM)],
                         ids=["ring", "tiled", "1x1-n68", "tiled-n20", "1x1"])
def test_conv_infer_unit_exact(shape, kid, act):
    """Eval-mode unit y = act(conv(x) + bias) + residual with integer bias and residual: one rounding, exact.  Strided residual and
    destination (channel slices); a ring shape, a tiled shape, 1x1 shapes and Cout % 8 == 4 shapes (the 8-byte stores)."""
    call, ptr, sp, fn = _abi()
    B, H, W, Cin, Cout, k, s, OH, OW = _shape(shape)
    assert fn["ep24_conv_kernel_for"](0, B, H, W, Cin, Cout, k, s, 0, 0) == kid
    r = ref_d1(shape)
    M = B * OH * OW
    bias = _ints((Cout,), 7)
    res = _ints((M, Cout), 8)
    v = rows(r["y"]) + bias
    want = ((v.clamp(min=0) if act == 2 else v) + res).to(BF)
    assert float((want.double() != (v.clamp(min=0) if act == 2 else v) + res).double().mean()) >= 0.01
    wf = r["w"].permute(0, 2, 3, 1).contiguous().to(BF).to(DEV)
    xb = Buf(B * H * W, Cin, 24, 8, fill=rows(r["x"]))
    rb = Buf(M, Cout, 24, 8, fill=res)
    yb = Buf(M, Cout, 40, 16)
    bd = bias.float().to(DEV)
    call("conv_fwd_infer_bf16", xb.ptr(), xb.ld, ptr(wf), ptr(bd), act, rb.ptr(), rb.ld, yb.ptr(), yb.ld, B, H, W, Cin, Cout, k, s, sp())
    yb.check(want, "eval-mode y")
    rb.check(res, "the residual after the launch")
    assert fn["ep24_conv_ring_timeouts"]() == 0


@pytest.mark.parametrize("f32", [True, False], ids=["fp32", "bf16"])
@pytest.mark.parametrize("Cout,col0", [(27, 0), (80, 28)])
def test_conv_head_form_exact(Cout, col0, f32):
    """The predictor form: 1x1 conv over a channel slice, + integer bias, pixel (n, hw) to row n * A + a0 + hw of a [B, A, ncols]
    tensor at column col0 - fp32 and bf16 output; every other row and column untouched."""
    call, ptr, sp, fn = _abi()
    B, H, W, Cin, A, a0, ncols = 3, 12, 12, 64, 200, 31, 108
    shape = (B, H, Cin, Cout, 1, 1)
    assert fn["ep24_conv_kernel_for"](0, B, H, W, Cin, Cout, 1, 1, 1 if f32 else 0, 1) == TILED
    r = ref_d1(shape)
    bias = _ints((Cout,), 7)
    want = (rows(r["y"]) + bias).reshape(B, H * W, Cout)
    dt = torch.float32 if f32 else BF
    xb = Buf(B * H * W, Cin, 32, 16, fill=rows(r["x"]))
    wf = r["w"].reshape(Cout, Cin).to(BF).to(DEV)
    bd = bias.float().to(DEV)
    exp = torch.full((B, A, ncols), SENT, dtype=dt)
    out = exp.to(DEV)
    call("conv_fwd_bf16", xb.ptr(), xb.ld, ptr(wf), ptr(out, col0), ncols, 1 if f32 else 0, A, a0, ptr(bd), None, 1, B, H, W, Cin, Cout, 1, 1, sp())
    exp[:, a0:a0 + H * W, col0:col0 + Cout] = want.to(dt)
    got = out.cpu()
    assert torch.equal(got, exp), (got != exp).nonzero()[:4].tolist()


def test_conv_pointer_form_epilogue_beyond_2gib():
    """A destination whose extent exceeds 2 GiB through its row stride (4 225 rows of 262 144 bf16): the wide epilogue's pointer form
    (dst_bytes == 0) - forward and accumulated input gradient.  Only the written columns and their 64 neighbours are filled and read."""
    call, ptr, sp, fn = _abi()
    shape = (1, 65, 16, 64, 3, 1)
    B, H, W, Cin, Cout, k, s, OH, OW = _shape(shape)
    M, LD = B * H * W, 262144
    assert ((M - 1) * LD + Cout) * 2 >= 2 ** 31
    assert fn["ep24_conv_kernel_for"](0, B, H, W, Cin, Cout, k, s, 0, 0) == TILED
    r = ref_d1(shape)
    assert r["frac_forms"] >= 0.01
    wf = r["w"].permute(0, 2, 3, 1).contiguous().to(BF).to(DEV)
    wd = r["w"].permute(1, 2, 3, 0).contiguous().to(BF).to(DEV)
    x = rows(r["x"]).to(BF).to(DEV)
    gy = rows(r["gy"]).to(BF).to(DEV)
    big = torch.empty(M, LD, dtype=BF, device=DEV)
    big[:, :Cout + 64] = SENT
    call("conv_fwd_bf16", ptr(x), Cin, ptr(wf), ptr(big), LD, 0, 0, 0, None, None, 1, B, H, W, Cin, Cout, k, s, sp())
    got = big[:, :Cout + 64].cpu()
    assert torch.equal(got[:, :Cout], rows(r["y"]).to(BF)) and bool((got[:, Cout:] == SENT).all())
    big[:, :Cin + 64] = SENT
    big[:, :Cin] = r["old"].to(BF).to(DEV)
    call("conv_dgrad_bf16", ptr(gy), Cout, ptr(wd), ptr(big), LD, 1, B, H, W, Cin, Cout, k, s, sp())
    got = big[:, :Cin + 64].cpu()
    assert torch.equal(got[:, :Cin], r["dx2_two"]) and bool((got[:, Cin:] == SENT).all())
