"""The kernels of csrc/backbone_ops.hip (im2col, the ReLU pair, both max pools, avgpool2, chanscale, colstats, stats_gather, incr_i64)
and of csrc/dwconv.hip (depthwise forward with batch statistics, input gradient, slab weight gradient) against
tests/backbone_reference.py, through the C ABI.  tests/test_backbone_reference.py shows without a GPU that the references equal torch's
max_pool2d / avg_pool2d / unfold / relu / conv2d(groups=C) with their autograd and that thirteen mutants are rejected on these inputs.

Every buffer a call reads or writes sits between two guards of 64 sentinel elements, whole buffers are compared - the pad columns of
strided rows and every buffer a call must not write included.  NaN equals NaN; every other pattern only itself.  Every family runs a
non-square map, tight rows (ld = C) and a slice 8 or 16 channels into wider rows (how the concatenation buffers hand out slices), and
both accumulate forms where the entry point has them.  What makes a case exact or discriminating is asserted on the reference before
any launch (dw_exact_conditions; the draw conditions of the pools are in the CPU module).

Bit for bit on any draw, special values included: both max pools forward (values and codes; ties, all-negative maps, NaN, -inf, -0,
random patterns), the maxpool3s2 backward (its fp32 order is fixed: kh outer, kw inner, then the old value, one rounding), the maxpool2
backward, both directions of avgpool2, chanscale, im2col, the ReLU pair (ATen's answers: NaN stays NaN, -0 stays -0, a NaN output passes
the gradient), stats_gather, incr_i64.  Bit for bit on integer draws: the depthwise z, dx in both forms, the slab sum, the statistics
summed over the replicas - those of the fp32 ACCUMULATOR, which differ from those of the stored bf16 z in most channels of these draws -
and colstats.  Against float64 under derived bounds (normal draws through bf16, w = 0.3 N(0, 1) in fp32; u = 2^-24; the full derivation
is the docstring of backbone_reference.py):
  z, dx      nine fused multiply-adds from a = 0, each one rounding of a sum that carries the earlier errors:
             |a - a64| <= ((1 + u)^9 - 1) sum|x w| =: e9; the accumulate form is one more rounded addition with |old| among the terms;
             the store adds at most half a bf16 ulp of the result
  sums       N fp32 terms added in ANY tree: every term passes at most N - 1 rounded additions, ((1 + u)^(N - 1) - 1) sum|terms|, which
             covers a lane's chain, the fold over the row slots and whatever pixels a workgroup owns; on top the terms' own error
             (none for sum x and for x dz, which is exact in fp32; one rounding for x^2; e9, and 2 |a| e9 + e9^2 + u (|a| + e9)^2 for
             a and fl(a a) of the depthwise statistics) and 2^-21 per workgroup word for the rounding to 2^-20 fixed point; the
             workgroups' words add as integers, exactly

The sizes come from the constants of the kernels:
  MAX_BLOCKS = 16384 workgroups of 256 lanes in cap_grid (backbone_ops.hip), one 8-channel item per lane: a grid-stride loop makes a second
      trip beyond 4 194 304 items - one case per kernel in backbone_reference.CAP (1 x 3 and 2 x 2 maps with up to 33 554 440 channels: the
      fewest bytes per item) and a 683 x 683 image with ld = 72 for im2col (466 489 rows x 9 chunks)
  ep24_colstats: one workgroup per 16 rows, at most 1024: M = 16 400 rows is the first beyond; 256 / (C / 8) row lanes: C = 24 and 200
      leave lanes without a row slot, C = 2048 gives a workgroup one row
  dwconv.hip: tpr = C / 8 lanes per row and rpb = 256 / tpr row slots, rpb = 1 from tpr >= 256 (C = 2048); C = 2056 makes a second channel
      pass with one group; the forward's grid of ~4 pixels per thread decides how many of R = 8 replicas are written (one workgroup: only
      replica 0); the weight gradient has one split per 16 rpb pixels, at most 256: C = 2048 with 4097 pixels is the first shape capped

Largest err / bound measured on an MI355X (the tests print them as BACKBONE-ERR before they assert):
  depthwise z            0.9997    (1, 3, 4, 2056) stride 1; 0.987 - 0.9995 elsewhere: nearly all of it the final rounding to bf16
  depthwise dx           0.9998    both accumulate forms, (1, 6, 5, 24) and (1, 3, 4, 2056) stride 2; the final rounding again
  depthwise statistics   0.793     (1, 3, 4, 2056) stride 2, four pixels: the fixed-point rounding is most of the bound; 0.03 - 0.31 elsewhere
  depthwise slab sum     0.318     (1, 3, 4, 2056) stride 2; 0.005 - 0.13 elsewhere
  colstats               0.982     M = 1, C = 2048, where the bound is the 2^-21 of the fixed-point rounding alone (0.875 at C = 200);
                                   0.20 at M = 15, 0.12 at M = 17, 0.003 at M = 300

Open item: the fused ReLU of the BatchNorm kernels (act_fwd, fmaxf) turns a NaN into 0 like the ReLU pair did before this module; it
belongs to those kernels and to tests/test_gpu_bn_exact.py and is not changed or pinned here.
"""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import backbone_reference as R  # noqa: E402
import update_reference as U  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
E_ARG, E_UNSUPPORTED = -1, -3
S16 = U.SENT16
PAIRS = {"tight": ("tight", "tight"), "slice": ("slice8", "slice16")}       # the layouts of a call's first and second map


def _abi():
    from ep24._lib import call, lib, stream_ptr
    return call, stream_ptr, lib()


def G(n, kind, fill=None):
    return U.Guarded(n, kind, DEV, fill)


def sync():
    torch.cuda.synchronize()


class Rows:
    """A [P, C] map of bf16 patterns as a slice of [P, ld] rows inside a guarded buffer; everything around the slice is sentinel."""

    def __init__(self, mat, C, layout, P=None):
        self.off, behind = R.LAYOUTS[layout]
        self.C, self.ld = C, self.off + C + behind
        self.P = P if mat is None else int(np.asarray(mat).size // C)
        self.img = np.full((self.P, self.ld), S16, dtype=np.uint16)
        if mat is not None:
            self.img[:, self.off:self.off + C] = np.asarray(mat, dtype=np.uint16).reshape(self.P, C)
        self.buf = G(self.P * self.ld, "bf16", self.img.reshape(-1))

    def ptr(self):
        return self.buf.ptr(self.off)

    def unchanged(self, what):
        self.buf.check(self.img.reshape(-1), what)

    def holds(self, mat, what):
        want = self.img.copy()
        want[:, self.off:self.off + self.C] = np.asarray(mat, dtype=np.uint16).reshape(self.P, self.C)
        self.buf.check(want.reshape(-1), what)

    def values(self):
        """the slice as float64 [P, C]"""
        win, _ = self.buf.read()
        return R.widen(win.reshape(self.P, self.ld)[:, self.off:self.off + self.C]).astype(np.float64)

    def accept(self, what):
        """the slice was compared under a bound: everything else bit for bit"""
        win, _ = self.buf.read()
        self.holds(win.reshape(self.P, self.ld)[:, self.off:self.off + self.C].copy(), what)


# ---------------------------------------------------------------------------------------------------------------------------
# max pools
def _maxpool(kind, shape, draw, layout):
    call, sp, _ = _abi()
    B, H, W, C = shape
    fwd, bwd = ("maxpool3s2_fwd", "maxpool3s2_bwd") if kind == 3 else ("maxpool2_fwd", "maxpool2_bwd")
    R.pool_conditions(kind, shape, draw)                              # before any launch
    x, vals, codes = R.pool_case(kind, shape, draw)
    Q = vals.size // C
    la, lb = PAIRS[layout]
    xr, yr, idx = Rows(R.bits_of(x), C, la), Rows(None, C, lb, P=Q), G(Q * C, "u8")
    call(fwd, xr.ptr(), xr.ld, yr.ptr(), yr.ld, idx.ptr(), B, H, W, C, sp())
    sync()
    yr.holds(R.bits_of(vals), "y")
    idx.check(codes.reshape(-1), "winner codes")
    xr.unchanged("x")
    dy, old = R.pool_bwd_case(kind, shape)
    for acc in (0, 1):
        dyr, dxr, ci = Rows(R.bits_of(dy), C, lb), Rows(R.bits_of(old) if acc else None, C, la, P=B * H * W), G(Q * C, "u8", codes.reshape(-1))
        call(bwd, dyr.ptr(), dyr.ld, ci.ptr(), dxr.ptr(), dxr.ld, acc, B, H, W, C, sp())
        sync()
        want = R.maxpool3s2_bwd_ref(dy, codes, old, acc, H, W) if kind == 3 else R.maxpool2_bwd_ref(dy, codes, old, acc)
        dxr.holds(want, "dx, accumulate %d" % acc)
        dyr.unchanged("dy")
        ci.check(codes.reshape(-1), "codes")


@pytest.mark.parametrize("layout", list(PAIRS))
@pytest.mark.parametrize("draw", list(R.POOL_DRAWS))
@pytest.mark.parametrize("shape", R.POOL3_SHAPES, ids=str)
def test_maxpool3s2_exact(shape, draw, layout):
    _maxpool(3, shape, draw, layout)


@pytest.mark.parametrize("layout", list(PAIRS))
@pytest.mark.parametrize("draw", list(R.POOL_DRAWS))
@pytest.mark.parametrize("shape", R.POOL2_SHAPES, ids=str)
def test_maxpool2_exact(shape, draw, layout):
    _maxpool(2, shape, draw, layout)


@pytest.mark.parametrize("layout", list(PAIRS))
@pytest.mark.parametrize("draw", list(R.AVG_DRAWS))
@pytest.mark.parametrize("shape", R.POOL2_SHAPES, ids=str)
def test_avgpool2_exact(shape, draw, layout):
    call, sp, _ = _abi()
    B, H, W, C = shape
    x, dy, old = R.avg_case(shape, draw)
    la, lb = PAIRS[layout]
    Q = B * (H // 2) * (W // 2)
    xr, yr = Rows(R.bits_of(x), C, la), Rows(None, C, lb, P=Q)
    call("avgpool2_fwd", xr.ptr(), xr.ld, yr.ptr(), yr.ld, B, H, W, C, sp())
    sync()
    yr.holds(R.avgpool2_ref(x), "y")
    xr.unchanged("x")
    for acc in (0, 1):
        dyr, dxr = Rows(R.bits_of(dy), C, lb), Rows(R.bits_of(old) if acc else None, C, la, P=B * H * W)
        call("avgpool2_bwd", dyr.ptr(), dyr.ld, dxr.ptr(), dxr.ld, acc, B, H, W, C, sp())
        sync()
        dxr.holds(R.avgpool2_bwd_ref(dy, old, acc), "dx, accumulate %d" % acc)
        dyr.unchanged("dy")


CHANSCALE = [(1, 1, 8), (3, 5, 24), (2, 17, 8), (1, 300, 24)]


@pytest.mark.parametrize("layout", list(R.LAYOUTS))
@pytest.mark.parametrize("B,HW,C", CHANSCALE)
def test_chanscale_exact(B, HW, C, layout):
    call, sp, _ = _abi()
    x, keep = R.chanscale_case(B, HW, C)
    xr, kg = Rows(R.bits_of(x), C, layout), G(B * C, "f32", U.bits32(keep).reshape(-1))
    call("chanscale", xr.ptr(), xr.ld, kg.ptr(), B, HW, C, sp())
    sync()
    xr.holds(R.chanscale_ref(x, keep), "x")
    kg.check(U.bits32(keep).reshape(-1), "keep")


def _im2col(case):
    call, sp, _ = _abi()
    B, C, H, W, k, s, p, ld = case
    bits = R.im2col_image(case)
    want = R.im2col_ref(bits, k, s, p, ld)
    img, rows = G(bits.size, "f32", bits.reshape(-1)), G(want.size, "bf16")
    call("im2col_bf16", img.ptr(), rows.ptr(), ld, B, C, H, W, k, s, p, sp())
    sync()
    got = rows.check(want.reshape(-1), "rows")
    assert not got.reshape(-1, ld)[:, k * k * C:].any(), "a pad column is not +0"
    img.check(bits.reshape(-1), "images")


@pytest.mark.parametrize("case", R.IM2COL_CASES, ids=str)
def test_im2col_exact(case):
    _im2col(case)


def test_im2col_beyond_the_grid_cap():
    assert R.im2col_items(R.IM2COL_BIG) > R.MAX_ITEMS
    _im2col(R.IM2COL_BIG)


def _relu(M, C, layout, yb, dyb):
    call, sp, _ = _abi()
    la, lb = PAIRS[layout]
    yr = Rows(yb, C, la)
    call("relu_fwd", yr.ptr(), yr.ld, M, C, sp())
    sync()
    out = R.relu_fwd_ref(yb)
    yr.holds(out, "y")
    dyr, outr = Rows(dyb, C, lb), Rows(out, C, la)
    call("relu_bwd", dyr.ptr(), dyr.ld, outr.ptr(), outr.ld, M, C, sp())
    sync()
    dyr.holds(R.relu_bwd_ref(dyb, out), "dy")
    outr.unchanged("y")


@pytest.mark.parametrize("layout", list(PAIRS))
@pytest.mark.parametrize("M,C", R.ROWS_SHAPES)
def test_relu_pair_is_aten(M, C, layout):
    """NaN stays NaN and passes the gradient, -0 stays -0 and stops it, as torch.relu and threshold_backward"""
    yb, dyb = R.relu_case(M, C)
    assert U.is_nan16(yb).any() and (yb == 0x8000).any() and not U.is_nan16(dyb.reshape(-1)[:6]).any()
    _relu(M, C, layout, yb, dyb)


# ---------------------------------------------------------------------------------------------------------------------------
# statistics
def _colstats(M, C, draw, layout, x=None):
    """x [M, C] in a slice; stats int64 [3][2][ld_stats] pre-filled, the call's pointer c0 channels in: replica 0 gets the sums added
    at c0 .. c0 + C, every other word stays"""
    call, sp, _ = _abi()
    x = R.colstats_case(C, draw)[:M] if x is None else x
    c0, ld_s = (0, C) if layout == "tight" else (8, C + 16)
    pre = R.stats_prefill(3 * 2 * ld_s, M + C).reshape(3, 2, ld_s)
    xr, st = Rows(R.bits_of(x), C, layout), G(pre.size, "i64", pre.reshape(-1))
    ref = R.colstats_ref(x)
    if draw == "integer":
        assert float(ref.max()) < 2 ** 24
    call("colstats", xr.ptr(), xr.ld, st.ptr(c0), ld_s, M, C, sp())
    sync()
    want = pre.copy()
    if draw == "integer":
        want[0, :, c0:c0 + C] += R.fix_words(ref)
        ratio = 0.0
    else:
        got = st.read()[0].reshape(3, 2, ld_s)
        delta = (got[0, :, c0:c0 + C] - pre[0, :, c0:c0 + C]).astype(np.float64) / R.FIX
        ratio = float((np.abs(delta - ref) / R.colstats_bound(x, R.colstats_blocks(M))).max())
        print("BACKBONE-ERR colstats M %d C %d: err / bound %.4f" % (M, C, ratio))
        assert ratio <= 1.0, ratio
        want[0, :, c0:c0 + C] = got[0, :, c0:c0 + C]
    st.check(want.reshape(-1), "stats M %d" % M)
    xr.unchanged("x")
    return ratio


@pytest.mark.parametrize("layout", ["tight", "slice8"])
@pytest.mark.parametrize("draw", ["integer", "general"])
@pytest.mark.parametrize("C", R.COLSTATS_C)
def test_colstats(C, draw, layout):
    for M in R.COLSTATS_M:
        _colstats(M, C, draw, layout)


def test_colstats_beyond_the_workgroup_cap():
    M, C = R.COLSTATS_BIG
    assert (M + 15) // 16 > R.COLSTATS_BLOCKS
    _colstats(M, C, "integer", "slice8", x=R.integer_draw((M, C), 5))


@pytest.mark.parametrize("C,ld_src,reps", R.GATHER_CASES)
def test_stats_gather_exact(C, ld_src, reps):
    call, sp, _ = _abi()
    src = R.stats_prefill(reps * 2 * ld_src, C).reshape(reps, 2, ld_src)
    sg, dg = G(src.size, "i64", src.reshape(-1)), G(reps * 2 * C, "i64")
    call("stats_gather", sg.ptr(), ld_src, dg.ptr(), C, reps, sp())
    sync()
    dg.check(R.stats_gather_ref(src, C).reshape(-1), "dst")
    sg.check(src.reshape(-1), "src")


def test_incr_i64_twice():
    call, sp, _ = _abi()
    for start in (41, -1, 2 ** 40):
        p = G(1, "i64", np.array([start], dtype=np.int64))
        call("incr_i64", p.ptr(), sp())
        call("incr_i64", p.ptr(), sp())
        sync()
        p.check(np.array([start + 2], dtype=np.int64), "counter")


# ---------------------------------------------------------------------------------------------------------------------------
# depthwise
def _dw_fwd(shape, stride, draw, form, layout):
    call, sp, _ = _abi()
    B, H, W, C = shape
    k = R.dw_case(shape, stride, draw)
    exact = draw != "general"
    if exact:
        R.dw_exact_conditions(k, shape in R.DW_MAIN)                 # before any launch
    la, lb = PAIRS[layout]
    M = k["M"]
    reps = {"null": 0, "r1": 1, "r8": 8}[form]
    pre = R.stats_prefill(max(reps, 1) * 2 * C, sum(shape)).reshape(-1, 2, C)
    xr, zr, wg = Rows(R.bits_of(k["x"]), C, la), Rows(None, C, lb, P=M), G(C * 9, "f32", U.bits32(k["w"]).reshape(-1))
    st = G(pre.size, "i64", pre.reshape(-1)) if reps else None
    call("dwconv_fwd_bf16", xr.ptr(), xr.ld, wg.ptr(), zr.ptr(), zr.ld, st.ptr() if reps else None, reps, B, H, W, C, 3, stride, sp())
    sync()
    ratios = {}
    if exact:
        zr.holds(R.bf16_from_f64(k["acc"]), "z")
    else:
        z = zr.values().reshape(k["acc"].shape)
        ratios["z"] = float((np.abs(z - k["acc"]) / R.dw_z_bound(k["mag"], z)).max())
        print("BACKBONE-ERR dwconv fwd %s stride %d %s: z err / bound %.4f" % (shape, stride, form, ratios["z"]))
        assert ratios["z"] <= 1.0, ratios
        zr.accept("z")
    xr.unchanged("x")
    wg.check(U.bits32(k["w"]).reshape(-1), "w")
    if reps:
        got = st.check(st.read()[0], "stats guards").reshape(reps, 2, C)
        delta = got - pre
        grid = R.dw_grid(M, C)
        assert not delta[min(grid, reps):].any(), "a replica beyond the grid's %d workgroups changed" % grid
        if exact:
            assert np.array_equal(delta.sum(0), R.fix_words(k["stats"])), "the statistics are not those of the fp32 accumulator"
        else:
            err = np.abs(delta.sum(0).astype(np.float64) / R.FIX - k["stats"])
            ratios["stats"] = float((err / R.dw_stats_bound(k["acc"], k["mag"], grid)).max())
            print("BACKBONE-ERR dwconv fwd %s stride %d %s: statistics err / bound %.4f (%d workgroups)" % (shape, stride, form, ratios["stats"], grid))
            assert ratios["stats"] <= 1.0, ratios
    return ratios


def _dw_dgrad(shape, stride, draw, layout):
    call, sp, _ = _abi()
    B, H, W, C = shape
    k = R.dw_case(shape, stride, draw)
    la, lb = PAIRS[layout]
    ratios = {}
    for acc in (0, 1):
        dzr, dxr, wg = Rows(R.bits_of(k["dz"]), C, lb), Rows(R.bits_of(k["old"]) if acc else None, C, la, P=B * H * W), G(C * 9, "f32", U.bits32(k["w"]).reshape(-1))
        call("dwconv_dgrad_bf16", dzr.ptr(), dzr.ld, wg.ptr(), dxr.ptr(), dxr.ld, acc, B, H, W, C, 3, stride, sp())
        sync()
        tot = k["dx"] + (k["old"] if acc else 0.0)
        if draw != "general":
            dxr.holds(R.bf16_from_f64(tot), "dx, accumulate %d" % acc)
        else:
            got = dxr.values().reshape(shape)
            bound = R.dw_z_bound(k["dmag"] + (np.abs(k["old"]) if acc else 0.0), got, 9 + acc)
            ratios["dx%d" % acc] = float((np.abs(got - tot) / bound).max())
            print("BACKBONE-ERR dwconv dgrad %s stride %d accumulate %d: err / bound %.4f" % (shape, stride, acc, ratios["dx%d" % acc]))
            assert ratios["dx%d" % acc] <= 1.0, ratios
            dxr.accept("dx")
        dzr.unchanged("dz")
        wg.check(U.bits32(k["w"]).reshape(-1), "w")
    return ratios


def _dw_wgrad(shape, stride, draw, layout):
    """The slab holds one row more than the splits: it, and the guards, stay untouched"""
    call, sp, lib = _abi()
    B, H, W, C = shape
    k = R.dw_case(shape, stride, draw)
    la, lb = PAIRS[layout]
    splits = lib.fn["ep24_dwconv_wgrad_splits"](B, H, W, C, stride)
    assert splits == R.dw_splits_ref(B, H, W, C, stride)
    xr, dzr, slab = Rows(R.bits_of(k["x"]), C, la), Rows(R.bits_of(k["dz"]), C, lb), G((splits + 1) * C * 9, "f32")
    call("dwconv_wgrad_slab_bf16", xr.ptr(), xr.ld, dzr.ptr(), dzr.ld, slab.ptr(), splits * C * 9, B, H, W, C, 3, stride, sp())
    sync()
    win = slab.check(slab.read()[0], "slab guards").reshape(splits + 1, C, 3, 3)
    assert bool(np.all(win[splits] == U.SENT32)), "the row behind the last split was written"
    assert not U.is_nan32(win[:splits]).any()
    total = U.from_bits32(win[:splits].reshape(-1)).reshape(splits, C, 3, 3).astype(np.float64).sum(0)
    xr.unchanged("x")
    dzr.unchanged("dz")
    if draw != "general":
        assert np.array_equal(total, k["dw"]), "slab sum"
        return {}
    bound = R.dw_sum_bound(k["wmag"], k["M"])
    ratio = float((np.abs(total - k["dw"]) / np.maximum(bound, 1e-300)).max())
    print("BACKBONE-ERR dwconv wgrad %s stride %d: slab sum err / bound %.4f (%d splits)" % (shape, stride, ratio, splits))
    assert ratio <= 1.0, ratio
    return {"dw": ratio}


DW_EXACT = [(s, "integer") for s in R.DW_MAIN + R.DW_BORDER] + [(s, "ternary") for s in R.DW_TERNARY]
DW_IDS = ["x".join(map(str, s)) for s, _ in DW_EXACT]


@pytest.mark.parametrize("layout", list(PAIRS))
@pytest.mark.parametrize("form", R.DW_STATS_FORMS)
@pytest.mark.parametrize("stride", [1, 2])
@pytest.mark.parametrize("shape,draw", DW_EXACT, ids=DW_IDS)
def test_dwconv_fwd_exact(shape, draw, stride, form, layout):
    _dw_fwd(shape, stride, draw, form, layout)


@pytest.mark.parametrize("layout", list(PAIRS))
@pytest.mark.parametrize("stride", [1, 2])
@pytest.mark.parametrize("shape,draw", DW_EXACT, ids=DW_IDS)
def test_dwconv_grads_exact(shape, draw, stride, layout):
    R.dw_exact_conditions(R.dw_case(shape, stride, draw), shape in R.DW_MAIN)
    _dw_dgrad(shape, stride, draw, layout)
    _dw_wgrad(shape, stride, draw, layout)


@pytest.mark.parametrize("stride", [1, 2])
@pytest.mark.parametrize("shape", R.DW_GENERAL, ids=str)
def test_dwconv_general_within_the_bounds(shape, stride):
    r = {}
    for form in ("r1", "r8"):
        for key, v in _dw_fwd(shape, stride, "general", form, "slice").items():
            r[key] = max(r.get(key, 0.0), v)
    r.update(_dw_dgrad(shape, stride, "general", "slice"))
    r.update(_dw_wgrad(shape, stride, "general", "slice"))
    print("BACKBONE-ERR dwconv %s stride %d: err / bound %s" % (shape, stride, " ".join("%s %.4f" % kv for kv in sorted(r.items()))))
    assert max(r.values()) <= 1.0, r


def test_dwconv_wgrad_at_the_split_cap():
    B, H, W, C = R.DW_WGRAD_CAP
    assert -(-B * H * W // 16) > R.DW_SPLIT_CAP and R.dw_rpb(C) == 1
    R.dw_exact_conditions(R.dw_case(R.DW_WGRAD_CAP, 1, "ternary"), False)
    _dw_wgrad(R.DW_WGRAD_CAP, 1, "ternary", "tight")


def test_dwconv_wgrad_splits():
    _, _, lib = _abi()
    f = lib.fn["ep24_dwconv_wgrad_splits"]
    for C in (8, 24, 200, 2048, 2056):
        rpb = R.dw_rpb(C)
        for M in (1, 16 * rpb, 16 * rpb + 1, 255 * 16 * rpb + 1, 300 * 16 * rpb):
            for stride in (1, 2):
                assert f(1, 1, M * stride, C, stride) == R.dw_splits_ref(1, 1, M * stride, C, stride) == min(256, -(-M // (16 * rpb))), (C, M, stride)
    for bad in ((0, 4, 4, 8, 1), (1, 0, 4, 8, 1), (1, 4, 0, 8, 1), (1, 4, 4, 12, 1), (1, 4, 4, 0, 1), (1, 4, 4, 8, 3), (1, 4, 4, 8, 0)):
        assert f(*bad) == -1 == R.dw_splits_ref(*bad), bad


# ---------------------------------------------------------------------------------------------------------------------------
# one case per kernel beyond the 16 384-workgroup cap of cap_grid: integer draws through tables, one vectorised pass on the host
def _cap_ints(name, shape, seed, lim):
    assert R.cap_items(name) > R.MAX_ITEMS
    q = R.small_int_draw(shape, seed, lim)
    return q, R.quarter_bits(q.astype(np.int16) * 4)


def test_cap_relu_pair():
    B, H, W, C = R.CAP["relu_fwd"]
    assert R.cap_items("relu_fwd") > R.MAX_ITEMS and R.CAP["relu_bwd"] == R.CAP["relu_fwd"]
    n = H * W * C
    yb, dyb = U.bf16_rne(U.random_bits(n, 1)), U.bf16_rne(U.random_bits(n, 2))
    _relu(H * W, C, "tight", yb.reshape(H * W, C), dyb.reshape(H * W, C))


def test_cap_chanscale():
    call, sp, _ = _abi()
    B, H, W, C = R.CAP["chanscale"]
    q, xb = _cap_ints("chanscale", (B, H * W, C), 3, 8)
    kq = R.small_int_draw((B, C), 4, 4)                                   # keep = kq / 4: every product is a bf16 number
    keep = kq.astype(np.float32) * np.float32(0.25)
    xr, kg = Rows(xb, C, "tight"), G(B * C, "f32", U.bits32(keep).reshape(-1))
    call("chanscale", xr.ptr(), xr.ld, kg.ptr(), B, H * W, C, sp())
    sync()
    prod = q.astype(np.int16) * kq.astype(np.int16)[:, None, :]
    want = R.quarter_bits(prod)
    want[(prod == 0) & ((q < 0)[...] ^ (kq < 0)[:, None, :])] = 0x8000    # 0 * negative and negative * 0 are -0
    xr.holds(want, "x")


def _cap_maxpool(kind):
    call, sp, _ = _abi()
    fwd, bwd = ("maxpool3s2_fwd", "maxpool3s2_bwd") if kind == 3 else ("maxpool2_fwd", "maxpool2_bwd")
    ref = R.maxpool3s2_ref if kind == 3 else R.maxpool2_ref
    B, H, W, C = R.CAP[fwd]
    q, xb = _cap_ints(fwd, (B, H, W, C), 5, 2)
    vals, codes = ref(q.astype(np.float32))
    Q = vals.size // C
    xr, yr, idx = Rows(xb, C, "tight"), Rows(None, C, "tight", P=Q), G(Q * C, "u8")
    call(fwd, xr.ptr(), xr.ld, yr.ptr(), yr.ld, idx.ptr(), B, H, W, C, sp())
    sync()
    yr.holds(R.quarter_bits(vals.astype(np.int16) * 4), "y")
    idx.check(codes.reshape(-1), "winner codes")
    del xr, yr, idx
    B, H, W, C = R.CAP[bwd]
    q, _ = _cap_ints(bwd, (B, H, W, C), 6, 2)
    _, codes = ref(q.astype(np.float32))
    g, old = R.small_int_draw(codes.shape, 7, 8), R.small_int_draw((B, H, W, C), 8, 8)
    Q = codes.size // C
    dyr, dxr, ci = Rows(R.quarter_bits(g.astype(np.int16) * 4), C, "tight"), Rows(R.quarter_bits(old.astype(np.int16) * 4), C, "tight"), G(Q * C, "u8", codes.reshape(-1))
    call(bwd, dyr.ptr(), dyr.ld, ci.ptr(), dxr.ptr(), dxr.ld, 1, B, H, W, C, sp())
    sync()
    gf, of = g.astype(np.float32), old.astype(np.float32)
    want = R.maxpool3s2_bwd_ref(gf, codes, of, 1, H, W) if kind == 3 else R.maxpool2_bwd_ref(gf, codes, of, 1)
    dxr.holds(want, "dx")


def test_cap_maxpool3s2():
    _cap_maxpool(3)


def test_cap_maxpool2():
    _cap_maxpool(2)


def test_cap_avgpool2():
    call, sp, _ = _abi()
    B, H, W, C = R.CAP["avgpool2_fwd"]
    q, xb = _cap_ints("avgpool2_fwd", (B, H, W, C), 9, 8)
    xr, yr = Rows(xb, C, "tight"), Rows(None, C, "tight", P=B * (H // 2) * (W // 2))
    call("avgpool2_fwd", xr.ptr(), xr.ld, yr.ptr(), yr.ld, B, H, W, C, sp())
    sync()
    q16 = q.astype(np.int16)
    yr.holds(R.quarter_bits(q16[:, 0::2, 0::2] + q16[:, 0::2, 1::2] + q16[:, 1::2, 0::2] + q16[:, 1::2, 1::2]), "y")     # sum / 4, a bf16 number
    del xr, yr
    B, H, W, C = R.CAP["avgpool2_bwd"]
    g, gb = _cap_ints("avgpool2_bwd", (B, H // 2, W // 2, C), 10, 8)
    old = R.small_int_draw((B, H, W, C), 11, 8)
    dyr, dxr = Rows(gb, C, "tight"), Rows(R.quarter_bits(old.astype(np.int16) * 4), C, "tight")
    call("avgpool2_bwd", dyr.ptr(), dyr.ld, dxr.ptr(), dxr.ld, 1, B, H, W, C, sp())
    sync()
    g4 = np.repeat(np.repeat(g.astype(np.int16), 2, axis=1), 2, axis=2)
    dxr.holds(R.quarter_bits(old.astype(np.int16) * 4 + g4), "dx")       # old + g / 4: at most 40 quarters, a bf16 number


# ---------------------------------------------------------------------------------------------------------------------------
def test_refusals():
    """Arguments an entry point rejects before any launch: an error code, and no buffer changes.  Every other argument of every call
    is valid, so nothing here could make a kernel act on a bad one."""
    _, sp, lib = _abi()
    B, H, W, C = 1, 4, 6, 8
    P = B * H * W
    bufs = {k: G(n, kind) for k, (n, kind) in dict(
        x=(P * C, "bf16"), y=(P * C, "bf16"), idx=(P * C, "u8"), cnt=(1, "i64"), stats=(8 * 2 * C, "i64"), stats2=(8 * 2 * C, "i64"),
        keep=(B * C, "f32"), img=(B * 3 * H * W, "f32"), rows=(P * 32, "bf16"), w=(C * 9, "f32"), slab=(C * 9, "f32")).items()}
    p = {k: b.ptr() for k, b in bufs.items()}
    st = sp()
    pool_f, pool_b = [p["x"], C, p["y"], C, p["idx"], B, H, W, C, st], [p["y"], C, p["idx"], p["x"], C, 0, B, H, W, C, st]
    good = {
        "ep24_maxpool3s2_fwd": pool_f, "ep24_maxpool2_fwd": pool_f, "ep24_maxpool3s2_bwd": pool_b, "ep24_maxpool2_bwd": pool_b,
        "ep24_avgpool2_fwd": [p["x"], C, p["y"], C, B, H, W, C, st],
        "ep24_avgpool2_bwd": [p["y"], C, p["x"], C, 0, B, H, W, C, st],
        "ep24_chanscale": [p["x"], C, p["keep"], B, H * W, C, st],
        "ep24_im2col_bf16": [p["img"], p["rows"], 32, B, 3, H, W, 3, 1, 1, st],
        "ep24_relu_fwd": [p["x"], C, P, C, st],
        "ep24_relu_bwd": [p["x"], C, p["y"], C, P, C, st],
        "ep24_colstats": [p["x"], C, p["stats"], C, P, C, st],
        "ep24_stats_gather": [p["stats"], C, p["stats2"], C, 8, st],
        "ep24_incr_i64": [p["cnt"], st],
        "ep24_dwconv_fwd_bf16": [p["x"], C, p["w"], p["y"], C, p["stats"], 8, B, H, W, C, 3, 1, st],
        "ep24_dwconv_dgrad_bf16": [p["y"], C, p["w"], p["x"], C, 0, B, H, W, C, 3, 1, st],
        "ep24_dwconv_wgrad_slab_bf16": [p["x"], C, p["y"], C, p["slab"], C * 9, B, H, W, C, 3, 1, st],
    }
    pool_f_bad = [("x", None), ("y", None), ("idx", None), ("C", 12), ("ld_x", 12), ("ld_y", 12)]
    pool_b_bad = [("dy", None), ("idx", None), ("dx", None), ("C", 12), ("ld_dy", 12), ("ld_dx", 12)]
    dw_bad = [("C", 12), ("C", 0), ("ksize", 5, E_UNSUPPORTED), ("stride", 3, E_UNSUPPORTED), ("B", 0), ("H", 0)]
    bad = {
        "ep24_maxpool3s2_fwd": pool_f_bad, "ep24_maxpool3s2_bwd": pool_b_bad,
        "ep24_maxpool2_fwd": pool_f_bad + [("H", 5), ("W", 5)], "ep24_maxpool2_bwd": pool_b_bad + [("H", 5), ("W", 5)],
        "ep24_avgpool2_fwd": [("x", None), ("y", None), ("C", 12), ("ld_x", 12), ("ld_y", 12), ("H", 5), ("W", 5)],
        "ep24_avgpool2_bwd": [("dy", None), ("dx", None), ("C", 12), ("ld_dy", 12), ("ld_dx", 12), ("H", 5), ("W", 5)],
        "ep24_chanscale": [("x", None), ("keep", None), ("C", 12), ("ld", 12), ("B", 0), ("HW", 0)],
        "ep24_im2col_bf16": [("images", None), ("rows", None), ("ld", 28), ("ld", 24), ("k", 9)],
        "ep24_relu_fwd": [("y", None), ("C", 12), ("ld", 12), ("M", 0)],
        "ep24_relu_bwd": [("dy", None), ("y", None), ("C", 12), ("ld_dy", 12), ("ld_y", 12), ("M", 0)],
        "ep24_colstats": [("x", None), ("stats", None), ("C", 12), ("C", 0), ("C", 2056), ("ld", 12), ("M", 0), ("ld_stats", 4)],
        "ep24_stats_gather": [("src", None), ("dst", None), ("C", 0), ("reps", 0), ("ld_src", 4)],
        "ep24_incr_i64": [("p", None)],
        "ep24_dwconv_fwd_bf16": [("x", None), ("w", None), ("z", None), ("ld_x", 12), ("ld_z", 12), ("stats_replicas", 0), ("x", p["x"] + 2)] + dw_bad,
        "ep24_dwconv_dgrad_bf16": [("dz", None), ("w", None), ("dx", None), ("ld_dz", 12), ("ld_dx", 12), ("dx", p["x"] + 2)] + dw_bad,
        "ep24_dwconv_wgrad_slab_bf16": [("x", None), ("dz", None), ("slab", None), ("ld_x", 12), ("ld_dz", 12), ("slab_floats", C * 9 - 1)] + dw_bad,
    }
    assert set(good) == set(bad) and len(good) == 16
    refused = 0
    for name, args in good.items():
        names = [a for _, a in lib.protos[name][1]]
        assert len(names) == len(args), name
        for case in bad[name]:
            key, val, code = case if len(case) == 3 else case + (E_ARG,)
            a = list(args)
            a[names.index(key)] = val
            assert lib.fn[name](*a) == code, (name, key, val)
            refused += 1
    assert refused == sum(len(v) for v in bad.values())
    sync()
    for k, b in bufs.items():
        b.check(np.full(b.n, b.sent, dtype=b.host.dtype), k)
