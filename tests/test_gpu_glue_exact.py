"""The glue kernels of csrc/elementwise.hip - SPP pools, nearest x2 upsample, rows_copy, head decode, bias column sums, the two stem
packers - against tests/glue_reference.py, through the C ABI.  tests/test_glue_reference.py shows without a GPU that the references
equal torch's max_pool2d / autograd / interpolate / unfold and that eleven mutants are rejected on these inputs.

Every buffer sits between two guards of 64 sentinel elements, whole buffers are compared - the pad columns of strided rows and every
buffer a call must not write included.  NaN equals NaN; every other pattern only itself.

Bit for bit: both forms of the SPP forward (values and the three code planes; ties, NaN, -inf, windows without a maximum), the SPP
backward on integer draws (both forms) and on normal draws in the gather form (its fp32 order is fixed: dy outer, dx inner, pools
13, 9, 5, then the old value), the upsample and rows_copy in both directions and both accumulate forms, columns 0 / 1 / 26.. and the
origin image of the decode, the decode's backward on dyadic draws, the column sums on integer draws (slab rows, the folded gradient and
the atomic form), both stem packers on random bit patterns.  Under a derived bound: the LDS form of the SPP backward on normal draws
(glue_reference.lds_bound: (terms - 1) 2^-24 sum|terms| + half a bf16 ulp, terms counted per element, at most 276 with the old value)
and the radii of the decode (no expf error figure is documented in the ROCm tree this was written against, so 2 ulp of the fp32
result against s * exp(t) in float64; the stride is a power of two, its product exact).

The sizes come from the constants of csrc/elementwise.hip:
  MAX_BLOCKS = 2048 workgroups of 256 lanes, one 8-channel item per lane: a grid-stride loop makes a second trip beyond 524 288 items -
      (2, 9, 8, 29136) for the SPP forward, (1, 18, 33, 7072) for the gather backward, (1, 3, 5, 279624) for the upsample and
      2049 x 2048 for rows_copy
  the 585-pixel LDS switch of ep24_spp_bwd (112 bytes of LDS per pixel, 64 KiB): 13 x 45 = 585 pixels (65 520 bytes) is the last
      map of the LDS form, 14 x 42 = 588 and 2 x 293 = 586 the first of the gather form
  32 pixels per stem_pack workgroup, at most 16 384 of them: 17 x 33 = 561 pixels leaves a partial workgroup, 725 x 725 = 525 625
      pixels makes a second trip (about a second on the host for its reference).  focus_pack's cap of 65 536 workgroups of 256
      pixels needs an 8192 x 8192 image and is left out.
  the column sum: one split per 4 rows, at most 64 (M = 255 is the last below the cap), 256 / ceil(N / 8) row lanes per split

Largest figures measured on an MI355X (the tests print them as GLUE-ERR before they assert):
  SPP backward, LDS form, normal draws, err / bound:  0.99998 at 13 x 45 and 20 x 20 (275 / 276 and 262 / 263 terms at most), 0.99996 at
      3 x 7; no element was further from the float64 sum than half a bf16 ulp of the result, so the additions' share of the bound
      went unused - the figure is a two-term sum that falls exactly between two bf16 numbers
  decode radii, ulp distance to float64:              0.776 (t = k / 1024, |t| <= 4, strides 8, 16, 32)
"""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import glue_reference as R  # noqa: E402
import update_reference as U  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
E_ARG = -1
S16 = U.SENT16


def _abi():
    from ep24._lib import call, lib, stream_ptr
    return call, stream_ptr, lib()


def G(n, kind, fill=None):
    return U.Guarded(n, kind, DEV, fill)


def sync():
    torch.cuda.synchronize()


def rows(P, ld, parts, pad=S16):
    """uint16 [P, ld] image: parts = [(column offset, uint16 [P, C] or flat)], everything else `pad`"""
    img = np.full((P, ld), pad, dtype=np.uint16)
    for off, a in parts:
        a = np.asarray(a, dtype=np.uint16).reshape(P, -1)
        img[:, off:off + a.shape[1]] = a
    return img


def b16(a, P):
    return R.b16(a).reshape(P, -1)


# ---------------------------------------------------------------------------------------------------------------------------
def _spp_fwd(shape, draw, layout):
    call, sp, _ = _abi()
    B, H, W, C = shape
    P = B * H * W
    x, vals, codes = R.spp_case(shape, draw)
    xb = b16(x, P)
    want_codes = codes.reshape(-1)
    outs = []
    for form in ("direct", "scratch"):
        idx = G(3 * P * C, "u8")
        scratch = G(9 * P * C, "u8") if form == "scratch" else None
        s_ptr = None if scratch is None else scratch.ptr()
        if layout == "cat":                                          # the engine's concatenation: x | y5 | y9 | y13, ld = 4 C
            ld = 4 * C
            cat = G(P * ld, "bf16", rows(P, ld, [(0, xb)]).reshape(-1))
            call("spp_fwd", cat.ptr(), ld, cat.ptr(C), cat.ptr(2 * C), cat.ptr(3 * C), ld, idx.ptr(), B, H, W, C, s_ptr, sp())
            sync()
            want = rows(P, ld, [(0, xb)] + [((p + 1) * C, b16(vals[p], P)) for p in range(3)])
            got = cat.check(want.reshape(-1), "x | y5 | y9 | y13 (%s)" % form)
        else:                                                        # separate buffers, 8 pad columns behind every row
            ld = C + 8
            xin = G(P * ld, "bf16", rows(P, ld, [(0, xb)]).reshape(-1))
            ys = [G(P * ld, "bf16") for _ in range(3)]
            call("spp_fwd", xin.ptr(), ld, ys[0].ptr(), ys[1].ptr(), ys[2].ptr(), ld, idx.ptr(), B, H, W, C, s_ptr, sp())
            sync()
            xin.check(rows(P, ld, [(0, xb)]).reshape(-1), "x (%s)" % form)
            got = np.concatenate([ys[p].check(rows(P, ld, [(0, b16(vals[p], P))]).reshape(-1), "y%d (%s)" % (5 + 4 * p, form)) for p in range(3)])
        got_idx = idx.check(want_codes, "winner codes (%s)" % form)
        if scratch is not None:
            scratch.check(scratch.read()[0], "scratch guards")
        outs.append((got.copy(), got_idx.copy()))
    assert U.same_bits(outs[0][0], outs[1][0]) and np.array_equal(outs[0][1], outs[1][1]), "the two forms differ"


@pytest.mark.parametrize("layout", ["cat", "pad"])
@pytest.mark.parametrize("draw", ["ties", "special"])
@pytest.mark.parametrize("shape", R.SPP_FWD_SHAPES, ids=str)
def test_spp_fwd_exact(shape, draw, layout):
    _spp_fwd(shape, draw, layout)


def test_spp_fwd_beyond_the_grid_cap():
    assert R.items(R.SPP_FWD_BIG) > R.MAX_ITEMS
    _spp_fwd(R.SPP_FWD_BIG, "special", "pad")


# ---------------------------------------------------------------------------------------------------------------------------
def _spp_bwd(shape, draw, accumulate, lds):
    """dy5 | dy9 | dy13 | 8 pad columns in one buffer (ld_dy = 3 C + 8), dx in the last C columns of a [P, 2 C] buffer (ld_dx = 2 C).
    With accumulate = 0 dx starts as the sentinel NaN: an old value that leaks into the result shows."""
    call, sp, _ = _abi()
    B, H, W, C = shape
    P = B * H * W
    assert (H * W * 112 <= 65536) == lds
    d5, d9, d13, codes, old = R.spp_bwd_case(shape, draw)
    ld_dy, ld_dx = 3 * C + 8, 2 * C
    dy_img = rows(P, ld_dy, [(0, b16(d5, P)), (C, b16(d9, P)), (2 * C, b16(d13, P))]).reshape(-1)
    dx_img = rows(P, ld_dx, [(C, b16(old, P))] if accumulate else []).reshape(-1)
    dy, dx, idx = G(P * ld_dy, "bf16", dy_img), G(P * ld_dx, "bf16", dx_img), G(3 * P * C, "u8", codes.reshape(-1))
    call("spp_bwd", dy.ptr(), dy.ptr(C), dy.ptr(2 * C), ld_dy, idx.ptr(), dx.ptr(C), ld_dx, accumulate, B, H, W, C, sp())
    sync()
    dy.check(dy_img, "dy")
    idx.check(codes.reshape(-1), "codes")
    got, _ = dx.read()
    got = got.reshape(P, ld_dx)
    tot, mag, cnt = R.spp_bwd_ref(d5, d9, d13, codes, old, accumulate)
    if draw == "integer":
        want = R.bf16_from_f64(tot)
    elif not lds:
        want = R.spp_bwd_ordered_ref(d5, d9, d13, codes, old, accumulate)
    else:
        g = U.from_bits32(U.bf16_widen(got[:, C:])).astype(np.float64).reshape(shape)
        assert int(cnt.max()) <= 276
        with np.errstate(all="ignore"):
            ratio = np.abs(g - tot) / R.lds_bound(mag, cnt, g)
            part = np.maximum(cnt - 1, 0) * 2.0 ** -24 * mag          # the bound's share for the additions
            used = np.where(part > 0, (np.abs(g - tot) - 0.5 * R.bf16_ulp(g)) / np.where(part > 0, part, 1.0), 0.0)
        ratio[~np.isfinite(g)] = np.inf
        print("GLUE-ERR spp_bwd lds %s accumulate %d: err / bound %.5f (beyond half an ulp: %.3f of the additions' share), most terms %d"
              % (shape, accumulate, float(ratio.max()), max(0.0, float(used.max())), int(cnt.max())))
        assert float(ratio.max()) <= 1.0, float(ratio.max())
        want = got[:, C:]
    dx.check(rows(P, ld_dx, [(0, dx_img.reshape(P, ld_dx)[:, :C]), (C, want)]).reshape(-1), "dx")


@pytest.mark.parametrize("accumulate", [0, 1])
@pytest.mark.parametrize("draw", ["integer", "general"])
@pytest.mark.parametrize("shape", R.SPP_BWD_LDS, ids=str)
def test_spp_bwd_lds_form(shape, draw, accumulate):
    _spp_bwd(shape, draw, accumulate, True)


@pytest.mark.parametrize("accumulate", [0, 1])
@pytest.mark.parametrize("draw", ["integer", "general"])
@pytest.mark.parametrize("shape", R.SPP_BWD_GATHER, ids=str)
def test_spp_bwd_gather_form(shape, draw, accumulate):
    _spp_bwd(shape, draw, accumulate, False)


def test_spp_bwd_gather_beyond_the_grid_cap():
    assert R.items(R.SPP_BWD_BIG) > R.MAX_ITEMS
    _spp_bwd(R.SPP_BWD_BIG, "integer", 1, False)


# ---------------------------------------------------------------------------------------------------------------------------
UP_ALL = R.UP_SHAPES + [R.UP_BIG]


@pytest.mark.parametrize("shape", UP_ALL, ids=str)
def test_upsample2_fwd_exact(shape):
    """A pure copy: random bf16 patterns.  x sits in the columns 8 .. 8 + C of [P, C + 16] rows, y in the last C columns of
    [4 P, 2 C] rows (a PAFPN join)."""
    call, sp, _ = _abi()
    B, H, W, C = shape
    P = B * H * W
    xb = R.bits16_draw(P * C, sum(shape)).reshape(P, C)
    ld_x, ld_y = C + 16, 2 * C
    x_img = rows(P, ld_x, [(8, xb)]).reshape(-1)
    x, y = G(P * ld_x, "bf16", x_img), G(4 * P * ld_y, "bf16")
    call("upsample2_fwd", x.ptr(8), ld_x, y.ptr(C), ld_y, B, H, W, C, sp())
    sync()
    want = R.upsample2_ref(xb.reshape(B, H, W, C))
    got = y.check(rows(4 * P, ld_y, [(C, want)]).reshape(-1), "y")
    assert np.array_equal(got.reshape(4 * P, ld_y)[:, C:], want.reshape(4 * P, C)), "a NaN payload or a zero's sign changed"
    x.check(x_img, "x")


def _upsample2_bwd(shape, draw, accumulate):
    call, sp, _ = _abi()
    B, H, W, C = shape
    P = B * H * W
    dyv, old = R.up_case(shape, draw)
    ld_dy, ld_dx = C + 8, 2 * C
    dy_img = rows(4 * P, ld_dy, [(0, b16(dyv, 4 * P))]).reshape(-1)
    dx_img = rows(P, ld_dx, [(C, b16(old, P))] if accumulate else []).reshape(-1)
    dy, dx = G(4 * P * ld_dy, "bf16", dy_img), G(P * ld_dx, "bf16", dx_img)
    call("upsample2_bwd", dy.ptr(), ld_dy, dx.ptr(C), ld_dx, accumulate, B, H, W, C, sp())
    sync()
    want = R.upsample2_bwd_ref(dyv, old, accumulate)
    dx.check(rows(P, ld_dx, [(0, dx_img.reshape(P, ld_dx)[:, :C]), (C, want)]).reshape(-1), "dx")
    dy.check(dy_img, "dy")


@pytest.mark.parametrize("accumulate", [0, 1])
@pytest.mark.parametrize("draw", ["integer", "general"])
@pytest.mark.parametrize("shape", R.UP_SHAPES, ids=str)
def test_upsample2_bwd_exact(shape, draw, accumulate):
    """dy fills the first C of C + 8 columns, dx the last C columns of [P, 2 C] rows; both draws bit for bit: the fp32 order is fixed"""
    _upsample2_bwd(shape, draw, accumulate)


def test_upsample2_bwd_beyond_the_grid_cap():
    assert R.items(R.UP_BIG) > R.MAX_ITEMS
    _upsample2_bwd(R.UP_BIG, "general", 1)


COPY_ALL = R.COPY_SHAPES + [R.COPY_BIG]


@pytest.mark.parametrize("mode", ["bits", "integer", "general"])
@pytest.mark.parametrize("M,C", COPY_ALL, ids=["%dx%d" % s for s in COPY_ALL])
def test_rows_copy_exact(M, C, mode):
    """bits: the plain copy of random patterns - NaN payloads, -0 and denormals arrive unchanged; integer / general: dst += src"""
    call, sp, _ = _abi()
    accumulate = int(mode != "bits")
    if mode == "bits":
        sb, ob = R.bits16_draw(M * C, M + C).reshape(M, C), np.full((M, C), S16, dtype=np.uint16)
    else:
        f = R.integer_draw if mode == "integer" else R.general_draw
        sb, ob = b16(f((M, C), M + C), M), b16(f((M, C), M + C + 1), M)
    ld_s, ld_d = C + 16, 2 * C
    s_img, d_img = rows(M, ld_s, [(8, sb)]).reshape(-1), rows(M, ld_d, [(C, ob)]).reshape(-1)
    src, dst = G(M * ld_s, "bf16", s_img), G(M * ld_d, "bf16", d_img)
    call("rows_copy", src.ptr(8), ld_s, dst.ptr(C), ld_d, accumulate, M, C, sp())
    sync()
    want = R.rows_copy_ref(sb, ob, accumulate)
    got = dst.check(rows(M, ld_d, [(C, want)]).reshape(-1), "dst")
    if mode == "bits":
        moved = got.reshape(M, ld_d)[:, C:]
        bad = np.flatnonzero((moved != sb).reshape(-1))
        assert bad.size == 0, "%d patterns changed on their way, first 0x%04X -> 0x%04X" % (bad.size, sb.reshape(-1)[bad[0]], moved.reshape(-1)[bad[0]])
    src.check(s_img, "src")


# ---------------------------------------------------------------------------------------------------------------------------
def ulp32_distance(got, want64):
    _, e = np.frexp(want64)
    return np.abs(got.astype(np.float64) - want64) / np.ldexp(1.0, e - 24)


@pytest.mark.parametrize("with_origin", [False, True], ids=["plain", "origin"])
@pytest.mark.parametrize("ncols", [27, 28, 40, 107])
@pytest.mark.parametrize("H,W", R.DECODE_MAPS)
def test_head_decode_fwd(H, W, ncols, with_origin):
    call, sp, _ = _abi()
    a0 = R.DECODE_A0
    raw = R.decode_fwd_case(H, W, ncols)
    B, A, _ = raw.shape
    worst = 0.0
    for s in R.DECODE_STRIDES:
        out = G(B * A * ncols, "f32", U.bits32(raw).reshape(-1))
        org = G(B * A * 26, "f32") if with_origin else None
        call("head_decode_fwd", out.ptr(), B, A, a0, H, W, s, ncols, None if org is None else org.ptr(), sp())
        sync()
        org0 = U.from_bits32(np.full(B * A * 26, U.SENT32, dtype=np.uint32)).reshape(B, A, 26)
        want, radii, worg = R.decode_fwd_ref(raw, a0, H, W, s, org0 if with_origin else None)
        got, _ = out.read()
        got = U.from_bits32(got).reshape(B, A, ncols)
        g = got[:, a0:a0 + H * W, 2:26]
        assert bool(np.all(np.isfinite(g)))
        d = float(ulp32_distance(g, radii).max())
        worst = max(worst, d)
        assert d <= 2.0, d
        want[:, a0:a0 + H * W, 2:26] = g                              # compared above; everything else bit for bit
        out.check(U.bits32(want).reshape(-1), "out, stride %g" % s)
        if with_origin:
            org.check(U.bits32(worg).reshape(-1), "origin, stride %g" % s)
    print("GLUE-ERR decode radii %dx%d ncols %d: %.3f ulp" % (H, W, ncols, worst))


@pytest.mark.parametrize("with_origin", [False, True], ids=["plain", "origin"])
@pytest.mark.parametrize("ncols", [28, 35, 40, 107])
@pytest.mark.parametrize("H,W", R.DECODE_MAPS)
def test_head_decode_bwd_exact(H, W, ncols, with_origin):
    call, sp, _ = _abi()
    a0 = R.DECODE_A0
    dout, outv, d_org = R.decode_bwd_case(H, W, ncols)
    B, A, _ = dout.shape
    C = ncols - 27
    ld_cls = (C + 7) & ~7
    cells = B * H * W
    for s in R.DECODE_STRIDES:
        do, ou, dg = G(dout.size, "f32", U.bits32(dout).reshape(-1)), G(outv.size, "f32", U.bits32(outv).reshape(-1)), G(d_org.size, "f32", U.bits32(d_org).reshape(-1))
        reg, cls = G(cells * 32, "bf16"), G(cells * ld_cls, "bf16")
        call("head_decode_bwd", do.ptr(), ou.ptr(), reg.ptr(), cls.ptr(), B, A, a0, H, W, s, ncols, dg.ptr() if with_origin else None, sp())
        sync()
        wr, wc = R.decode_bwd_ref(dout, outv, a0, H, W, s, d_org if with_origin else None)
        got_r = reg.check(wr.reshape(-1), "d_regobj, stride %g" % s)
        got_c = cls.check(wc.reshape(-1), "d_cls, stride %g" % s)
        assert not got_r.reshape(cells, 32)[:, 27:].any() and not got_c.reshape(cells, ld_cls)[:, C:].any(), "a pad column is not +0"
        do.check(U.bits32(dout).reshape(-1), "dout")
        ou.check(U.bits32(outv).reshape(-1), "out")
        dg.check(U.bits32(d_org).reshape(-1), "d_origin")


# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("wide", [False, True], ids=["padded", "wide"])
@pytest.mark.parametrize("N", R.COLSUM_N)
def test_colsum_exact(N, wide):
    """Integer draw: every partial and every total is an fp32 number.  The slab holds two rows more than the splits: they, and the
    guards, stay untouched.  The fold goes into a gradient that is not zero."""
    call, sp, lib = _abi()
    ld = (N + 7) // 8 * 8 + (16 if wide else 0)
    g8 = R.colsum_draw(ld)
    g_img = R.int_bits(g8).reshape(-1)
    g = G(g_img.size, "bf16", g_img)
    grad0 = np.random.default_rng(N).integers(-100, 101, N).astype(np.float64)
    for M in R.COLSUM_M:
        splits = lib.fn["ep24_colsum_splits"](M)
        assert splits == R.colsum_splits_ref(M)
        slab = G((splits + 2) * N, "f32")
        call("colsum_slab", g.ptr(), ld, slab.ptr(), M, N, sp())
        sync()
        want = np.full((splits + 2, N), U.SENT32, dtype=np.uint32)
        want[:splits] = U.bits32(R.colsum_slab_ref(g8, M, N, splits)).reshape(splits, N)
        slab.check(want.reshape(-1), "slab M %d" % M)
        total = R.colsum_ref(g8, M, N)
        grad = G(N, "f32", U.bits32(grad0))
        desc = torch.tensor([0, N, splits, 0], dtype=torch.int64, device=DEV)
        call("wgrad_reduce", desc.data_ptr(), 1, N, grad.ptr(), slab.ptr(), sp())
        sync()
        grad.check(U.bits32(grad0 + total), "folded gradient M %d" % M)
        db = G(N, "f32", U.bits32(grad0))
        call("colsum", g.ptr(), ld, db.ptr(), M, N, sp())
        sync()
        db.check(U.bits32(grad0 + total), "atomic column sum M %d" % M)
    g.check(g_img, "g")


# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,H,W", R.STEM_IMAGES)
def test_focus_pack_exact(B, H, W):
    call, sp, _ = _abi()
    bits = R.image_bits(B, H, W, 11)
    img, out = G(bits.size, "f32", bits.reshape(-1)), G(B * (H // 2) * (W // 2) * 16, "bf16")
    call("focus_pack", img.ptr(), out.ptr(), B, H, W, sp())
    sync()
    out.check(R.focus_ref(bits).reshape(-1), "focus map")
    img.check(bits.reshape(-1), "images")


STEM_ALL = [(s, ld) for s in R.STEM_IMAGES for ld in R.STEM_LD] + [(R.STEM_BIG, 112)]


@pytest.mark.parametrize("image,ld", STEM_ALL, ids=["%dx%dx%d-ld%d" % (s + (ld,)) for s, ld in STEM_ALL])
def test_stem_pack_exact(image, ld):
    call, sp, _ = _abi()
    B, H, W = image
    bits = R.image_bits(B, H, W, 12)
    P = B * (H // 2) * (W // 2)
    img, out = G(bits.size, "f32", bits.reshape(-1)), G(P * ld, "bf16")
    call("stem_pack", img.ptr(), out.ptr(), ld, B, H, W, sp())
    sync()
    out.check(R.stem_rows_ref(bits, ld).reshape(-1), "stem rows")
    img.check(bits.reshape(-1), "images")


# ---------------------------------------------------------------------------------------------------------------------------
def test_refusals():
    """Arguments an entry point rejects before any launch: EP24_E_ARG, and no buffer changes.  Every other argument of every call is
    valid, so nothing here could make a kernel act on a bad one."""
    _, sp, lib = _abi()
    B, H, W, C = 1, 4, 6, 8
    P = B * H * W
    bufs = {k: G(n, kind) for k, (n, kind) in dict(
        x=(P * C, "bf16"), y5=(P * C, "bf16"), y9=(P * C, "bf16"), y13=(P * C, "bf16"), idx=(3 * P * C, "u8"), scratch=(9 * P * C, "u8"),
        up=(4 * P * C, "bf16"), img=(B * 3 * H * W, "f32"), f16=(6 * 16, "bf16"), stem=(6 * 112, "bf16"),
        out=(2 * 30 * 40, "f32"), dout=(2 * 30 * 40, "f32"), org=(2 * 30 * 26, "f32"), reg=(2 * 16 * 32, "bf16"), cls=(2 * 16 * 16, "bf16"),
        g=(8 * 32, "bf16"), slab=(2 * 27, "f32"), db=(27, "f32")).items()}
    p = {k: b.ptr() for k, b in bufs.items()}
    st = sp()
    good = {
        "ep24_spp_fwd": [p["x"], C, p["y5"], p["y9"], p["y13"], C, p["idx"], B, H, W, C, p["scratch"], st],
        "ep24_spp_bwd": [p["y5"], p["y9"], p["y13"], C, p["idx"], p["x"], C, 0, B, H, W, C, st],
        "ep24_upsample2_fwd": [p["x"], C, p["up"], C, B, H, W, C, st],
        "ep24_upsample2_bwd": [p["up"], C, p["x"], C, 0, B, H, W, C, st],
        "ep24_rows_copy": [p["x"], C, p["y5"], C, 0, P, C, st],
        "ep24_stem_pack": [p["img"], p["stem"], 112, B, H, W, st],
        "ep24_focus_pack": [p["img"], p["f16"], B, H, W, st],
        "ep24_head_decode_fwd": [p["out"], 2, 30, 5, 4, 4, 8.0, 40, p["org"], st],
        "ep24_head_decode_bwd": [p["dout"], p["out"], p["reg"], p["cls"], 2, 30, 5, 4, 4, 8.0, 40, p["org"], st],
        "ep24_colsum_slab": [p["g"], 32, p["slab"], 8, 27, st],
        "ep24_colsum": [p["g"], 32, p["db"], 8, 27, st],
    }
    bad = {
        "ep24_spp_fwd": [("C", 12), ("ld_x", 12), ("ld_y", 12), ("x", None), ("y5", None), ("y9", None), ("y13", None), ("idx", None),
                         ("scratch", p["scratch"] + 4), ("scratch", p["scratch"] + 2)],
        "ep24_spp_bwd": [("C", 12), ("ld_dy", 12), ("ld_dx", 12), ("dy5", None), ("dy9", None), ("dy13", None), ("idx", None), ("dx", None),
                         ("idx", p["idx"] + 4), ("idx", p["idx"] + 1)],
        "ep24_upsample2_fwd": [("C", 12), ("ld_x", 12), ("ld_y", 12), ("x", None), ("y", None)],
        "ep24_upsample2_bwd": [("C", 12), ("ld_dy", 12), ("ld_dx", 12), ("dy", None), ("dx", None)],
        "ep24_rows_copy": [("C", 12), ("ld_src", 12), ("ld_dst", 12), ("src", None), ("dst", None)],
        "ep24_stem_pack": [("H", 5), ("W", 5), ("images", None), ("rows", None), ("ld", 104), ("ld", 116), ("B", 0), ("images", p["img"] + 4)],
        "ep24_focus_pack": [("H", 5), ("W", 5), ("images", None), ("f16", None), ("B", 0), ("images", p["img"] + 4)],
        "ep24_head_decode_fwd": [("out", None), ("a0", 15), ("a0", -1), ("A", 20), ("ncols", 26)],
        "ep24_head_decode_bwd": [("dout", None), ("out", None), ("d_regobj", None), ("d_cls", None), ("a0", 15), ("a0", -1), ("A", 20), ("ncols", 27)],
        "ep24_colsum_slab": [("g", None), ("slab", None), ("N", 2049), ("N", 0), ("M", 0), ("ld", 24), ("ld", 36)],
        "ep24_colsum": [("g", None), ("db", None), ("N", 0)],
    }
    refused = 0
    for name, args in good.items():
        names = [a for _, a in lib.protos[name][1]]
        assert len(names) == len(args), name
        for key, val in bad[name]:
            a = list(args)
            a[names.index(key)] = val
            assert lib.fn[name](*a) == E_ARG, (name, key, val)
            refused += 1
    assert refused == sum(len(v) for v in bad.values()) == 72
    sync()
    for k, b in bufs.items():
        b.check(np.full(b.n, b.sent, dtype=b.host.dtype), k)
