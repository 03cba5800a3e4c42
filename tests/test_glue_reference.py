"""tests/glue_reference.py against torch on the CPU, the conditions on its draws, and its mutants: every wrong variant listed in MUTANTS
is told from the true reference by at least one input that tests/test_gpu_glue_exact.py feeds to the kernels.  No GPU."""
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import glue_reference as R  # noqa: E402
import update_reference as U  # noqa: E402

ALL_SPP = R.SPP_FWD_SHAPES + [s for s in R.SPP_BWD_LDS + R.SPP_BWD_GATHER if s not in R.SPP_FWD_SHAPES]


def nchw(a):
    return torch.from_numpy(np.ascontiguousarray(np.moveaxis(a, -1, 1)))


def nhwc(t):
    return np.ascontiguousarray(np.moveaxis(t.detach().numpy(), 1, -1))


def winner_position(codes_p):
    """flat y * W + x of every output's winner"""
    B, H, W, C = codes_p.shape
    dy, dx = R.decode_codes(codes_p)
    y, x = np.arange(H)[None, :, None, None], np.arange(W)[None, None, :, None]
    return (y + dy) * W + (x + dx)


# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("draw", ["ties", "special"])
@pytest.mark.parametrize("shape", ALL_SPP, ids=str)
def test_spp_ref_is_max_pool2d(shape, draw):
    x, vals, codes = R.spp_case(shape, draw)
    some = False
    for p, k in enumerate((5, 9, 13)):
        v, i = F.max_pool2d(nchw(x), k, 1, k // 2, return_indices=True)
        U.assert_same(U.bits32(vals[p]), U.bits32(nhwc(v)), "values of window %d" % k)
        has_max = ~(vals[p] == R.NEG)                               # NaN counts: it is a winner torch reports too
        assert np.array_equal(winner_position(codes[p])[has_max], nhwc(i)[has_max]), k
        assert bool(np.all(codes[p][~has_max] == R.CENTRE))
        some |= bool((~has_max).any())
    if draw == "special":
        assert some and np.isnan(vals).any(), "the special draw must hold a window without a maximum and a NaN"
        assert bool(np.all(vals[2][0, shape[1] // 2, shape[2] // 2, [0, -1]] == R.NEG)), "the 13-window that is entirely -inf"


@pytest.mark.parametrize("draw", ["ties", "special"])
@pytest.mark.parametrize("shape", ALL_SPP, ids=str)
def test_spp_direct_is_separable(shape, draw):
    x, vals, codes = R.spp_case(shape, draw)
    v2, c2 = R.spp_ref_separable(x)
    U.assert_same(U.bits32(vals), U.bits32(v2), "values")
    assert np.array_equal(codes, c2)


@pytest.mark.parametrize("shape", [R.SPP_FWD_BIG, R.SPP_BWD_BIG], ids=str)
def test_spp_separable_on_the_grid_stride_shapes(shape):
    """Channels are independent: the separable reference of the whole map equals the direct one on its first and last 16 channels."""
    assert R.items(shape) > R.MAX_ITEMS and R.items(shape) < R.MAX_ITEMS * 1.01
    x, vals, codes = R.spp_case(shape, "special")
    for sl in (slice(0, 16), slice(-16, None)):
        v, c = R.spp_ref(x[..., sl])
        U.assert_same(U.bits32(vals[..., sl]), U.bits32(v), "values")
        assert np.array_equal(codes[..., sl], c)


def test_ties_condition():
    """At least half of all 13-windows of the ties draw hold their maximum more than once (a condition on the inputs: without ties
    the first-maximum rule is not tested)."""
    for shape in ALL_SPP:
        if shape[1] * shape[2] == 1:
            continue
        x, vals, _ = R.spp_case(shape, "ties")
        xp = np.pad(x, ((0, 0), (6, 6), (6, 6), (0, 0)), constant_values=R.NEG)
        B, H, W, C = shape
        count = sum((xp[:, 6 + dy:6 + dy + H, 6 + dx:6 + dx + W] == vals[2]) for dy in range(-6, 7) for dx in range(-6, 7))
        assert float((count > 1).mean()) >= 0.5, (shape, float((count > 1).mean()))


def test_spp_bwd_ref_is_autograd():
    """No ties (a permutation, float64): the gradient of sum(pool_k * g_k); ties: the scatter through torch's indices."""
    for shape in [(2, 3, 7, 8), (1, 13, 12, 8), (2, 20, 20, 8)]:
        B, H, W, C = shape
        rng = np.random.default_rng(sum(shape))
        x = rng.permutation(B * H * W * C).reshape(shape).astype(np.float32)
        gs = [R.integer_draw(shape, 60 + i) for i in range(3)]
        xt = nchw(x).double().requires_grad_(True)
        sum((F.max_pool2d(xt, k, 1, k // 2) * nchw(g).double()).sum() for k, g in zip((5, 9, 13), gs)).backward()
        _, codes = R.spp_ref(x)
        tot, mag, cnt = R.spp_bwd_ref(*gs, codes, None, 0)
        assert np.array_equal(tot, nhwc(xt.grad)), shape
        assert int(cnt.sum()) == 3 * x.size and float(mag.sum()) == sum(float(np.abs(g).sum()) for g in gs)
        # ties
        x = R.ties_draw(shape, 5)
        _, codes = R.spp_ref(x)
        old = R.integer_draw(shape, 70)
        want = old.astype(np.float64).copy()
        for k, g in zip((5, 9, 13), gs):
            _, i = F.max_pool2d(nchw(x), k, 1, k // 2, return_indices=True)
            b, y, xx, c = np.meshgrid(*[np.arange(n) for n in shape], indexing="ij")
            pos = nhwc(i)
            np.add.at(want, (b, pos // W, pos % W, c), g.astype(np.float64))
        assert np.array_equal(R.spp_bwd_ref(*gs, codes, old, 1)[0], want), shape
        # on integers the ordered fp32 form is the exact one
        assert np.array_equal(R.spp_bwd_ordered_ref(*gs, codes, old, 1), R.bf16_from_f64(want))


def test_bf16_from_f64_rounds_once():
    b = U.random_bits(4096, 3)
    b = b[(((b >> 23) & 0xFF) > 40) & (((b >> 23) & 0xFF) < 215)]
    assert np.array_equal(R.bf16_from_f64(U.from_bits32(b).astype(np.float64)), U.bf16_rne(b))
    # a value that rounding to float32 first would carry to the wrong side of a bf16 tie
    x = np.array([1.0 + 2.0 ** -8 + 2.0 ** -40, 1.0 + 2.0 ** -8 - 2.0 ** -40, -0.0, 0.0, 257.0, 258.0, 259.0])
    assert list(R.bf16_from_f64(x)) == [0x3F81, 0x3F80, 0x8000, 0x0000, 0x4380, 0x4381, 0x4382]
    t = torch.from_numpy(U.from_bits32(b).copy()).to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16)
    assert np.array_equal(U.bf16_rne(b), t)


@pytest.mark.parametrize("shape", R.UP_SHAPES, ids=str)
def test_upsample_refs_are_interpolate(shape):
    x = R.general_draw(shape, 1)
    xt = nchw(x).double().requires_grad_(True)
    y = F.interpolate(xt, scale_factor=2, mode="nearest")
    assert np.array_equal(R.upsample2_ref(x), nhwc(y).astype(np.float32))
    dy, old = R.up_case(shape, "integer")
    (y * nchw(dy).double()).sum().backward()
    for acc in (0, 1):
        want = nhwc(xt.grad) + (old if acc else 0.0)
        assert np.array_equal(R.upsample2_bwd_ref(dy, old, acc), R.bf16_from_f64(want))
    # the general draw: the fp32 sum of four bf16 numbers and an old value stays within the summation bound of the float64 one
    dy, old = R.up_case(shape, "general")
    got = U.from_bits32(U.bf16_widen(R.upsample2_bwd_ref(dy, old, 1))).astype(np.float64).reshape(shape)
    B, H, W, C = shape
    blk = dy.astype(np.float64).reshape(B, H, 2, W, 2, C)
    tot, mag = blk.sum((2, 4)) + old, np.abs(blk).sum((2, 4)) + np.abs(old)
    assert bool(np.all(np.abs(got - tot) <= 4 * 2.0 ** -24 * mag + 0.5 * R.bf16_ulp(got)))


def test_rows_copy_ref():
    b = R.bits16_draw(4096, 2)
    assert np.array_equal(R.rows_copy_ref(b, None, 0), b)
    s, o = R.general_draw((64, 16), 3), R.general_draw((64, 16), 4)
    want = (torch.from_numpy(s) + torch.from_numpy(o)).to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16)
    assert np.array_equal(R.rows_copy_ref(R.b16(s).reshape(64, 16), R.b16(o).reshape(64, 16), 1), want)


@pytest.mark.parametrize("B,H,W", R.STEM_IMAGES + [(1, 4, 6)])
def test_stem_refs_are_focus_and_unfold(B, H, W):
    bits = R.image_bits(B, H, W, 9)
    keep = ~U.is_nan32(bits)                                       # torch.equal has no NaN for NaN
    img = torch.from_numpy(U.from_bits32(np.where(keep, bits, 0)).reshape(B, 3, H, W).copy())
    bits = np.where(keep, bits, 0).astype(np.uint32)
    tl, tr, bl, br = img[..., ::2, ::2], img[..., ::2, 1::2], img[..., 1::2, ::2], img[..., 1::2, 1::2]
    foc = torch.cat((tl, bl, tr, br), dim=1)                         # Focus.forward
    f = R.focus_ref(bits)
    want = foc.to(torch.bfloat16).permute(0, 2, 3, 1).contiguous().view(torch.int16).numpy().view(np.uint16)
    assert np.array_equal(f[..., :12], want) and not f[..., 12:].any()
    finite = torch.nan_to_num(foc.to(torch.bfloat16).float(), posinf=3e38, neginf=-3e38)     # unfold multiplies nothing, but keep it finite
    cols = F.unfold(finite, 3, padding=1).reshape(B, 12, 9, -1).permute(0, 3, 2, 1).reshape(-1, 108)
    for ld in R.STEM_LD:
        rows = R.stem_rows_ref(bits, ld)
        assert rows.shape == (B * (H // 2) * (W // 2), ld) and not rows[:, 108:].any()
        got = torch.from_numpy(U.from_bits32(U.bf16_widen(rows[:, :108])).reshape(-1, 108).copy())
        assert torch.equal(torch.nan_to_num(got, posinf=3e38, neginf=-3e38), cols)


def test_decode_refs_are_the_head():
    for (H, W) in R.DECODE_MAPS:
        for s in R.DECODE_STRIDES:
            raw = R.decode_fwd_case(H, W, 40)
            a0 = R.DECODE_A0
            org0 = np.full((2, raw.shape[1], 26), 7.0, dtype=np.float32)
            out, radii, org = R.decode_fwd_ref(raw, a0, H, W, s, org0)
            lvl = torch.from_numpy(raw[:, a0:a0 + H * W].copy()).double().requires_grad_(True)
            yv, xv = torch.meshgrid([torch.arange(H), torch.arange(W)], indexing="ij")
            grid = torch.stack((xv, yv), 2).view(1, -1, 2)
            dec = torch.cat([(lvl[..., :2] + grid) * s, torch.exp(lvl[..., 2:26]) * s, lvl[..., 26:]], -1)
            assert np.array_equal(out[:, a0:a0 + H * W, :2].astype(np.float64), dec[..., :2].detach().numpy())      # exact in fp32
            assert np.allclose(radii, dec[..., 2:26].detach().numpy(), rtol=1e-15)
            keep = np.ones(raw.shape, dtype=bool)
            keep[:, a0:a0 + H * W, :26] = False
            assert np.array_equal(U.bits32(out).reshape(raw.shape)[keep], U.bits32(raw).reshape(raw.shape)[keep])
            assert np.array_equal(org[:, a0:a0 + H * W], raw[:, a0:a0 + H * W, :26]) and bool(np.all(org[:, :a0] == 7.0)) and bool(np.all(org[:, a0 + H * W:] == 7.0))
            # backward: autograd through the decode, the L1 branch's gradient added to the raw regression outputs
            dout, _, d_org = R.decode_bwd_case(H, W, 40)
            (dec * torch.from_numpy(dout[:, a0:a0 + H * W]).double()).sum().backward()
            outd = dout.copy()
            outd[:, a0:a0 + H * W, 2:26] = dec[..., 2:26].detach().numpy().astype(np.float32)
            reg, cls = R.decode_bwd_ref(dout, outd, a0, H, W, s, None)
            g = lvl.grad.numpy()
            got = U.from_bits32(U.bf16_widen(reg)).reshape(2, H * W, 32).astype(np.float64)
            assert bool(np.all(np.abs(got[..., :27] - g[..., :27]) <= 2.0 ** -8 * np.abs(g[..., :27]) + 1e-30)) and not got[..., 27:].any()
            assert np.array_equal(U.from_bits32(U.bf16_widen(cls)).reshape(2, H * W, 16)[..., :13], dout[:, a0:a0 + H * W, 27:]) and not cls.reshape(2, H * W, 16)[..., 13:].any()
            reg2, _ = R.decode_bwd_ref(dout, outd, a0, H, W, s, d_org)
            got2 = U.from_bits32(U.bf16_widen(reg2)).reshape(2, H * W, 32).astype(np.float64)
            g2 = g[..., :26] + d_org[:, a0:a0 + H * W]
            assert bool(np.all(np.abs(got2[..., :26] - g2) <= 2.0 ** -8 * np.abs(g2) + 1e-30))


def test_decode_bwd_draw_is_exact_in_fp32():
    """dout * out + d_origin of the dyadic draw is an fp32 number, so a fused and a separate multiply-add give the same bits."""
    dout, out, d_org = R.decode_bwd_case(3, 5, 107)
    exact = dout.astype(np.float64)[..., :26] * out.astype(np.float64)[..., :26] + d_org
    assert U.exact32(exact) and U.exact32(dout.astype(np.float64)[..., :2] * 32.0 + d_org[..., :2])
    m, _ = np.frexp(dout.astype(np.float64))
    assert bool(np.all(m * 16 == np.rint(m * 16)))


@pytest.mark.parametrize("N", R.COLSUM_N)
def test_colsum_slab_ref_counts_every_row_once(N):
    ld = (N + 7) // 8 * 8
    g = R.colsum_draw(ld)
    chunks = (N + 7) // 8
    rpp = 256 // chunks
    for M in R.COLSUM_M:
        splits = R.colsum_splits_ref(M)
        owner, _ = R.colsum_owner(M, N, splits)
        seen = np.zeros(M, dtype=np.int64)
        for b in range(splits):                                    # the layout as stated: rows b rpp + r + k splits rpp
            for r in range(rpp):
                rows = np.arange(b * rpp + r, M, splits * rpp)
                seen[rows] += 1
                assert bool(np.all(owner[rows] == b))
        assert bool(np.all(seen == 1)), (M, N)
        slab = R.colsum_slab_ref(g, M, N, splits)
        assert slab.shape == (splits, N) and np.array_equal(slab.sum(0), R.colsum_ref(g, M, N))
        assert np.array_equal(R.colsum_ref(g, M, N), g[:M, :N].astype(np.int64).sum(0).astype(np.float64))
        assert U.exact32(slab) and float(np.abs(slab).max()) < 2 ** 24
    assert [R.colsum_splits_ref(M) for M in (1, 4, 5, 255, 256, 257, 40000)] == [1, 1, 2, 64, 64, 64, 64]


# ---------------------------------------------------------------------------------------------------------------------------
# the mutants: each returns True if some input of the GPU test tells it from the true reference
def _spp_fwd_mutant(**kw):
    hit = []
    for shape in R.SPP_FWD_SHAPES:
        for draw in ("ties", "special"):
            x, vals, codes = R.spp_case(shape, draw)
            v, c = R.spp_ref(x, **kw)
            hit.append((shape, draw, not (U.same_bits(U.bits32(v), U.bits32(vals)) and np.array_equal(c, codes))))
    return hit


def _m_last_tie():
    return _spp_fwd_mutant(tie="last")


def _m_radius():
    return _spp_fwd_mutant(radii=(2, 6, 6))


def _m_cross():
    return _spp_fwd_mutant(cross=True)


def _m_swap():
    return _spp_fwd_mutant(swap=True)


def _bwd_mutants(kind):
    """kind 'drop': accumulate ignores old; 'round': the sum is rounded to bf16 before old is added"""
    hit = []
    for shape in R.SPP_BWD_LDS + R.SPP_BWD_GATHER:
        for draw in ("integer", "general"):
            a = R.spp_bwd_case(shape, draw)
            if draw == "general" and shape in R.SPP_BWD_LDS:        # compared under lds_bound
                tot, mag, cnt = R.spp_bwd_ref(*a, 1)
                mt, _, _ = R.spp_bwd_ref(*a, 0) if kind == "drop" else R.spp_bwd_ref(*a, 1, round_first=True)
                got = U.from_bits32(U.bf16_widen(R.bf16_from_f64(mt))).astype(np.float64).reshape(shape)
                hit.append((shape, draw, bool(np.any(np.abs(got - tot) > R.lds_bound(mag, cnt, got)))))
            elif draw == "general":
                want = R.spp_bwd_ordered_ref(*a, 1)
                got = R.spp_bwd_ordered_ref(*a, 0) if kind == "drop" else R.spp_bwd_ordered_ref(*a, 1, round_first=True)
                hit.append((shape, draw, not np.array_equal(got, want)))
            else:
                want = R.bf16_from_f64(R.spp_bwd_ref(*a, 1)[0])
                mt = R.spp_bwd_ref(*a, 0)[0] if kind == "drop" else R.spp_bwd_ref(*a, 1, round_first=True)[0]
                hit.append((shape, draw, not np.array_equal(R.bf16_from_f64(mt), want)))
    for shape in R.UP_SHAPES:
        for draw in ("integer", "general"):
            dy, old = R.up_case(shape, draw)
            got = R.upsample2_bwd_ref(dy, old, 0) if kind == "drop" else R.upsample2_bwd_ref(dy, old, 1, round_first=True)
            hit.append((("up",) + shape, draw, not np.array_equal(got, R.upsample2_bwd_ref(dy, old, 1))))
    return hit


def _m_drop_old():
    hit = _bwd_mutants("drop")
    for M, C in R.COPY_SHAPES:
        s, o = R.b16(R.integer_draw((M, C), 1)), R.b16(R.integer_draw((M, C), 2))
        hit.append((("copy", M, C), "integer", not np.array_equal(R.rows_copy_ref(s, o, 0), R.rows_copy_ref(s, o, 1))))
    return hit


def _m_round_first():
    return _bwd_mutants("round")


def _m_parity():
    hit = []
    for shape in R.UP_SHAPES:
        x = R.general_draw(shape, 1)
        hit.append((shape, "forward", not np.array_equal(R.upsample2_ref(x, transposed=True), R.upsample2_ref(x))))
        dy, old = R.up_case(shape, "general")
        hit.append((shape, "backward", not np.array_equal(R.upsample2_bwd_ref(dy, old, 1, order="col"), R.upsample2_bwd_ref(dy, old, 1))))
    return hit


def _m_decode_x():
    hit = []
    for (H, W) in R.DECODE_MAPS:
        raw = R.decode_fwd_case(H, W, 27)
        hit.append(((H, W), "raw", not np.array_equal(R.decode_fwd_ref(raw, R.DECODE_A0, H, W, 8.0, x_mod=H)[0], R.decode_fwd_ref(raw, R.DECODE_A0, H, W, 8.0)[0])))
    return hit


def _m_class_pad():
    hit = []
    for ncols in (28, 35, 40, 107):
        dout, out, _ = R.decode_bwd_case(3, 5, ncols)
        hit.append((ncols, "dyadic", not np.array_equal(R.decode_bwd_ref(dout, out, R.DECODE_A0, 3, 5, 8.0, zero_pad=False, pad_fill=U.SENT16)[1],
                                                         R.decode_bwd_ref(dout, out, R.DECODE_A0, 3, 5, 8.0)[1])))
    return hit


def _m_colsum():
    hit = []
    for N in (1, 27, 256):
        g = R.colsum_draw((N + 7) // 8 * 8)
        for M in R.COLSUM_M:
            sp = R.colsum_splits_ref(M)
            hit.append(((M, N), "integer", not np.array_equal(R.colsum_slab_ref(g, M, N, sp, drop_last_group=True), R.colsum_slab_ref(g, M, N, sp))))
    return hit


def _m_tap_order():
    return [((B, H, W), "bits", not np.array_equal(R.stem_rows_ref(R.image_bits(B, H, W, 9), 112, dx_major=True), R.stem_rows_ref(R.image_bits(B, H, W, 9), 112)))
            for B, H, W in R.STEM_IMAGES]


MUTANTS = {
    "the last maximum wins a tie": _m_last_tie,
    "radius 6 where 4 is meant": _m_radius,
    "a window runs across the image boundary": _m_cross,
    "the winner code has dy and dx swapped": _m_swap,
    "accumulate drops the old value": _m_drop_old,
    "accumulate rounds to bf16 before it adds": _m_round_first,
    "the upsample swaps the row and column parity": _m_parity,
    "the decode uses hw % H for x": _m_decode_x,
    "the class pad is not zeroed": _m_class_pad,
    "the column sum drops the last partial row group": _m_colsum,
    "the stem tap order is dx-major": _m_tap_order,
}


@pytest.mark.parametrize("name", list(MUTANTS))
def test_mutant_is_rejected(name):
    hit = MUTANTS[name]()
    assert any(h for _, _, h in hit), (name, hit)
    if name in ("the upsample swaps the row and column parity", "the decode uses hw % H for x", "the stem tap order is dx-major"):
        # a square map cannot tell rows from columns: a non-square input must be among those that do
        hw = lambda k: k[-2:] if len(k) == 2 else k[1:3]
        assert any(h for k, _, h in hit if hw(k)[0] != hw(k)[1]), hit
    if name == "a window runs across the image boundary":
        assert not any(h for k, _, h in hit if k[0] == 1) and any(h for k, _, h in hit if k[0] > 1)


def test_every_family_has_a_non_square_case():
    for fam in (R.SPP_FWD_SHAPES, R.SPP_BWD_LDS, R.SPP_BWD_GATHER, R.UP_SHAPES):
        assert any(h != w for _, h, w, _ in fam)
    assert any(h != w for h, w in R.DECODE_MAPS) and any(h != w for _, h, w in R.STEM_IMAGES)
    assert R.items(R.UP_BIG) > R.MAX_ITEMS and R.COPY_BIG[0] * (R.COPY_BIG[1] // 8) > R.MAX_ITEMS
    B, H, W = R.STEM_BIG
    assert B * (H // 2) * (W // 2) > 16384 * 32
    assert 13 * 45 * 112 <= 65536 < 14 * 42 * 112 and 2 * 293 * 112 > 65536 and 20 * 20 * 112 <= 65536 < 25 * 25 * 112
