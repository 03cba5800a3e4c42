"""tests/backbone_reference.py against torch on the CPU, the conditions on its draws and shapes, and its mutants: every wrong variant
listed in MUTANTS is told from the true reference by at least one input that tests/test_gpu_backbone_exact.py feeds to the kernels.
No GPU."""
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import backbone_reference as R  # noqa: E402
import update_reference as U  # noqa: E402

POOLS = [(3, s) for s in R.POOL3_SHAPES] + [(2, s) for s in R.POOL2_SHAPES]
POOL_IDS = ["k%d-%s" % (k, "x".join(map(str, s))) for k, s in POOLS]


def nchw(a):
    return torch.from_numpy(np.ascontiguousarray(np.moveaxis(a, -1, 1)))


def nhwc(t):
    return np.ascontiguousarray(np.moveaxis(t.detach().numpy(), 1, -1))


def torch_pool(kind, t):
    return F.max_pool2d(t, 3, 2, 1, return_indices=True) if kind == 3 else F.max_pool2d(t, 2, 2, return_indices=True)


def winner_position(kind, codes, W):
    """flat y * W + x of every output's winner"""
    B, OH, OW, C = codes.shape
    c = codes.astype(np.int64)
    oy, ox = np.arange(OH)[None, :, None, None], np.arange(OW)[None, None, :, None]
    if kind == 3:
        return (2 * oy - 1 + c // 3) * W + (2 * ox - 1 + c % 3)
    return (2 * oy + c // 2) * W + (2 * ox + c % 2)


def same16(a, b):
    return U.same_bits(np.asarray(a, dtype=np.uint16).reshape(-1), np.asarray(b, dtype=np.uint16).reshape(-1))


# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("draw", list(R.POOL_DRAWS))
@pytest.mark.parametrize("kind,shape", POOLS, ids=POOL_IDS)
def test_max_pool_refs_are_max_pool2d(kind, shape, draw):
    x, vals, codes = R.pool_case(kind, shape, draw)
    v, i = torch_pool(kind, nchw(x))
    U.assert_same(U.bits32(vals).reshape(-1), U.bits32(nhwc(v)).reshape(-1), "values")
    assert np.array_equal(winner_position(kind, codes, shape[2]), nhwc(i)), "winners"
    assert set(np.unique(codes)) <= R.legal_codes(kind, shape[1], shape[2])


@pytest.mark.parametrize("kind,shape", POOLS, ids=POOL_IDS)
def test_max_pool_draw_conditions(kind, shape):
    for draw in R.POOL_DRAWS:
        R.pool_conditions(kind, shape, draw)


def test_tie_figures_of_the_7x9_map():
    x = R.ties_draw((3, 7, 9, 24), 1)
    v3, c3 = R.maxpool3s2_ref(x)
    assert R.tied_fraction(3, x, v3) >= 0.5 and set(np.unique(c3)) == set(range(9))
    x = R.ties_draw((3, 6, 8, 24), 1)
    v2, c2 = R.maxpool2_ref(x)
    assert R.tied_fraction(2, x, v2) >= 0.3 and set(np.unique(c2)) == set(range(4))


@pytest.mark.parametrize("kind,shape", POOLS, ids=POOL_IDS)
def test_max_pool_bwd_refs_are_autograd(kind, shape):
    """No ties (a permutation, float64): the gradient of sum(pool * g); ties: the scatter through torch's indices.  Integer gradients,
    so the ordered fp32 sum is the exact one."""
    B, H, W, C = shape
    x = np.random.default_rng(sum(shape)).permutation(B * H * W * C).reshape(shape).astype(np.float32)
    ref = R.maxpool3s2_ref if kind == 3 else R.maxpool2_ref
    _, codes = ref(x)
    g, old = R.integer_draw(codes.shape, 61), R.integer_draw(shape, 62)
    xt = nchw(x).double().requires_grad_(True)
    (torch_pool(kind, xt)[0] * nchw(g).double()).sum().backward()
    for acc in (0, 1):
        got = R.maxpool3s2_bwd_ref(g, codes, old, acc, H, W) if kind == 3 else R.maxpool2_bwd_ref(g, codes, old, acc)
        assert np.array_equal(got.reshape(-1), R.bf16_from_f64(nhwc(xt.grad) + (old if acc else 0.0)))
    x, _, codes = R.pool_case(kind, shape, "ties")
    _, i = torch_pool(kind, nchw(x))
    want = old.astype(np.float64).copy()
    b, _, _, c = np.meshgrid(np.arange(B), np.arange(codes.shape[1]), np.arange(codes.shape[2]), np.arange(C), indexing="ij")
    pos = nhwc(i)
    np.add.at(want, (b, pos // W, pos % W, c), g.astype(np.float64))
    got = R.maxpool3s2_bwd_ref(g, codes, old, 1, H, W) if kind == 3 else R.maxpool2_bwd_ref(g, codes, old, 1)
    assert np.array_equal(got.reshape(-1), R.bf16_from_f64(want))


@pytest.mark.parametrize("shape", R.POOL2_SHAPES, ids=str)
def test_avgpool_refs_are_avg_pool2d(shape):
    x, dy, old = R.avg_case(shape, "integer")
    xt = nchw(x).double().requires_grad_(True)
    y = F.avg_pool2d(xt, 2)
    assert np.array_equal(R.avgpool2_ref(x).reshape(-1), R.bf16_from_f64(nhwc(y)))
    (y * nchw(dy).double()).sum().backward()
    for acc in (0, 1):
        assert np.array_equal(R.avgpool2_bwd_ref(dy, old, acc).reshape(-1), R.bf16_from_f64(nhwc(xt.grad) + (old if acc else 0.0)))
    # normal draws: the fp32 sum of four bf16 numbers stays within the summation bound of the float64 mean
    x = R.general_draw(shape, 5)
    B, H, W, C = shape
    blk = x.astype(np.float64).reshape(B, H // 2, 2, W // 2, 2, C)
    got = R.widen(R.avgpool2_ref(x)).astype(np.float64)
    assert bool(np.all(np.abs(got - blk.mean((2, 4))) <= 3 * 2.0 ** -24 * np.abs(blk).sum((2, 4)) * 0.25 + 0.5 * R.bf16_ulp(got)))
    # four -0 average to +0 (the sum starts from +0), a NaN stays a NaN
    z = np.full((1, 2, 2, 8), np.float32(-0.0))
    assert not R.avgpool2_ref(z).any()
    z[0, 1, 1, 3] = np.nan
    assert U.is_nan16(R.avgpool2_ref(z)).sum() == 1


def test_chanscale_ref():
    x, keep = R.chanscale_case(3, 15, 24)
    want = (torch.from_numpy(x) * torch.from_numpy(keep)[:, None, :]).to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16)
    assert same16(R.chanscale_ref(x, keep), want)
    assert np.isnan(x).any() and (keep == 0).any() and (keep == 1.25).any()


@pytest.mark.parametrize("case", R.IM2COL_CASES, ids=str)
def test_im2col_ref_is_unfold(case):
    B, C, H, W, k, s, p, ld = case
    bits = R.im2col_image(case)
    keep = ~U.is_nan32(bits) & ((bits & 0x7F800000) != 0x7F800000)         # unfold copies, but torch.equal has no NaN for NaN
    bits = np.where(keep, bits, 0).astype(np.uint32)
    img = torch.from_numpy(U.from_bits32(bits.reshape(-1)).reshape(B, C, H, W).copy())
    cols = F.unfold(img, k, padding=p, stride=s)
    L = cols.shape[-1]
    assert L == R.im2col_out(H, k, s, p) * R.im2col_out(W, k, s, p)
    cols = cols.reshape(B, C, k * k, L).permute(0, 3, 2, 1).reshape(B * L, k * k * C)
    want = cols.to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16)
    rows = R.im2col_ref(bits, k, s, p, ld)
    assert rows.shape == (B * L, ld) and ld % 8 == 0 and ld > k * k * C
    assert np.array_equal(rows[:, :k * k * C], want) and not rows[:, k * k * C:].any()


@pytest.mark.parametrize("M,C", R.ROWS_SHAPES)
def test_relu_refs_are_aten(M, C):
    """torch.relu and its autograd on the very patterns of the GPU test: NaN stays, -0 stays, a NaN output passes the gradient"""
    yb, dyb = R.relu_case(M, C)
    u = torch.from_numpy(R.widen(yb).copy()).requires_grad_(True)
    out = torch.relu(u)
    assert same16(R.relu_fwd_ref(yb), out.detach().to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16))
    fwd = R.relu_fwd_ref(yb)
    assert fwd.reshape(-1)[1] == 0x8000 and U.is_nan16(fwd.reshape(-1)[0]) and fwd.reshape(-1)[3] == 0
    out.backward(torch.from_numpy(R.widen(dyb).copy()))
    got = R.relu_bwd_ref(dyb, fwd)                                     # the kernel sees the stored OUTPUT
    assert same16(got, u.grad.to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16))
    assert got.reshape(-1)[0] == dyb.reshape(-1)[0] != 0 and got.reshape(-1)[1] == 0 and got.reshape(-1)[5] == dyb.reshape(-1)[5]
    assert float(torch.relu(torch.tensor(float("nan")))) != float(torch.relu(torch.tensor(float("nan"))))
    assert np.signbit(float(torch.relu(torch.tensor(-0.0))))


ALL_DW = [(s, "integer") for s in R.DW_MAIN + R.DW_BORDER] + [(s, "ternary") for s in R.DW_TERNARY + [R.DW_WGRAD_CAP]] + [(s, "general") for s in R.DW_GENERAL]


@pytest.mark.parametrize("stride", [1, 2])
@pytest.mark.parametrize("shape,draw", [c for c in ALL_DW if c[0][3] <= 200], ids=lambda v: str(v))
def test_depthwise_refs_are_conv2d(shape, draw, stride):
    B, H, W, C = shape
    k = R.dw_case(shape, stride, draw)
    xt = nchw(k["x"]).double().requires_grad_(True)
    wt = torch.from_numpy(k["w"]).double().reshape(C, 1, 3, 3).requires_grad_(True)
    z = F.conv2d(xt, wt, None, stride, 1, 1, C)
    assert z.shape[2:] == (R.dw_out(H, stride), R.dw_out(W, stride))
    (z * nchw(k["dz"]).double()).sum().backward()
    tol = 0.0 if draw != "general" else 1e-12
    for got, want, mag in ((k["acc"], nhwc(z), k["mag"]), (k["dx"], nhwc(xt.grad), k["dmag"]), (k["dw"], wt.grad.numpy().reshape(C, 3, 3), k["wmag"])):
        assert got.shape == want.shape and bool(np.all(np.abs(got - want) <= tol * mag)), shape
        assert bool(np.all(np.abs(got) <= mag + 1e-300))


@pytest.mark.parametrize("stride", [1, 2])
@pytest.mark.parametrize("shape,draw", [c for c in ALL_DW if c[1] != "general"], ids=lambda v: str(v))
def test_depthwise_exact_conditions(shape, draw, stride):
    k = R.dw_case(shape, stride, draw)
    R.dw_exact_conditions(k, shape in R.DW_MAIN)
    if shape in R.DW_MAIN:
        assert float(np.abs(k["acc"]).max()) <= 9 * 8 * 32


def test_float32_emulation_stays_inside_the_bounds():
    """The kernel's operation sequence in numpy float32 (sequential fused multiply-adds emulated in float64 and rounded once each)
    stays inside the bounds of the general class; so do pairwise and reversed sums."""
    for shape in R.DW_GENERAL[:2]:
        for stride in (1, 2):
            k = R.dw_case(shape, stride, "general")
            a = np.zeros(k["acc"].shape, dtype=np.float32)
            for kh, kw, v in R._dw_taps(k["x"], stride):
                a = (v * k["w"].astype(np.float64)[:, kh, kw] + a.astype(np.float64)).astype(np.float32)
            z = R.widen(R.rounds(a)).astype(np.float64)
            assert bool(np.all(np.abs(z - k["acc"]) <= R.dw_z_bound(k["mag"], z)))
            flat = a.reshape(-1, shape[3])
            for order in (flat, flat[::-1]):
                s1 = np.zeros(shape[3], dtype=np.float32)
                s2 = np.zeros(shape[3], dtype=np.float32)
                for row in order:
                    s1, s2 = s1 + row, s2 + row * row
                got = np.stack([s1, s2]).astype(np.float64)
                assert bool(np.all(np.abs(got - k["stats"]) <= R.dw_stats_bound(k["acc"], k["mag"], 1)))
    x = R.colstats_case(24, "general")
    s1, s2 = np.zeros(24, dtype=np.float32), np.zeros(24, dtype=np.float32)
    for row in x:
        s1, s2 = s1 + row, s2 + row * row
    assert bool(np.all(np.abs(np.stack([s1, s2]).astype(np.float64) - R.colstats_ref(x)) <= R.colstats_bound(x, 1)))


def test_sizes_come_from_the_kernel_constants():
    for name in R.CAP:
        assert R.MAX_ITEMS < R.cap_items(name) <= R.MAX_ITEMS + 8, name
    assert R.MAX_ITEMS < R.im2col_items(R.IM2COL_BIG) < R.MAX_ITEMS * 1.01
    assert R.colstats_blocks(16384) == 1024 and (R.COLSTATS_BIG[0] + 15) // 16 == 1025 and R.colstats_blocks(R.COLSTATS_BIG[0]) == 1024
    assert [R.dw_rpb(c) for c in (8, 24, 200, 2048, 2056)] == [256, 85, 10, 1, 1]
    B, H, W, C = R.DW_WGRAD_CAP
    assert B * H * W == 4097 and R.dw_splits_ref(B, H, W, C, 1) == 256 and -(-4097 // 16) == 257
    for c in (8, 24, 200, 2048):
        rpb = R.dw_rpb(c)
        assert R.dw_splits_ref(1, 16 * rpb, 1, c, 1) == 1 and R.dw_splits_ref(1, 16 * rpb + 1, 1, c, 1) == 2
    assert R.dw_splits_ref(1, 256 * 16, 1, 2048, 1) == 256 and R.dw_splits_ref(1, 255 * 16, 1, 2048, 1) == 255 and R.dw_splits_ref(4, 256 * 16, 1, 2048, 1) == 256
    assert [R.dw_splits_ref(*a) for a in ((0, 4, 4, 8, 1), (1, 0, 4, 8, 1), (1, 4, 0, 8, 1), (1, 4, 4, 12, 1), (1, 4, 4, 0, 1), (1, 4, 4, 8, 3), (1, 4, 4, 8, 0))] == [-1] * 7
    # the statistics forms: R = 8 is run on a one-workgroup grid and on a grid of several
    grids = [R.dw_grid(R.dw_case(s, 1, d)["M"], s[3]) for s, d in ALL_DW if d != "general"]
    assert 1 in grids and any(g > 1 for g in grids) and any(g >= 8 for g in grids)
    for fam in (R.POOL3_SHAPES, R.POOL2_SHAPES, R.DW_MAIN, R.DW_BORDER, R.DW_TERNARY, R.DW_GENERAL):
        assert any(h != w for _, h, w, _ in fam)
    assert any(c[2] != c[3] for c in R.IM2COL_CASES) and any(c[2] % 2 for c in R.IM2COL_CASES) and any(c[2] % 2 == 0 for c in R.IM2COL_CASES)
    assert {(b, c) for b, _, _, c in R.POOL3_SHAPES} == set(R.BC) == {(b, c) for b, _, _, c in R.POOL2_SHAPES}


# ---------------------------------------------------------------------------------------------------------------------------
# the mutants: each returns [(input, draw, told apart)] over inputs of the GPU test
def differ(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape != b.shape or not U.same_bits(a.reshape(-1), b.reshape(-1))


def _pool_mutant(draws, kinds=(3, 2), **kw):
    hit = []
    for kind, shape in POOLS:
        if kind not in kinds:
            continue
        for draw in draws:
            x, vals, codes = R.pool_case(kind, shape, draw)
            v, c = (R.maxpool3s2_ref if kind == 3 else R.maxpool2_ref)(x, **kw)
            hit.append(((kind,) + shape, draw, differ(U.bits32(v), U.bits32(vals)) or differ(c, codes)))
    return hit


def _m_last_tie():
    return _pool_mutant(["ties"], tie="last")


def _m_nan_loses():
    return _pool_mutant(["special", "bits"], nan_wins=False)


def _m_zero_pad():
    return _pool_mutant(["negative"], kinds=(3,), pad="zero")


def _m_floor():
    return _pool_mutant(["ties"], kinds=(3,), oh="floor")


def _m_avg(**kw):
    return [(s, d, differ(R.avgpool2_ref(R.avg_case(s, d)[0], **kw), R.avgpool2_ref(R.avg_case(s, d)[0]))) for s in R.POOL2_SHAPES for d in R.AVG_DRAWS]


def _m_avg_order():
    return _m_avg(order="col")


def _m_avg_round():
    return _m_avg(round_pairs=True)


def _m_im2col():
    return [(c, "bits", differ(R.im2col_ref(R.im2col_image(c), *c[4:], channel_major=True), R.im2col_ref(R.im2col_image(c), *c[4:]))) for c in R.IM2COL_CASES]


def _dw_cases(strides=(1, 2)):
    return [(s, st, R.dw_case(s, st, "integer")) for s in R.DW_MAIN + R.DW_BORDER for st in strides]


def _m_parity():
    return [(s, st, differ(R.bf16_from_f64(R.dw_dgrad_ref(k["dz"], k["w"], st, s[1], s[2], parity=False)[0]), R.bf16_from_f64(k["dx"]))) for s, st, k in _dw_cases((2,))]


def _m_two_roundings():
    return [(s, st, differ(R.rounds(R.widen(R.bf16_from_f64(k["dx"])).reshape(s) + k["old"]).reshape(-1), R.bf16_from_f64(k["dx"] + k["old"]))) for s, st, k in _dw_cases()]


def _m_stats_of_z():
    return [(s, st, not np.array_equal(k["stats"], k["stats_z"])) for s, st, k in _dw_cases()]


def _m_stats_overwrite():
    hit = []
    for s, st, k in _dw_cases():
        pre = R.stats_prefill(2 * s[3], 7)
        hit.append((s, st, not np.array_equal(pre + R.fix_words(k["stats"]).reshape(-1), R.fix_words(k["stats"]).reshape(-1))))
    return hit


def _m_relu_nan():
    return [((M, C), "bits", differ(R.relu_fwd_ref(R.relu_case(M, C)[0], zero_nan=True), R.relu_fwd_ref(R.relu_case(M, C)[0]))) for M, C in R.ROWS_SHAPES]


def _m_relu_bwd_nan():
    hit = []
    for M, C in R.ROWS_SHAPES:
        y, dy = R.relu_case(M, C)
        out = R.relu_fwd_ref(y)
        hit.append(((M, C), "bits", differ(R.relu_bwd_ref(dy, out, zero_nan=True), R.relu_bwd_ref(dy, out))))
    return hit


MUTANTS = {
    "the last maximum wins a tie": _m_last_tie,
    "NaN does not win": _m_nan_loses,
    "the max pool pads with zeros": _m_zero_pad,
    "OH = H // 2 in maxpool3s2": _m_floor,
    "avgpool2 adds x10 before x01": _m_avg_order,
    "avgpool2 rounds the row sums to bf16": _m_avg_round,
    "im2col columns are channel-major": _m_im2col,
    "the stride-2 input gradient drops the parity test": _m_parity,
    "the accumulating input gradient rounds twice": _m_two_roundings,
    "the statistics are those of bf16(z)": _m_stats_of_z,
    "the statistics overwrite": _m_stats_overwrite,
    "relu zeroes NaN": _m_relu_nan,
    "relu_bwd zeroes where y is NaN": _m_relu_bwd_nan,
}


@pytest.mark.parametrize("name", list(MUTANTS))
def test_mutant_is_rejected(name):
    hit = MUTANTS[name]()
    assert any(h for _, _, h in hit), (name, hit)
    if name in ("relu zeroes NaN", "relu_bwd zeroes where y is NaN", "the max pool pads with zeros", "im2col columns are channel-major"):
        assert all(h for _, _, h in hit), (name, hit)                   # every input of the family tells these apart
    if name == "OH = H // 2 in maxpool3s2":
        assert all(h == bool(k[2] % 2 or k[3] % 2) or k[2] == 1 or k[3] == 1 for k, _, h in hit), hit
