"""tests/f32_reference.py against torch in float64 on the CPU, the conditions on its cases, and its mutants: every wrong variant listed
in MUTANTS is told from the true reference by at least one case that tests/test_gpu_f32_exact.py feeds to the kernels.  No GPU."""
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import f32_reference as R  # noqa: E402
import update_reference as U  # noqa: E402


def nchw(a):
    return torch.from_numpy(np.ascontiguousarray(np.moveaxis(a, -1, 1)))


def nhwc(t):
    return np.ascontiguousarray(np.moveaxis(t.detach().numpy(), 1, -1))


def close(a, b, rtol=1e-11):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return bool(np.all(np.abs(a - b) <= rtol * (np.abs(b) + 1e-3)))


# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", R.CONV_SHAPES, ids=str)
@pytest.mark.parametrize("s", R.CONV_S)
@pytest.mark.parametrize("k", R.CONV_K)
def test_conv_refs_are_conv2d_and_its_autograd(k, s, shape):
    """Integer draws: float64 is exact, so the three references equal torch's conv2d, its input gradient and its weight gradient
    exactly; the term counts are those of the taps inside the map."""
    B, H, W = shape
    Cin, Cout = 3, 4
    x, w, dy = R.ints((B, H, W, Cin), 1), R.ints((Cout, k * k, Cin), 2, -4, 4), R.ints((B,) + R.out_size(H, W, k, s) + (Cout,), 3)
    xt = nchw(x).requires_grad_(True)
    wt = torch.from_numpy(w.reshape(Cout, k, k, Cin)).permute(0, 3, 1, 2).contiguous().requires_grad_(True)
    y = F.conv2d(xt, wt, stride=s, padding=(k - 1) // 2)
    tot, mag, cnt = R.conv_ref(x, w, H, W, k, s, 0)
    assert np.array_equal(tot, nhwc(y))
    ones = F.conv2d(torch.ones_like(xt), torch.ones_like(wt), stride=s, padding=(k - 1) // 2)
    assert np.array_equal(np.broadcast_to(cnt, tot.shape), nhwc(ones)) and bool(np.all(mag >= np.abs(tot)))
    (y * nchw(dy)).sum().backward()
    dx, _, cd = R.conv_ref(dy, w, H, W, k, s, 1)
    assert np.array_equal(dx, nhwc(xt.grad))
    assert int(cd.sum()) * Cin == int(cnt.sum()) * Cout          # the transposed form visits the same (tap, pixel) pairs
    dw, _, cw = R.wgrad_ref(x, dy, k, s)
    assert np.array_equal(dw, wt.grad.permute(0, 2, 3, 1).reshape(Cout, k * k, Cin).numpy())
    assert int(cw[0, :, 0].sum()) * Cin == int(cnt.sum())


def test_read_w_honours_the_strides():
    buf = np.arange(200.0)
    w = R.read_w(buf, 50, 7, 3, 4, 5)
    assert w[2, 3, 4] == 2 * 50 + 3 * 7 + 4 and w.shape == (3, 4, 5)
    assert not np.array_equal(w, R.read_w(buf, 50, 7, 3, 4, 5, swap=True))


def _torch_act(u, act):
    return [lambda v: v, F.silu, torch.relu, lambda v: F.leaky_relu(v, float(R.F01))][act](u)


@pytest.mark.parametrize("act", R.BN_ACT)
@pytest.mark.parametrize("M,C", [(2, 3), (257, 9), (1000, 1)])
def test_bn_refs_are_batch_norm_and_its_autograd(M, C, act):
    z, gamma, beta, rm, rv, res = R.bn_fwd_draw(M, C, "normal")
    r = R.bn_fwd_ref(z, gamma, beta, rm, rv, R.MOMENTUM, act, res)
    zt, gt, bt = (torch.from_numpy(a.copy()).requires_grad_(True) for a in (z, gamma, beta))
    rmt, rvt = torch.from_numpy(rm.copy()), torch.from_numpy(rv.copy())
    bn = F.batch_norm(zt, rmt, rvt, gt, bt, True, R.MOMENTUM, R.EPS)
    y = _torch_act(bn, act) + torch.from_numpy(res)
    mean, var = z.mean(0), z.var(0)
    assert close(r["y"].v, y.detach().numpy()) and close(r["rmean"].v, rmt.numpy()) and close(r["rvar"].v, rvt.numpy())
    assert close(r["save"].v, np.concatenate([mean, 1.0 / np.sqrt(var + R.EPS)]))
    # backward, with the float64 statistics as the saved ones
    dy = R.normal((M, C), 5)
    (y * torch.from_numpy(dy)).sum().backward()
    b = R.bn_bwd_ref(dy, z, mean, 1.0 / np.sqrt(var + R.EPS), gamma, beta, np.zeros(C), np.zeros(C), act)
    assert close(b["dz"].v, zt.grad.numpy(), 1e-8) and close(b["ggrad"].v, gt.grad.numpy(), 1e-9) and close(b["bgrad"].v, bt.grad.numpy(), 1e-9)
    assert close(b["sums"].v, np.concatenate([gt.grad.numpy(), bt.grad.numpy()]), 1e-9)


def test_bn_exact_draws_are_exact():
    """M a power of two: the mean, the variance and u are fp32 numbers, so save is float32 of the float64 value and one sequence of
    fp32 operations is left; the constant channel has var = 0 and invstd = 1 / sqrt(eps)."""
    for M in (1, 2, 256):
        z, gamma, beta, rm, rv, res = R.bn_fwd_draw(M, 9, "exact")
        mean, var, inv = R.bn_stats_ref(z)
        assert U.exact32(mean.v) and np.array_equal(mean.v, z.mean(0)) and np.array_equal(var.v, ((z - z.mean(0)) ** 2).sum(0) / M)
        assert var.v[8] == 0 and inv.v[8] == 1.0 / np.sqrt(R.EPS) and (M == 1) == bool(np.all(var.v == 0))
        assert U.exact32((z - mean.v)) and bool(np.all(np.log2(np.abs(gamma)) % 1 == 0)) and not beta.any()
        dy, zb, mean_b, inv_b, g, b, _, _ = R.bn_bwd_draw(M, 9, "exact")
        zh = (zb - mean_b) * inv_b
        assert U.exact32(zh) and U.exact32(zh * g + b) and U.exact32(dy * zh)


def test_every_fixed_sequence_is_within_its_own_bound():
    """The float32 emulations (and float32 of the float64 value elsewhere) of every bounded case satisfy the bound derived for it, and
    a case is bit for bit exactly where it says so."""
    cases = [R.conv_case(*p) for p in R.CONV_PARAMS] + [R.wgrad_case(*p) for p in R.WGRAD_PARAMS] + [R.bn_fwd_case(*p) for p in R.BN_PARAMS] + \
            [R.bn_bwd_case(*p) for p in R.BN_PARAMS] + [R.spp_bwd_case(*p) for p in R.SPP_BWD_PARAMS] + [R.colsum_case(*p) for p in R.COLSUM_PARAMS] + \
            [R.conv_stem_case(d) for d in ("int", "normal")] + [R.conv_head_case(d) for d in ("int", "normal")]
    soft = 0
    for c in cases:
        for k, w in c.want.items():
            assert w.ratio(w.bits) <= 1.0, k
            soft += int(w.soft.sum())
            assert not (c.exact and w.soft.any())
            if w.soft.any():
                assert bool(np.all(w.bound[w.soft] > 0)) and bool(np.all(np.isfinite(w.bound[w.soft])))
    assert soft > 10000


def test_case_conditions():
    """What the case lists must contain."""
    totals = [p[2][0] * np.prod(R.out_size(p[2][1], p[2][2], p[0], p[1])) * R.conv_channels(*p[:4])[1] for p in R.CONV_PARAMS if not p[3]]
    assert any(t > 256 and t % 256 for t in totals)
    for k in R.CONV_K:
        for s in R.CONV_S:
            assert {R.conv_channels(k, s, sh, tr) for sh in R.CONV_SHAPES for tr in (0, 1)} >= set(R.CONV_CH[:2])
    assert {R.conv_channels(k, s, sh, 0) for k in R.CONV_K for s in R.CONV_S for sh in R.CONV_SHAPES} == set(R.CONV_CH)
    for act in R.BN_ACT:                                  # every form of the BatchNorm call with every activation
        v = {R.bn_variant(M, C, act) for M in R.BN_M for C in R.BN_C}
        for i in range(3):
            assert {x[i] for x in v} == {False, True}, (act, i)
        assert any(R.bn_variant(1, C, act)[1] for C in R.BN_C), "M = 1 with running statistics: the unb = var branch"
        g = {(R.BN_M.index(M) + R.BN_C.index(C) + act) % 4 != 3 for M in R.BN_M for C in R.BN_C}
        assert g == {False, True}
    assert R.COPY_M * R.COPY_C % 256 and R.COPY_M * R.COPY_C > 256
    x = R.spp_inputs("special", (1, 14, 5), 1)
    assert np.isnan(x[1]).any() and bool((x[1] == R.NEG).any())
    head = R.conv_head_case("int")
    y = head.want["y"].bits.reshape(2, R.HEAD_A, -1)
    assert bool(np.all(y[:, [0, -1]] == np.uint32(U.SENT32))) and not bool(np.any(y[:, 1:-1] == np.uint32(U.SENT32)))


# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dr", ["ties", "special"])
@pytest.mark.parametrize("C", R.SPP_C)
@pytest.mark.parametrize("shape", R.SPP_MAPS, ids=str)
def test_spp_ref_is_max_pool2d(shape, C, dr):
    x, vals, idx = R.spp_inputs(dr, shape, C)
    for p, k in enumerate((5, 9, 13)):
        v, i = F.max_pool2d(nchw(x), k, 1, k // 2, return_indices=True)
        U.assert_same(U.bits32(vals[p]), U.bits32(nhwc(v)), "values of window %d" % k)
        assert np.array_equal(idx[p], nhwc(i).astype(np.int32)), k
    if dr == "special":                                   # (with one channel a map of up to 3x3 lies inside every window of its NaN)
        assert np.isnan(vals).any() and (bool((vals[0] == R.NEG).any()) or (C == 1 and shape[1] * shape[2] <= 9)), "a NaN and a window without a maximum"


def test_spp_ref_on_the_two_nan_map():
    x, vals, idx = R.spp_inputs("nan33", (1, 3, 3), 1)
    v, i = F.max_pool2d(nchw(x), 5, 1, 2, return_indices=True)
    assert bool(np.all(np.isnan(nhwc(v)))) and bool(np.all(nhwc(i) == 5))
    assert bool(np.all(np.isnan(vals))) and bool(np.all(idx == 5))
    mv, mi = R.spp_fwd_ref(x, nan=False)                  # what a pool that ignores NaN reports
    assert bool(np.all(mv == 9)) and bool(np.all(mi == 7))


@pytest.mark.parametrize("C", R.SPP_C)
@pytest.mark.parametrize("shape", R.SPP_MAPS, ids=str)
def test_spp_bwd_ref_is_autograd(shape, C):
    """The ties draw: torch routes each gradient to the index it reported, the first maximum."""
    x, _, idx = R.spp_inputs("ties", shape, C)
    B, H, W = shape
    dys, old = R.ints((3, B, H, W, C), 4), R.ints((B, H, W, C), 5)
    xt = nchw(x).double().requires_grad_(True)
    sum((F.max_pool2d(xt, k, 1, k // 2) * nchw(g)).sum() for k, g in zip((5, 9, 13), dys)).backward()
    for acc in (0, 1):
        r = R.spp_bwd_ref(dys, idx, old, acc)
        assert np.array_equal(r.v, nhwc(xt.grad) + (old if acc else 0.0))


def test_upsample_refs_are_interpolate():
    B, H, W = R.UP_SHAPE
    x = R.normal((B, H, W, R.UP_C), 1)
    xt = nchw(x).requires_grad_(True)
    y = F.interpolate(xt, scale_factor=2, mode="nearest")
    assert np.array_equal(R.upsample2_ref(x), nhwc(y))
    dy, old = R.ints((B, 2 * H, 2 * W, R.UP_C), 2), R.ints((B, H, W, R.UP_C), 3)
    (y * nchw(dy)).sum().backward()
    for acc in (0, 1):
        assert np.array_equal(R.upsample2_bwd_ref(dy, old, acc).astype(np.float64), nhwc(xt.grad) + (old if acc else 0.0))


@pytest.mark.parametrize("B,H,W", R.STEM_IMAGES + [(1, 6, 4)])
def test_stem_ref_is_focus_and_unfold(B, H, W):
    img = R.normal((B, 3, H, W), 9).astype(np.float32)
    t = torch.from_numpy(img)
    tl, tr, bl, br = t[..., ::2, ::2], t[..., ::2, 1::2], t[..., 1::2, ::2], t[..., 1::2, 1::2]
    foc = torch.cat((tl, bl, tr, br), dim=1)              # Focus.forward
    cols = F.unfold(foc, 3, padding=1).reshape(B, 12, 9, -1).permute(0, 3, 2, 1).reshape(-1, 108)
    for ld in R.STEM_LD:
        got = R.stem_rows_ref(U.bits32(img).reshape(B, 3, H, W), ld)
        assert got.shape == (B * (H // 2) * (W // 2), ld) and not got[:, 108:].any()
        assert np.array_equal(U.from_bits32(got[:, :108]).reshape(-1, 108), cols.numpy())


def test_decode_bwd_ref_is_autograd():
    B, H, W, a0, C = 2, R.DEC_H, R.DEC_W, R.DEC_A0, 3
    A = a0 + H * W + R.DEC_TAIL
    t = torch.from_numpy(R.normal((B, H * W, 27 + C), 1, 0.5)).requires_grad_(True)
    yv, xv = torch.meshgrid([torch.arange(H), torch.arange(W)], indexing="ij")
    grid = torch.stack((xv, yv), 2).view(1, -1, 2)
    dec = torch.cat([(t[..., :2] + grid) * R.DEC_S, torch.exp(t[..., 2:26]) * R.DEC_S, t[..., 26:]], -1)
    dout, out, org = R.dyadic4((B, A, 27 + C), 2), np.zeros((B, A, 27 + C)), R.dyadic4((B, A, 26), 3)
    out[:, a0:a0 + H * W] = dec.detach().numpy()
    (dec * torch.from_numpy(dout[:, a0:a0 + H * W])).sum().backward()
    reg, cls = R.decode_bwd_ref(dout, out, a0, H, W, R.DEC_S, org)
    g = t.grad.numpy()
    want = g[..., :27].copy()
    want[..., :26] += org[:, a0:a0 + H * W]
    got = U.from_bits32(reg).reshape(B, H * W, 32)
    tol = 1e-6 * (np.abs(g[..., :27]) + np.abs(np.pad(org[:, a0:a0 + H * W], ((0, 0), (0, 0), (0, 1)))) + 1.0)      # fp32 against float64
    assert bool(np.all(np.abs(got[..., :27] - want) <= tol)) and not got[..., 27:].any()
    gc = U.from_bits32(cls).reshape(B, H * W, 8)
    assert np.array_equal(gc[..., :C], g[..., 27:].astype(np.float32)) and not cls.reshape(B, H * W, 8)[..., C:].any()


def test_colsum_ref():
    for p in R.COLSUM_PARAMS:
        c = R.colsum_case(*p)
        g = U.from_bits32(c.bufs["g"][1]).reshape(p[0], 32)[:, :p[1]].astype(np.float64)
        old = U.from_bits32(c.bufs["db"][1]).astype(np.float64)
        w = c.want["db"]
        want = (w.val if w.soft.any() else w.floats())
        assert close(want, old + g.sum(0), 1e-12)


# ---------------------------------------------------------------------------------------------------------------------------
# the mutants: (family, [(builder, parameters)]) lists; a mutant is rejected by a case if the comparison the GPU test makes fails
def _hits(builder, params, mut):
    return [(builder.__name__,) + tuple(p) for p in params if R.rejects(builder(*p), builder(*p, mut=mut))]


CONV_T = [p for p in R.CONV_PARAMS if p[3]]
CONV_F = [p for p in R.CONV_PARAMS if not p[3]]
BN_RUN = [p for p in R.BN_PARAMS if R.bn_variant(*p[:3])[1]]
DRAWS2 = [("int",), ("normal",)]


def _no_acc():
    return (_hits(R.conv_case, [p for p in R.CONV_PARAMS if p[4]], "no_acc") + _hits(R.wgrad_case, R.WGRAD_PARAMS, "no_acc") +
            _hits(R.bn_bwd_case, R.BN_PARAMS, "no_acc") + _hits(R.spp_bwd_case, [p for p in R.SPP_BWD_PARAMS if p[3]], "no_acc") +
            _hits(R.up_bwd_case, [(d, 1) for d in ("int", "normal")], "no_acc") + _hits(R.copy_case, [("int",), ("normal",)], "no_acc") +
            _hits(R.colsum_case, R.COLSUM_PARAMS, "no_acc"))


MUTANTS = {
    "a tap offset off by one": lambda: _hits(R.conv_case, CONV_F, "tap") + _hits(R.wgrad_case, R.WGRAD_PARAMS, "tap"),
    "the ny % s test dropped in the transposed conv": lambda: _hits(R.conv_case, CONV_T, "no_mod"),
    "sy >= OH dropped": lambda: _hits(R.conv_case, CONV_T, "no_oh"),
    "the bias added in the transposed form": lambda: _hits(R.conv_case, CONV_T, "bias_t"),
    "accumulate ignored": _no_acc,
    "y_row0 ignored": lambda: _hits(R.conv_head_case, DRAWS2, "row0"),
    "wt and wco swapped": lambda: _hits(R.conv_case, R.CONV_PARAMS, "swap_w") + _hits(R.conv_head_case, DRAWS2, "swap_w"),
    "the biased variance in running_var": lambda: _hits(R.bn_fwd_case, BN_RUN, "biased"),
    "M for M - 1": lambda: _hits(R.bn_fwd_case, BN_RUN, "m_for_m1"),
    "M - 1 for M in the variance": lambda: _hits(R.bn_fwd_case, [p for p in R.BN_PARAMS if p[0] > 1], "m1_var"),
    "num_batches bumped once per channel": lambda: _hits(R.bn_fwd_case, R.BN_PARAMS, "nbt_c"),
    "the residual added before the activation": lambda: _hits(R.bn_fwd_case, R.BN_PARAMS, "res_first"),
    "the last maximum for the first": lambda: _hits(R.spp_fwd_case, R.SPP_FWD_PARAMS, "last"),
    "NaN not propagated in the pool": lambda: _hits(R.spp_fwd_case, R.SPP_FWD_PARAMS, "no_nan"),
    "the idx planes in another order": lambda: _hits(R.spp_fwd_case, R.SPP_FWD_PARAMS, "planes"),
    "the Focus patches top-right before bottom-left": lambda: _hits(R.stem_case, [(i, ld) for i in R.STEM_IMAGES for ld in R.STEM_LD], "patch"),
    "the radii gradient without * out": lambda: _hits(R.decode_case, R.DEC_PARAMS, "no_out"),
    "d_origin with stride 27 for 26": lambda: _hits(R.decode_case, R.DEC_PARAMS, "stride27"),
    "the pad columns of d_cls not zeroed": lambda: _hits(R.decode_case, R.DEC_PARAMS, "pad"),
    "the upsample gradient summed as a chain": lambda: _hits(R.up_bwd_case, [(d, a) for d in ("int", "normal") for a in (0, 1)], "chain"),
}


@pytest.mark.parametrize("name", list(MUTANTS))
def test_mutant_is_rejected(name):
    hit = MUTANTS[name]()
    assert hit, name
    fam = {h[0] for h in hit}
    if name == "accumulate ignored":                      # by every family that accumulates
        assert fam == {"conv_case", "wgrad_case", "bn_bwd_case", "spp_bwd_case", "up_bwd_case", "copy_case", "colsum_case"}, fam
        assert any(h[0] == "conv_case" and h[1:5] == (1, 2, (1, 6, 4), 1) for h in hit), "k = 1, s = 2 on an even map: the old value in the odd rows"
    if name == "a tap offset off by one":
        assert fam == {"conv_case", "wgrad_case"}
    if name == "the ny % s test dropped in the transposed conv":
        assert all(h[2] == 2 for h in hit) and any(h[1:4] == (1, 2, (1, 6, 4)) for h in hit)
    if name == "sy >= OH dropped":
        assert any(h[1:4] == (3, 2, (1, 6, 4)) for h in hit)
    if name == "NaN not propagated in the pool":
        assert all(h[3] != "ties" for h in hit) and any(h[3] == "nan33" for h in hit)
    if name == "the last maximum for the first":
        assert any(h[3] == "ties" for h in hit)
    if name == "d_origin with stride 27 for 26":
        assert all(h[2] for h in hit)
    if name == "the upsample gradient summed as a chain":
        assert all(h[1] == "normal" for h in hit), "integer sums are the same in every order"
