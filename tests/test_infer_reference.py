"""tests/infer_reference.py on the CPU: the references against independent code (torch's batch_norm and conv2d, the oracle's eval
head and postprocess), the conditions on the draws of tests/test_gpu_infer_exact.py (each large case passes its grid cap by less than
a workgroup's worth and a tail, the fold layout has the chunks it claims, ties and thresholds are equal in bits), the float32
emulations against the bounds the GPU test uses (printed as INFER-REF err / bound), and sixteen planted mutants, each rejected by the
comparison the GPU test makes on an input the GPU test feeds.  No GPU."""
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import infer_reference as R  # noqa: E402
import update_reference as U  # noqa: E402

f32 = np.float32
T64 = lambda a: torch.from_numpy(np.ascontiguousarray(np.asarray(a, dtype=np.float64)))  # noqa: E731


# ---------------------------------------------------------------------------------------------------------------------------
def test_fma32_rounds_once():
    """3 * (2^24 + 2) 2^-24 lies exactly between two fp32 numbers; -+2^-70 decides, which float64 cannot see"""
    b = f32((2 ** 24 + 2) * 2.0 ** -24)
    lo, hi = f32((3 * 2 ** 24 + 4) * 2.0 ** -24), f32((3 * 2 ** 24 + 8) * 2.0 ** -24)
    r, redone = R.fma32(np.array([3.0, 3.0, 3.0], dtype=f32), np.array([b, b, b]), np.array([-2.0 ** -70, 2.0 ** -70, 0.0], dtype=f32))
    assert list(r) == [lo, hi, hi] and redone == 2
    rng = np.random.default_rng(0)
    a, bb, c = R.bf(rng.standard_normal(4096, dtype=f32)), rng.standard_normal(4096, dtype=f32), rng.standard_normal(4096, dtype=f32)
    want = torch.addcmul(T64(c), T64(a), T64(bb)).float().numpy()        # float64 then fp32: right wherever nothing was redone
    got, redone = R.fma32(a, bb, c)
    assert redone == 0 and np.array_equal(got, want)


@pytest.mark.parametrize("M,C", R.BN_SHAPES)
def test_bn_act_infer_ref_is_batch_norm(M, C):
    """float64: F.batch_norm(training=False), the activation, the residual; then the fp32 emulation against the float64 form of its
    own scale / shift under bn_tol (act 1) and under the bf16 rounding alone (act 0, 2, 3)."""
    d = R.bn_draw(M, C)
    zt = T64(d["z"])
    bn = F.batch_norm(zt, T64(d["mean"]), T64(d["var"]), T64(d["gamma"]), T64(d["beta"]), False, 0.0, d["eps"])
    acts = {0: lambda u: u, 1: F.silu, 2: torch.relu, 3: lambda u: F.leaky_relu(u, 0.1)}
    sc64, sh64 = R.bn_consts64(d["gamma"], d["beta"], d["mean"], d["var"], d["eps"])
    sc, sh = R.bn_consts32(d["gamma"], d["beta"], d["mean"], d["var"], d["eps"])
    assert np.allclose(sc, sc64, rtol=2.0 ** -22) and np.allclose(sh, sh64, rtol=0, atol=2.0 ** -22 * (np.abs(d["beta"]) + np.abs(d["mean"] * sc64)).max())
    u, redone = R.fma32(d["z"], sc[None, :], sh[None, :])
    worst = 0.0
    for act in (0, 1, 2, 3):
        for res in (None, d["res"]):
            want = acts[act](bn) + (0 if res is None else T64(res))
            _, _, y64 = R.bn_act_infer_ref64(d["z"], sc64, sh64, act, res)
            fin = np.isfinite(y64)
            assert np.array_equal(np.isnan(y64), torch.isnan(want).numpy()) and np.array_equal(y64[~fin & ~np.isnan(y64)], want.numpy()[~fin & ~np.isnan(y64)])
            assert np.allclose(y64[fin], want.numpy()[fin], rtol=1e-12, atol=1e-12)
            assert np.isnan(y64[0, 1]) and (act == 2 or not np.isfinite(y64[M - 1, 5])), "the planted NaN / inf must come through"
            # the emulation against the float64 form of ITS scale and shift
            _, a64, y64e = R.bn_act_infer_ref64(d["z"], sc, sh, act, res)
            got = U.from_bits32(U.bf16_widen(R.bn_act_infer_ref(u, act, res))).astype(np.float64).reshape(M, C)
            tol = R.bn_tol(d["z"], sc, sh, d["mean"], d["beta"], a64, y64e, act)
            fin = np.isfinite(y64e)
            assert np.array_equal(np.isnan(got), np.isnan(y64e)) and np.array_equal(got[~fin & ~np.isnan(y64e)], y64e[~fin & ~np.isnan(y64e)])
            worst = max(worst, float((np.abs(got[fin] - y64e[fin]) / tol[fin]).max()))
    print("INFER-REF bn_act_infer %dx%d: emulation err / bound %.3f, %d fma redone in rationals" % (M, C, worst, redone))
    assert worst <= 1.0


def test_fold_ref_then_conv_is_conv_then_bn():
    """float64 conv -> BatchNorm(eval) against the conv over the folded bf16 weights + bias, within the bf16 rounding of the weights"""
    L = R.fold_layout("small")
    flat, bstat = R.fold_draw("small")
    wf, bias = R.fold_bn_ref(L, flat, bstat)
    rng = np.random.default_rng(5)
    for s, d in enumerate(L.desc):
        mo, po, co, t, ci, cp, go, bo, mu, vo, bi, _ = (int(v) for v in d)
        k = 3 if t == 9 else 1
        w = T64(flat[mo:mo + co * t * ci]).reshape(co, k, k, ci).permute(0, 3, 1, 2)
        x = T64(rng.standard_normal((2, ci, 5, 5)))
        conv = F.conv2d(x, w, padding=k // 2)
        if float(L.eps[s]) > 0:
            want = F.batch_norm(conv, T64(bstat[mu:mu + co]), T64(bstat[vo:vo + co]), T64(flat[go:go + co]), T64(flat[bo:bo + co]), False, 0.0, float(L.eps[s]))
        else:                                                           # F.batch_norm refuses eps = 0: its formula written out
            v = lambda a: T64(a)[None, :, None, None]  # noqa: E731
            want = (conv - v(bstat[mu:mu + co])) / torch.sqrt(v(bstat[vo:vo + co])) * v(flat[go:go + co]) + v(flat[bo:bo + co])
        rows = wf[po:po + co * t * cp].reshape(co, t, cp)
        assert bool(np.all(rows[:, :, ci:] == U.SENT16)), "a pad column was written"
        wq = T64(U.from_bits32(U.bf16_widen(rows[:, :, :ci].reshape(-1)))).reshape(co, k, k, ci).permute(0, 3, 1, 2)
        b = T64(U.from_bits32(bias[bi:bi + co]))
        got = F.conv2d(x, wq, b, padding=k // 2)
        scale = T64(flat[go:go + co]) / torch.sqrt(T64(bstat[vo:vo + co]) + float(L.eps[s]))
        mag = F.conv2d(x.abs(), (w * scale[:, None, None, None]).abs(), padding=k // 2)
        tol = 2.0 ** -8 * 1.001 * mag + 2.0 ** -21 * (T64(flat[bo:bo + co]).abs() + (T64(bstat[mu:mu + co]) * scale).abs())[None, :, None, None]
        assert bool(((got - want).abs() <= tol).all()), s
    used = np.ones(L.wf_n, dtype=bool)
    for d in L.desc:
        used[int(d[1]):int(d[1]) + int(d[2] * d[3] * d[5])] = False
    assert used.any() and bool(np.all(wf[used] == U.SENT16)), "the gaps between the packed segments"


def _oracle_head(raw_lvl, H, W, s):
    """the oracle's Head.forward(train=False) on one level whose convolutions are the identity: its decode and nothing else"""
    from oracle import model as om
    B, _, ncols = raw_lvl.shape
    h = om.Head.__new__(om.Head)
    torch.nn.Module.__init__(h)
    ident = lambda x: x  # noqa: E731
    h.strides, h.stems, h.cls_convs, h.reg_convs = (s,), [ident], [ident], [ident]
    h.reg_preds, h.obj_preds, h.cls_preds = [lambda f: f[:, :26]], [lambda f: f[:, 26:27]], [lambda f: f[:, 27:]]
    feat = T64(raw_lvl).reshape(B, H, W, ncols).permute(0, 3, 1, 2)
    return om.Head.forward(h, [feat], train=False).numpy()


@pytest.mark.parametrize("H,W", R.DECODE_MAPS)
def test_decode_eval_ref_is_the_oracle_head(H, W):
    worst_r = worst_s = 0.0
    for ncols in R.DECODE_NCOLS[1:]:
        raw = R.decode_case(2, H, W, ncols)
        a0 = R.DECODE_A0
        lvl = raw[:, a0:a0 + H * W]
        for s in R.DECODE_STRIDES:
            out, radii, scores = R.decode_eval_ref(raw, a0, H, W, s)
            with np.errstate(all="ignore"):
                want = _oracle_head(lvl, H, W, s)
            fin = np.isfinite(lvl[..., :2].astype(np.float64))
            assert np.array_equal(out[:, a0:a0 + H * W, :2].astype(np.float64)[fin], want[..., :2][fin])           # exact in fp32: t = k / 1024
            assert np.allclose(radii, want[..., 2:26], rtol=1e-15, equal_nan=True) and np.allclose(scores, want[..., 26:], rtol=1e-15, atol=0, equal_nan=True)
            keep = np.ones(raw.shape, dtype=bool)
            keep[:, a0:a0 + H * W] = False
            assert np.array_equal(U.bits32(out).reshape(raw.shape)[keep], U.bits32(raw).reshape(raw.shape)[keep]), "a row outside the map changed"
            er, br, es, bs = R.decode_errors(out[:, a0:a0 + H * W], lvl, s, radii, scores)
            assert br == 0 and bs == 0, (br, bs)
            worst_r, worst_s = max(worst_r, er), max(worst_s, es)
    print("INFER-REF decode %dx%d: fp32 emulation radii %.3f of %g ulp, sigmoid %.3f of %g ulp" % (H, W, worst_r, R.RADII_ULP, worst_s, R.SCORE_ULP))
    assert worst_r <= R.RADII_ULP and worst_s <= R.SCORE_ULP


def _same_dets(got, want):
    assert len(got) == len(want)
    for a, b in zip(got, want):
        assert (a is None) == (b is None)
        if a is not None:
            assert a.shape == tuple(b.shape) and U.same_bits(U.bits32(a), U.bits32(b.numpy())), "detections differ"


@pytest.mark.parametrize("tag", ["a", "b", "large"])
def test_postprocess_ref_is_the_oracle_on_the_end_to_end_draws(golden, tag):
    """the draws of tests/test_gpu_infer.py (the synthetic head is a draw generator, not code under test)"""
    from ep24 import synth
    from oracle import post as opost
    if tag == "large":
        raw = synth.make_raw_head(2, size=1280, seed=7)
        pred = synth.decode_head(raw, size=1280)
        pred[..., 26:] = torch.sigmoid(raw[..., 26:] + 3.0)
        args = (80, 0.25, 0.5, False)
    else:
        z = golden("g9_postprocess_" + tag)
        raw = synth.make_raw_head(3, seed=int(z["head_seed"]), num_classes=80)
        pred = synth.decode_head(raw)
        g = torch.Generator().manual_seed(int(z["noise_seed"]))
        pred[..., 26:] = torch.sigmoid(raw[..., 26:] + 4.5 + torch.randn(raw[..., 26:].shape, generator=g))
        pred[2, :, 26] = 0.0
        args = (80, 0.7, 0.45, bool(int(z["agnostic"])))
    want = opost.postprocess(pred.clone(), *args)
    _same_dets(R.postprocess_ref(pred.numpy(), *args), want)
    assert any(w is not None and len(w) > 3 for w in want)


@pytest.mark.parametrize("agnostic", [False, True])
def test_stage_refs_are_the_oracle_on_the_new_draws(agnostic):
    """prepare_draw without its NaN rows (the oracle's torch.max and its rectangle propagate NaN where the kernel's rule is stated in
    include/ep24.h); the NMS draws against the oracle's nms / batched_nms (ties by row are defined there: lexsort)."""
    from oracle import post as opost
    for C in R.PREP_C:
        p = R.prepare_draw(1000, C)
        p = p[~np.isnan(p).any(1)]
        for conf in (R.CONF_THRE, 0.0):
            want = opost.postprocess(torch.from_numpy(p[None].copy()), C, conf, R.NMS_THRE, agnostic)
            _same_dets(R.postprocess_ref(p[None], C, conf, R.NMS_THRE, agnostic), want)
            assert want[0] is not None
    for name, A, P, ns, draw in R.NMS_CASES:
        _, _, score, cls, rect = R.nms_case(name)
        for b in range(len(ns)):
            with np.errstate(all="ignore"):
                cand = np.flatnonzero(score[b] >= 0)
            assert cand.size == ns[b]
            got = R.nms_ref(score[b], cls[b], rect[b], R.NMS_THRE, agnostic)
            if cand.size == 0:
                assert got.size == 0
                continue
            bx, sc, ci = torch.from_numpy(rect[b][cand]), torch.from_numpy(score[b][cand]), torch.from_numpy(cls[b][cand])
            k = opost.nms(bx, sc, R.NMS_THRE) if agnostic else opost.batched_nms(bx, sc, ci, R.NMS_THRE)
            assert np.array_equal(got, cand[k.numpy()]), (name, b)
            if draw == "general" and ns[b] > 100:
                assert 0.2 <= 1 - got.size / ns[b] <= 0.85, "about half suppressed: %g" % (1 - got.size / ns[b])


def test_edge_images_mean_what_they_claim():
    score, cls, rect = R.edge_images()
    names = list(R.EDGE_IMAGES)
    keep = lambda n, thr, ag: list(R.nms_ref(score[names.index(n)], cls[names.index(n)], rect[names.index(n)], thr, ag))  # noqa: E731
    iou = R.iou32(rect[0, 0], rect[0, 1:2])[0]
    assert U.bits32(iou)[()] == U.bits32(f32(R.NMS_THRE))[()] == U.bits32(f32(R.NMS_THRE_BELOW))[()] + 1
    for ag in (0, 1):
        assert keep("threshold pair", R.NMS_THRE, ag) == [0, 1] and keep("threshold pair", R.NMS_THRE_BELOW, ag) == [0]
        assert keep("degenerate pair", R.NMS_THRE, ag) == [0, 2] and np.isnan(R.iou32(rect[1, 0], rect[1, 2:3])[0])
        assert keep("chain", R.NMS_THRE, ag) == [2, 1]
    i_ab, i_bc, i_ac = R.iou32(rect[2, 2], rect[2, 0:1])[0], R.iou32(rect[2, 0], rect[2, 1:2])[0], R.iou32(rect[2, 2], rect[2, 1:2])[0]
    assert i_ab > 0.5 and i_bc > 0.5 and i_ac < 0.5
    assert keep("cross-class pair", R.NMS_THRE, 0) == [1, 0, 2] and keep("cross-class pair", R.NMS_THRE, 1) == [1, 2]
    assert np.signbit(score[3, 2]) and score[3, 2] == 0, "-0.0 is a candidate"


# ---------------------------------------------------------------------------------------------------------------------------
def test_the_inputs_reach_what_they_claim():
    # grid caps: beyond the cap by less than one workgroup's worth and a tail
    M, C = R.BN_CAP
    items = M * (C // 8)
    assert R.BN_MAX_BLOCKS * R.BN_ITEMS_PER_BLOCK < items <= (R.BN_MAX_BLOCKS + 2) * R.BN_ITEMS_PER_BLOCK and R.bn_grid(M, C) == R.BN_MAX_BLOCKS
    assert all(R.bn_grid(m, c) < R.BN_MAX_BLOCKS for m, c in R.BN_SHAPES) and max(c for _, c in R.BN_SHAPES) == R.BN_MAX_C
    assert all(len({0, *(x for x in lay)}) == (4 if name == "strided" else 1) and all(x % 8 == 0 for x in lay) for name, lay in R.BN_LAYOUTS.items())
    Lb = R.fold_layout("big")
    assert R.FOLD_CAP < Lb.total < R.FOLD_CAP + R.FOLD_CHUNK
    assert int(((Lb.prefix > R.FOLD_CAP) & (Lb.prefix < Lb.total)).sum()) >= 2, "the second trip's chunk must hold three segments"
    B, H, W, ncols = R.DECODE_CAP
    assert R.DECODE_MAX_ITEMS < B * H * W * ncols < R.DECODE_MAX_ITEMS + 64 * 256 and H != W
    assert R.PREP_MAX_ROWS < R.PREP_CAP[0] < R.PREP_MAX_ROWS + 512
    assert (R.GATHER_N[-1] - 1) * 29 <= R.GATHER_MAX_ITEMS < R.GATHER_N[-1] * 29 and R.GATHER_A >= R.GATHER_N[-1] and R.GATHER_NCOLS != 29
    # the small fold layout
    L = R.fold_layout("small")
    numel = np.diff(L.prefix)
    assert {24, 96, 1000, 1024, 1048} <= set(int(v) for v in numel)
    per_chunk = [int(((L.prefix[:-1] < (c + 1) * R.FOLD_CHUNK) & (L.prefix[1:] > c * R.FOLD_CHUNK)).sum()) for c in range(-(-L.total // R.FOLD_CHUNK))]
    assert max(per_chunk) >= 3 and per_chunk[0] >= 3, per_chunk
    assert 2048 in L.prefix[1:-1] and L.total % R.FOLD_CHUNK != 0 and L.total_channels % 256 != 0 and L.total_channels > 256
    assert len(set(float(e) for e in L.eps)) == L.n_seg and 0.0 in L.eps
    assert len(set(L.orders)) == 7, "two tables in the same order"
    assert any(s[2] == 12 and s[3] == 16 for s in L.segs) and any(s[2] == 3 and s[3] == 8 for s in L.segs) and {1, 9} == {s[1] for s in L.segs}
    assert R.fold_layout("one").n_seg == 1
    flat, bstat = R.fold_draw("small")
    for d in L.desc:                                                    # every table read by the call is finite; the rest is NaN
        assert np.isfinite(flat[d[0]:d[0] + d[2] * d[3] * d[4]]).all() and np.isfinite(flat[d[6]:d[6] + d[2]]).all() and np.isfinite(bstat[d[9]:d[9] + d[2]]).all()
    assert int(np.isfinite(flat).sum()) == L.total + 2 * L.total_channels and int(np.isfinite(bstat).sum()) == 2 * L.total_channels
    # the BatchNorm draws
    for M, C in R.BN_SHAPES:
        d = R.bn_draw(M, C)
        assert (d["gamma"] < 0).any() and (d["gamma"] > 0).any() and (d["var"] == 0).any() and d["eps"] < 1.01e-3
        assert int(np.isnan(d["z"]).sum()) == 1 and int(np.isposinf(d["z"]).sum()) == 1 and int(np.isneginf(d["z"]).sum()) == 1
    assert {R.BN_EPS[s] for s in R.BN_SHAPES} == {1e-3, 1e-5}
    # the decode draws
    for (H, W) in R.DECODE_MAPS:
        for ncols in R.DECODE_NCOLS:
            raw = R.decode_case(2, H, W, ncols)
            lvl = raw[:, R.DECODE_A0:R.DECODE_A0 + H * W]
            for lo, hi in ((2, 26), (26, ncols)):
                blk = lvl[..., lo:hi]
                for v in R.PLANTED:
                    hit = np.isnan(blk) if np.isnan(v) else (blk == f32(v)) & (np.signbit(blk) == np.signbit(f32(v)))
                    assert hit.any(), (H, W, ncols, lo, v)
            assert raw.shape[1] > H * W + R.DECODE_A0 and R.DECODE_A0 > 0
    assert any(h != w for h, w in R.DECODE_MAPS)
    # the prepare draw
    ray = R.ray_factors()
    for C in R.PREP_C:
        p = R.prepare_draw(1000, C)
        score, conf, cls, rect = R.post_prepare_ref(p, C, R.CONF_THRE, ray)
        i = np.arange(1000) % 16
        assert bool(np.all(U.bits32(score[i == 3]) == U.bits32(f32(R.CONF_THRE)))), "obj * conf = conf_thre in bits"
        prod = (p[i == 4, 26] * conf[i == 4]).astype(f32)
        assert bool(np.all(U.bits32(prod) == U.bits32(f32(R.CONF_THRE)) - 1)) and bool(np.all(score[i == 4] == -1)), "one ulp below"
        assert bool(np.all(np.isnan(conf[i == 5]) & (cls[i == 5] == 0) & (score[i == 5] == -1))), "a leading NaN stays"
        assert bool(np.all(np.isnan(conf[i == 10]) & (cls[i == 10] == 0)))
        assert bool(np.all(score[i == 7] == -1)) and not np.isnan(rect).any()
        if C >= 2:
            assert bool(np.all(~np.isnan(conf[i == 6]) & (cls[i == 6] < C - 1))), "a NaN behind the start is passed over"
            rep = p[i == 2, 27:]
            assert bool(np.all((rep == rep.max(1, keepdims=True)).sum(1) >= 2)) and bool(np.all(cls[i == 2] == 0))
        assert bool(np.all(cls[i == 1] == 0)) and (p[i == 8, 2:26] < 0).any() and not p[i == 9, 2:26].any()
        assert bool(np.all(rect[i == 9, 0] == rect[i == 9, 2])), "zero radii: a zero-area rectangle"
        s0 = R.post_prepare_ref(p, C, 0.0, ray)[0]
        assert bool(np.all((s0 >= 0) | np.isnan(p[:, 26] * conf)))
    # the NMS draws
    _, _, score, _, _ = R.nms_case("all-equal")
    assert len(set(U.bits32(score[0][score[0] >= 0]).tolist())) == 1, "equal scores in bits"
    _, _, score, _, _ = R.nms_case("zeros")
    z = score[0][score[0] >= 0]
    assert set(U.bits32(z).tolist()) == {0, 0x80000000}
    ns = sorted({n for c in R.NMS_CASES for n in c[3]})
    assert {0, 1, 2, 1023, 1024, 1025, 2049} <= set(ns) and {1, 7, 1024, 2100} == {c[1] for c in R.NMS_CASES}
    assert any(c[1] == c[2] for c in R.NMS_CASES) and any(c[2] > c[1] for c in R.NMS_CASES) and all(c[2] & (c[2] - 1) == 0 for c in R.NMS_CASES)
    assert any(len(c[3]) == 3 and c[3][1] == 0 and c[3][0] > 0 and c[3][2] > 0 for c in R.NMS_CASES), "an empty image between two full ones"
    assert any(np.isnan(R.nms_case(c[0])[2]).any() for c in R.NMS_CASES), "NaN scores"
    # the Python-entry draw
    first, second = R.postprocess_ref(R.entry_draw(False), 2, 0.25, 0.5, False), R.postprocess_ref(R.entry_draw(True), 2, 0.25, 0.5, False)
    assert first[0] is not None and first[1] is not None and second[0] is not None and second[1] is None
    assert len(first[1]) < 64 and len(second[0]) < 64


# ---------------------------------------------------------------------------------------------------------------------------
# the mutants: each returns [(input, rejected)] over inputs of the GPU test, told apart by the comparison the GPU test makes
def _fold_mutant(kind, layout="small"):
    L = R.fold_layout(layout)
    flat, bstat = R.fold_draw(layout)
    wf, bias = R.fold_bn_ref(L, flat, bstat)
    mwf, mbias = R.fold_bn_ref(L, flat, bstat, mutant=kind)
    return [(layout, not (U.same_bits(mwf, wf) and U.same_bits(mbias, bias)))]


def _bn_images(M, C, act, res, **kw):
    d = R.bn_draw(M, C)
    sc, sh = R.bn_consts32(d["gamma"], d["beta"], d["mean"], d["var"], d["eps"])
    u, _ = R.fma32(d["z"], sc[None, :], sh[None, :])
    return R.bn_act_infer_ref(u, act, d["res"] if res else None), R.bn_act_infer_ref(u, act, d["res"] if res else None, **kw)


def _m_bn_trip():
    hit = []
    for M, C in R.BN_SHAPES:
        want, _ = _bn_images(M, C, 0, False)
        got = want.reshape(-1, 8).copy()
        got[R.bn_grid(M, C) * 256:] = U.SENT16                          # the items of the second trip keep what y held
        hit.append(((M, C), not U.same_bits(got.reshape(-1), want.reshape(-1))))
    return hit


def _m_res_first():
    return [((M, C, act), not U.same_bits(*_bn_images(M, C, act, True, res_first=True))) for M, C in R.BN_SHAPES[:3] for act in (2, 3)]


def _decode_mutant(**kw):
    hit = []
    for (H, W) in R.DECODE_MAPS:
        raw = R.decode_case(2, H, W, 28)
        a0 = R.DECODE_A0
        out, radii, scores = R.decode_eval_ref(raw, a0, H, W, 8.0)
        mut, _, _ = R.decode_eval_ref(raw, a0, H, W, 8.0, **kw)
        lv = slice(a0, a0 + H * W)
        er, br, es, bs = R.decode_errors(mut[:, lv], raw[:, lv], 8.0, radii, scores)
        ok = U.same_bits(U.bits32(mut[:, lv, :2]), U.bits32(out[:, lv, :2])) and er <= R.RADII_ULP and es <= R.SCORE_ULP and br == 0 and bs == 0
        hit.append(((H, W), not ok))
    return hit


def _prepare_mutant(**kw):
    hit = []
    ray = R.ray_factors()
    for C in R.PREP_C:
        for N in R.PREP_N:
            p = R.prepare_draw(N, C)
            a, b = R.post_prepare_ref(p, C, R.CONF_THRE, ray), R.post_prepare_ref(p, C, R.CONF_THRE, ray, **kw)
            hit.append(((N, C), not all(U.same_bits(U.bits32(x) if x.dtype == f32 else x, U.bits32(y) if y.dtype == f32 else y) for x, y in zip(a, b))))
    return hit


def _nms_mutant(images, thrs=(R.NMS_THRE,), agnostics=(0, 1), **kw):
    hit = []
    for name, (score, cls, rect) in images.items():
        for thr in thrs:
            for ag in agnostics:
                a, b = R.nms_want(score, cls, rect, thr, ag, 0x5A5A5A5A), R.nms_want(score, cls, rect, thr, ag, 0x5A5A5A5A, **kw)
                hit.append(((name, thr, ag), not (np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]))))
    return hit


def _nms_inputs():
    out = {"edges": R.edge_images()}
    for c in R.NMS_CASES:
        out[c[0]] = R.nms_case(c[0])[2:]
    return out


def _m_gather():
    pred, conf, cls, perm = R.gather_draw()
    return [(n, not U.same_bits(U.bits32(R.gather_ref(pred, conf, cls, perm[:n], swap=True)), U.bits32(R.gather_ref(pred, conf, cls, perm[:n])))) for n in R.GATHER_N[1:]]


MUTANTS = {
    "eps[0] for every segment": lambda: _fold_mutant("eps0"),
    "the packed rows are Cin apart, not Cin_pad": lambda: _fold_mutant("stride_cin"),
    "the output channel is computed from Cin_pad": lambda: _fold_mutant("co_cin_pad"),
    "the bias reads the variance for the mean": lambda: _fold_mutant("bias_var_for_mean"),
    "the fold drops its second grid-stride trip": lambda: _fold_mutant("one_trip", "big"),
    "bn_act_infer drops its second grid-stride trip": _m_bn_trip,
    "the residual is added before the activation": _m_res_first,
    "the decode swaps the x and y grid": lambda: _decode_mutant(swap_xy=True),
    "the sigmoid starts at column 27": lambda: _decode_mutant(sig_from=27),
    "the last maximum wins among equal class scores": lambda: _prepare_mutant(last_max=True),
    "> instead of >= at conf_thre": lambda: _prepare_mutant(strict=True),
    ">= instead of > at nms_thre": lambda: _nms_mutant({"edges": R.edge_images()}, thrs=(R.NMS_THRE, R.NMS_THRE_BELOW), ge=True),
    "a dead row still suppresses": lambda: _nms_mutant(_nms_inputs(), non_greedy=True),
    "ties are ordered by descending row": lambda: _nms_mutant(_nms_inputs(), tie_desc=True),
    "the class rule is dropped in class-aware mode": lambda: _nms_mutant(_nms_inputs(), agnostics=(0,), drop_class=True),
    "columns 27 and 28 of the gather are swapped": _m_gather,
}


def test_mutants_are_rejected():
    assert len(MUTANTS) >= 14
    print()
    failed = []
    for name, fn in MUTANTS.items():
        hit = fn()
        n = sum(1 for _, h in hit if h)
        print("INFER-REF mutant %-52s rejected by %3d of %3d inputs" % (name, n, len(hit)))
        if n == 0:
            failed.append(name)
    assert not failed, failed
    # what a particular input must do
    trip = _m_bn_trip()                                                 # a second trip exists from 257 items on
    assert all(h for k, h in trip if k[0] * (k[1] // 8) > 256) and not any(h for k, h in trip if k[0] * (k[1] // 8) <= 256)
    assert any(h for k, h in _decode_mutant(swap_xy=True) if k[0] != k[1]), "a non-square map must tell x from y"
    edges = dict(_nms_mutant({"edges": R.edge_images()}, thrs=(R.NMS_THRE, R.NMS_THRE_BELOW), ge=True))
    assert all(edges[("edges", R.NMS_THRE, ag)] for ag in (0, 1)), "IoU == nms_thre must tell > from >="
