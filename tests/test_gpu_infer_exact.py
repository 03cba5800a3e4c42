"""The inference kernels of csrc/infer.hip - ep24_bn_act_infer, ep24_fold_bn, ep24_head_decode_eval, ep24_post_prepare, ep24_post_nms
(with nms_compact_sort of csrc/nms_sort.h), ep24_post_gather - against tests/infer_reference.py, through the C ABI.
tests/test_infer_reference.py shows without a GPU that the references equal torch's batch_norm / conv2d and the oracle's eval head and
postprocess, that every input reaches what it claims, and that sixteen mutants are rejected on these inputs.

Every buffer sits between two guards of 64 sentinel elements and whole buffers are compared: the pad columns of strided rows, the
Cin_pad - Cin columns and the gaps of the folded weights, the rows of `out` outside the decoded map, keep beyond keep_count, and every
input a call must not write.  NaN equals NaN; every other pattern only itself.

Bit for bit against the float32 emulation (separate IEEE operations, the one fmaf of bn_act_infer rounded once): bn_act_infer with
act 0, 2, 3, both outputs of fold_bn (division and square root are correctly rounded in the default build, and the device agrees),
columns 0 and 1 of the decode, all four outputs of post_prepare, keep / keep_count of post_nms, the gathered rows.  Under a bound:
bn_act_infer's SiLU (bn_reference.tol_y with S_SILU = 2^-18, the float64 form evaluated from the emulated scale / shift), the
decode's radii (2 ulp of s exp(t); s is a power of two) and scores (3 ulp of 1 / (1 + exp(-t)): 2 ulp of expf scaled by
e / (1 + e) <= 1, half an ulp each for the addition and the division), with 0, 1, NaN and inf required exactly where the float64
value is one of them or lies beyond the fp32 range.  Where exp(t) is a denormal fp32 number (the planted -88.8 and -100) an ulp is
2^-149 and the radii's unit is s times that: expf's own spacing carried through the exact product.

The sizes come from the constants of csrc/infer.hip:
  bn_act_infer   2048 workgroups x 512 items: (2049, 4096) = 1 049 088 items; every shape above 256 items makes a second trip
  fold_bn        8192 workgroups x 1024 elements: 8 389 244 elements, the 636 of the second trip in three segments
  decode         4096 x 256 elements: 99 x 100 x 107 = 1 059 300
  post_prepare   4096 x 256 rows: 1 048 876 rows, C = 1
  post_nms       1024 lanes: 1023 / 1024 / 1025 / 2049 candidates; the bitonic pad 1025 -> 2048, 2049 -> 4096
  post_gather    1024 x 256 elements: 9040 rows x 29

Found by these cases and fixed in csrc/infer.hip: bn_act_infer's ReLU turned a NaN into 0 (fmaxf), now ATen's relu; the decode's
sigmoid gave 0 below t = -88.72, where expf(-t) overflows and the answer is a denormal number, now expf(t) there (every other t
keeps its bits).  New host guards: bn_act_infer refuses C > 8192 (64 KiB of LDS), fold_bn refuses total_channels <= 0.

75 cases; on an MI355X the file takes 5.2 s, its slowest case 2.0 s (bn_act_infer at 2049 x 4096: eight launches and the fmaf of
8.4 M elements on the host); post_prepare beyond its cap 0.4 s, fold_bn beyond its cap 0.2 s.  Largest figures, printed as INFER-ERR
before each assertion and measured against the float64 references:
  decode radii      0.776 of 2 ulp    (99 x 100 map; 0.68 - 0.77 on the small maps, strides 8, 16, 32)
  decode sigmoid    1.798 of 3 ulp
  SiLU err / bound  0.996 of 1        (0.593 at 1 x 8; the figure is a bf16 rounding decision next to a tie, as in test_gpu_bn_exact.py)
The device kept expf's denormal results (t = -88.8, -100): nothing is flushed to zero.
"""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import infer_reference as R  # noqa: E402
import update_reference as U  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
E_ARG = -1
I32_SENT = 0x5A5A5A5A


def _abi():
    from ep24._lib import call, lib, stream_ptr
    return call, stream_ptr, lib()


def G(n, kind, fill=None):
    return U.Guarded(n, kind, DEV, fill)


def sync():
    torch.cuda.synchronize()


def unchanged(buf, what):
    """an input buffer and its guards are as they were uploaded"""
    buf.check(buf.host[U.GUARD:U.GUARD + buf.n], what)


def report(what, **figures):
    print("INFER-ERR %s: %s" % (what, ", ".join("%s %.3f" % kv for kv in figures.items())))


# ---------------------------------------------------------------------------------------------------------------------------
BN_ALL = [(s, lay) for s in R.BN_SHAPES + [R.BN_CAP] for lay in R.BN_LAYOUTS]


@pytest.mark.parametrize("shape,layout", BN_ALL, ids=["%dx%d-%s" % (s + (lay,)) for s, lay in BN_ALL])
def test_bn_act_infer(shape, layout):
    """act 0 .. 3, with and without a residual, on one draw: negative gamma, running_var = 0, a NaN and both infinities in z.  y starts
    as the sentinel, so an item the grid-stride loop skipped shows."""
    call, sp, _ = _abi()
    M, C = shape
    d, sc, sh, u = R.bn_case(M, C)
    ld_z, ld_y, ld_r = (C + x for x in R.BN_LAYOUTS[layout])
    z = G(M * ld_z, "bf16", R.strided(R.b16(d["z"]).reshape(M, C), ld_z, C))
    res = G(M * ld_r, "bf16", R.strided(R.b16(d["res"]).reshape(M, C), ld_r, C))
    vec = {k: G(C, "f32", U.bits32(d[k])) for k in ("gamma", "beta", "mean", "var")}
    for with_res in (False, True):
        r = d["res"] if with_res else None
        for act in (0, 1, 2, 3):
            y = G(M * ld_y, "bf16")
            call("bn_act_infer", z.ptr(), ld_z, vec["gamma"].ptr(), vec["beta"].ptr(), vec["mean"].ptr(), vec["var"].ptr(), y.ptr(), ld_y,
                 res.ptr() if with_res else None, ld_r, M, C, d["eps"], act, sp())
            sync()
            what = "y, act %d, residual %d" % (act, with_res)
            if act != 1:
                y.check(R.strided(R.bn_act_infer_ref(u, act, r), ld_y, C), what)
                continue
            got_bits = y.read()[0].reshape(M, ld_y)[:, :C]
            got = U.from_bits32(U.bf16_widen(got_bits.reshape(-1))).astype(np.float64).reshape(M, C)
            _, a64, y64 = R.bn_act_infer_ref64(d["z"], sc, sh, 1, r)
            fin = np.isfinite(y64)
            assert np.array_equal(np.isnan(got), np.isnan(y64)) and np.array_equal(got[~fin & ~np.isnan(y64)], y64[~fin & ~np.isnan(y64)]), what
            tol = R.bn_tol(d["z"], sc, sh, d["mean"], d["beta"], a64, y64, 1)
            ratio = float((np.abs(got[fin] - y64[fin]) / tol[fin]).max())
            report("bn_act_infer SiLU %dx%d %s residual %d" % (M, C, layout, with_res), err_over_bound=ratio)
            assert ratio <= 1.0, ratio
            y.check(R.strided(got_bits, ld_y, C), what + " (pad columns, guards)")
    for k, b in list(vec.items()) + [("z", z), ("residual", res)]:
        unchanged(b, k)


def test_bn_act_infer_refusals():
    """EP24_E_ARG before any launch: C = 12, odd strides, M = 0, and C = 8200 (2 C floats of LDS would pass 64 KiB)"""
    _, sp, lib = _abi()
    fn = lib.fn["ep24_bn_act_infer"]
    big = 8200
    z, y, res = G(2 * big, "bf16"), G(2 * big, "bf16"), G(2 * big, "bf16")
    v = [G(big, "f32", np.zeros(big, dtype=np.uint32)) for _ in range(4)]
    good = dict(ld_z=16, ld_y=16, res=res.ptr(), ld_res=16, M=2, C=8)
    for bad in (dict(C=12), dict(ld_z=12), dict(ld_y=20), dict(ld_res=12), dict(M=0), dict(C=0), dict(C=big, ld_z=big, ld_y=big, ld_res=big), dict(C=big, res=None, ld_z=big, ld_y=big)):
        a = dict(good, **bad)
        rc = fn(z.ptr(), a["ld_z"], v[0].ptr(), v[1].ptr(), v[2].ptr(), v[3].ptr(), y.ptr(), a["ld_y"], a["res"], a["ld_res"], a["M"], a["C"], 1e-3, 1, sp())
        assert rc == E_ARG, bad
    assert "8192" in lib.last_error()
    assert fn(None, 16, v[0].ptr(), v[1].ptr(), v[2].ptr(), v[3].ptr(), y.ptr(), 16, None, 16, 2, 8, 1e-3, 1, sp()) == E_ARG
    sync()
    for b in (z, y, res):
        unchanged(b, "a refused call wrote")


# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["small", "one", "big"])
def test_fold_bn(name):
    """Packed weights and bias bit for bit; the pad columns, the gaps between segments and the guards keep the sentinel."""
    call, sp, _ = _abi()
    L = R.fold_layout(name)
    fl, bs = R.fold_draw(name)
    flat, bstat = G(L.flat_n, "f32", U.bits32(fl)), G(L.bstat_n, "f32", U.bits32(bs))
    desc, prefix, cprefix = G(L.desc.size, "i64", L.desc.reshape(-1)), G(L.n_seg + 1, "i64", L.prefix), G(L.n_seg + 1, "i64", L.cprefix)
    eps = G(L.n_seg, "f32", U.bits32(L.eps))
    wf, bias = G(L.wf_n, "bf16"), G(L.bias_n, "f32")
    call("fold_bn", flat.ptr(), bstat.ptr(), desc.ptr(), prefix.ptr(), cprefix.ptr(), eps.ptr(), L.n_seg, L.total, L.total_channels, wf.ptr(), bias.ptr(), sp())
    sync()
    want_wf, want_bias = R.fold_bn_ref(L, fl, bs)
    wf.check(want_wf, "folded weights (%s)" % name)
    bias.check(want_bias, "bias (%s)" % name)
    for k, b in dict(flat=flat, bstat=bstat, desc=desc, prefix=prefix, cprefix=cprefix, eps=eps).items():
        unchanged(b, k)


def test_fold_bn_refusals():
    _, sp, lib = _abi()
    L = R.fold_layout("one")
    fl, bs = R.fold_draw("one")
    flat, bstat = G(L.flat_n, "f32", U.bits32(fl)), G(L.bstat_n, "f32", U.bits32(bs))
    desc, prefix, cprefix = G(L.desc.size, "i64", L.desc.reshape(-1)), G(2, "i64", L.prefix), G(2, "i64", L.cprefix)
    eps, wf, bias = G(1, "f32", U.bits32(L.eps)), G(L.wf_n, "bf16"), G(L.bias_n, "f32")
    good = [flat.ptr(), bstat.ptr(), desc.ptr(), prefix.ptr(), cprefix.ptr(), eps.ptr(), 1, L.total, L.total_channels, wf.ptr(), bias.ptr(), sp()]
    for at, val in ((8, 0), (8, -1), (7, 0), (6, 0), (0, None), (9, None), (10, None)):
        a = list(good)
        a[at] = val
        assert lib.fn["ep24_fold_bn"](*a) == E_ARG, (at, val)
    sync()
    unchanged(wf, "a refused call wrote the weights")
    unchanged(bias, "a refused call wrote the bias")


# ---------------------------------------------------------------------------------------------------------------------------
def _decode(B, H, W, ncols, strides):
    call, sp, _ = _abi()
    a0 = R.DECODE_A0
    raw = R.decode_case(B, H, W, ncols)
    A = raw.shape[1]
    lv = slice(a0, a0 + H * W)
    wr = ws = 0.0
    for s in strides:
        out = G(raw.size, "f32", U.bits32(raw).reshape(-1))
        call("head_decode_eval", out.ptr(), B, A, a0, H, W, s, ncols, sp())
        sync()
        want, radii, scores = R.decode_eval_ref(raw, a0, H, W, s)
        got = U.from_bits32(out.read()[0]).reshape(B, A, ncols)
        er, br, es, bs = R.decode_errors(got[:, lv], raw[:, lv], s, radii, scores)
        wr, ws = max(wr, er), max(ws, es)
        report("decode %dx%d ncols %d stride %g" % (H, W, ncols, s), radii_ulp=er, sigmoid_ulp=es)
        assert br == 0 and bs == 0, "%d radii, %d scores that must be exactly 0, 1, NaN or inf are not" % (br, bs)
        assert er <= R.RADII_ULP and es <= R.SCORE_ULP, (er, es)
        want[:, lv, 2:] = got[:, lv, 2:]                                 # compared above; columns 0, 1 and every other row bit for bit
        out.check(U.bits32(want).reshape(-1), "out, stride %g" % s)
    return wr, ws


@pytest.mark.parametrize("ncols", R.DECODE_NCOLS)
@pytest.mark.parametrize("H,W", R.DECODE_MAPS)
def test_head_decode_eval(H, W, ncols):
    _decode(2, H, W, ncols, R.DECODE_STRIDES)


def test_head_decode_eval_beyond_the_grid_cap():
    B, H, W, ncols = R.DECODE_CAP
    assert B * H * W * ncols > R.DECODE_MAX_ITEMS
    _decode(B, H, W, ncols, [16.0])


# ---------------------------------------------------------------------------------------------------------------------------
def _prepare(N, C, conf_thre):
    call, sp, _ = _abi()
    p = R.prepare_draw(N, C)
    ray = R.ray_factors()
    pred, rays = G(p.size, "f32", U.bits32(p).reshape(-1)), G(48, "f32", U.bits32(ray))
    score, conf, cls, rect = G(N, "f32"), G(N, "f32"), G(N, "i32"), G(4 * N, "f32")
    call("post_prepare", pred.ptr(), 27 + C, C, N, conf_thre, rays.ptr(), score.ptr(), conf.ptr(), cls.ptr(), rect.ptr(), sp())
    sync()
    ws, wc, wk, wr = R.post_prepare_ref(p, C, conf_thre, ray)
    score.check(U.bits32(ws), "score")
    conf.check(U.bits32(wc), "class_conf")
    cls.check(wk, "class_pred")
    rect.check(U.bits32(wr).reshape(-1), "rectangle")
    unchanged(pred, "pred")
    unchanged(rays, "ray factors")


@pytest.mark.parametrize("conf_thre", [R.CONF_THRE, 0.0])
@pytest.mark.parametrize("N", R.PREP_N)
@pytest.mark.parametrize("C", R.PREP_C)
def test_post_prepare(C, N, conf_thre):
    """First maximum, >= at conf_thre (equal in bits and one ulp below), NaN class scores (a leading NaN stays, any other is passed
    over), NaN objectness, negative and zero radii: all four outputs bit for bit."""
    _prepare(N, C, conf_thre)


def test_post_prepare_beyond_the_grid_cap():
    N, C = R.PREP_CAP
    assert N > R.PREP_MAX_ROWS
    _prepare(N, C, R.CONF_THRE)


def test_post_prepare_refusals():
    _, sp, lib = _abi()
    pred, rays = G(4 * 29, "f32"), G(48, "f32")
    outs = [G(4, "f32"), G(4, "f32"), G(4, "i32"), G(16, "f32")]
    good = [pred.ptr(), 29, 2, 4, 0.25, rays.ptr()] + [o.ptr() for o in outs] + [sp()]
    for at, val in ((1, 28), (1, 30), (2, 0), (3, 0), (0, None), (5, None), (6, None), (9, None)):
        a = list(good)
        a[at] = val
        assert lib.fn["ep24_post_prepare"](*a) == E_ARG, (at, val)
    sync()
    for o in outs:
        unchanged(o, "a refused call wrote")


# ---------------------------------------------------------------------------------------------------------------------------
def _nms(score, cls, rect, A, P, thr, agnostic, what):
    """Scratch full of garbage (dead = 0xFF, random keys, idx = -1), keep / keep_count full of sentinels."""
    call, sp, _ = _abi()
    B = score.shape[0]
    sc, cl, rc = G(B * A, "f32", U.bits32(score).reshape(-1)), G(B * A, "i32", cls.reshape(-1)), G(B * A * 4, "f32", U.bits32(rect).reshape(-1))
    skey, sidx, dead = G(B * P, "f32", U.random_bits(B * P, 3)), G(B * P, "i32", np.full(B * P, -1, dtype=np.int32)), G(B * P, "u8", np.full(B * P, 0xFF, dtype=np.uint8))
    keep, count = G(B * A, "i32"), G(B, "i32")
    call("post_nms", sc.ptr(), cl.ptr(), rc.ptr(), B, A, thr, agnostic, skey.ptr(), sidx.ptr(), dead.ptr(), keep.ptr(), count.ptr(), P, sp())
    sync()
    wk, wc = R.nms_want(score, cls, rect, thr, agnostic, I32_SENT)
    count.check(wc, "keep_count, " + what)
    keep.check(wk.reshape(-1), "keep (the sentinel beyond keep_count), " + what)
    for k, b in dict(score=sc, cls=cl, rect=rc).items():
        unchanged(b, k)
    for b in (skey, sidx, dead):
        b.check(b.read()[0], "scratch guards")
    return wc


@pytest.mark.parametrize("agnostic", [0, 1])
@pytest.mark.parametrize("name", [c[0] for c in R.NMS_CASES])
def test_post_nms(name, agnostic):
    A, P, score, cls, rect = R.nms_case(name)
    _nms(score, cls, rect, A, P, R.NMS_THRE, agnostic, name)


@pytest.mark.parametrize("agnostic", [0, 1])
@pytest.mark.parametrize("thr", [R.NMS_THRE, R.NMS_THRE_BELOW], ids=["at-0.5", "one-ulp-below"])
def test_post_nms_edges(thr, agnostic):
    """IoU == nms_thre keeps both and one ulp less suppresses; 0 / 0 keeps both; a row killed by a dead row survives; same box, two
    classes; -0.0 is a candidate"""
    score, cls, rect = R.edge_images()
    wc = _nms(score, cls, rect, 3, 4, thr, agnostic, "edges")
    assert list(wc) == [2 if thr == R.NMS_THRE else 1, 2, 2, 2 if agnostic else 3]


def test_post_nms_refusals():
    _, sp, lib = _abi()
    A = 7
    sc, cl, rc = G(A, "f32"), G(A, "i32"), G(4 * A, "f32")
    skey, sidx, dead, keep, count = G(8, "f32"), G(8, "i32"), G(8, "u8"), G(A, "i32"), G(1, "i32")
    good = [sc.ptr(), cl.ptr(), rc.ptr(), 1, A, 0.5, 0, skey.ptr(), sidx.ptr(), dead.ptr(), keep.ptr(), count.ptr(), 8, sp()]
    for at, val in ((12, 4), (12, 12), (12, 7), (12, 0), (3, 0), (4, 0), (0, None), (10, None), (11, None)):
        a = list(good)
        a[at] = val
        assert lib.fn["ep24_post_nms"](*a) == E_ARG, (at, val)
    sync()
    for b in (skey, sidx, dead, keep, count):
        unchanged(b, "a refused call wrote")


# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", R.GATHER_N)
def test_post_gather(n):
    """keep is the front of a permutation (not sorted); det holds two rows more than n: they, and the guards, keep the sentinel"""
    call, sp, _ = _abi()
    p, conf, cls, perm = R.gather_draw()
    A, ncols = p.shape
    pred, cf, cl = G(p.size, "f32", U.bits32(p).reshape(-1)), G(A, "f32", U.bits32(conf)), G(A, "i32", cls)
    kp = np.full(A, I32_SENT, dtype=np.int32)
    kp[:n] = perm[:n]
    keep, det = G(A, "i32", kp), G((n + 2) * 29, "f32")
    call("post_gather", pred.ptr(), ncols, cf.ptr(), cl.ptr(), keep.ptr(), n, det.ptr(), sp())
    sync()
    want = np.full((n + 2) * 29, U.SENT32, dtype=np.uint32)
    want[:n * 29] = U.bits32(R.gather_ref(p, conf, cls, perm[:n])).reshape(-1)
    got = det.check(want, "det")
    if n:
        assert np.array_equal(got[:n * 29].reshape(n, 29)[:, :27], U.bits32(p[perm[:n], :27]).reshape(n, 27)), "a pattern changed on its way"
    for k, b in dict(pred=pred, conf=cf, cls=cl, keep=keep).items():
        unchanged(b, k)


# ---------------------------------------------------------------------------------------------------------------------------
def test_postprocess_entry_reuses_its_scratch():
    """Two calls of ep24.infer.postprocess with the same (B, A): the second one's image 1 has nothing above the threshold.  Nothing
    of the first call may survive in count, keep or dead: [det, None], equal to the stage-level reference."""
    from ep24 import infer
    ws = None
    for second in (False, True):
        p = R.entry_draw(second)
        got = infer.postprocess(torch.from_numpy(p).to(DEV), 2, conf_thre=0.25, nms_thre=0.5)
        want = R.postprocess_ref(p, 2, 0.25, 0.5, False)
        assert [g is None for g in got] == [w is None for w in want] == [False, second]
        for g, w in zip(got, want):
            if w is not None:
                assert tuple(g.shape) == w.shape
                U.assert_same(U.bits32(g.cpu().numpy()).reshape(-1), U.bits32(w).reshape(-1), "detections, call %d" % (1 + second))
        assert ws is None or infer._scratch[(2, 64, DEV)] is ws, "the second call must run on the first call's scratch"
        ws = infer._scratch[(2, 64, DEV)]
