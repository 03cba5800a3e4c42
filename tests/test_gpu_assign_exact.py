"""The SimOTA assignment kernels (csrc/assign.hip) and the loss reduction and gradient kernels (csrc/loss.hip) stage by stage against
tests/assign_reference.py, through the C ABI.

Bit for bit: ep24_dynamic_k (match, ks) on tied, dyadic, boundary and general draws, with every non-candidate slot of pw / cost
poisoned in a second copy; ep24_assign_resolve; pw of ep24_assign_cost_range against ep24_circle_pairwise on the same rows; the
exactly representable outputs of ep24_loss_finalize and the state it carries; the count column, the zero columns and the unmatched
rows of ep24_loss_terms / ep24_loss_grad; ep24_loss_grad_decode against ep24_loss_grad followed by ep24_head_decode_bwd.  Against
float64 under bounds derived in assign_reference's docstring: cost, the weights and losses of finalize, every other partial sum and
gradient element.  Mask bits of ep24_assign_candidates are compared for every (anchor, label) outside the reference's own margin.
tests/test_assign_reference.py shows without a GPU that the references agree with the oracle where it is defined, that float32
emulations stay inside the bounds and that thirteen planted mutants are rejected on these inputs.

Every buffer sits between two guards of 64 sentinel elements, whole buffers are compared, and a buffer a call must not write is
compared as well.  Every call is inside the ABI's documented preconditions; the two refused calls return their code before a launch.

Paths reached (tests/test_assign_reference.py asserts the inputs' side of it): dynamic_k_kernel<33> up to A = 8 448 and
dynamic_k_kernel<0> at 8 449 and 8 705; on images with labels P in {0, 1, 9, 10, 11, A}; k = 10, the floor at 1 (also with P = 0,
at every A: the cost loop ends at once), truncation at 3.0 and one fp32 step below 4.0; cost workgroups with 0, 1, 63, 64 candidates, one, two and thirteen batches of
256 pairs, a lens queue exactly full (64 candidates x 4 labels x 24 lens rays) and empty; C = 96 filling the class scratch; a block
with all 256 anchors matched; ncols = 128 and 256 (no column carry in the row writer) and 257 (drow = 0).

The float32 emulations of tests/test_assign_reference.py reach err / tol = 0.33 (finalize), 0.07 / 0.66 (pw / cost), 0.2 (partial
sums), 0.5 (gradient), 0.07 (angle sum).  Measured on an MI355X (the tests print FIN-ERR, COST-ERR, TERMS-ERR, GRAD-ERR before they
assert): 0.41 (finalize, nblocks = 2), 0.15 / 0.65 (pw / cost), 0.21 (partial sums, A = 257, C = 1), 0.56 (gradient, A = 256,
C = 230).  85 cases; wall time of the file on the device 8.1 s, the slowest case (dynamic_k at A = 8 447) 0.92 s.
"""
import os
import struct
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import assign_reference as R  # noqa: E402
import update_reference as UR  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F32 = np.float32


def _abi():
    from ep24._lib import call, lib, stream_ptr
    return call, stream_ptr, lib()


def G(n, kind, fill=None):
    return UR.Guarded(n, kind, DEV, fill)


def GF(a):
    """a float32 array as a guarded buffer"""
    a = np.ascontiguousarray(a, dtype=F32)
    return G(a.size, "f32", UR.bits32(a).reshape(-1))


def GB(bits):
    bits = np.ascontiguousarray(bits, dtype=np.uint32)
    return G(bits.size, "f32", bits.reshape(-1))


def G64(a):
    return G(a.size, "i64", R.u64(a).reshape(-1))


def GI(a):
    a = np.ascontiguousarray(a, dtype=np.int32)
    return G(a.size, "i32", a.reshape(-1))


def sync():
    torch.cuda.synchronize()


def unchanged(*bufs):
    for i, b in enumerate(bufs):
        b.check(b.host[UR.GUARD:UR.GUARD + b.n], "input %d" % i)


def window(buf, what):
    """the window's bit patterns; both guards must still hold the sentinel"""
    win, whole = buf.read()
    g = np.concatenate([whole[:UR.GUARD], whole[UR.GUARD + buf.n:]])
    assert bool(np.all(g == np.array(buf.sent).astype(g.dtype))), "%s: a guard element was written" % what
    return win


# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("A", R.DYNK_A)
def test_dynamic_k_exact(A):
    """28 launches of 4 images (num_gt 0, 1, 50, 7, rotated against the layouts so that each layout - no candidate at all and
    anchors 0 and A - 1 among them - meets an image with labels) per A, each a second time with NaN / +inf / -inf in every non-candidate slot of
    pw and cost: match and ks bit for bit, ks rows of g >= num_gt and of the image without labels untouched, no match bit of
    g >= num_gt (the expected words have none), inputs untouched."""
    call, sp, _ = _abi()
    B = 4
    for kind, gi, grp in R.dynk_groups():
        c = R.dynk_case(A, kind, gi)
        ng, ib, ic = GI(c["num_gt"]), G64(c["in_box"]), G64(c["in_ctr"])
        for poisoned in (False, True):
            if poisoned:
                pw = GB(np.stack([R.poison(c["pw"][b], c["cand"][b]) for b in range(B)]))
                cost = GB(np.stack([R.poison(c["cost"][b], c["cand"][b]) for b in range(B)]))
            else:
                pw, cost = GF(c["pw"]), GF(c["cost"])
            match, ks = G(B * A, "i64", np.zeros(B * A, dtype=np.int64)), G(B * R.G_MAX, "i32")
            call("dynamic_k", pw.ptr(), cost.ptr(), ng.ptr(), ib.ptr(), ic.ptr(), match.ptr(), ks.ptr(), B, A, sp())
            sync()
            what = "A=%d %s %s%s" % (A, kind, "/".join(grp), " poisoned" if poisoned else "")
            match.check(R.u64(c["match"]).reshape(-1), "match " + what)
            ks.check(c["ks"].astype(np.int32).reshape(-1), "ks " + what)
            unchanged(pw, cost, ng, ib, ic)


@pytest.mark.parametrize("A", R.RESOLVE_A)
def test_resolve_exact(A):
    call, sp, _ = _abi()
    c = R.resolve_case(A)
    B = 4
    match, pw, cost, ng = G64(c["match"]), GF(c["pw"]), GF(c["cost"]), GI(c["num_gt"])
    mg, mi = G(B * A, "i32"), G(B * A, "f32")
    call("assign_resolve", match.ptr(), pw.ptr(), cost.ptr(), ng.ptr(), mg.ptr(), mi.ptr(), B, A, sp())
    sync()
    mg.check(c["mg"].reshape(-1), "matched_gt")
    mi.check(UR.bits32(c["mi"]).reshape(-1), "matched_iou")
    unchanged(match, pw, cost, ng)


# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rays", R.COST_RAYS)
@pytest.mark.parametrize("C", R.COST_C)
def test_cost_range(C, rays):
    """4 images (num_gt 1, 4, 5, 50), workgroups with 64, 0, 1, 63, 64 and 37 candidates; the whole range through ep24_assign_cost
    and through ep24_assign_cost_range, then ranges that start off a multiple of 64, cut a workgroup, are empty or hold one anchor.
    pw equals ep24_circle_pairwise on the same rows bit for bit, pw and cost agree with float64 under the derived bound, and every
    entry of a non-candidate anchor, of g >= num_gt and outside the range keeps its sentinel."""
    call, sp, _ = _abi()
    c = R.cost_case(C, rays)
    B, A, ncols = 4, R.COST_A, 27 + C
    out, lab, ng, ib, ic = GF(c["outputs"]), GF(c["labels"]), GI(c["num_gt"]), G64(c["in_box"]), G64(c["in_ctr"])
    pair = np.full((B, R.G_MAX, A), R.SENT32, dtype=np.uint32)
    for b in range(B):
        n = int(c["num_gt"][b])
        gt, pd, o = GF(c["labels"][b, :n, 1:]), GF(c["outputs"][b, :, :26]), G(n * A, "f32")
        call("circle_pairwise", gt.ptr(), pd.ptr(), o.ptr(), n, A, sp())
        sync()
        pair[b, :n] = window(o, "pairwise").reshape(n, A)
        unchanged(gt, pd)
    worst_pw = worst_cost = 0.0
    for entry, (lo, hi) in [("assign_cost", (0, A))] + [("assign_cost_range", r) for r in R.COST_RANGES]:
        pw, cost = G(B * R.G_MAX * A, "f32"), G(B * R.G_MAX * A, "f32")
        args = [out.ptr(), ncols, lab.ptr(), ng.ptr(), ib.ptr(), ic.ptr(), pw.ptr(), cost.ptr(), B, A, C]
        call(entry, *(args + ([lo, hi] if entry == "assign_cost_range" else []) + [sp()]))
        sync()
        refs = [R.cost_ref(c["outputs"][b], c["labels"][b], c["in_box"][b], c["in_ctr"][b], c["num_gt"][b], lo, hi) for b in range(B)]
        w = np.stack([r["written"] for r in refs])
        assert int(w.sum()) == sum(int(n) for n in c["num_gt"]) * int(((c["cand"] >= lo) & (c["cand"] < hi)).sum())
        got_pw = pw.check(np.where(w, pair, np.uint32(R.SENT32)).reshape(-1), "pw [%d, %d)" % (lo, hi)).reshape(w.shape)
        assert not UR.is_nan32(pair[w]).any()
        assert bool(np.all(got_pw[~w] == np.uint32(R.SENT32))), "pw: an entry outside the written set was touched"
        got_cost = window(cost, "cost").reshape(w.shape)
        assert bool(np.all(got_cost[~w] == np.uint32(R.SENT32))), "cost: an entry outside the written set was touched"
        if w.any():
            st = lambda k: np.stack([r[k] for r in refs])[w]
            worst_pw = max(worst_pw, UR.err_ratio(UR.from_bits32(got_pw[w]), st("pw"), st("tol_pw")))
            worst_cost = max(worst_cost, UR.err_ratio(UR.from_bits32(got_cost[w]), st("cost"), st("tol_cost")))
    unchanged(out, lab, ng, ib, ic)
    print("COST-ERR C=%d %s: largest err / tol pw %.3f cost %.3f" % (C, rays, worst_pw, worst_cost))
    assert worst_pw <= 1.0 and worst_cost <= 1.0


def test_cost_refuses_97_classes_and_a_bad_range():
    _, sp, L = _abi()
    c = R.cost_case(96, "mixed")
    B, A = 4, R.COST_A
    out97 = G(B * A * (27 + 97), "f32", np.zeros(B * A * (27 + 97), dtype=np.uint32))
    out96 = GF(c["outputs"])
    lab, ng, ib, ic = GF(c["labels"]), GI(c["num_gt"]), G64(c["in_box"]), G64(c["in_ctr"])
    pw, cost = G(B * R.G_MAX * A, "f32"), G(B * R.G_MAX * A, "f32")
    fn = L.fn["ep24_assign_cost_range"]
    rc = fn(out97.ptr(), 27 + 97, lab.ptr(), ng.ptr(), ib.ptr(), ic.ptr(), pw.ptr(), cost.ptr(), B, A, 97, 0, A, sp())
    assert rc == R.E_UNSUPPORTED, (rc, L.last_error())
    rc = fn(out96.ptr(), 27 + 96, lab.ptr(), ng.ptr(), ib.ptr(), ic.ptr(), pw.ptr(), cost.ptr(), B, A, 96, 10, A + 1, sp())
    assert rc == R.E_ARG, (rc, L.last_error())
    sync()
    for buf in (pw, cost):
        buf.check(np.full(buf.n, R.SENT32, dtype=np.uint32), "nothing is written by a refused call")


# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("A", R.CAND_A)
def test_candidates_outside_the_margin(A):
    """labels from synth.make_labels(size=256): 50 convex, 50 star, 1, 0, and 50 with a zero row in the middle (the count is 49 and
    the first 49 rows are used).  num_gt exact; every mask bit of a pair outside the reference's margin; no bit of g >= num_gt."""
    from ep24 import synth
    call, sp, _ = _abi()
    for kind, n, seed in R.CAND_SETS:
        labels, xs, ys, st = R.candidate_inputs(synth, A, kind, n, seed)
        ref = R.candidates_ref(labels, xs, ys, st)
        want_b, want_c, dec_b, dec_c = R.candidates_expected(ref)
        assert ref["num_gt"] == (49 if kind == "hole" else n)
        lab, gx, gy, gs = GF(labels), GF(xs), GF(ys), GF(st)
        ng, ib, ic = G(1, "i32"), G(A, "i64"), G(A, "i64")
        call("assign_candidates", lab.ptr(), gx.ptr(), gy.ptr(), gs.ptr(), ng.ptr(), ib.ptr(), ic.ptr(), 1, A, sp())
        sync()
        ng.check([ref["num_gt"]], "num_gt")
        for got, want, dec, what in ((window(ib, "in_box"), want_b, dec_b, "in_box"), (window(ic, "in_ctr"), want_c, dec_c, "in_ctr")):
            got = got.view(np.uint64)
            assert int((got >> np.uint64(ref["num_gt"])).max()) == 0, what + ": a bit of g >= num_gt"
            for g in range(ref["num_gt"]):
                bad = (((got >> np.uint64(g)) & np.uint64(1)) != ((want >> np.uint64(g)) & np.uint64(1))) & dec[g]
                assert not bad.any(), (what, kind, g, np.flatnonzero(bad)[:5])
        unchanged(lab, gx, gy, gs)


# ---------------------------------------------------------------------------------------------------------------------------
def _finalize(partials, num_gt, state):
    call, sp, _ = _abi()
    p, ng, res = GF(partials), GI(num_gt), G(64, "f32")
    call("loss_finalize", p.ptr(), partials.shape[0], ng.ptr(), len(num_gt), state.ptr(), res.ptr(), sp())
    sync()
    unchanged(p, ng)
    return window(res, "result"), window(state, "state")


@pytest.mark.parametrize("nb", R.FIN_NBLOCKS)
def test_finalize(nb):
    """Integer partials whose count column sums to 1, 64, 256 and 0: the exactly representable outputs and the new state bit for
    bit, the weights and weighted losses under the bound; three calls in a row on one state buffer (ones; the first call's state;
    a state with a zero entry, where the ratio clamps to 2); then a general draw entirely under the bound."""
    num_gt = [3, 0, 50]
    worst = 0.0
    for count in R.FIN_COUNTS:
        state = GF(np.ones(26, dtype=F32))
        st = np.ones(26, dtype=F32)
        for step in range(3):
            p = R.finalize_partials(nb, count, seed=step)
            if step == 1:
                p[:, 3] = 0                                                        # l[3] = 0: the next call divides by 0 + 1e-8
            res, l, tol, _ = R.finalize_ref(p, num_gt, st)
            got, got_state = _finalize(p, num_gt, state)
            assert bool(np.all(got[57:] == np.uint32(R.SENT32))), "result[57..63] was written"
            for i in R.FIN_EXACT:
                assert got[i] == UR.bits32(F32(res[i])), (nb, count, step, i, float(UR.from_bits32(got[i:i + 1])[0]), res[i])
            assert res[27] == max(count, 1) and res[28] == 53
            UR.assert_same(got_state, UR.bits32(l.astype(F32)), "state")
            if step == 2:
                assert st[3] == 0 and l[3] / 1e-8 > 2                              # the ratio of column 3 clamps to 2
            w = R.FIN_WRITTEN
            worst = max(worst, R.check_bound(got[w], res[w], np.maximum(tol[w], 1e-300), "result"))
            st = l.astype(F32)
    p = R.finalize_general(nb, 2)
    st = np.linspace(0.2, 3.0, 26).astype(F32)
    res, l, tol, tol_l = R.finalize_ref(p, num_gt, st)
    got, got_state = _finalize(p, num_gt, GF(st))
    w = R.FIN_WRITTEN
    worst = max(worst, R.check_bound(got[w], res[w], np.maximum(tol[w], 1e-300), "result"), R.check_bound(got_state, l, tol_l, "state"))
    assert bool(np.all(got[57:] == np.uint32(R.SENT32)))
    print("FIN-ERR nblocks=%d: largest err / tol %.3f" % (nb, worst))
    assert worst <= 1.0


# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", R.LOSS_C)
@pytest.mark.parametrize("A", R.LOSS_A)
def test_terms_and_grad(A, C):
    """4 images whose 256-anchor blocks are matched entirely, in lanes 0 and 63 of each wave, once, not at all, or by a random 1 %,
    with and without the L1 branch; grad_scale null and a device scalar 0.5.  Exact: the count column, columns 28 .. 31, the iou /
    cls / l1 columns of a block without a match, every element of an unmatched row of dout (+0 but column 26) and of d_origin,
    the sign pattern of d_origin; everything else under the derived bounds.  All of dout / d_origin / partials is written, nothing
    outside (guards; A = 257 and 513 end inside a block)."""
    call, sp, _ = _abi()
    B, ncols = 4, 27 + C
    nblk = (A + 255) // 256
    res = R.loss_result()
    worst_t = worst_g = 0.0
    for shift, scale in ((0, None), (1, 0.5)):
        c = R.loss_case(A, C, shift)
        pv, pe = R.terms_ref(c, True)
        dv, de, ov, oe = R.grad_ref(c, res, None, True)
        f = 1.0 if scale is None else scale                                        # a power of two scales values and bounds exactly
        out, lab, mg, mi = GF(c["outputs"]), GF(c["labels"]), GI(c["matched_gt"]), GF(c["matched_iou"])
        org, xs, ys, st, rs = GF(c["origin"]), GF(c["xs"]), GF(c["ys"]), GF(c["strides"]), GF(res)
        gsc = None if scale is None else GF(np.array([scale], dtype=F32))
        unmatched = np.repeat((c["matched_gt"] < 0)[:, :, None], ncols, 2)
        unmatched[:, :, 26] = False
        for l1 in (False, True):
            part = G(B * nblk * R.NS, "f32")
            l1_args = [org.ptr(), xs.ptr(), ys.ptr(), st.ptr()] if l1 else [None, None, None, None]
            call("loss_terms", out.ptr(), ncols, lab.ptr(), mg.ptr(), mi.ptr(), part.ptr(), B, A, C, *(l1_args + [sp()]))
            sync()
            want_v, want_e = pv.copy(), pe.copy()
            if not l1:
                want_v[:, 27] = want_e[:, 27] = 0
            got = window(part, "partials").reshape(B * nblk, R.NS)
            assert bool(np.all(got[:, 28:] == 0)) and np.array_equal(UR.from_bits32(got[:, 26]), want_v[:, 26].astype(F32))
            empty = want_v[:, 26] == 0
            assert bool(np.all(got[empty][:, list(range(24)) + [25, 27]] == 0))
            worst_t = max(worst_t, R.check_bound(got, want_v, want_e, "partials"))
            dout = G(B * A * ncols, "f32")
            dorg = G(B * A * 26, "f32") if l1 else None
            call("loss_grad", out.ptr(), ncols, lab.ptr(), mg.ptr(), mi.ptr(), rs.ptr(), None if gsc is None else gsc.ptr(), dout.ptr(),
                 B, A, C, *(l1_args + [dorg.ptr() if l1 else None, sp()]))
            sync()
            got = window(dout, "dout").reshape(B, A, ncols)
            assert bool(np.all(got[unmatched] == 0)), "an element of an unmatched row is not +0"
            assert not bool(np.any(got == np.uint32(R.SENT32))), "an element of dout was not written"
            worst_g = max(worst_g, R.check_bound(got, dv * f, de * f, "dout"))
            if l1:
                got = window(dorg, "d_origin").reshape(B, A, 26)
                assert bool(np.all(got[c["matched_gt"] < 0] == 0)), "d_origin of an unmatched row is not +0"
                sign = np.sign(ov)
                gv = UR.from_bits32(got)
                assert np.array_equal(np.sign(gv), sign.astype(F32)), "sign pattern of d_origin"
                worst_g = max(worst_g, R.check_bound(got, ov * f, oe * f, "d_origin"))
        unchanged(out, lab, mg, mi, org, xs, ys, st, rs)
    print("TERMS-ERR A=%d C=%d: largest err / tol %.3f   GRAD-ERR %.3f" % (A, C, worst_t, worst_g))
    assert worst_t <= 1.0 and worst_g <= 1.0


DECODE_LEVELS = [[(19, 19, 8.0)], [(19, 19, 8.0), (9, 11, 16.0)], [(19, 19, 8.0), (9, 11, 16.0), (5, 5, 32.0)]]


@pytest.mark.parametrize("nlev", [1, 2, 3])
@pytest.mark.parametrize("C", [1, 3, 8, 80])
def test_grad_decode_equals_the_two_launch_form(C, nlev):
    """ep24_loss_grad_decode against ep24_loss_grad followed by ep24_head_decode_bwd of every level, whole bf16 buffers bit for bit
    (ld_cls = 8, 8, 8, 80; levels of 361, 99 and 25 cells: no multiple of 256, the second and third start inside a block).  Block 0
    of image 0 has all 256 anchors matched."""
    call, sp, _ = _abi()
    levels = DECODE_LEVELS[nlev - 1]
    B, ncols, ld = 4, 27 + C, (C + 7) // 8 * 8
    A = sum(h * w for h, w, _ in levels)
    c = R.loss_case(A, C, 0, seed=nlev)
    assert c["patterns"][(0, 0)] == "all"
    out, lab, mg, mi, rs = GF(c["outputs"]), GF(c["labels"]), GI(c["matched_gt"]), GF(c["matched_iou"]), GF(R.loss_result())
    dout = G(B * A * ncols, "f32")
    call("loss_grad", out.ptr(), ncols, lab.ptr(), mg.ptr(), mi.ptr(), rs.ptr(), None, dout.ptr(), B, A, C, None, None, None, None, None, sp())
    want, got, rows = [], [], []
    a0 = 0
    for h, w, s in levels:
        ro, cl = G(B * h * w * 32, "bf16"), G(B * h * w * ld, "bf16")
        call("head_decode_bwd", dout.ptr(), out.ptr(), ro.ptr(), cl.ptr(), B, A, a0, h, w, s, ncols, None, sp())
        want.append((ro, cl))
        ro, cl = G(B * h * w * 32, "bf16"), G(B * h * w * ld, "bf16")
        assert ro.ptr() % 16 == 0 and cl.ptr() % 16 == 0
        got.append((ro, cl))
        rows.append([h * w, struct.unpack("<I", struct.pack("<f", s))[0], ro.ptr(), cl.ptr()])
        a0 += h * w
    table = torch.tensor(rows, dtype=torch.int64)
    call("loss_grad_decode", out.ptr(), ncols, lab.ptr(), mg.ptr(), mi.ptr(), rs.ptr(), B, A, C, nlev, table.data_ptr(), sp())
    sync()
    for k, ((w_ro, w_cl), (g_ro, g_cl)) in enumerate(zip(want, got)):
        ro_w, cl_w = window(w_ro, "two-launch reg+obj"), window(w_cl, "two-launch classes")      # guards against the sentinel itself
        assert not bool(np.any(ro_w == np.uint16(UR.SENT16))) and not bool(np.any(cl_w == np.uint16(UR.SENT16)))
        UR.assert_same(window(g_ro, "fused reg+obj rows of level %d" % k), ro_w, "reg+obj rows of level %d" % k)
        UR.assert_same(window(g_cl, "fused class rows of level %d" % k), cl_w, "class rows of level %d" % k)
    assert any(float(np.abs(UR.from_bits32(UR.bf16_widen(w_ro.read()[0]))).max()) > 0 for w_ro, _ in want)
    unchanged(out, lab, mg, mi, rs)
