"""tests/assign_reference.py without a GPU: (a) on tie-free draws its selection and conflict rule equal oracle.assign.dynamic_k (which
keeps torch.topk and therefore cannot be asked about ties), its cost equals oracle.assign.assign_image, its weights equal
oracle.loss.LossOracle's; (b) every dyadic case tests/test_gpu_assign_exact.py runs is exact; (c) float32 emulations written with other
sum orders stay inside the derived bounds (the largest err / tol is printed: not too tight); (d) each planted mutant is rejected by at
least one of the GPU file's inputs (not too loose)."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import assign_reference as R  # noqa: E402
import update_reference as UR  # noqa: E402

F32 = np.float32


def test_helper_never_imports_the_package():
    src = open(R.__file__.replace(".pyc", ".py")).read()
    assert "import ep24" not in src and "from ep24" not in src


# ------------------------------------------------------------------------------------------------------------- (a)
@pytest.mark.parametrize("seed", [0, 1, 2])
def test_selection_equals_the_oracle_without_ties(seed):
    """oracle.assign.dynamic_k works on the gathered [G, P] matrices; tie-free general draws make torch.topk's order irrelevant"""
    from oracle.assign import dynamic_k
    rng = np.random.default_rng(seed)
    A, G = 700, [3, 17, 50][seed]
    cand = np.sort(rng.choice(A, 150, replace=False))
    in_box, in_ctr = R.cand_masks(cand, A, rng)
    pw = rng.random((R.G_MAX, A)).astype(F32)
    cost = (rng.standard_normal((R.G_MAX, A)) * 0.3).astype(F32)                   # close costs: conflicts between labels occur
    for g in range(G):                                                              # no tie inside a row, none inside a column
        assert np.unique(pw[g, cand]).size == cand.size and np.unique(cost[g, cand]).size == cand.size
    assert all(np.unique(cost[:G, a]).size == G for a in cand)
    match, ks = R.dynamic_k_ref(pw, cost, in_box, in_ctr, G)
    mg, mi = R.resolve_ref(match, pw, cost, G)
    fg = torch.zeros(A, dtype=torch.bool)
    fg[torch.from_numpy(cand)] = True
    num_fg, _, ious, gt_idx, oks = dynamic_k(torch.from_numpy(cost[:G, cand]), torch.from_numpy(pw[:G, cand]), torch.arange(G), fg)
    assert list(ks[:G]) == list(oks) and bool(np.all(ks[G:] == R.SENT_I32))
    assert np.array_equal(np.flatnonzero(mg >= 0), np.flatnonzero(fg.numpy())) and num_fg == int((mg >= 0).sum())
    assert np.array_equal(mg[mg >= 0], gt_idx.numpy()) and np.array_equal(mi[mg >= 0], ious.numpy())
    assert int((np.array([bin(int(m)).count("1") for m in match]) > 1).sum()) > 0     # the conflict rule was used
    assert int((match >> np.uint64(G)).max()) == 0


def test_torch_topk_does_not_take_the_lower_index():
    """why the reference is a stable sort and not the oracle: on equal values torch.topk returns SOME of them (which ones differs
    between builds, so nothing is asserted about it); the reference returns the lowest anchors"""
    got = torch.topk(torch.tensor([1.0, 2, 2, 2, 0, 2, 2]), 3).indices.tolist()
    assert set(got) <= {1, 2, 3, 5, 6}
    pw = np.zeros((R.G_MAX, 7), dtype=F32)
    pw[0] = [1, 2, 2, 2, 0, 2, 2]
    pw1 = np.full((R.G_MAX, 7), 0.5, dtype=F32)                                      # top-10 sum 3.5 -> k = 3: the three lowest 2s
    m, ks = R.dynamic_k_ref(pw1, -pw, np.ones(7, dtype=np.uint64), np.zeros(7, dtype=np.uint64), 1)
    assert ks[0] == 3 and list(np.flatnonzero(m)) == [1, 2, 3]


def test_finalize_equals_the_oracle_weights():
    """two calls of oracle.loss.LossOracle on a 64-pixel case (84 anchors): the second carries the first call's losses as state"""
    from ep24 import synth
    from oracle.loss import LossOracle
    labels = synth.make_labels(2, [3, 2], size=64, seed=5)
    raw = synth.make_raw_head(2, size=64, seed=6)
    lf = LossOracle(80)
    st = np.ones(26, dtype=F32)
    for call in range(2):
        out = synth.decode_head(raw if call == 0 else raw * 0.9 + 0.02, size=64)
        loss, wl, lo, lc, _, ratio, draw = lf(synth.outputs_train_tuple(out, size=64), labels)
        w = torch.cat([draw[3].reshape(-1), draw[4].reshape(1), draw[5].reshape(1)]).double().numpy()
        l = np.concatenate([(wl / draw[3]).double().numpy(), [float(lo), float(lc)]])
        nfg = round(ratio * 5)
        assert nfg >= 1
        p = np.zeros((1, R.NS), dtype=F32)
        p[0, :26], p[0, 26] = (l * nfg).astype(F32), nfg
        res, l_new, _, _ = R.finalize_ref(p, [3, 2], st)
        assert np.allclose(np.concatenate([res[29:53], res[53:55]]), w, rtol=2e-6, atol=0)
        assert np.isclose(res[0], float(loss), rtol=2e-6) and res[28] == 5 and res[55] == nfg
        st = l_new.astype(F32)


# ------------------------------------------------------------------------------------------------------------- (b)
@pytest.mark.parametrize("A", R.DYNK_A)
def test_every_dyadic_selection_case_is_exact(A):
    """every prefix sum of the top-10 is an fp32 number in double as well: the expected k does not depend on the order of the sum.
    Also what the cases are meant to reach: P in {0, 1, 9, 10, 11, A}, k = 10, the floor, truncation just below an integer."""
    seen_p, seen_k = set(), set()
    for kind, gi, grp in R.dynk_groups():
        c = R.dynk_case(A, kind, gi)
        for b in range(4):
            cand = c["cand"][b]
            if c["num_gt"][b] > 0:                                                  # an image without labels runs no selection
                seen_p.add(cand.size)
                if cand.size == 0:                                                  # the floor at 1, and nothing to take
                    assert bool(np.all(c["ks"][b, :c["num_gt"][b]] == 1)) and not c["match"][b].any()
                    seen_k.add(("P0", A))
            assert float(c["pw"][b].min()) >= 0.0 and float(c["pw"][b].max()) <= 1.0
            for g in range(int(c["num_gt"][b])):
                seen_k.add((kind, int(c["ks"][b, g])))
                if kind == "general":
                    continue
                v = np.sort(c["pw"][b, g, cand].astype(np.float64))[::-1][:10]
                pre = np.cumsum(v)
                assert bool(np.all(pre.astype(F32).astype(np.float64) == pre)), (A, kind, gi, b, g)
                assert max(1, int(pre[-1]) if pre.size else 0) == c["ks"][b, g]
            assert bool(np.all(c["ks"][b, int(c["num_gt"][b]):] == R.SENT_I32))
            assert int((c["match"][b] >> np.uint64(c["num_gt"][b])).max()) == 0      # no bit of g >= num_gt (num_gt = 0: no bit)
    assert {0, 1, min(9, A), min(10, A), min(11, A), A} <= seen_p and ("P0", A) in seen_k, seen_p
    if A >= 11:
        assert ("ones", 10) in seen_k and ("tiny", 1) in seen_k and ("sum3", 3) in seen_k and ("below4", 3) in seen_k
        assert ("equal", 5) in seen_k


def test_every_layout_meets_an_image_with_labels():
    live = {name: set() for name in R.LAYOUTS}
    for num_gt, grp in R.DYNK_GROUPS:
        assert sorted(num_gt) == [0, 1, 7, 50]
        for n, name in zip(num_gt, grp):
            if n:
                live[name].add(n)
    assert all(live.values()), live
    assert live["none"] == {7, 50} and live["ends"] == {50}
    for A in (9, 8449, 8705):                                                       # the layouts are what their names say
        rng = np.random.default_rng(0)
        assert R.layout("none", A, rng).size == 0 and list(R.layout("ends", A, rng)) == [0, A - 1]
        assert list(R.layout("last", A, rng)) == [A - 1] and R.layout("all", A, rng).size == A
    t = R.layout("thread11", 8705, np.random.default_rng(0))
    assert t.size == 11 and set(t % 256) == {37} and t[0] == 37 and t[-1] == 37 + 256 * 33


@pytest.mark.parametrize("nb", R.FIN_NBLOCKS)
def test_integer_partials_fold_exactly(nb):
    for count in R.FIN_COUNTS:
        p = R.finalize_partials(nb, count)
        assert float(p[:, 26].sum()) == count and not p[:, 28:].any()
        want = p.astype(np.float64).sum(0)
        assert float(want.max()) < 2 ** 24
        assert np.array_equal(R.finalize_fold(p).astype(np.float64), want)
        res, l, _, _ = R.finalize_ref(p, [1, 2], np.ones(26, dtype=F32))
        for i in R.FIN_EXACT:
            assert UR.exact32(res[i:i + 1]), (nb, count, i)
        assert UR.exact32(l)


# ------------------------------------------------------------------------------------------------------------- (c)
def test_finalize_bound_holds_a_float32_emulation():
    worst = 0.0
    for nb in R.FIN_NBLOCKS:
        for seed, st in enumerate([np.ones(26, dtype=F32), np.linspace(0.2, 3.0, 26).astype(F32)]):
            p = R.finalize_general(nb, seed)
            res, l, tol, tol_l = R.finalize_ref(p, [5, 6], st)
            got, gl = R.finalize_f32(p, [5, 6], st)
            for use in (got, R.finalize_f32(p, [5, 6], st, R.finalize_fold(p))[0]):
                w = R.FIN_WRITTEN
                worst = max(worst, UR.err_ratio(use[w], res[w], np.maximum(tol[w], 1e-300)))
            worst = max(worst, UR.err_ratio(gl, l, tol_l))
    print("FIN-EMU largest err / tol = %.3f" % worst)
    assert worst <= 1.0


# ------------------------------------------------------------------------------------------------------------- (d)
def _select(v, idx, n, largest, tie_high=False, keep_slots=False):
    """n rounds of arg-best over (value, anchor) as the kernel runs them; tie_high: equal values go to the higher anchor;
    keep_slots: a pick at anchor >= 256 (a slot j > 0 of its thread) is not removed and wins again"""
    alive = np.ones(idx.size, dtype=bool)
    out = []
    key = -v.astype(np.float64) if largest else v.astype(np.float64)
    for _ in range(n):
        if not alive.any():
            break
        best = key[alive].min()
        c = np.flatnonzero(alive & (key == best))
        i = c[-1] if tie_high else c[0]
        out.append(i)
        if not (keep_slots and idx[i] >= 256):
            alive[i] = False
    return np.array(out, dtype=np.int64)


def _dynk_mutant(c, b, how):
    pw, cost, ng, A = c["pw"][b], c["cost"][b], int(c["num_gt"][b]), c["pw"].shape[2]
    match = np.zeros(A, dtype=np.uint64)
    ks = np.full(R.G_MAX, R.SENT_I32, dtype=np.int64)
    for g in range(ng):
        if how == "per_label":
            cand = np.flatnonzero(((c["in_box"][b] | c["in_ctr"][b]) >> np.uint64(g)) & np.uint64(1))
        elif how == "non_candidate":
            cand = np.arange(A)
        else:
            cand = c["cand"][b]
        if how == "drop_last":
            cand = cand[cand != A - 1]
        kw = dict(tie_high=how == "tie_high", keep_slots=how == "keep_slots")
        top = _select(pw[g, cand], cand, 10, True, **kw)
        total = R.sum32(pw[g, cand[top]])
        k = int(np.rint(total)) if how == "round" else int(np.trunc(total))
        if how != "no_floor":
            k = max(1, k)
        ks[g] = k
        pick = _select(cost[g, cand], cand, k, False, **kw)
        match[cand[pick]] |= np.uint64(1 << g)
    return match, ks


def test_the_round_based_selection_is_the_reference():
    """_select without a fault (rounds of arg-best, as the kernel runs) gives what the stable sort gives"""
    for A in (257, 8449):
        for kind in ("dyadic", "equal", "general"):
            c = R.dynk_case(A, kind, 1)
            for b in range(4):
                m, ks = _dynk_mutant(c, b, "none")
                assert np.array_equal(m, c["match"][b]) and np.array_equal(ks, c["ks"][b])


@pytest.mark.parametrize("how", ["tie_high", "keep_slots", "per_label", "round", "no_floor", "drop_last", "non_candidate"])
def test_selection_mutants_are_rejected(how):
    hit = 0
    for A in (257, 8449) if how == "keep_slots" else (9, 257):
        for kind, gi, _ in R.dynk_groups():
            c = R.dynk_case(A, kind, gi)
            for b in range(4):
                m, ks = _dynk_mutant(c, b, how)
                hit += int(not (np.array_equal(m, c["match"][b]) and np.array_equal(ks, c["ks"][b])))
    assert hit > 0, how


def _resolve_mutant(c, b, how):
    ng, A = int(c["num_gt"][b]), c["match"].shape[1]
    mg = np.full(A, -1, dtype=np.int32)
    for a in np.flatnonzero(c["match"][b]):
        m = int(c["match"][b, a])
        bits = [g for g in range(R.G_MAX) if (m >> g) & 1]
        col = c["cost"][b, :ng, a]
        if len(bits) == 1:
            mg[a] = bits[0]
        elif how == "claiming_only":
            mg[a] = bits[int(np.argmin(col[bits]))]
        else:                                                                       # last_wins
            mg[a] = int(np.flatnonzero(col == col.min())[-1])
    return mg


@pytest.mark.parametrize("how", ["claiming_only", "last_wins"])
def test_resolve_mutants_are_rejected(how):
    hit = 0
    for A in R.RESOLVE_A:
        c = R.resolve_case(A)
        for b in range(4):
            hit += int(not np.array_equal(_resolve_mutant(c, b, how), c["mg"][b]))
    assert hit > 0


def test_resolve_cases_hold_what_they_promise():
    c = R.resolve_case(257)
    pop = np.array([[bin(int(m)).count("1") for m in row] for row in c["match"]])
    assert {0, 1, 2, 5} <= set(pop.reshape(-1).tolist())
    assert int((c["match"][3] == np.uint64(1 << 49)).sum()) > 0 and int((c["match"] == np.uint64(1)).sum()) > 0
    unclaimed = 0
    for b in range(4):
        for a in np.flatnonzero(pop[b] > 1):
            unclaimed += int(not (int(c["match"][b, a]) >> int(c["mg"][b, a])) & 1)
        assert int((c["match"][b] >> np.uint64(c["num_gt"][b])).max()) == 0
    assert unclaimed > 0 and not c["match"][0].any() and bool(np.all(c["mg"][0] == -1))


@pytest.mark.parametrize("how", ["drop_last_row", "drop_tail"])
def test_finalize_fold_mutants_are_rejected(how):
    hit = {}
    for nb in R.FIN_NBLOCKS:
        p = R.finalize_partials(nb, 64)
        hit[nb] = not np.array_equal(R.finalize_fold(p, **{how: True}), R.finalize_fold(p))
    assert hit[137] and hit[129] and (how == "drop_tail" or all(hit.values())), hit


# ------------------------------------------------------------------------------------------------------------- the other stages
def test_error_codes_are_the_header_s():
    import re
    text = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "ep24.h")).read()
    code = lambda n: int(re.search(r"#define\s+%s\s+\(?(-?\d+)\)?" % n, text).group(1))
    assert code("EP24_E_ARG") == R.E_ARG and code("EP24_E_UNSUPPORTED") == R.E_UNSUPPORTED
    assert code("EP24_MAX_GT") == R.G_MAX and code("EP24_LABEL_COLS") == R.LCOLS and code("EP24_NUM_SUMS") == R.NS


def _words(mask):
    """bool [G, A] -> uint64 [A]"""
    w = np.zeros(mask.shape[1], dtype=np.uint64)
    for g in range(mask.shape[0]):
        w |= mask[g].astype(np.uint64) << np.uint64(g)
    return w


def test_cost_equals_the_oracle():
    """oracle.assign.assign_image(detail=True) on a 128-pixel synthetic head (336 anchors, 6 labels): pw, cls_cost and cost of every
    (label, candidate) whose 24 rays keep 1e-4 of the larger radius from a branch boundary (the clip to +-0.99 makes the lens area
    jump there), under the bound derived for the same fp32 sequence of operations"""
    from ep24 import synth
    from oracle.assign import assign_image
    n, C = 6, 80
    labels = synth.make_labels(1, n, size=128, seed=8)
    out = synth.decode_head(synth.make_raw_head(1, size=128, seed=9), size=128)[0]
    xs, ys, st = synth.anchor_grid(128)
    _, det = assign_image(labels[0, :n, 1:], labels[0, :n, 0], out[:, :26], out[:, 27:], out[:, 26:27], xs, ys, st, C, detail=True)
    fg = det["fg_pre"].numpy()
    ib, ic = _words(det["in_box"].numpy()), _words(det["in_ctr"].numpy())
    assert np.array_equal(R.cand_of(ib, ic), np.flatnonzero(fg)) and fg.sum() > 30
    ref = R.cost_ref(out.numpy(), labels[0].numpy(), ib, ic, n)
    ok = (ref["margin"][:n][:, fg].min(2) >= 1e-4)
    assert ok.mean() > 0.9
    worst = {}
    for k, tol in (("pw", "tol_pw"), ("cost", "tol_cost"), ("cls_cost", "tol_cost")):
        worst[k] = UR.err_ratio(det[k].numpy()[ok], ref[k][:n][:, fg][ok], ref[tol][:n][:, fg][ok])
    print("COST-ORACLE largest err / tol: %s" % worst)
    assert max(worst.values()) <= 1.0
    assert bool(np.all(ref["both_cost"][:n][:, fg] == 100000.0 * (~det["in_both"].numpy())))


@pytest.mark.parametrize("C", R.COST_C)
def test_cost_bound_holds_a_float32_emulation_and_the_cases_reach_their_paths(C):
    worst = [0.0, 0.0]
    for rays in R.COST_RAYS:
        c = R.cost_case(C, rays)
        assert int(c["labels"][..., 0].max()) < C and c["outputs"].shape[2] == 27 + C
        per_wg = [int(((c["cand"] >= 64 * i) & (c["cand"] < 64 * i + 64)).sum()) for i in range(6)]
        assert per_wg == [64, 0, 1, 63, 64, 37]
        for b in range(4):
            a = (c["outputs"][b], c["labels"][b], c["in_box"][b], c["in_ctr"][b], c["num_gt"][b])
            ref = R.cost_ref(*a)
            w = ref["written"]
            assert w.sum() == c["cand"].size * c["num_gt"][b] and not w[c["num_gt"][b]:].any()
            assert float(ref["margin"][w].min()) >= 0.01 and float(ref["cmax"][w].max()) <= 0.9
            br = ref["branch"][w]
            lens_share = float((br == 2).mean())
            assert {"lens": lens_share == 1.0, "none": lens_share == 0.0, "mixed": 0.1 < lens_share < 0.9}[rays]
            assert rays != "none" or ((br == 0).any() and (br == 1).any())
            assert (ref["both_cost"][w] == 0).any() and (ref["both_cost"][w] == 100000.0).any()
            pw, cost = R.cost_f32(*a)
            assert np.isnan(pw[~w]).all() and float(ref["pw"][w].min()) >= 0 and float(ref["pw"][w].max()) <= 1
            worst[0] = max(worst[0], UR.err_ratio(pw[w], ref["pw"][w], ref["tol_pw"][w]))
            worst[1] = max(worst[1], UR.err_ratio(cost[w], ref["cost"][w], ref["tol_cost"][w]))
            big = ref["both_cost"][w] > 0                                           # a few ulp of the largest addend, nothing wider
            assert float((ref["tol_cost"][w][big] / 100000.0).max()) < 8 * R.U and float(ref["tol_cost"][w][~big].max()) < 2e-3
    print("COST-EMU C=%d largest err / tol: pw %.3f cost %.3f" % (C, worst[0], worst[1]))
    assert max(worst) <= 1.0


def test_cost_ranges_cut_where_they_should():
    lo_hi = R.COST_RANGES
    assert lo_hi[0] == (0, R.COST_A) and lo_hi[1][0] % 64 != 0 and lo_hi[1][1] % 64 != 0 and lo_hi[2][0] == lo_hi[2][1]
    assert list(R.cost_candidates()[(R.cost_candidates() >= lo_hi[3][0]) & (R.cost_candidates() < lo_hi[3][1])]) == [168]


@pytest.mark.parametrize("A", R.CAND_A)
def test_candidates_agree_with_the_oracle_and_few_pairs_are_skipped(A):
    from ep24 import synth
    from oracle.assign import candidate_masks
    worst = 0.0
    for kind, n, seed in R.CAND_SETS:
        labels, xs, ys, st = R.candidate_inputs(synth, A, kind, n, seed)
        ref = R.candidates_ref(labels, xs, ys, st)
        ng = ref["num_gt"]
        assert ng == (49 if kind == "hole" else n)
        ib, ic, dec_b, dec_c = R.candidates_expected(ref)
        assert not dec_b[ng:].any() and not dec_c[ng:].any()
        assert int((ib >> np.uint64(ng)).max()) == 0 and int((ic >> np.uint64(ng)).max()) == 0
        if ng == 0:
            assert not ib.any() and not ic.any()
            continue
        assert 1 - dec_b[:ng].mean() <= R.CAND_SKIP_CAP and 1 - dec_c[:ng].mean() <= R.CAND_SKIP_CAP, (kind, A)
        t = torch.from_numpy
        _, _, ob, oc = candidate_masks(t(labels[:ng, 1:]), t(xs), t(ys), t(st))
        bit = lambda w: ((w[None, :] >> np.arange(ng, dtype=np.uint64)[:, None]) & np.uint64(1)).astype(bool)
        assert not ((bit(ib) != ob.numpy()) & dec_b[:ng]).any() and not ((bit(ic) != oc.numpy()) & dec_c[:ng]).any()
        deg, ctr = R.candidates_f32(labels, xs, ys, st)
        fin = np.isfinite(ref["tol_deg"][:ng])
        worst = max(worst, float((np.abs(deg - ref["deg"][:ng])[fin] / ref["tol_deg"][:ng][fin]).max()))
        assert bool(np.all(np.abs(ctr - ref["ctr"][:ng]) <= ref["tol_ctr"][:ng]))
        if A == 1344 and ng >= 49:
            assert bit(ib).sum() > 1000 and bit(ic).sum() > 1000
    print("CAND-EMU A=%d largest err / tol of the angle sum %.3f" % (A, worst))
    assert worst <= 1.0


def test_the_sum_bounds_cover_the_kernel_s_own_trees():
    """m_sum's n against the longest chain of inexact additions in loss_terms_kernel, for every count of matched anchors in a block
    and every C the GPU file runs (the argument is m_sum's docstring)"""
    cd = lambda a, b: -(-a // b)
    for M in range(1, 257):
        waves = min(4, M)
        assert R.kernel_sum_depth(cd(M, 4), 1, waves) <= M                                  # a ray column
        assert R.kernel_sum_depth(cd(M, 4), 26, waves) <= 26 + M                            # the L1 column
        assert R.kernel_sum_depth(1, min(M, 64), cd(M, 64)) <= M                            # the objectness of M anchors
        for C in R.LOSS_C:
            assert R.kernel_sum_depth(cd(M, 4) * cd(C, 64), min(C, 64), waves) <= C + M, (M, C)
    for nb in R.FIN_NBLOCKS:                                                                # finalize: a group's rows, then the groups
        per = cd(nb, 8)
        assert (per - 1) + min(7, cd(nb, per) - 1) <= nb


LOSS_CPU = [(1, 1), (255, 3), (256, 101), (257, 229), (513, 230), (513, 80)]


@pytest.mark.parametrize("A,C", LOSS_CPU)
def test_loss_bounds_hold_float32_emulations(A, C):
    wt = wg = 0.0
    res = R.loss_result()
    for shift in (0, 1):
        c = R.loss_case(A, C, shift)
        pv, pe = R.terms_ref(c, True)
        wt = max(wt, R.check_bound(UR.bits32(R.terms_ref(c, True, f32=True)), pv, pe, "partials"))
        dv, de, ov, oe = R.grad_ref(c, res, None, True)
        d32, o32 = R.grad_ref(c, res, None, True, f32=True)
        wg = max(wg, R.check_bound(UR.bits32(d32), dv, de, "dout"), R.check_bound(UR.bits32(o32), ov, oe, "d_origin"))
        assert np.array_equal(np.sign(o32), np.sign(ov).astype(F32))
        # what is exact by construction
        assert not pe[:, 26].any() and not pe[:, 28:].any() and not pv[:, 28:].any()
        un = c["matched_gt"] < 0
        assert not de[un][:, :26].any() and not de[un][:, 27:].any() and not dv[un][:, :26].any() and bool(np.all(de[..., 26] > 0))
        assert not ov[un].any() and bool(np.all(np.abs(ov[~un]) == 1.0 / 64))
    print("LOSS-EMU A=%d C=%d largest err / tol: partial sums %.3f gradient %.3f" % (A, C, wt, wg))
    assert wt <= 1.0 and wg <= 1.0


def test_loss_cases_hold_what_they_promise():
    seen = set()
    for A in R.LOSS_A:
        for shift in (0, 1):
            c = R.loss_case(A, 3, shift)
            seen |= set(c["patterns"].values())
            for (b, blk), p in c["patterns"].items():
                m = c["matched_gt"][b, blk * 256:blk * 256 + 256] >= 0
                if p == "all":
                    assert m.all()
                elif p == "lanes":
                    assert list(np.flatnonzero(m)) == [t for t in range(m.size) if t % 64 in (0, 63)]
                elif p == "one":
                    assert m.sum() == 1
                elif p == "none":
                    assert not m.any()
            assert int(c["matched_gt"].max()) == 49 or A == 1
    assert seen == set(R.PATTERNS)
    full = R.loss_case(513, 3, 0)
    assert (full["matched_gt"][0, :256] >= 0).all()
    assert sorted(27 + C for C in R.LOSS_C) == [28, 30, 107, 128, 256, 257]
    c = R.loss_case(257, 80, 0)                                                      # every ray sits in its branch by construction
    m = c["matched_gt"] >= 0
    lab = c["labels"][np.arange(4)[:, None], np.maximum(c["matched_gt"], 0)][m]
    _, cx, cy, r1, e1 = R.label_geometry(lab)
    o = c["outputs"][m].astype(np.float64)
    ray = R.ray_ref(r1, o[:, 2:26], np.hypot(cx - o[:, 0], cy - o[:, 1])[:, None], e1, 0.0, 0.0)
    assert float(ray["margin"].min()) >= 0.01 and float(ray["cmax"].max()) <= 0.9 and set(np.unique(ray["branch"])) == {0, 1, 2}


def _grad_mutant(c, res, how, ncols):
    d32, _ = R.grad_ref(c, res, None, False, f32=True)
    B, A, _ = d32.shape
    if how == "col26":                                                               # matched rows from the unmatched formula
        so = 1.0 / (1.0 + np.exp(-c["outputs"][..., 26].astype(np.float64)))
        m = c["matched_gt"] >= 0
        d32[..., 26][m] = (res[53] / res[27] * so[m]).astype(F32)
    else:                                                                            # the cooperative writer one row off
        if 256 % ncols:
            return d32
        un = c["matched_gt"] < 0
        for b in range(B):
            for a in range(A - 1):
                if un[b, a] and (a + 1) % 256:
                    d32[b, a] = np.where(np.arange(ncols) == 26, d32[b, a + 1, 26] if un[b, a + 1] else F32(0), F32(0))
    return d32


@pytest.mark.parametrize("how", ["col26", "row_off"])
def test_gradient_mutants_are_rejected(how):
    res = R.loss_result()
    hit = {}
    for C in (101, 229, 80):
        c = R.loss_case(257, C, 0)
        dv, de, _, _ = R.grad_ref(c, res, None, False)
        good, _ = R.grad_ref(c, res, None, False, f32=True)
        assert R.check_bound(UR.bits32(good), dv, de, "dout") <= 1.0
        try:
            hit[C] = R.check_bound(UR.bits32(_grad_mutant(c, res, how, 27 + C)), dv, de, "dout") > 1.0
        except AssertionError:
            hit[C] = True
    assert hit[101] and hit[229] and (how == "row_off" or hit[80]), hit
