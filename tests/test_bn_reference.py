"""tests/bn_reference.py without a GPU: (a) its float64 formulas equal float64 autograd of F.batch_norm + activation (+ residual);
(b) every exactness / discrimination precondition holds for every case tests/test_gpu_bn_exact.py runs; (c) every float64 tolerance
holds a float32 emulation of the kernels' expressions (not too tight) and rejects the mutants a case claims to catch (not too loose):
projection terms dropped, k2's sign flipped, last row skipped, replicas beyond the 8th ignored, a clamped replica added again,
LeakyReLU's derivative replaced by the identity's."""
import os
import sys

import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bn_reference as R  # noqa: E402

BF = torch.bfloat16


def test_helper_never_imports_the_package():
    src = open(R.__file__.replace(".pyc", ".py")).read()
    assert "import ep24" not in src and "from ep24" not in src


# ------------------------------------------------------------------------------------------------------------- (a)
def _torch_act(u, act):
    return F.silu(u) if act == 1 else F.relu(u) if act == 2 else F.leaky_relu(u, 0.1) if act == 3 else u


@pytest.mark.parametrize("with_res", [False, True])
@pytest.mark.parametrize("act", [0, 1, 2, 3])
@pytest.mark.parametrize("M,C", [(37, 16), (1, 8), (2, 8)])
def test_formulas_equal_float64_autograd(M, C, act, with_res):
    g = torch.Generator().manual_seed(5 + act)
    z = (torch.randn(M, C, generator=g, dtype=torch.float64) * 1.5 + 0.3).requires_grad_(True)
    gamma = (torch.rand(C, generator=g, dtype=torch.float64) + 0.5).requires_grad_(True)
    beta = (torch.rand(C, generator=g, dtype=torch.float64) - 0.5).requires_grad_(True)
    res = torch.randn(M, C, generator=g, dtype=torch.float64) if with_res else None
    dy = torch.randn(M, C, generator=g, dtype=torch.float64) + 0.5
    old = torch.randn(M, C, generator=g, dtype=torch.float64)
    rm0, rv0 = torch.randn(C, generator=g, dtype=torch.float64), torch.rand(C, generator=g, dtype=torch.float64) + 0.5
    zd = z.detach()
    r = R.fwd_ref(zd, zd.sum(0), (zd * zd).sum(0), gamma.detach(), beta.detach(), act, res, rm0, rv0)
    if M == 1:                      # F.batch_norm refuses one value per channel in training mode: the guard of the unbiased variance
        assert torch.equal(r["var"], torch.zeros(C, dtype=torch.float64)) or float(r["var"].abs().max()) < 1e-12
        assert float((r["rvar"] - ((1 - R.MOMENTUM) * rv0 + R.MOMENTUM * r["var"])).abs().max()) == 0.0
        assert float((r["y"] - (_torch_act(beta.detach().expand(M, C), act) + (res if with_res else 0))).abs().max()) < 1e-9
        return
    rm, rv = rm0.clone(), rv0.clone()
    u = F.batch_norm(z, rm, rv, gamma, beta, True, R.MOMENTUM, R.EPS)
    y = _torch_act(u, act) + (res if with_res else 0)
    y.backward(dy)
    tol = 1e-12
    assert float((r["y"] - y.detach()).abs().max()) < tol
    assert float((r["rmean"] - rm).abs().max()) < tol and float((r["rvar"] - rv).abs().max()) < tol
    assert float((r["mean"] - zd.mean(0)).abs().max()) < tol and float((r["invstd"] - 1 / torch.sqrt(zd.var(0, unbiased=False) + R.EPS)).abs().max()) < tol
    a = (dy, zd, r["mean"], r["invstd"], gamma.detach(), beta.detach())
    sg, sb, ag, ab = R.bwd_sums(*a, act)
    assert float((sg - gamma.grad).abs().max()) < tol * M and float((sb - beta.grad).abs().max()) < tol * M
    assert bool((ag >= sg.abs()).all()) and bool((ab >= sb.abs()).all())
    d = R.dz_ref(*a, sg, sb, act)
    assert float((d["dz"] - z.grad).abs().max()) < tol
    # accumulate form: a second consumer's gradient on top of `old`
    z.grad = old.clone()
    _torch_act(F.batch_norm(z, rm, rv, gamma, beta, True, R.MOMENTUM, R.EPS), act).backward(dy)
    assert float((old + d["dz"] - z.grad).abs().max()) < tol


def test_split_and_fold():
    total = torch.randint(-10 ** 9, 10 ** 9, (2, 40))
    for reps in (1, 2, 3, 8, 9):
        p = R.split_replicas(total, reps, 7)
        assert torch.equal(R.fold(p), total) and p.shape[0] == reps
        if reps > 1:
            assert int(p.abs().min()) > (1 << 20)                     # no replica is (nearly) empty
        if reps == 9:
            assert not torch.equal(R.fold(p, "reps_beyond_8"), total)
            assert torch.equal(R.fold(p, "clamped_duplicate"), total + 7 * p[8])


def test_cases_reach_the_paths_they_name():
    assert R.rpb(8) == 256 and R.rpb(24) == 85 and 85 * 3 == 255                        # thread 255 idle
    assert R.reduce_grid(2053, 2048) == 512 and -(-2053 // 4) > 512 and 2053 - 4 * 512 < 512     # capped; a partial second batch
    assert R.fused_grid(1027, 2048) == 256 and R.fused_grid(1025, 2048) == 256 and 1027 - 4 * 256 < 256
    assert 2056 // 8 == 257                                                             # second pass of the reduce with one group
    assert 4096 // 8 > 256 and R.apply_rows(4100, 4096) == 16 and R.apply_rows(4096, 2056) == 8
    assert all(R.fused_grid(M, C) <= 256 and C <= 2048 for M, C in R.A_FUSED + R.A_FUSED_TOL)
    assert all(M & (M - 1) == 0 for M, C in R.A_FUSED) and all(M & (M - 1) for M, C in R.A_FUSED_TOL)
    for M, C in [(130, 40), (1100, 24), (40, 2056), (123400, 136)]:
        assert not R.fwd_fixed_group(M, C)
    for M, C in [(70, 1024), (65600, 256)]:
        assert R.fwd_fixed_group(M, C)
    assert -(-(70 * 128) // (R.fwd_grid(70, 1024) * 256)) > 4                           # a second iteration of the 4-chunk loop
    assert R.fwd_grid(65600, 256) == 2048 and R.fwd_grid(123400, 136) == 2048 and 65600 * 32 > 2048 * 1024 and 123400 * 17 > 2048 * 1024
    cases = R.fwd_cases()
    assert {c[5] for c in cases} == set(R.REPS_B) and {c[3] for c in cases} == {False, True} and {c[4] for c in cases} == {0, 1, 2}
    assert {(c[2], c[3]) for c in cases if c[0] * c[1] < 10 ** 6} == {(a, r) for a in range(4) for r in (False, True)}
    assert {c[3] for c in R.b_bwd_cases()} == set(R.REPS_A)


# ------------------------------------------------------------------------------------------------------------- (b), (c) part A
@pytest.mark.parametrize("act", [0, 2])
@pytest.mark.parametrize("M,C", R.A_REDUCE)
def test_exact_reduce_preconditions_and_mutants(M, C, act):
    d, sg, sb = R.exact_reduce_ref(M, C, act)
    a = [d[k] for k in ("dy", "z", "mean", "invstd", "gamma", "beta")]
    g2, b2 = R.bwd_sums(*a, act, mutant="last_row")[:2]
    assert not torch.equal(R.fix_of(g2, R.FIXG), sg) and not torch.equal(R.fix_of(b2, R.FIXG), sb)
    # the float32 emulation gives the same integers (row after row; any other order too, by the precondition)
    eg, eb = R.emulate_sums(d, act)
    assert torch.equal(eg, sg) and torch.equal(eb, sb)
    if act == 2:                                                        # ReLU's derivative at u == 0 is 0, not 1
        u, du, zhat = R.bwd_terms(*a, act)
        at0 = (u == 0)
        assert bool(((d["dy"] != 0) & at0).any()) and bool((du[at0] == 0).all())


@pytest.mark.parametrize("act", [0, 2])
@pytest.mark.parametrize("M,C,zero", R.A_APPLY)
def test_exact_apply_preconditions_and_mutants(M, C, zero, act):
    sg, sb = R.forged_sums(M, C, zero)
    d, r = R.exact_apply_ref(M, C, act, sg, sb, need_projection=not zero)
    want = r["dz"].to(BF)
    a = [d[k] for k in ("dy", "z", "mean", "invstd", "gamma", "beta")]
    assert torch.equal(R.emulate_dz(d, sg, sb, act), want)
    assert torch.equal(R.emulate_dz(d, sg, sb, act, d["old"].to(BF)), r["two"])
    if not zero:
        for mutant in ("no_projection", "k2_sign"):
            m = R.dz_ref(*a, sg.double() / R.FIXG, sb.double() / R.FIXG, act, mutant)["dz"].to(BF)
            assert float((m != want).double().mean()) >= 0.01, mutant
    for reps in R.a_reps(M, C):
        parts = R.split_replicas(torch.stack([sg, sb]), reps, 17)
        assert torch.equal(R.fold(parts), torch.stack([sg, sb]))
        if reps == 9:
            for mutant in ("reps_beyond_8", "clamped_duplicate"):
                assert bool((R.fold(parts, mutant) != torch.stack([sg, sb])).all()), mutant


@pytest.mark.parametrize("act", [0, 2])
@pytest.mark.parametrize("M,C", R.A_FUSED)
def test_exact_fused_preconditions(M, C, act):
    d, sg, sb = R.exact_reduce_ref(M, C, act)
    d, r = R.exact_apply_ref(M, C, act, sg, sb)                       # the TRUE sums: still every intermediate representable
    a = [d[k] for k in ("dy", "z", "mean", "invstd", "gamma", "beta")]
    want = r["dz"].to(BF)
    assert torch.equal(R.emulate_dz(d, sg, sb, act), want)
    for mutant in ("no_projection", "k2_sign"):
        m = R.dz_ref(*a, sg.double() / R.FIXG, sb.double() / R.FIXG, act, mutant)["dz"].to(BF)
        assert float((m != want).double().mean()) >= 0.01, mutant


@pytest.mark.parametrize("act", [0, 2])
@pytest.mark.parametrize("M,C", R.A_FUSED_TOL)
def test_fused_tail_case_tolerance(M, C, act):
    """M = 2^k + 1 / + 3: the sums stay exact, dz is compared under part B's bound (no SiLU: S = 0)."""
    d, sg, sb = R.exact_reduce_ref(M, C, act)
    a = [d[k] for k in ("dy", "z", "mean", "invstd", "gamma", "beta")]
    r = R.dz_ref(*a, sg.double() / R.FIXG, sb.double() / R.FIXG, act)
    assert R.is_f32(1 + sg.double() / R.FIXG) and R.is_f32(1 + sb.double() / R.FIXG)
    tol = R.tol_dz(r, d["mean"], act)
    e = (R.emulate_dz(d, sg, sb, act).double() - r["dz"]).abs()
    assert bool((e <= tol).all()), float((e / tol.clamp(min=1e-300)).max())
    big = r["dz"].abs().amax(0)                                       # the projection terms matter in most channels
    assert float((r["k2"].abs() >= 0.05 * big).double().mean()) >= 0.5 and float(r["k2"].abs().max()) >= 0.05 * float(big.max())
    for mutant in ("no_projection", "k2_sign"):
        m = R.dz_ref(*a, sg.double() / R.FIXG, sb.double() / R.FIXG, act, mutant)["dz"]
        assert float(((m.to(BF).double() - r["dz"]).abs() > tol).double().mean()) >= 0.01, mutant


# ------------------------------------------------------------------------------------------------------------- (b), (c) part B
def _fwd_errs(d, r, e, M, act, with_running):
    """-> {name: max err / tol} of an outcome e (float32 / bf16 tensors or arrays) against the reference r."""
    t = lambda v: torch.as_tensor(v).double()
    out = dict(mean=((t(e["mean"]) - r["mean"]).abs() / R.tol_mean(r).clamp(min=2.0 ** -149)).max(),
               invstd=((t(e["invstd"]) - r["invstd"]).abs() / R.tol_invstd(r)).max(),
               y=((e["y"].double() - r["y"]).abs() / R.tol_y(r, d["z"].double(), d["beta"].double(), act).clamp(min=1e-300)).max())
    if with_running:
        out["rmean"] = ((t(e["rmean"]) - r["rmean"]).abs() / R.tol_rmean(r, d["rmean0"].double())).max()
        out["rvar"] = ((t(e["rvar"]) - r["rvar"]).abs() / R.tol_rvar(r, M, d["rvar0"].double())).max()
    return {k: float(v) for k, v in out.items()}


@pytest.mark.parametrize("M,C,act,with_res,running,reps", R.fwd_cases(), ids=lambda v: str(int(v)))
def test_forward_tolerances(M, C, act, with_res, running, reps):
    d, r = R.fwd_case_ref(M, C, act, with_res, bool(running))
    stats = torch.stack([d["s1"], d["s2"]])
    parts = R.split_replicas(stats, reps, 23)
    e = R.emulate_fwd(d["z"], d["s1"], d["s2"], d["gamma"], d["beta"], act, d["res"] if with_res else None,
                      d["rmean0"] if running else None, d["rvar0"] if running else None)
    errs = _fwd_errs(d, r, e, M, act, bool(running))
    assert max(errs.values()) <= 1.0, errs
    # mutants of the replica fold: only the cases with a second batch of replicas claim them
    if reps == 9 and M * C < 10 ** 6:
        for mutant in ("reps_beyond_8", "clamped_duplicate"):
            s = R.fold(parts, mutant)
            e2 = R.emulate_fwd(d["z"], s[0], s[1], d["gamma"], d["beta"], act, d["res"] if with_res else None,
                               d["rmean0"] if running else None, d["rvar0"] if running else None)
            errs = _fwd_errs(d, r, e2, M, act, bool(running))
            assert errs["mean"] > 1.0 and errs["y"] > 1.0 and (not running or errs["rmean"] > 1.0), (mutant, errs)
    # a forward that skips the last row leaves the sentinel there
    tol_last = R.tol_y(r, d["z"].double(), d["beta"].double(), act)[-1]
    assert bool(((R.SENT - r["y"][-1]).abs() > tol_last).all())


def test_forward_tolerance_at_mean_std_ratios():
    """The invstd / y bounds against the emulation at mean / std of 1, 8, 32 and 100 (beyond what the GPU cases draw)."""
    g = torch.Generator().manual_seed(9)
    M, C = 500, 64
    for ratio in (1.0, 8.0, 32.0, 100.0):
        z = (torch.randn(M, C, generator=g) * 0.5 + ratio * 0.5).to(BF)
        gamma, beta = (torch.rand(C, generator=g) + 0.5).float(), (torch.rand(C, generator=g) - 0.5).float()
        zd = z.double()
        s1, s2 = R.fix_of(zd.sum(0), R.FIX), R.fix_of((zd * zd).sum(0), R.FIX)
        for act in (0, 1):
            r = R.fwd_ref(zd, s1.double() / R.FIX, s2.double() / R.FIX, gamma.double(), beta.double(), act)
            e = R.emulate_fwd(z, s1, s2, gamma, beta, act, None, None, None)
            errs = _fwd_errs(dict(z=z, beta=beta), r, e, M, act, False)
            assert max(errs.values()) <= 1.0, (ratio, errs)


@pytest.mark.parametrize("M,C,act,reps", R.b_bwd_cases(), ids=lambda v: str(int(v)))
def test_backward_tolerances(M, C, act, reps):
    d, s, r = R.bwd_case_ref(M, C, act)
    a = [d[k].double() for k in ("dy", "z", "mean", "invstd", "gamma", "beta")]
    tg, tb = R.tol_sums(M, s["ag"], act), R.tol_sums(M, s["ab"], act)
    # the emulation stays inside
    eg, eb = R.emulate_sums(d, act)
    assert bool(((eg.double() / R.FIXG - s["sg"]).abs() <= tg).all()) and bool(((eb.double() / R.FIXG - s["sb"]).abs() <= tb).all())
    tol = R.tol_dz(r, a[2], act)
    old = d["old"].double()
    tol_acc = R.tol_dz_acc(r, a[2], act, old)
    e = (R.emulate_dz(d, s["sg_fix"], s["sb_fix"], act).double() - r["dz"]).abs()
    assert bool((e <= tol).all()), float((e / tol).max())
    e = (R.emulate_dz(d, s["sg_fix"], s["sb_fix"], act, d["old"]).double() - (r["dz"] + old)).abs()
    assert bool((e <= tol_acc).all()), float((e / tol_acc).max())
    # the mutants fall outside
    g2, b2 = R.bwd_sums(*a, act, mutant="last_row")[:2]
    assert bool(((g2 - s["sg"]).abs() > tg).any()) and bool(((b2 - s["sb"]).abs() > tb).any())
    mutants = ["no_projection", "k2_sign"] + (["leaky_as_identity"] if act == 3 else [])
    for mutant in mutants:
        m = R.bwd_case_ref(M, C, act, mutant)[2]["dz"]
        assert float(((m.to(BF).double() - r["dz"]).abs() > tol).double().mean()) >= 0.01, mutant
        assert float((((m + old).to(BF).double() - (r["dz"] + old)).abs() > tol_acc).double().mean()) >= 0.01, mutant
    if act == 3:                    # the sums too: the identity's derivative adds 0.9 dy wherever u <= 0
        sg3, sb3 = R.bwd_sums(*a, act, mutant="leaky_as_identity")[:2]
        assert bool(((sg3 - s["sg"]).abs() > tg).all()) and bool(((sb3 - s["sb"]).abs() > tb).all())
    # the one-launch form applies its own sums: the bound grows by what their tolerance moves dz, and still rejects the mutants
    tol1 = tol + R.tol_dz_sums(r, a[2], a[3], tg, tb)
    assert float((tol1 / tol).median()) < 1.5                        # (the any-order bound of the sums is M e: visible only where dz is near 0)
    for mutant in mutants:
        m = R.bwd_case_ref(M, C, act, mutant)[2]["dz"]
        assert float(((m.to(BF).double() - r["dz"]).abs() > tol1).double().mean()) >= 0.01, mutant
    assert float((R.tol_grad(s["sg"]) / s["sg"].abs().clamp(min=1)).max()) < 1e-6
    # a last row nobody wrote keeps the sentinel / the old value
    assert bool(((R.SENT - r["dz"][-1]).abs() > tol[-1]).all())
    assert bool(((old[-1] - (r["dz"][-1] + old[-1])).abs() > tol_acc[-1]).any())
    if reps == 9:
        parts = R.split_replicas(torch.stack([s["sg_fix"], s["sb_fix"]]), reps, 29)
        for mutant in ("reps_beyond_8", "clamped_duplicate"):
            f = R.fold(parts, mutant).double() / R.FIXG
            m = R.dz_ref(*a, f[0], f[1], act)["dz"]
            assert float(((m - r["dz"]).abs() > tol).double().mean()) >= 0.5, mutant
