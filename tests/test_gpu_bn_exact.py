"""The BatchNorm + activation kernels (csrc/elementwise.hip) against tests/bn_reference.py, through the C ABI.

Part A - backward, BIT FOR BIT (act 0 and 2).  The reduce and apply kernels take save = (mean, invstd) and the fixed-point sums as
INPUTS, so the test forges them: z in multiples of 1/4, dy in multiples of 1/8, mean, invstd, gamma and beta from short lists of
dyadic values.  Then sc, sh, u, zhat and du * zhat are exact in fp32, every fp32 partial sum of the reduce is exact in any order
(sum|du zhat| 2^7 < 2^24, sum|du| 2^3 < 2^24, asserted on the reference), and with sums that are multiples of M / 64 (M a power of
two) k1, k2, k3 and both fma of the apply are fp32 numbers: dz has one right answer, bf16(float64 formula), for the accumulate
form bf16(float(bf16(o)) + old).  Where M is no power of two the forged sums are 0 (dz = k1 du: exact for any M: the row tails).

Part B - forward (all four activations) and the SiLU / LeakyReLU backward against float64 computed from the same fixed-point
sums, under bounds derived from the fp32 formulas (bn_reference.tol_*): one bf16 ulp per element plus the propagated fp32 terms.
tests/test_bn_reference.py shows on the CPU that a float32 emulation of the kernels stays inside every bound and that each mutant
(projection terms dropped, k2's sign, last row skipped, replicas beyond the 8th ignored, a clamped replica added again, identity
derivative for LeakyReLU) falls outside on every case that claims it.

Every operand and destination sits in a sentinel-filled buffer (3 guard rows before and after; guard columns in the slice layout,
where every operand has its own stride and channel offset), and whole buffers are compared.  Each test prints its largest err / tol.

The SiLU slack S (bn_reference.S_SILU, v_exp_f32 + v_rcp_f32) is 2^-18 relative for |u| <= 16.  Measured on an MI355X (largest err / tol
over all cases and both layouts; 1.0 is the bound, and ~0.99 is where a bf16 rounding decision falls on the other side of a tie):
  forward   y 0.996 (SiLU cases 0.995; the SAME cases with S = 0: 0.996), save mean 0.989, save invstd 0.461, running mean 0.519, var 0.475
  backward  reduce sums 0.068 (SiLU 0.019, with S = 0: 0.057), apply dz 0.996, apply_acc dz 0.995, one-launch dz 0.990 (its sums 0.068),
            gamma_grad / beta_grad 0.72; SiLU dz with S = 0: 0.996; one-launch row-tail cases (M = 1025, 1027): dz 0.996
No SiLU case exceeds 1 - not even with S = 0 - so S stays at its starting value.
"""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bn_reference as R  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BF = torch.bfloat16
ISENT = 0x5A5A5A5A5A5A                # guard replicas of the fixed-point sums
KEYS = ("dy", "z", "mean", "invstd", "gamma", "beta")


def _abi():
    from ep24._lib import call, lib, ptr, stream_ptr
    return call, ptr, stream_ptr, lib()


def buf(M, C, lay, fill=None):
    return R.Buf(M, C, lay[0], lay[1], dev=DEV, fill=fill)


def vec(t):
    return R.Vec(t, dev=DEV)


class Sums:
    """[1 + reps + 1][2][C] int64: the replicas between two guard replicas."""

    def __init__(self, parts):
        self.reps, _, self.C = parts.shape
        self.host = torch.full((self.reps + 2, 2, self.C), ISENT, dtype=torch.int64)
        self.host[1:-1] = parts
        self.dev = self.host.to(DEV)

    def ptr(self, offset=0):
        return self.dev.data_ptr() + (2 * self.C + offset) * 8

    def parts(self):
        got = self.dev.cpu()
        assert bool((got[0] == ISENT).all()) and bool((got[-1] == ISENT).all()), "a replica outside [0, reps) was written"
        return got[1:-1]


def report(name, **ratios):
    print("BN-ERR %s: %s" % (name, ", ".join("%s %.3g" % (k, float(v)) for k, v in ratios.items())))


def ratio(got, want, tol):
    return float(((got.double() - want).abs() / tol.clamp(min=1e-300)).max())


def consts(d):
    return vec(torch.stack([d["mean"], d["invstd"]])), vec(d["gamma"]), vec(d["beta"])


def bwd_args(dyb, zb, save, gamma, beta, sums):
    return (dyb.ptr(), dyb.ld, zb.ptr(), zb.ld, save.ptr(), gamma.ptr(), beta.ptr(), sums.ptr(0), sums.ptr(sums.C))


def _gid(M, C, **grids):
    return "%dx%d-" % (M, C) + "-".join("%s%d" % (k, v) for k, v in grids.items())


# ---------------------------------------------------------------------------------------------------------------------------
def test_act_outside_0_to_3_is_refused():
    """All five entry points, before any pointer is looked at (every pointer argument is NULL here)."""
    call, ptr, sp, L = _abi()
    nargs = {"ep24_bn_act_fwd": (21, 19), "ep24_bn_act_bwd_reduce": (14, 11), "ep24_bn_act_bwd_apply": (18, 15), "ep24_bn_act_bwd_fused": (19, 15),
             "ep24_bn_act_bwd_apply_acc": (18, 15)}
    for name, (n, iact) in nargs.items():
        assert len(L.protos[name][1]) == n and L.protos[name][1][iact][1] == "act"
        for act in (-1, 4, 255):
            args = [(None if "*" in t else (0.0 if t == "float" else 0)) for t, _ in L.protos[name][1]]
            args[iact] = act
            assert L.fn[name](*args) == -1, (name, act)                # EP24_E_ARG
            assert "act=%d" % act in L.last_error(), L.last_error()


# ---------------------------------------------------------------------------------------------------------------------------
# part A
REDUCE_CASES = [(M, C, reps) for M, C in R.A_REDUCE for reps in R.a_reps(M, C)]


@pytest.mark.parametrize("layout", list(R.LAYOUTS))
@pytest.mark.parametrize("act", [0, 2], ids=["identity", "relu"])
@pytest.mark.parametrize("M,C,reps", REDUCE_CASES, ids=[_gid(M, C, grid=R.reduce_grid(M, C), reps=r) for M, C, r in REDUCE_CASES])
def test_reduce_exact(M, C, reps, act, layout):
    call, ptr, sp, L = _abi()
    d, sg, sb = R.exact_reduce_ref(M, C, act)
    lay = R.LAYOUTS[layout]
    dyb, zb = buf(M, C, lay["dy"], d["dy"]), buf(M, C, lay["z"], d["z"])
    save, gamma, beta = consts(d)
    sums = Sums(torch.zeros(reps, 2, C, dtype=torch.int64))
    call("bn_act_bwd_reduce", *bwd_args(dyb, zb, save, gamma, beta, sums), M, C, act, reps, sp())
    parts = sums.parts()
    got = parts.sum(0)
    assert torch.equal(got[0], sg), "sum(du zhat) differs on channels %s" % (got[0] != sg).nonzero().flatten().tolist()[:16]
    assert torch.equal(got[1], sb), "sum(du) differs on channels %s" % (got[1] != sb).nonzero().flatten().tolist()[:16]
    grid = R.reduce_grid(M, C)
    assert bool((parts[grid:] == 0).all())                              # workgroup b adds to replica b % reps
    if min(grid, reps) > 1:
        assert bool((parts[1] != 0).any())
    dyb.check(d["dy"], "dy after the reduce")
    zb.check(d["z"], "z after the reduce")
    for v in (save, gamma, beta):
        v.check_guards("constants")


APPLY_CASES = [(M, C, zero, reps) for M, C, zero in R.A_APPLY for reps in R.a_reps(M, C)]


@pytest.mark.parametrize("layout", list(R.LAYOUTS))
@pytest.mark.parametrize("act", [0, 2], ids=["identity", "relu"])
@pytest.mark.parametrize("M,C,zero,reps", APPLY_CASES,
                         ids=[_gid(M, C, apply=R.apply_grid(M, C), acc=R.acc_grid(M, C), reps=r) + ("-zero" if z else "") for M, C, z, r in APPLY_CASES])
def test_apply_and_apply_acc_exact(M, C, zero, reps, act, layout):
    call, ptr, sp, L = _abi()
    sg, sb, d, r = R.apply_case(M, C, act, zero)
    lay = R.LAYOUTS[layout]
    dyb, zb = buf(M, C, lay["dy"], d["dy"]), buf(M, C, lay["z"], d["z"])
    save, gamma, beta = consts(d)
    total = torch.stack([sg, sb])
    parts = R.split_replicas(total, reps, 17)
    want_g = torch.stack([1 + sg.double() / R.FIXG, 1 + sb.double() / R.FIXG])
    for name, fill, want in (("bn_act_bwd_apply", None, r["dz"].to(BF)), ("bn_act_bwd_apply_acc", d["old"], r["two"])):
        sums = Sums(parts)
        grads = vec(torch.ones(2, C))
        dzb = buf(M, C, lay["dz"], fill)
        call(name, *bwd_args(dyb, zb, save, gamma, beta, sums), grads.ptr(0), grads.ptr(C), dzb.ptr(), dzb.ld, M, C, act, reps, sp())
        dzb.check(want, name + " dz")
        grads.check(want_g, name + " gamma_grad / beta_grad")
        assert torch.equal(sums.parts(), parts)
    dyb.check(d["dy"], "dy after the apply")
    zb.check(d["z"], "z after the apply")


@pytest.mark.parametrize("layout", list(R.LAYOUTS))
@pytest.mark.parametrize("entry", ["bn_act_bwd_apply", "bn_act_bwd_apply_acc"])
@pytest.mark.parametrize("M,C", R.A_MARK, ids=["%dx%d" % s for s in R.A_MARK])
def test_nan_marker_in_the_ninth_replica(M, C, entry, layout):
    """EP24_FIXG_MARK in replica 8 of 9, one channel: that channel's gradients and its dz column are NaN, every other channel exact."""
    call, ptr, sp, L = _abi()
    act, reps, bad = 2, 9, C - 3
    sg, sb, d, r = R.apply_case(M, C, act, False)
    lay = R.LAYOUTS[layout]
    dyb, zb = buf(M, C, lay["dy"], d["dy"]), buf(M, C, lay["z"], d["z"])
    save, gamma, beta = consts(d)
    parts = R.split_replicas(torch.stack([sg, sb]), reps, 17)
    parts[8, :, bad] = R.FIXG_MARK
    acc = entry.endswith("acc")
    want = (r["two"] if acc else r["dz"].to(BF)).clone()
    want[:, bad] = float("nan")
    want_g = torch.stack([1 + sg.double() / R.FIXG, 1 + sb.double() / R.FIXG])
    want_g[:, bad] = float("nan")
    sums, grads = Sums(parts), vec(torch.ones(2, C))
    dzb = buf(M, C, lay["dz"], d["old"] if acc else None)
    call(entry, *bwd_args(dyb, zb, save, gamma, beta, sums), grads.ptr(0), grads.ptr(C), dzb.ptr(), dzb.ld, M, C, act, reps, sp())
    dzb.check(want, "dz with a marked channel")
    grads.check(want_g, "gradients with a marked channel")


def _fused(call, sp, L, dyb, zb, save, gamma, beta, lay, M, C, act, reps):
    sums, grads = Sums(torch.zeros(reps, 2, C, dtype=torch.int64)), vec(torch.ones(2, C))
    dzb = buf(M, C, lay["dz"])
    bar = torch.zeros(2, dtype=torch.int32, device=DEV)
    call("bn_act_bwd_fused", *bwd_args(dyb, zb, save, gamma, beta, sums), grads.ptr(0), grads.ptr(C), dzb.ptr(), dzb.ld, M, C, act, reps, ptr_of(bar), sp())
    torch.cuda.synchronize()
    assert bar.tolist() == [R.fused_grid(M, C), 0], "the wait's counter did not reach the grid size"
    assert L.fn["ep24_conv_ring_timeouts"]() == 0
    return sums, grads, dzb


def ptr_of(t):
    return t.data_ptr()


FUSED_CASES = [(M, C, reps) for M, C in R.A_FUSED for reps in R.a_reps(M, C)]


@pytest.mark.parametrize("layout", list(R.LAYOUTS))
@pytest.mark.parametrize("act", [0, 2], ids=["identity", "relu"])
@pytest.mark.parametrize("M,C,reps", FUSED_CASES, ids=[_gid(M, C, grid=R.fused_grid(M, C), reps=r) for M, C, r in FUSED_CASES])
def test_fused_exact(M, C, reps, act, layout):
    """Reduce, grid-wide wait and apply in one launch on the exact draw: the sums it leaves, the gradients and dz bit for bit."""
    call, ptr, sp, L = _abi()
    d, sg, sb = R.exact_reduce_ref(M, C, act)
    d, r = R.exact_apply_ref(M, C, act, sg, sb)
    lay = R.LAYOUTS[layout]
    dyb, zb = buf(M, C, lay["dy"], d["dy"]), buf(M, C, lay["z"], d["z"])
    save, gamma, beta = consts(d)
    sums, grads, dzb = _fused(call, sp, L, dyb, zb, save, gamma, beta, lay, M, C, act, reps)
    assert torch.equal(sums.parts().sum(0), torch.stack([sg, sb]))
    grads.check(torch.stack([1 + sg.double() / R.FIXG, 1 + sb.double() / R.FIXG]), "gamma_grad / beta_grad")
    dzb.check(r["dz"].to(BF), "dz")
    again = _fused(call, sp, L, dyb, zb, save, gamma, beta, lay, M, C, act, reps)
    assert torch.equal(again[2].dev, dzb.dev) and torch.equal(again[1].dev, grads.dev)


@pytest.mark.parametrize("layout", list(R.LAYOUTS))
@pytest.mark.parametrize("act", [0, 2], ids=["identity", "relu"])
@pytest.mark.parametrize("M,C", R.A_FUSED_TOL, ids=[_gid(M, C, grid=R.fused_grid(M, C)) for M, C in R.A_FUSED_TOL])
def test_fused_row_tail(M, C, act, layout):
    """M just above a power of two, grid capped at 256, a partial second row batch, dy with a non-zero mean: 1 / M is not exact, so
    the sums and the gradients are compared bit for bit and dz under part B's bound (no SiLU in it)."""
    call, ptr, sp, L = _abi()
    d, sg, sb = R.exact_reduce_ref(M, C, act)
    r = R.dz_ref(*[d[k] for k in KEYS], sg.double() / R.FIXG, sb.double() / R.FIXG, act)
    lay = R.LAYOUTS[layout]
    reps = 8
    dyb, zb = buf(M, C, lay["dy"], d["dy"]), buf(M, C, lay["z"], d["z"])
    save, gamma, beta = consts(d)
    sums, grads, dzb = _fused(call, sp, L, dyb, zb, save, gamma, beta, lay, M, C, act, reps)
    assert torch.equal(sums.parts().sum(0), torch.stack([sg, sb]))
    grads.check(torch.stack([1 + sg.double() / R.FIXG, 1 + sb.double() / R.FIXG]), "gamma_grad / beta_grad")
    dzb.check_guards("dz")
    q = ratio(dzb.got(), r["dz"], R.tol_dz(r, d["mean"], act))
    report("fused-tail %dx%d act %d %s" % (M, C, act, layout), dz=q)
    assert q <= 1.0
    again = _fused(call, sp, L, dyb, zb, save, gamma, beta, lay, M, C, act, reps)
    assert torch.equal(again[2].dev, dzb.dev) and torch.equal(again[1].dev, grads.dev)


# ---------------------------------------------------------------------------------------------------------------------------
# part B
FWD = R.fwd_cases()


@pytest.mark.parametrize("layout", list(R.LAYOUTS))
@pytest.mark.parametrize("M,C,act,with_res,running,reps", FWD,
                         ids=["%s-%s%s-run%d" % (_gid(c[0], c[1], grid=R.fwd_grid(c[0], c[1]), reps=c[5]), R.ACT_NAMES[c[2]], "-res" if c[3] else "", c[4]) for c in FWD])
def test_forward_against_float64(M, C, act, with_res, running, reps, layout):
    """running: 0 = null running statistics (both counters still count), 1 = statistics and both counters, 2 = statistics, second
    counter null."""
    call, ptr, sp, L = _abi()
    d, r = R.fwd_case_ref(M, C, act, with_res, bool(running))
    lay = R.LAYOUTS[layout]
    zb, yb = buf(M, C, lay["z"], d["z"]), buf(M, C, lay["y"])
    rb = buf(M, C, lay["res"], d["res"]) if with_res else None
    parts = R.split_replicas(torch.stack([d["s1"], d["s2"]]), reps, 23)
    stats = Sums(parts)
    gamma, beta, save = vec(d["gamma"]), vec(d["beta"]), vec(torch.full((2, C), R.SENT))
    rmean, rvar = vec(d["rmean0"]), vec(d["rvar0"])
    nbt = torch.tensor([41, 5, 77], dtype=torch.int64, device=DEV)
    call("bn_act_fwd", zb.ptr(), zb.ld, stats.ptr(0), reps, gamma.ptr(), beta.ptr(), rmean.ptr() if running else None, rvar.ptr() if running else None,
         nbt.data_ptr(), nbt.data_ptr() + 8 if running != 2 else None, save.ptr(), yb.ptr(), yb.ld, rb.ptr() if with_res else None, rb.ld if with_res else 0,
         M, C, R.EPS, R.MOMENTUM, act, sp())
    assert nbt.tolist() == [42, 6 if running != 2 else 5, 77]
    assert torch.equal(stats.parts(), parts)
    yb.check_guards("y")
    zb.check(d["z"], "z after the forward")
    for v in (save, rmean, rvar, gamma, beta):
        v.check_guards("per-channel vectors")
    sv = save.got().reshape(2, C)
    q = dict(mean=ratio(sv[0], r["mean"], R.tol_mean(r).clamp(min=2.0 ** -149)), invstd=ratio(sv[1], r["invstd"], R.tol_invstd(r)))
    tol = R.tol_y(r, d["z"].double(), d["beta"].double(), act)
    q["y"] = ratio(yb.got(), r["y"], tol)
    if act == 1:                                                        # what the SiLU slack is needed for
        q["y_S0"] = ratio(yb.got(), r["y"], R.tol_y(r, d["z"].double(), d["beta"].double(), act, S=0.0))
    if running:
        q["rmean"] = ratio(rmean.got(), r["rmean"], R.tol_rmean(r, d["rmean0"].double()))
        q["rvar"] = ratio(rvar.got(), r["rvar"], R.tol_rvar(r, M, d["rvar0"].double()))
    else:
        rmean.check(d["rmean0"], "running_mean nobody passed")
        rvar.check(d["rvar0"], "running_var nobody passed")
    report("fwd %dx%d %s res%d run%d reps%d %s" % (M, C, R.ACT_NAMES[act], with_res, running, reps, layout), **q)
    assert all(v <= 1.0 for k, v in q.items() if k != "y_S0"), q


BWD = R.b_bwd_cases()


@pytest.mark.parametrize("layout", list(R.LAYOUTS))
@pytest.mark.parametrize("M,C,act,reps", BWD, ids=["%s-%s" % (_gid(c[0], c[1], reduce=R.reduce_grid(c[0], c[1]), apply=R.apply_grid(c[0], c[1]), reps=c[3]),
                                                              R.ACT_NAMES[c[2]]) for c in BWD])
def test_backward_against_float64(M, C, act, reps, layout):
    """SiLU and LeakyReLU: the reduce's sums, then apply and apply_acc on the reference's sums (forged, split over the replicas with
    cancelling parts), then the one-launch form (C <= 2048) on its own sums."""
    call, ptr, sp, L = _abi()
    d, s, r = R.bwd_case_ref(M, C, act)
    a = [d[k].double() for k in KEYS]
    lay = R.LAYOUTS[layout]
    dyb, zb = buf(M, C, lay["dy"], d["dy"]), buf(M, C, lay["z"], d["z"])
    save, gamma, beta = consts(d)
    tg, tb = R.tol_sums(M, s["ag"], act), R.tol_sums(M, s["ab"], act)
    q = {}
    sums = Sums(torch.zeros(reps, 2, C, dtype=torch.int64))
    call("bn_act_bwd_reduce", *bwd_args(dyb, zb, save, gamma, beta, sums), M, C, act, reps, sp())
    got = sums.parts().sum(0).double() / R.FIXG
    q["sg"], q["sb"] = ratio(got[0], s["sg"], tg), ratio(got[1], s["sb"], tb)
    if act == 1:
        q["sg_S0"], q["sb_S0"] = ratio(got[0], s["sg"], R.tol_sums(M, s["ag"], act, S=0.0)), ratio(got[1], s["sb"], R.tol_sums(M, s["ab"], act, S=0.0))
    parts = R.split_replicas(torch.stack([s["sg_fix"], s["sb_fix"]]), reps, 29)
    sgq, sbq = s["sg_fix"].double() / R.FIXG, s["sb_fix"].double() / R.FIXG
    tol = R.tol_dz(r, a[2], act)
    old = d["old"].double()
    for name, fill, want, t in (("bn_act_bwd_apply", None, r["dz"], tol), ("bn_act_bwd_apply_acc", d["old"], r["dz"] + old, R.tol_dz_acc(r, a[2], act, old))):
        fsums, grads = Sums(parts), vec(torch.ones(2, C))
        dzb = buf(M, C, lay["dz"], fill)
        call(name, *bwd_args(dyb, zb, save, gamma, beta, fsums), grads.ptr(0), grads.ptr(C), dzb.ptr(), dzb.ld, M, C, act, reps, sp())
        dzb.check_guards(name + " dz")
        grads.check_guards(name + " gradients")
        gg = grads.got().reshape(2, C)
        key = name[len("bn_act_bwd_"):]
        q[key] = ratio(dzb.got(), want, t)
        q[key + "_gg"], q[key + "_bg"] = ratio(gg[0], 1 + sgq, R.tol_grad(sgq)), ratio(gg[1], 1 + sbq, R.tol_grad(sbq))
        if act == 1:
            q[key + "_S0"] = ratio(dzb.got(), want, R.tol_dz(r, a[2], act, S=0.0) + (t - tol))
    if C <= 2048:
        assert R.fused_grid(M, C) <= 256
        usums, grads, dzb = _fused(call, sp, L, dyb, zb, save, gamma, beta, lay, M, C, act, reps)
        got1 = usums.parts().sum(0).double() / R.FIXG
        dzb.check_guards("one-launch dz")
        gg = grads.got().reshape(2, C)
        q["fused_sg"], q["fused_sb"] = ratio(got1[0], s["sg"], tg), ratio(got1[1], s["sb"], tb)
        q["fused"] = ratio(dzb.got(), r["dz"], tol + R.tol_dz_sums(r, a[2], a[3], tg, tb))
        q["fused_gg"], q["fused_bg"] = ratio(gg[0], 1 + got1[0], R.tol_grad(got1[0])), ratio(gg[1], 1 + got1[1], R.tol_grad(got1[1]))
        again = _fused(call, sp, L, dyb, zb, save, gamma, beta, lay, M, C, act, reps)
        assert torch.equal(again[2].dev, dzb.dev) and torch.equal(again[1].dev, grads.dev)
    dyb.check(d["dy"], "dy after the backward")
    zb.check(d["z"], "z after the backward")
    report("bwd %dx%d %s reps%d %s" % (M, C, R.ACT_NAMES[act], reps, layout), **q)
    assert all(v <= 1.0 for k, v in q.items() if not k.endswith("_S0")), q
