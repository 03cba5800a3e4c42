"""The BatchNorm + activation kernels (csrc/elementwise.hip) where a thread walks MORE THAN TWO batches of its four-row ring.

The three kernels keep four 16-byte rows (chunks, in the forward) per thread in flight and refill a row's registers as soon as the row
is done, so the ring wraps once per batch.  In tests/test_gpu_bn_exact.py no thread of the forward, the reduce or the one-launch form
walks more than two batches, and the apply more only at (4100, 4096) (checked with bn_reference's geometry helpers): the loop that
refills runs at most once there, never after a refill.  These cases run it two and three times: three and four batches, with a partial
last one, on the fixed-group and the moving-group path of the forward, with one and with many rows per block in the backward.  Every
case asserts the batch count and the path it claims through the same helpers.

References, draws, layouts and tolerances are tests/bn_reference.py's, unchanged: part A's exact construction (act 0 and 2; forged zero
sums, so any M is exact) bit for bit, and the float64 formulas under tol_y / tol_dz / tol_sums for SiLU.  The float64 references of the
large shapes are evaluated on the device (the formulas are plain torch).  Every operand and destination sits in a sentinel-filled
buffer and whole buffers are compared.  Each test prints its largest err / tol.

Measured on an MI355X (largest err / tol; 1.0 is the bound, ~0.99 is a bf16 rounding decision on the other side of a tie): forward y
0.963 - 0.996, save mean 0.711, invstd 0.392, running mean 0.362, var 0.276; SiLU apply dz 0.995, apply_acc 0.993, gamma_grad / beta_grad
0.73; SiLU reduce sums 1.3e-6 (the bound of tol_sums grows with M: 1 600 003 rows); the exact cases are bit for bit.
"""
import functools
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bn_reference as R  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BF = torch.bfloat16
ISENT = 0x5A5A5A5A5A5A
KEYS = ("dy", "z", "mean", "invstd", "gamma", "beta")
U = 4                                     # rows (chunks) per batch in all three kernels

FWD_SHAPES = [(4200000, 8, True), (1400000, 24, False)]          # (M, C, fixed group)
APPLY_SHAPES = [(8200, 2048), (270000, 64)]
REDUCE_EXACT = (5003, 2048)
REDUCE_TOL = (1600003, 8)


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


def guards_on_device(b, what):
    """Everything outside the window is the sentinel still (the window is compared under a tolerance by the caller); on the device:
    these buffers have up to 200 M elements."""
    t = b.dev.clone()
    b.window(t)[:] = R.SENT
    bad = int((t != R.SENT).sum())
    assert bad == 0, "%s: %d elements outside the window were written" % (what, bad)


def same_on_device(b, what):
    """The whole buffer is what was uploaded (an input the kernel must not touch)."""
    assert torch.equal(b.dev, b.host.to(DEV)), what


def fwd_batches(M, C):
    chunks = -(-(M * (C >> 3)) // (R.fwd_grid(M, C) * 256))          # of the busiest thread
    return chunks, -(-chunks // U)


def row_batches(M, C, grid):
    """-> rows of the busiest thread (row slot 0 of block 0), its batches, rows of the idlest (the last slot of the last block)."""
    step = grid * R.rpb(C)
    rows = -(-M // step)
    return rows, -(-rows // U), M // step


# ---------------------------------------------------------------------------------------------------------------------------
# forward: 9 chunks per thread = 3 batches, the last with one chunk (or none: the threads past the tail have 8)
@pytest.mark.parametrize("with_res", [False, True], ids=["plain", "res"])
@pytest.mark.parametrize("layout", list(R.LAYOUTS))
@pytest.mark.parametrize("M,C,fixed", FWD_SHAPES, ids=["%dx%d-%s" % (M, C, "fixed" if f else "moving") for M, C, f in FWD_SHAPES])
def test_forward_three_batches(M, C, fixed, layout, with_res):
    call, ptr, sp, L = _abi()
    assert R.fwd_grid(M, C) == 2048 and fwd_batches(M, C) == (9, 3) and R.fwd_fixed_group(M, C) == fixed
    act, reps = 1, 8
    d = R.draw_fwd(M, C)
    lay = R.LAYOUTS[layout]
    zb, yb = buf(M, C, lay["z"], d["z"]), buf(M, C, lay["y"])
    rb = buf(M, C, lay["res"], d["res"]) if with_res else None
    parts = R.split_replicas(torch.stack([d["s1"], d["s2"]]), reps, 23)
    stats = Sums(parts)
    gamma, beta, save = vec(d["gamma"]), vec(d["beta"]), vec(torch.full((2, C), R.SENT))
    rmean, rvar = vec(d["rmean0"]), vec(d["rvar0"])
    nbt = torch.tensor([41, 5, 77], dtype=torch.int64, device=DEV)
    call("bn_act_fwd", zb.ptr(), zb.ld, stats.ptr(0), reps, gamma.ptr(), beta.ptr(), rmean.ptr(), rvar.ptr(), nbt.data_ptr(), nbt.data_ptr() + 8,
         save.ptr(), yb.ptr(), yb.ld, rb.ptr() if with_res else None, rb.ld if with_res else 0, M, C, R.EPS, R.MOMENTUM, act, sp())
    assert nbt.tolist() == [42, 6, 77]
    assert torch.equal(stats.parts(), parts)
    # the float64 reference on the device, from the same fixed-point sums
    dd = lambda t: t.to(DEV).double()
    z64, beta64 = dd(d["z"]), dd(d["beta"])
    r = R.fwd_ref(z64, dd(d["s1"]) / R.FIX, dd(d["s2"]) / R.FIX, dd(d["gamma"]), beta64, act, dd(d["res"]) if with_res else None,
                  dd(d["rmean0"]), dd(d["rvar0"]))
    assert float(r["u"].abs().max()) <= 16                              # what S_SILU covers
    guards_on_device(yb, "y")
    same_on_device(zb, "z after the forward")
    if with_res:
        same_on_device(rb, "the residual after the forward")
    for v in (save, rmean, rvar, gamma, beta):
        v.check_guards("per-channel vectors")
    sv = save.got().reshape(2, C).to(DEV)
    q = dict(mean=ratio(sv[0], r["mean"], R.tol_mean(r).clamp(min=2.0 ** -149)), invstd=ratio(sv[1], r["invstd"], R.tol_invstd(r)),
             y=ratio(yb.window(yb.dev), r["y"], R.tol_y(r, z64, beta64, act)),
             rmean=ratio(rmean.got().to(DEV), r["rmean"], R.tol_rmean(r, dd(d["rmean0"]))),
             rvar=ratio(rvar.got().to(DEV), r["rvar"], R.tol_rvar(r, M, dd(d["rvar0"]))))
    report("pipeline fwd %dx%d %s res%d" % (M, C, layout, with_res), **q)
    assert all(v <= 1.0 for v in q.values()), q


# ---------------------------------------------------------------------------------------------------------------------------
# apply: 16 rows per thread = 4 batches; the threads of the last blocks have 15, a partial last batch
def _apply_geometry(M, C):
    assert R.apply_rows(M, C) == 16
    grid = R.apply_grid(M, C)
    rows, batches, fewest = row_batches(M, C, grid)
    assert (rows, batches, fewest) == (16, 4, 15), (rows, batches, fewest)
    return grid


APPLY_EXACT = [(M, C, act, entry) for M, C in APPLY_SHAPES for act in (0, 2) for entry in ("bn_act_bwd_apply", "bn_act_bwd_apply_acc")
               if entry == "bn_act_bwd_apply" or (M, C) == APPLY_SHAPES[0]]


@pytest.mark.parametrize("layout", list(R.LAYOUTS))
@pytest.mark.parametrize("M,C,act,entry", APPLY_EXACT, ids=["%dx%d-%s-%s" % (M, C, R.ACT_NAMES[a], e[len("bn_act_bwd_"):]) for M, C, a, e in APPLY_EXACT])
def test_apply_four_batches_exact(M, C, act, entry, layout):
    """Part A's construction with forged zero sums (dz = k1 du: exact for any M), bit for bit; gamma_grad / beta_grad = 1 + 0."""
    call, ptr, sp, L = _abi()
    grid = _apply_geometry(M, C)
    if entry.endswith("acc"):
        assert R.acc_grid(M, C) == grid
    if (M, C) == APPLY_SHAPES[0]:
        assert grid == 513 and M - 15 * grid == 505                    # blocks below 505 walk 16 rows, the others 15
    reps = 8
    sg, sb, d, r = R.apply_case(M, C, act, True)
    lay = R.LAYOUTS[layout]
    dyb, zb = buf(M, C, lay["dy"], d["dy"]), buf(M, C, lay["z"], d["z"])
    save, gamma, beta = consts(d)
    parts = R.split_replicas(torch.stack([sg, sb]), reps, 17)
    acc = entry.endswith("acc")
    sums, grads = Sums(parts), vec(torch.ones(2, C))
    dzb = buf(M, C, lay["dz"], d["old"] if acc else None)
    call(entry, *bwd_args(dyb, zb, save, gamma, beta, sums), grads.ptr(0), grads.ptr(C), dzb.ptr(), dzb.ld, M, C, act, reps, sp())
    dzb.check(r["two"] if acc else r["dz"].to(BF), entry + " dz")
    grads.check(torch.ones(2, C), entry + " gamma_grad / beta_grad")
    assert torch.equal(sums.parts(), parts)
    dyb.check(d["dy"], "dy after the apply")
    zb.check(d["z"], "z after the apply")


@functools.lru_cache(maxsize=1)
def _silu_apply_ref(M, C):
    """draw_bwd's operands, the true sums rounded to 2^-36 as the forged input, dz and its tolerance in float64 - on the device."""
    d = R.draw_bwd(M, C, 1)
    a = [d[k].to(DEV).double() for k in KEYS]
    sg, sb, ag, ab = R.bwd_sums(*a, 1)
    sgf, sbf = R.fix_of(sg, R.FIXG), R.fix_of(sb, R.FIXG)
    r = R.dz_ref(*a, sgf.double() / R.FIXG, sbf.double() / R.FIXG, 1)
    assert float(r["u"].abs().max()) <= 16
    big = float(r["dz"].abs().max())                                    # the projection terms are of the size of dz
    assert float(r["k2"].abs().max()) >= 0.05 * big and float((r["k3"] * a[1]).abs().max()) >= 0.05 * big
    old = d["old"].to(DEV).double()
    return d, sgf.cpu(), sbf.cpu(), r, R.tol_dz(r, a[2], 1), old, R.tol_dz_acc(r, a[2], 1, old)


def split_large(total, reps, seed):
    """bn_reference.split_replicas for sums beyond its 2^50 (270 000 rows of O(1) terms are ~2^54 in 2^-36 fixed point): [reps, ...] int64
    parts that sum to `total` exactly, all but the last random below 2^46, every part inside the kernels' +-2^56 range of a replica."""
    g = torch.Generator().manual_seed(seed)
    parts = torch.randint(-(1 << 46), 1 << 46, (reps,) + tuple(total.shape), generator=g, dtype=torch.int64)
    parts[reps - 1] = total - parts[:reps - 1].sum(0)
    assert bool((parts.sum(0) == total).all()) and int(parts.abs().max()) < (1 << 56)
    return parts


APPLY_SILU = [(M, C, entry) for M, C in APPLY_SHAPES for entry in ("bn_act_bwd_apply", "bn_act_bwd_apply_acc")
              if entry == "bn_act_bwd_apply" or (M, C) == APPLY_SHAPES[0]]


@pytest.mark.parametrize("layout", list(R.LAYOUTS))
@pytest.mark.parametrize("M,C,entry", APPLY_SILU, ids=["%dx%d-silu-%s" % (M, C, e[len("bn_act_bwd_"):]) for M, C, e in APPLY_SILU])
def test_apply_four_batches_silu(M, C, entry, layout):
    call, ptr, sp, L = _abi()
    _apply_geometry(M, C)
    act, reps = 1, 8
    d, sgf, sbf, r, tol, old, tol_acc = _silu_apply_ref(M, C)
    lay = R.LAYOUTS[layout]
    dyb, zb = buf(M, C, lay["dy"], d["dy"]), buf(M, C, lay["z"], d["z"])
    save, gamma, beta = consts(d)
    parts = split_large(torch.stack([sgf, sbf]), reps, 29)
    acc = entry.endswith("acc")
    sums, grads = Sums(parts), vec(torch.ones(2, C))
    dzb = buf(M, C, lay["dz"], d["old"] if acc else None)
    call(entry, *bwd_args(dyb, zb, save, gamma, beta, sums), grads.ptr(0), grads.ptr(C), dzb.ptr(), dzb.ld, M, C, act, reps, sp())
    guards_on_device(dzb, entry + " dz")
    grads.check_guards(entry + " gradients")
    gg = grads.got().reshape(2, C).double()
    sgq, sbq = sgf.double() / R.FIXG, sbf.double() / R.FIXG
    q = dict(dz=ratio(dzb.window(dzb.dev), r["dz"] + old if acc else r["dz"], tol_acc if acc else tol),
             gg=ratio(gg[0], 1 + sgq, R.tol_grad(sgq)), bg=ratio(gg[1], 1 + sbq, R.tol_grad(sbq)))
    assert torch.equal(sums.parts(), parts)
    same_on_device(dyb, "dy after the apply")
    same_on_device(zb, "z after the apply")
    report("pipeline %s %dx%d silu %s" % (entry[len("bn_act_bwd_"):], M, C, layout), **q)
    assert all(v <= 1.0 for v in q.values()), q


# ---------------------------------------------------------------------------------------------------------------------------
# reduce
@pytest.mark.parametrize("layout", list(R.LAYOUTS))
@pytest.mark.parametrize("act", [0, 2], ids=["identity", "relu"])
def test_reduce_three_batches_exact(act, layout):
    """(5003, 2048): grid 512 (capped), 10 rows per thread in blocks below 395 and 9 above: 3 batches, the last with 2 rows or 1.  Part
    A's construction: every fp32 partial sum is exact in any order (asserted on the reference), so the sums have one right answer."""
    call, ptr, sp, L = _abi()
    M, C = REDUCE_EXACT
    reps = 8
    grid = R.reduce_grid(M, C)
    assert grid == 512 and row_batches(M, C, grid) == (10, 3, 9) and M - 9 * grid == 395
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
    assert bool((parts != 0).any(-1).any(-1).all())                    # every replica took its workgroups' sums
    dyb.check(d["dy"], "dy after the reduce")
    zb.check(d["z"], "z after the reduce")
    for v in (save, gamma, beta):
        v.check_guards("constants")


@pytest.mark.parametrize("layout", list(R.LAYOUTS))
def test_reduce_four_batches_silu(layout):
    """(1600003, 8): 256 rows per block, grid 512 (capped), 13 rows per thread for the first rows' slots and 12 for the rest: 4 batches,
    the last with one row or none.  SiLU under tol_sums."""
    call, ptr, sp, L = _abi()
    M, C = REDUCE_TOL
    act, reps = 1, 8
    grid = R.reduce_grid(M, C)
    assert grid == 512 and R.rpb(C) == 256 and row_batches(M, C, grid) == (13, 4, 12)
    d = R.draw_bwd(M, C, act)
    a = [d[k].to(DEV).double() for k in KEYS]
    sg, sb, ag, ab = [t.cpu() for t in R.bwd_sums(*a, act)]
    lay = R.LAYOUTS[layout]
    dyb, zb = buf(M, C, lay["dy"], d["dy"]), buf(M, C, lay["z"], d["z"])
    save, gamma, beta = consts(d)
    sums = Sums(torch.zeros(reps, 2, C, dtype=torch.int64))
    call("bn_act_bwd_reduce", *bwd_args(dyb, zb, save, gamma, beta, sums), M, C, act, reps, sp())
    parts = sums.parts()
    got = parts.sum(0).double() / R.FIXG
    q = dict(sg=ratio(got[0], sg, R.tol_sums(M, ag, act)), sb=ratio(got[1], sb, R.tol_sums(M, ab, act)))
    assert bool((parts != 0).any(-1).any(-1).all())
    same_on_device(dyb, "dy after the reduce")
    same_on_device(zb, "z after the reduce")
    for v in (save, gamma, beta):
        v.check_guards("constants")
    report("pipeline reduce %dx%d silu %s" % (M, C, layout), **q)
    assert all(v <= 1.0 for v in q.values()), q
