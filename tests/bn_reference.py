"""Float64 references, draws, layouts and tolerances of the BatchNorm + activation kernels (ep24_bn_act_fwd, _bwd_reduce, _bwd_apply,
_bwd_apply_acc, _bwd_fused).  A helper, not a test module: tests/test_bn_reference.py checks it on the CPU (the formulas against
float64 autograd, every precondition of every GPU case, every tolerance against a float32 emulation and against mutants), and
tests/test_gpu_bn_exact.py runs the kernels against it.  It never imports the package under test.

The kernels' input contract (include/ep24.h): the forward takes the batch statistics as [reps][2][C] int64 sums of z and z * z in
2^-20 fixed point; the backward takes save = (mean, invstd) and gives / takes [reps][2][C] int64 sums of du * zhat and du in 2^-36
fixed point.  Per channel:
    mean = s1 / M, var = max(s2 / M - mean^2, 0), invstd = 1 / sqrt(var + eps), sc = gamma * invstd, sh = beta - mean * sc
    y  = act(z * sc + sh) (+ residual)
    du = dy * act'(z * sc + sh), zhat = (z - mean) * invstd, sg = sum(du * zhat), sb = sum(du)
    dz = k1 * du - k2 - k3 * z,  k1 = sc, k3 = k1 * invstd * sg / M, k2 = k1 * sb / M - k3 * mean
act: 0 identity, 1 SiLU, 2 ReLU (derivative 0 at u <= 0), 3 LeakyReLU(0.1) (derivative 0.1 at u <= 0).
"""
import functools

import numpy as np
import torch

BF = torch.bfloat16
F64 = torch.float64
SENT = -7.0                      # finite, exact in bf16 and fp32
GUARD = 3                        # rows before the first and after the last row of every [M, C] operand
VGUARD = 8                       # floats before and after every per-channel fp32 vector (keeps its 16-byte alignment)
FIX = 2.0 ** 20                  # forward statistics
FIXG = 2.0 ** 36                 # backward sums
FIXG_MARK = 1 << 57              # EP24_FIXG_MARK: "this partial sum was NaN or out of range"
EPS, MOMENTUM = float(np.float32(1e-3)), float(np.float32(0.03))       # the float arguments as the kernels receive them
ACT_NAMES = {0: "identity", 1: "silu", 2: "relu", 3: "leaky"}
S_SILU = 2.0 ** -18              # relative slack of the SiLU's v_exp_f32 + v_rcp_f32 (the GPU module's docstring has the measurement)


# ---------------------------------------------------------------------------------------------------------------------------
# launch geometry, as csrc/elementwise.hip derives it (only for the parametrize ids and the "this shape reaches that path" asserts)
def rows_grid(M, C, rows_per_thread, max_blocks, nt=256):
    tpr = C >> 3
    rpb = 1 if tpr >= nt else nt // tpr
    return max(1, min(max_blocks, -(-M // (rpb * rows_per_thread))))


def rpb(C, nt=256):
    return 1 if (C >> 3) >= nt else nt // (C >> 3)


def flat_grid(M, C, per_thread):
    return max(1, min(2048, -(-(M * (C >> 3)) // (256 * per_thread))))


def fwd_per(M, C):
    return 8 if (C >= 1024 or (C <= 128 and M * C >= (12 << 20))) else 4


def fwd_grid(M, C):
    return flat_grid(M, C, fwd_per(M, C))


def fwd_fixed_group(M, C):
    return (fwd_grid(M, C) * 256) % (C >> 3) == 0


def reduce_grid(M, C):
    return rows_grid(M, C, 4, 512)


def fused_grid(M, C):
    return rows_grid(M, C, 4, 256)


def apply_rows(M, C):
    return 8 if M * C <= (16 << 20) else 16


def apply_grid(M, C):
    return rows_grid(M, C, apply_rows(M, C), 2048)


def acc_grid(M, C):
    return rows_grid(M, C, 16, 2048)


# ---------------------------------------------------------------------------------------------------------------------------
# layouts: (ld - C, channel offset) per operand; every operand of the slice layout has its own stride and its own offset
LAYOUTS = {
    "dense": dict(z=(0, 0), y=(0, 0), res=(0, 0), dy=(0, 0), dz=(0, 0)),
    "slice": dict(z=(24, 8), y=(40, 16), res=(56, 24), dy=(40, 24), dz=(56, 16)),
}


class Buf:
    """A [GUARD + M + GUARD, ld] buffer full of the sentinel with a [M, C] window at channel offset `off`; `dev` is where the kernels
    see it."""

    def __init__(self, M, C, extra_ld, off, dev="cpu", dtype=BF, fill=None):
        self.M, self.C, self.ld, self.off = M, C, C + extra_ld, off
        self.host = torch.full((M + 2 * GUARD, self.ld), SENT, dtype=dtype)
        if fill is not None:
            self.window(self.host)[:] = fill.to(dtype)
        self.dev = self.host.to(dev)

    def window(self, t):
        return t[GUARD:GUARD + self.M, self.off:self.off + self.C]

    def ptr(self):
        return self.dev.data_ptr() + (GUARD * self.ld + self.off) * self.dev.element_size()

    def got(self):
        return self.window(self.dev.cpu())

    def check(self, want, what):
        """The whole buffer bit for bit (NaN equals NaN): `want` inside the window, what the buffer held everywhere else."""
        exp = self.host.clone()
        self.window(exp)[:] = want.to(exp.dtype)
        assert_same(self.dev.cpu(), exp, what, self)

    def check_guards(self, what):
        """Everything outside the window is as it was (the window is compared under a tolerance by the caller)."""
        exp = self.host.clone()
        got = self.dev.cpu()
        self.window(exp)[:] = self.window(got)
        assert_same(got, exp, what + " (outside the window)", self)


def assert_same(got, exp, what, buf=None):
    same = (got == exp) | (torch.isnan(got) & torch.isnan(exp))
    if bool(same.all()):
        return
    bad = (~same).nonzero()
    where = ""
    if buf is not None:
        inside = ((bad[:, 0] >= GUARD) & (bad[:, 0] < GUARD + buf.M) & (bad[:, 1] >= buf.off) & (bad[:, 1] < buf.off + buf.C)).sum().item()
        where = " (%d inside the window, %d outside; window row %d, channel %d)" % (inside, len(bad) - inside, bad[0, 0] - GUARD, bad[0, 1] - buf.off)
    i = tuple(bad[0].tolist())
    raise AssertionError("%s: %d of %d elements differ%s; first at %s: got %s, want %s" % (what, len(bad), got.numel(), where, list(i), got[i].item(), exp[i].item()))


class Vec:
    """[n, C] fp32 per-channel vectors with VGUARD sentinel floats before and after."""

    def __init__(self, fill, dev="cpu"):
        fill = fill.float().reshape(-1)
        self.n = fill.numel()
        self.host = torch.full((self.n + 2 * VGUARD,), SENT, dtype=torch.float32)
        self.host[VGUARD:VGUARD + self.n] = fill
        self.dev = self.host.to(dev)

    def ptr(self, offset=0):
        return self.dev.data_ptr() + (VGUARD + offset) * 4

    def got(self):
        return self.dev.cpu()[VGUARD:VGUARD + self.n]

    def check(self, want, what):
        exp = self.host.clone()
        exp[VGUARD:VGUARD + self.n] = want.float().reshape(-1)
        assert_same(self.dev.cpu(), exp, what)

    def check_guards(self, what):
        got = self.dev.cpu()
        exp = self.host.clone()
        exp[VGUARD:VGUARD + self.n] = got[VGUARD:VGUARD + self.n]
        assert_same(got, exp, what + " (guards)")


# ---------------------------------------------------------------------------------------------------------------------------
# float64 formulas
def act_f(u, act):
    if act == 1:
        return u * torch.sigmoid(u)
    if act == 2:
        return u.clamp(min=0)
    if act == 3:
        return torch.where(u > 0, u, 0.1 * u)
    return u


def act_g(u, act, mutant=None):
    if act == 1:
        s = torch.sigmoid(u)
        return s * (1 + u * (1 - s))
    if act == 2:
        return (u > 0).to(u.dtype)
    if act == 3 and mutant != "leaky_as_identity":
        return torch.where(u > 0, torch.ones_like(u), torch.full_like(u, 0.1))
    return torch.ones_like(u)


def fix_of(v, scale):
    """Real sums -> the int64 fixed-point word a kernel holds."""
    return (v.double() * scale).round().long()


def split_replicas(total, reps, seed):
    """[...] int64 -> [reps, ...] int64 parts that sum to it exactly, every part but the last a large random number (|part| < 2^50)
    - so a fold that drops, repeats or reorders a replica is off by ~2^45 units, and every replica (the last one too) is non-zero."""
    g = torch.Generator().manual_seed(seed)
    parts = torch.randint(-(1 << 46), 1 << 46, (reps,) + tuple(total.shape), generator=g, dtype=torch.int64)
    parts[reps - 1] = total - parts[:reps - 1].sum(0)
    assert bool((parts.sum(0) == total).all()) and int(parts.abs().max()) < (1 << 50)
    return parts


def fold(parts, mutant=None):
    """The exact integer fold of the replicas; two wrong folds of the kernels' 8-at-a-time batches as mutants."""
    if mutant == "reps_beyond_8":
        return parts[:8].sum(0)
    if mutant == "clamped_duplicate" and parts.shape[0] > 8 and parts.shape[0] % 8:
        return parts.sum(0) + (8 - parts.shape[0] % 8) * parts[parts.shape[0] // 8 * 8]
    return parts.sum(0)


def fwd_stats(s1, s2, M, eps=EPS):
    """Real sums of z and z * z (float64, [C]) -> mean, biased variance (clamped), invstd, unbiased variance."""
    mean = s1 / M
    var = (s2 / M - mean * mean).clamp(min=0)
    return mean, var, 1 / torch.sqrt(var + eps), (var * M / (M - 1) if M > 1 else var)


def fwd_ref(z, s1, s2, gamma, beta, act, res=None, rmean=None, rvar=None, eps=EPS, momentum=MOMENTUM):
    """The forward from the SUMS (the kernel never looks at z for its statistics).  All float64."""
    M = z.shape[0]
    mean, var, inv, unb = fwd_stats(s1, s2, M, eps)
    sc = gamma * inv
    u = z * sc + (beta - mean * sc)
    a = act_f(u, act)
    r = dict(mean=mean, var=var, invstd=inv, sc=sc, u=u, a=a, y=a + res if res is not None else a, ez2=s2 / M)
    if rmean is not None:
        r["rmean"] = (1 - momentum) * rmean + momentum * mean
        r["rvar"] = (1 - momentum) * rvar + momentum * unb
    return r


def bwd_terms(dy, z, mean, inv, gamma, beta, act, mutant=None):
    sc = gamma * inv
    u = z * sc + (beta - mean * sc)
    du = dy * act_g(u, act, mutant)
    zhat = (z - mean) * inv
    return u, du, zhat


def bwd_sums(dy, z, mean, inv, gamma, beta, act, mutant=None):
    """-> sg = sum(du * zhat), sb = sum(du) and the sums of the terms' magnitudes (for the tolerance)."""
    u, du, zhat = bwd_terms(dy, z, mean, inv, gamma, beta, act, mutant)
    t = du * zhat
    if mutant == "last_row":
        return t[:-1].sum(0), du[:-1].sum(0), t.abs().sum(0), du.abs().sum(0)
    return t.sum(0), du.sum(0), t.abs().sum(0), du.abs().sum(0)


def dz_ref(dy, z, mean, inv, gamma, beta, sg, sb, act, mutant=None):
    """-> dict(dz, and the pieces the preconditions and tolerances need)."""
    M = z.shape[0]
    u, du, zhat = bwd_terms(dy, z, mean, inv, gamma, beta, act, mutant)
    k1 = gamma * inv
    k3 = k1 * inv * (sg / M)
    k2a, k2b = k1 * (sb / M), k3 * mean
    k2 = k2a - k2b
    if mutant == "no_projection":
        k2, k3 = torch.zeros_like(k2), torch.zeros_like(k3)
    if mutant == "k2_sign":
        k2 = -k2
    inner = k1 * du - k2
    dz = inner - k3 * z
    return dict(dz=dz, u=u, du=du, k1=k1, k2=k2, k3=k3, k2a=k2a, k2b=k2b, inner=inner, dy=dy, z=z)


def two_roundings(o, old):
    return (o.to(BF).double() + old).to(BF)


def one_rounding(o, old):
    return (o + old).to(BF)


def is_f32(t):
    return bool((t.float().double() == t).all())


# ---------------------------------------------------------------------------------------------------------------------------
# tolerances (all against float64; e = 2^-24 is the unit roundoff of fp32)
def eps_c(r, eps=EPS):
    """Relative error bound of invstd per channel.  var = s2/M - mean^2 in fp32: from_fix, the division, the square and the
    subtraction each round at the size of E[z^2] (<= 4 e E[z^2] in all), and invstd = (var + eps)^-1/2 halves the relative error of
    var + eps and adds the rsqrt's own (2 e): <= 2^-22 + 2^-22 E[z^2] / (var + eps) with room."""
    return 2.0 ** -22 + 2.0 ** -22 * r["ez2"] / (r["var"] + eps)


def tol_mean(r):
    return 2.0 ** -23 * r["mean"].abs()


def tol_invstd(r):
    return eps_c(r) * r["invstd"]


def tol_rmean(r, rmean0, momentum=MOMENTUM):
    # the blend rounds 1 - momentum, two products and their sum in fp32: at most 4 e of the two products' magnitudes
    return momentum * tol_mean(r) + 2.0 ** -22 * ((1 - momentum) * rmean0.abs() + momentum * r["mean"].abs()) + 2.0 ** -149


def tol_rvar(r, M, rvar0, momentum=MOMENTUM, eps=EPS):
    # relative error of var + eps is 2 eps_c (invstd's, doubled); of var itself at most (var + eps) / var times that
    unb = r["var"] * (M / (M - 1) if M > 1 else 1)
    return momentum * (2 * eps_c(r) * (r["var"] + eps) * (M / (M - 1) if M > 1 else 1) + 2.0 ** -22 * unb) + 2.0 ** -22 * ((1 - momentum) * rvar0.abs() + momentum * unb)


def tol_y(r, z, beta, act, S=S_SILU):
    """|y - y64| <= 2^-8 |y64| + 1.1 (eps_c + 2^-22)(|z sc| + |mean sc|) + 2^-23 |beta| + S |act(u)|.  One bf16 rounding (half an ulp
    is 2^-9 relative at the worst; 2^-8 leaves room for the fp32 roundings behind it), the error of sc (eps_c plus the product's e)
    carried through u = z sc + (beta - mean sc) (every activation is 1-Lipschitz up to SiLU's 1.1), and for SiLU the hardware
    exp / rcp."""
    sc = r["sc"].abs()
    return 2.0 ** -8 * r["y"].abs() + 1.1 * (eps_c(r) + 2.0 ** -22) * (z.abs() * sc + r["mean"].abs() * sc) + 2.0 ** -23 * beta.abs() + (S if act == 1 else 0.0) * r["a"].abs()


def tol_sums(M, abs_terms, act, S=S_SILU):
    """|sum - sum64| <= (M 2^-24 + S) sum|terms| + M 2^-37: sound for any order of the fp32 additions (at most M - 1 of them touch a
    term, each e relative), the few roundings inside a term (sc, sh, u, zhat, the product: a handful of e, below the first M e),
    SiLU's derivative from the hardware exp / rcp, and one rounding to 2^-36 fixed point per workgroup (at most M workgroups)."""
    return (M * 2.0 ** -24 + (S if act == 1 else 0.0)) * abs_terms + M * 2.0 ** -37


def tol_dz(d, mean, act, S=S_SILU):
    """|dz - dz64| <= 2^-8 |dz64| + 2^-21 (|k1 du| + |k1 sb/M| + |k3 mean| + |k3 z|) + dact |k1 dy|: the bf16 rounding as for y; each of the
    four fp32 pieces is a product of at most four rounded factors followed by at most two fma roundings (<= 8 e = 2^-21); and du = dy
    act'(u) carries act' = s (1 + u (1 - s)) from the hardware sigmoid (relative S on s, twice, and |u| times it) and from u's own fp32
    error (|act''| <= 1/2, |delta u| <= 2^-22 (|z sc| + |mean sc| + |beta|), folded into S (1 + |u|) for |u| <= 16)."""
    dact = 4 * S * (1 + d["u"].abs()) if act == 1 else 0.0
    return (2.0 ** -8 * d["dz"].abs() + 2.0 ** -21 * ((d["k1"] * d["du"]).abs() + d["k2a"].abs() + d["k2b"].abs() + (d["k3"] * d["z"]).abs())
            + dact * (d["k1"] * d["dy"]).abs())


def tol_dz_sums(d, mean, inv, tg, tb):
    """What an error of the two sums (at most tg, tb: tol_sums) moves dz by, through k2 and k3: the one-launch form applies the sums
    its own first pass added."""
    M = d["z"].shape[0]
    k1 = d["k1"].abs()
    return k1 / M * (tb + (mean * inv).abs() * tg) + k1 * inv.abs() / M * tg * d["z"].abs()


def tol_grad(s):
    """gamma_grad / beta_grad = 1 + sum: the sum decoded to fp32 (e |sum|) and one fp32 addition (e |1 + sum|)."""
    return 2.0 ** -23 * (1 + s.abs())


def tol_dz_acc(d, mean, act, old, S=S_SILU):
    """The accumulate form rounds o to bf16, adds old in fp32 and rounds again: 2^-8 of o and 2^-8 of the sum."""
    return tol_dz(d, mean, act, S) + 2.0 ** -8 * (d["dz"] + old).abs()


# ---------------------------------------------------------------------------------------------------------------------------
# draws
def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _choice(vals, n, g):
    v = torch.tensor(vals, dtype=F64)
    return v[torch.randint(0, len(vals), (n,), generator=g)]


@functools.lru_cache(maxsize=None)
def draw_exact(M, C, seed=1):
    """Part A: operands and constants with which every intermediate of the backward is an exact dyadic number in fp32.  dy has a
    per-channel offset (a non-zero mean: the projection terms are as large as the rest).  Shared, never written."""
    g = _gen(seed * 1000003 + M * 131 + C)
    z = torch.randint(-16, 17, (M, C), generator=g).double() / 4
    shift = torch.randint(-6, 7, (C,), generator=g)
    dy = (torch.randint(-16, 17, (M, C), generator=g) + shift).clamp(-16, 16).double() / 8
    return dict(z=z, dy=dy, mean=_choice([0, .25, -.25, .5, -.5, 1, -1], C, g), invstd=_choice([.5, 1, 2], C, g),
                gamma=_choice([-1, .5, 1, 2], C, g), beta=_choice([-.5, 0, .25, 1], C, g),
                old=torch.randint(-64, 65, (M, C), generator=g).double() / 8,
                kg=torch.randint(-64, 65, (C,), generator=g), kb=torch.randint(-64, 65, (C,), generator=g))


def exact_reduce_ref(M, C, act):
    """-> draw, the two sums as 2^-36 integers, after asserting that they are exact in fp32 in ANY order."""
    d = draw_exact(M, C)
    sg, sb, ag, ab = bwd_sums(d["dy"], d["z"], d["mean"], d["invstd"], d["gamma"], d["beta"], act)
    assert float(ag.max()) * 2 ** 7 < 2 ** 24 and float(ab.max()) * 2 ** 3 < 2 ** 24
    u, du, zhat = bwd_terms(d["dy"], d["z"], d["mean"], d["invstd"], d["gamma"], d["beta"], act)
    assert bool(((du * zhat * 64).round() == du * zhat * 64).all()) and bool(((du * 8).round() == du * 8).all())
    for t in (u, zhat, d["gamma"] * d["invstd"], d["beta"] - d["mean"] * d["gamma"] * d["invstd"], d["mean"] * d["invstd"]):
        assert is_f32(t)
    assert bool((u == 0).any()), "no row with u == 0"
    return d, fix_of(sg, FIXG), fix_of(sb, FIXG)


def forged_sums(M, C, zero):
    """Part A apply: sums that are multiples of M / 64 with |sum| <= M (0 where M is no power of two) as 2^-36 integers."""
    d = draw_exact(M, C)
    if zero:
        return torch.zeros(C, dtype=torch.int64), torch.zeros(C, dtype=torch.int64)
    assert M & (M - 1) == 0
    return d["kg"] * M * (1 << 30), d["kb"] * M * (1 << 30)


@functools.lru_cache(maxsize=1)
def apply_case(M, C, act, zero):
    """Forged sums and their exact reference, kept for the next layout of the same case."""
    sg, sb = forged_sums(M, C, zero)
    return (sg, sb) + exact_apply_ref(M, C, act, sg, sb, need_projection=not zero)


def exact_apply_ref(M, C, act, sg_fix, sb_fix, need_projection=True):
    """-> draw, d (dz_ref's dict) with the sums given as 2^-36 integers; asserts that every fp32 intermediate of the kernel is
    representable (so bf16(float64 formula) is the one right answer) and that the case discriminates."""
    d = draw_exact(M, C)
    sg, sb = sg_fix.double() / FIXG, sb_fix.double() / FIXG
    r = dz_ref(d["dy"], d["z"], d["mean"], d["invstd"], d["gamma"], d["beta"], sg, sb, act)
    assert is_f32(sg) and is_f32(sb) and is_f32(1 + sg) and is_f32(1 + sb)
    k3a = r["k1"] * d["invstd"]
    for t in (sg / M, sb / M, r["k1"], k3a, r["k3"], r["k2a"], r["k2b"], r["k2"], r["k1"] * r["du"], r["inner"], r["k3"] * d["z"], r["dz"]):
        assert is_f32(t)
    r["frac_rounded"] = float((r["dz"].to(BF).double() != r["dz"]).double().mean())
    r["two"], r["one"] = two_roundings(r["dz"], d["old"]), one_rounding(r["dz"], d["old"])
    r["frac_forms"] = float((r["two"] != r["one"]).double().mean())
    if need_projection:
        assert r["frac_rounded"] >= 0.01, r["frac_rounded"]
        assert r["frac_forms"] >= 0.01, r["frac_forms"]
        assert float((r["k2"] != 0).double().mean()) >= 0.8 and float((r["k3"] != 0).double().mean()) >= 0.8
    return d, r


@functools.lru_cache(maxsize=4)
def draw_fwd(M, C, seed=2):
    """Part B forward: bf16 z with a per-channel mean / std ratio of up to 8 (|u| <= 16 is asserted by the caller), channel 3 constant, a
    residual, float32 constants; the statistics are the true sums of z rounded to 2^-20 - except the constant channel's second sum,
    forged 3 units BELOW M v^2: E[z^2] - mean^2 is negative before the clamp."""
    g = _gen(seed * 1000003 + M * 131 + C)
    std = 0.25 + 1.75 * torch.rand(C, generator=g)
    ch = torch.arange(C)
    ratio = (1.0 + (ch * 3) % 8) * (1 - 2 * ((ch // 8) % 2))           # 1 .. 8 within every 8 channels, both signs where C > 8
    z = (torch.randn(M, C, generator=g) * std + ratio * std)
    if M == 1:                       # one row: var = 0 whatever z is, and the bound of y grows with z^2 / eps - keep |z| <= 2
        z = z / 8
    z = z.to(BF)
    cc = 3
    z[:, cc] = 1.75
    res = torch.randn(M, C, generator=g).to(BF)
    gamma = ((torch.rand(C, generator=g) + 0.5) * (torch.randint(0, 2, (C,), generator=g) * 2 - 1)).float()
    beta = (torch.rand(C, generator=g) - 0.5).float()
    rmean0, rvar0 = torch.randn(C, generator=g).float(), (torch.rand(C, generator=g) + 0.5).float()
    zd = z.double()
    s1, s2 = fix_of(zd.sum(0), FIX), fix_of((zd * zd).sum(0), FIX)
    s2[cc] = int(round(M * 1.75 * 1.75 * FIX)) - 3
    return dict(z=z, res=res, gamma=gamma, beta=beta, rmean0=rmean0, rvar0=rvar0, s1=s1, s2=s2, const_channel=cc)


@functools.lru_cache(maxsize=1)
def fwd_case_ref(M, C, act, with_res, with_running=True):
    d = draw_fwd(M, C)
    r = fwd_ref(d["z"].double(), d["s1"].double() / FIX, d["s2"].double() / FIX, d["gamma"].double(), d["beta"].double(), act,
                d["res"].double() if with_res else None, d["rmean0"].double() if with_running else None, d["rvar0"].double() if with_running else None)
    cc = d["const_channel"]
    assert float(d["s2"][cc]) / FIX / M - (float(d["s1"][cc]) / FIX / M) ** 2 < 0 and float(r["var"][cc]) == 0.0
    if M > 1:
        ratio = (r["mean"].abs() / r["var"].sqrt().clamp(min=1e-30))
        ratio[cc] = 0
        assert 4 <= float(ratio.max()) <= 12, float(ratio.max())
    assert float(r["u"].abs().max()) <= 16 or act != 1 or M == 1, float(r["u"].abs().max())
    return d, r


@functools.lru_cache(maxsize=None)
def draw_bwd(M, C, act, seed=3):
    """Part B backward (act 1, 3): bf16 z and dy, float32 save / gamma / beta as the kernels get them.  dy = noise + a per-channel
    offset + a per-channel multiple of zhat: sb / M and sg / M are O(1), so |k2| and |k3 z| are of the size of dz.  For LeakyReLU no u may
    sit where the fp32 rounding of u decides its sign: such z move by 1/2."""
    g = _gen(seed * 1000003 + M * 131 + C + act)
    mean = (torch.randn(C, generator=g)).float()
    inv = (0.5 + 1.5 * torch.rand(C, generator=g)).float()
    gamma = ((torch.rand(C, generator=g) + 0.5) * (torch.randint(0, 2, (C,), generator=g) * 2 - 1)).float()
    beta = (torch.rand(C, generator=g) - 0.5).float()
    z = (torch.randn(M, C, generator=g) / inv + mean).to(BF)
    sc = gamma.double() * inv.double()
    sh = beta.double() - mean.double() * sc
    for _ in range(8):
        zd = z.double()
        near = (zd * sc + sh).abs() <= 2.0 ** -18 * ((zd * sc).abs() + sh.abs() + 1e-30)
        if act != 3 or not bool(near.any()):
            break
        z = torch.where(near, (zd + 0.5).to(BF), z)
    zhat = (z.double() - mean.double()) * inv.double()
    off = 0.5 + torch.rand(C, generator=g)
    along = (0.5 + torch.rand(C, generator=g)) * (torch.randint(0, 2, (C,), generator=g) * 2 - 1)
    dy = (torch.randn(M, C, generator=g) + off + along * zhat).to(BF)
    old = torch.randn(M, C, generator=g).to(BF)
    return dict(z=z, dy=dy, mean=mean, invstd=inv, gamma=gamma, beta=beta, old=old)


@functools.lru_cache(maxsize=2)
def bwd_case_ref(M, C, act, mutant=None):
    """-> draw, true sums (float64), their tolerance terms, dz from the FORGED sums (the true ones rounded to 2^-36)."""
    d = draw_bwd(M, C, act)
    a = [d[k].double() for k in ("dy", "z", "mean", "invstd", "gamma", "beta")]
    sg, sb, ag, ab = bwd_sums(*a, act)
    sgf, sbf = fix_of(sg, FIXG), fix_of(sb, FIXG)
    r = dz_ref(*a, sgf.double() / FIXG, sbf.double() / FIXG, act, mutant)
    if mutant is None:
        u = r["u"]
        assert float(u.abs().max()) <= 16, float(u.abs().max())
        if act == 3:
            assert bool((u.abs() > 2.0 ** -18 * ((a[1] * r["k1"]).abs() + (a[5] - a[2] * r["k1"]).abs())).all())
        big = float(r["dz"].abs().max())
        assert float(r["k2"].abs().max()) >= 0.05 * big and float((r["k3"] * a[1]).abs().max()) >= 0.05 * big
        # ... and not only in one channel: in most of them, against the channel's own dz
        bigc = r["dz"].abs().amax(0)
        assert float((r["k2"].abs() >= 0.05 * bigc).double().mean()) >= 0.5 and float(((r["k3"] * a[1]).abs().amax(0) >= 0.05 * bigc).double().mean()) >= 0.5
    return d, dict(sg=sg, sb=sb, ag=ag, ab=ab, sg_fix=sgf, sb_fix=sbf), r


# ---------------------------------------------------------------------------------------------------------------------------
# float32 emulation of the kernels' expressions (numpy; fmaf through a float64 product: exact, then one rounding)
f32 = np.float32


def _fma(a, b, c):
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(f32)


def _sigmoid32(x):
    # 1 / (1 + exp(-x)) with exp as exp2(x * log2(e)) in fp32, as __expf lowers
    e = np.exp2((-x * f32(1.4426950408889634)).astype(f32)).astype(f32)
    return (f32(1) / (f32(1) + e)).astype(f32)


def _act32(u, act):
    if act == 1:
        return (u * _sigmoid32(u)).astype(f32)
    if act == 3:
        return np.where(u > 0, u, (f32(0.1) * u).astype(f32))
    return np.maximum(u, f32(0)) if act == 2 else u


def _actg32(u, act):
    if act == 0:
        return np.ones_like(u)
    if act == 2:
        return (u > 0).astype(f32)
    if act == 3:
        return np.where(u > 0, f32(1), f32(0.1)).astype(f32)
    s = _sigmoid32(u)
    return (s * _fma(u, (f32(1) - s).astype(f32), np.ones_like(u))).astype(f32)


def _bf(t32):
    return torch.from_numpy(np.ascontiguousarray(t32)).to(BF)


def emulate_fwd(z, s1_fix, s2_fix, gamma, beta, act, res, rmean0, rvar0, eps=EPS, momentum=MOMENTUM):
    """z, res: bf16 tensors; s*_fix: int64 [C] (already folded); gamma ...: float32 tensors.  -> dict of float32 / bf16 results."""
    M = z.shape[0]
    m32 = f32(M)
    ff = lambda v: (v.numpy().astype(np.float64) * (1.0 / FIX)).astype(f32)        # from_fix
    mean = (ff(s1_fix) / m32).astype(f32)
    var = ((ff(s2_fix) / m32).astype(f32) - (mean * mean).astype(f32)).astype(f32)
    var = np.where(var < 0, f32(0), var)
    inv = (f32(1) / np.sqrt((var + f32(eps)).astype(f32))).astype(f32)
    g, b = gamma.numpy(), beta.numpy()
    sc = (g * inv).astype(f32)
    sh = (b - (mean * sc).astype(f32)).astype(f32)
    u = _fma(z.float().numpy(), sc[None, :], sh[None, :])
    a = _act32(u, act)
    if res is not None:
        a = (a + res.float().numpy()).astype(f32)
    out = dict(mean=mean, invstd=inv, y=_bf(a))
    if rmean0 is not None:
        unb = ((var * m32).astype(f32) / f32(M - 1)).astype(f32) if M > 1 else var
        mo = f32(momentum)
        out["rmean"] = (((f32(1) - mo) * rmean0.numpy()).astype(f32) + (mo * mean).astype(f32)).astype(f32)
        out["rvar"] = (((f32(1) - mo) * rvar0.numpy()).astype(f32) + (mo * unb).astype(f32)).astype(f32)
    return out


def _consts32(d):
    mean, inv, g, b = (d[k].float().numpy() for k in ("mean", "invstd", "gamma", "beta"))
    sc = (g * inv).astype(f32)
    return mean, inv, sc, (b - (mean * sc).astype(f32)).astype(f32)


def emulate_sums(d, act):
    """Row after row in fp32 (one of the orders the bound covers), then one rounding to 2^-36 fixed point.  -> int64 sg, sb."""
    mean, inv, sc, sh = _consts32(d)
    mi = (mean * inv).astype(f32)
    z, dy = d["z"].float().numpy(), d["dy"].float().numpy()
    du = (dy * _actg32(_fma(z, sc[None, :], sh[None, :]), act)).astype(f32)
    zhat = _fma(z, inv[None, :], -mi[None, :])
    sg, sb = np.zeros(z.shape[1], f32), np.zeros(z.shape[1], f32)
    for m in range(z.shape[0]):
        sb = (sb + du[m]).astype(f32)
        sg = _fma(du[m], zhat[m], sg)
    to_fix = lambda v: torch.from_numpy(np.rint(v.astype(np.float64) * FIXG).astype(np.int64))
    return to_fix(sg), to_fix(sb)


def emulate_dz(d, sg_fix, sb_fix, act, old=None):
    """-> bf16 dz (the accumulate form with `old`: two roundings)."""
    mean, inv, sc, sh = _consts32(d)
    M = d["z"].shape[0]
    z, dy = d["z"].float().numpy(), d["dy"].float().numpy()
    invM = (f32(1) / f32(M)).astype(f32)
    fg = lambda v: (v.numpy().astype(np.float64) * (1.0 / FIXG)).astype(f32)
    sg, sb = fg(sg_fix), fg(sb_fix)
    k1 = sc
    k3 = ((k1 * inv).astype(f32) * (sg * invM).astype(f32)).astype(f32)
    k2 = ((k1 * (sb * invM).astype(f32)).astype(f32) - (k3 * mean).astype(f32)).astype(f32)
    du = (dy * _actg32(_fma(z, sc[None, :], sh[None, :]), act)).astype(f32)
    o = _fma(-k3[None, :] * np.ones_like(z), z, _fma(k1[None, :] * np.ones_like(z), du, -k2[None, :] * np.ones_like(z)))
    o = _bf(o)
    if old is not None:
        o = (old.float() + o.float()).to(BF)
    return o


# ---------------------------------------------------------------------------------------------------------------------------
# the cases of tests/test_gpu_bn_exact.py (tests/test_bn_reference.py checks every one of them on the CPU)
REPS_A = (1, 3, 8, 9)
REPS_B = (1, 2, 8, 9)
# part A, reduce: (33, 8) one thread per row; C = 24: 85 rows per block, thread 255 idle; (2053, 2048) / (1027, 2048): grid capped (512 /
# the fused kernel's 256), second row batch partial; (4096, 2056): second pass over the channel groups with one group
A_REDUCE = [(33, 8), (64, 24), (257, 24), (2053, 2048), (1027, 2048), (4096, 2056)]
# part A, apply and apply_acc: (M, C, zero sums).  Non-zero forged sums need a power of two M; zero sums give the row tails.
A_APPLY = [(33, 8, True), (32, 8, False), (64, 24, False), (257, 24, True), (256, 24, False), (2053, 2048, True), (2048, 2048, False),
           (1027, 2048, True), (4096, 2056, False), (4100, 4096, True)]
A_FUSED = [(32, 8), (64, 24), (256, 24), (2048, 2048)]                  # exact: M a power of two
A_FUSED_TOL = [(1025, 2048), (1027, 2048)]                              # 1 / M is not exact: sums exact, dz under part B's bound
A_MARK = [(64, 24), (2048, 2048)]
FWD_SMALL = [(1, 8), (33, 8), (130, 40), (1100, 24), (70, 1024), (40, 2056)]
FWD_LARGE = [(65600, 256), (123400, 136)]
B_BWD = [(33, 8), (257, 24), (1027, 2048), (4096, 2056)]


def a_reps(M, C):
    """Every replica count on the small shapes, one (rotating) on the large."""
    return list(REPS_A) if M * C <= (1 << 16) else [REPS_A[(M + C // 8) % 4]]


def fwd_cases():
    """(M, C, act, with_res, running, reps); running: 0 none (null pointers), 1 both counters, 2 statistics with null counters."""
    out = []
    for i, (M, C) in enumerate(FWD_SMALL):
        for act in (0, 1, 2, 3):
            out.append((M, C, act, bool((i + act) % 2), (i + act // 2 + act) % 3, REPS_B[(i + act) % 4]))
    for i, (M, C) in enumerate(FWD_LARGE):
        for act in (1, 2):
            out.append((M, C, act, bool((i + act) % 2), (i + act) % 2, REPS_B[2 + (i + act) % 2]))
    return out


def b_bwd_cases():
    return [(M, C, act, REPS_A[(i + act) % 4]) for i, (M, C) in enumerate(B_BWD) for act in (1, 3)]
