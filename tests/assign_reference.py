"""References, draws and case builders of the SimOTA assignment kernels (csrc/assign.hip: ep24_assign_candidates, ep24_assign_cost,
ep24_assign_cost_range, ep24_dynamic_k, ep24_assign_resolve) and of the loss reduction and gradient (csrc/loss.hip: ep24_loss_terms,
ep24_loss_finalize, ep24_loss_grad; ep24_loss_grad_decode is compared with the two-launch form on the same cases).  A helper, not a
test module: tests/test_assign_reference.py checks it on the CPU (against the oracle where the oracle is defined, the exactness of
every dyadic case, the bounds over float32 emulations, the skip cap of the candidate masks, every mutant rejected) and
tests/test_gpu_assign_exact.py runs the kernels against it.  It never imports the package under test.  Sentinel buffers and bit
comparisons come from tests/update_reference.py.

The written contract of ep24_dynamic_k (assign.hip: "ties -> lower anchor index", "ties -> smaller index"), as a stable sort:
    candidates of an image: anchors a with (in_box[a] | in_ctr[a]) != 0 - any bit, the image's foreground set, not one label's
    for g < num_gt:  the min(10, P) largest pw[g, cand] by (value descending, anchor ascending), summed in that order in float32
                     k = max(1, trunc(sum));  the min(k, P) smallest cost[g, cand] by (value ascending, anchor ascending) get bit g
    nothing of g >= num_gt is written.  With pw in [0, 1] (what the cost kernel produces) the sum of min(10, P) values is at most P,
    so k > P happens only through the floor at 1 with P = 0.
ep24_assign_resolve: match == 0 -> (-1, 0.0); one bit -> that label; several bits -> the argmin of cost[:num_gt, a] over ALL labels of
the image (the first on equal cost), whether its bit is set or not; matched_iou = pw[g, a].

Bounds.  U = 2^-24 is the unit roundoff of fp32: one rounding moves a value v by at most U |v|; a library function documented to k ulp
moves its result by at most 2 k U |result| (one ulp of a number just above a power of two is 2 U of it).  The figures used are those of
the OpenCL 3.0 full profile, which the device library follows: exp 3, log 3, log1p 2, acos 4, sin 4 ulp; sqrt and the division are
correctly rounded (hipcc's default).  Every bound below is a first-order propagation through the kernel's own sequence of operations,
written next to the operation, times SECOND = 1 + 2^-20 for the products of errors; a sum of n terms evaluated in any order carries at
most n U sum|terms| besides the errors of its terms (update_reference.general_tol states the same rule; m_sum says why n covers
the kernels' own trees).  No figure comes from a
device.

  ray (geom.h::ray_giou), inputs r1 (label), r2 (prediction), d with absolute errors e1, e2, ed:
    rmin2 = rmin rmin:  2 rmin e + U rmin2          (likewise rmax2, d2)
    contained |r1 - r2| >= d: inter = pi rmin2:  pi e(rmin2) + U inter              disjoint d >= r1 + r2: inter = 0 exactly
    lens:  n1 = rmin2 + d2 - rmax2: the three errors + U (|rmin2 + d2| + |n1|);  den1 = 2 rmin d + 1e-8: 2 (rmin ed + d e) + 2 U den1
           c1 = n1 / den1: e(n1) / den1 + |c1| e(den1) / den1 + U |c1|;  a1 = acos(c1): e(c1) / sqrt(1 - c1^2) + 8 U a1
           s1 = sin(a1): e(a1) + 8 U;  inter = a1 rmin2 + a2 rmax2 - rmin d s1: product rule on each term + U per product, then
           U (|t1 + t2| + |inter|) for the two additions.  The error is thus in units of the terms a r^2 - of the two circles' areas -
           not of the (possibly much smaller) result, as tests/test_gpu_loss.py::test_circle_inter_vs_golden_g1_and_oracle has it.
    uni = area1 + area2 - inter, iou = inter / (uni + 1e-6), cl, cs = pi cl^2, q = (cs - uni) / cs, giou = iou - q: sums add errors
    plus U of each partial result, a quotient x / y carries e(x) / y + |x / y| e(y) / y + U |x / y|.
  The builders keep every ray at least 1 % of the larger radius from |r1 - r2| = d and from d = r1 + r2 and every lens cosine within
  +-0.9, so the branch and the clip to +-0.99 are the same in fp32 and in float64 (the input errors are a few U).
  pw = (sum of 24 terms) / 24 / 2: the terms' errors + 24 U sum|terms|, + U pw for the division by 24 (the halving is exact).
  cost = cls_cost + 3 (-log(pw + 1e-8)) + 100000 [not in both]:  p = sqrt(sigmoid(cls) sigmoid(obj)) with sigmoid = 1 / (1 + exp(-x)):
    8 U per sigmoid (exp 6 U, sum and quotient U each), 17 U the product, 9.5 U the root;  -log1p(-p): e(p) / (1 - p) + 4 U |.|;
    -log(p): e(p) / p + 6 U |.|;  the class sum: the terms' errors + C U sum;  every addition of the cost: U of its result - with the
    100000 present that is 0.006, which sets the scale there.

  finalize (loss.hip::loss_finalize_kernel):  sums over nblocks rows: nblocks U sum|partials| (exact for the integer draws);
    l = sum / nfg: + U |l|;  r = clamp(l / (state + 1e-8), 0, 2): |r| (e(l) / |l| + 3 U) (the clamp does not enlarge an error);
    e = exp(r / 20): e (e(r) / 20 + U r / 20 + 6 U);  den = sum of 26 e: their errors + 26 U den;  w = 26 e / den:
    w (e(e) / e + e(den) / den + 2 U);  w l: w l (e(w) / w + e(l) / l + U);  loss: the errors of its 27 terms + 27 U sum|terms|.

  candidates (assign.hip::candidates_kernel): derived at candidates_ref;  loss_terms / loss_grad: the same rules carried through
  geom.h::ray_loss_grad operation by operation by the Err class of section (e).
"""
import functools

import numpy as np

from update_reference import U, SENT32, NAN32, Guarded, assert_same, bits32, from_bits32, err_ratio  # noqa: F401

G_MAX = 50
LCOLS = 51
NS = 32
SECOND = 1.0 + 2.0 ** -20
PI32 = float(np.float32(np.pi))
SENT_I32 = 0x5A5A5A5A
INF32, NINF32 = 0x7F800000, 0xFF800000
E_ARG, E_UNSUPPORTED = -1, -3                     # include/ep24.h (tests/test_assign_reference.py pins them to its text)
F32 = np.float32


def cand_of(in_box, in_ctr):
    return np.flatnonzero((np.asarray(in_box, dtype=np.uint64) | np.asarray(in_ctr, dtype=np.uint64)) != 0)


# ---------------------------------------------------------------------------------------------------------------------------
# (a) ep24_dynamic_k and ep24_assign_resolve
def sum32(values):
    """float32 sum in the given order"""
    s = F32(0.0)
    for v in values:
        s = F32(s + F32(v))
    return s


def dynamic_k_ref(pw, cost, in_box, in_ctr, num_gt, ks_init=None):
    """pw, cost float32 [50, A]; in_box, in_ctr uint64 [A] -> (match uint64 [A], ks int64 [50]; rows g >= num_gt keep ks_init)"""
    A = pw.shape[1]
    match = np.zeros(A, dtype=np.uint64)
    ks = np.full(G_MAX, SENT_I32 if ks_init is None else ks_init, dtype=np.int64)
    cand = cand_of(in_box, in_ctr)
    P = cand.size
    for g in range(int(num_gt)):
        order = np.argsort(-pw[g, cand].astype(np.float64), kind="stable")          # value descending, anchor ascending
        total = sum32(pw[g, cand[order[:min(10, P)]]])
        k = max(1, int(np.trunc(total)))
        ks[g] = k
        pick = np.argsort(cost[g, cand].astype(np.float64), kind="stable")[:min(k, P)]
        match[cand[pick]] |= np.uint64(1 << g)
    return match, ks


def resolve_ref(match, pw, cost, num_gt):
    """match uint64 [A]; pw, cost float32 [50, A] -> (matched_gt int32 [A], matched_iou float32 [A])"""
    A = match.shape[0]
    mg = np.full(A, -1, dtype=np.int32)
    mi = np.zeros(A, dtype=np.float32)
    for a in np.flatnonzero(match):
        m = int(match[a])
        if bin(m).count("1") == 1:
            g = m.bit_length() - 1
        else:
            g = int(np.argmin(cost[:int(num_gt), a]))                              # numpy: the first of equal minima
        mg[a], mi[a] = g, pw[g, a]
    return mg, mi


# candidate layouts: name -> anchors (sorted, unique, < A).  `thread`: all in the slots t, t + 256, ... of one thread (A <= 256: one
# anchor); `wave`: all in one wave's first slots; `perwave`: one per wave in each of the first slots of four different threads
DYNK_A = [1, 9, 255, 256, 257, 8447, 8448, 8449, 8705]
LAYOUTS = ["none", "last", "ends", "thread9", "thread11", "wave9", "wave10", "wave11", "perwave", "all", "random"]
VALUES = ["equal", "dyadic", "sum3", "below4", "ones", "tiny", "general"]


def layout(name, A, rng):
    if name == "none":
        a = []
    elif name == "last":
        a = [A - 1]
    elif name == "ends":
        a = [0, A - 1]
    elif name.startswith("thread"):
        t = 37 % A
        a = list(range(t, A, 256))
        n = int(name[6:])
        if len(a) > n:                                                             # keep the first, the last and slots between
            a = sorted(set([a[0], a[-1]] + list(rng.choice(a[1:-1], n - 2, replace=False))))
    elif name.startswith("wave"):
        n = int(name[4:])
        a = sorted(rng.choice(np.arange(64, 128) % A, min(n, 64, A), replace=False)) if A >= 128 else list(range(min(n, A)))
    elif name == "perwave":
        a = [x for x in (5, 64 + 63, 128, 192 + 17, 256 + 5, 512 + 64 + 63) if x < A]
    elif name == "all":
        a = list(range(A))
    else:
        a = sorted(rng.choice(A, min(A, 40), replace=False))
    return np.array(sorted(set(int(x) for x in a)), dtype=np.int64)


def cand_masks(cand, A, rng):
    """-> in_box, in_ctr uint64 [A]: every candidate has one or two bits somewhere in 0 .. 49 (often of one label only, often in one
    of the two words only), every other anchor none"""
    ib, ic = np.zeros(A, dtype=np.uint64), np.zeros(A, dtype=np.uint64)
    for i, a in enumerate(cand):
        g = np.uint64(1) << np.uint64(49 if i % 5 == 0 else rng.integers(0, G_MAX))
        how = i % 3
        if how != 1:
            ib[a] |= g
        if how != 0:
            ic[a] |= np.uint64(1) << np.uint64(rng.integers(0, G_MAX)) if how == 2 else g
    return ib, ic


def draw_values(kind, cand, A, rng):
    """-> pw, cost float32 [50, A].  Non-candidate slots hold values of the same draw that would win if they were looked at."""
    P = cand.size
    if kind == "general":
        pw = rng.random((G_MAX, A)).astype(F32)
        cost = (rng.standard_normal((G_MAX, A)) * 3 + 100000.0 * rng.integers(0, 2, (G_MAX, A))).astype(F32)
        return pw, cost
    cost = rng.integers(0, 8, (G_MAX, A)).astype(F32)                              # small integers: ties are the rule
    if kind == "equal":
        return np.full((G_MAX, A), 0.5, dtype=F32), np.full((G_MAX, A), 2.0, dtype=F32)
    if kind == "dyadic":
        return (rng.integers(0, 65, (G_MAX, A)) / 64.0).astype(F32), cost
    if kind == "ones":
        return np.ones((G_MAX, A), dtype=F32), cost
    if kind == "tiny":
        return np.full((G_MAX, A), 2.0 ** -10, dtype=F32), cost
    # sum3: 1 + 3/4 + 3/4 + 1/2 = 3 exactly; below4: 1 + 1 + 1 + (1 - 2^-22) = 4 - 2^-22, the fp32 number below 4.  The four sit on
    # candidates chosen per label, every other candidate holds 0, every non-candidate 1 (it would change the sum).
    top = [1.0, 0.75, 0.75, 0.5] if kind == "sum3" else [1.0, 1.0, 1.0, 1.0 - 2.0 ** -22]
    pw = np.ones((G_MAX, A), dtype=F32)
    for g in range(G_MAX):
        pw[g, cand] = 0.0
        if P:
            at = rng.choice(cand, min(4, P), replace=False)
            pw[g, at] = np.array(top[:at.size], dtype=F32)
    return pw, cost


def poison(x, cand):
    """bit patterns of x with every non-candidate slot NaN, +inf or -inf in turn"""
    b = bits32(x).copy()
    keep = np.zeros(x.shape[1], dtype=bool)
    keep[cand] = True
    pat = np.array([NAN32, INF32, NINF32, 0xFFC00001], dtype=np.uint32)[np.arange(x.shape[1]) % 4]
    b[:, ~keep] = pat[~keep]
    return b


# (num_gt of the four images, their layouts): every launch holds 0, 1, 50 and 7 labels, rotated so that EVERY layout meets an image
# with labels ('none' - P = 0, where k = 1 finds nothing - twice); the images without labels take what is left
DYNK_GROUPS = [([0, 1, 50, 7], ["all", "last", "all", "thread9"]),
               ([7, 0, 1, 50], ["none", "ends", "thread11", "wave9"]),
               ([50, 7, 0, 1], ["ends", "perwave", "none", "wave10"]),
               ([1, 50, 7, 0], ["wave11", "none", "random", "random"])]


def dynk_groups():
    """The launches of one A: each value kind with each of the four groups -> [(kind, group index, layouts)]"""
    return [(v, gi, grp) for v in VALUES for gi, (_, grp) in enumerate(DYNK_GROUPS)]


@functools.lru_cache(maxsize=3)
def dynk_case(A, kind, gi):
    """One launch: dict(pw, cost [4, 50, A] float32, in_box, in_ctr [4, A] uint64, num_gt [4], cand: [anchors per image],
    match [4, A] uint64, ks [4, 50] int64 with the sentinel where nothing is written).  Shared: treat as read-only."""
    num_gt, grp = DYNK_GROUPS[gi]
    rng = np.random.default_rng(1000 * A + 10 * VALUES.index(kind) + gi)
    B = len(grp)
    c = dict(pw=np.zeros((B, G_MAX, A), dtype=F32), cost=np.zeros((B, G_MAX, A), dtype=F32), in_box=np.zeros((B, A), dtype=np.uint64),
             in_ctr=np.zeros((B, A), dtype=np.uint64), num_gt=np.array(num_gt, dtype=np.int32), cand=[],
             match=np.zeros((B, A), dtype=np.uint64), ks=np.zeros((B, G_MAX), dtype=np.int64), layouts=grp)
    for b, name in enumerate(grp):
        cand = layout(name, A, rng)
        c["cand"].append(cand)
        c["in_box"][b], c["in_ctr"][b] = cand_masks(cand, A, rng)
        c["pw"][b], c["cost"][b] = draw_values(kind, cand, A, rng)
        c["match"][b], c["ks"][b] = dynamic_k_ref(c["pw"][b], c["cost"][b], c["in_box"][b], c["in_ctr"][b], c["num_gt"][b])
    return c


RESOLVE_A = [1, 255, 256, 257]
RESOLVE_NUM_GT = [0, 1, 5, 50]


@functools.lru_cache(maxsize=8)
def resolve_case(A):
    """match words per anchor in turn: 0, bit 0, the highest label's bit, two bits, five bits, several bits whose labels are all
    dearer than a label without a bit, several bits of equal cost.  cost holds small integers, pw multiples of 2^-6."""
    rng = np.random.default_rng(77 + A)
    B = len(RESOLVE_NUM_GT)
    pw = (rng.integers(0, 65, (B, G_MAX, A)) / 64.0).astype(F32)
    cost = rng.integers(0, 4, (B, G_MAX, A)).astype(F32)
    match = np.zeros((B, A), dtype=np.uint64)
    for b, ng in enumerate(RESOLVE_NUM_GT):
        for a in range(A):
            kind = (a + b) % 7
            if ng == 0 or kind == 0:
                continue
            if kind == 1 or ng == 1:
                bits = [0]
            elif kind == 2:
                bits = [ng - 1]
            else:
                bits = list(rng.choice(ng, min(ng, 2 if kind == 3 else 5 if kind == 4 else 3), replace=False))
                if kind == 5 and ng > len(bits):                                   # the cheapest label of all has no bit
                    cost[b, :ng, a] = rng.integers(5, 9, ng)
                    free = [g for g in range(ng) if g not in bits]
                    cost[b, free[len(free) // 2], a] = 1.0
                if kind == 6:
                    cost[b, :ng, a] = 3.0                                          # all equal: label 0 wins, bit or no bit
            for g in bits:
                match[b, a] |= np.uint64(1 << int(g))
    want = [resolve_ref(match[b], pw[b], cost[b], ng) for b, ng in enumerate(RESOLVE_NUM_GT)]
    return dict(pw=pw, cost=cost, match=match, num_gt=np.array(RESOLVE_NUM_GT, dtype=np.int32),
                mg=np.stack([w[0] for w in want]), mi=np.stack([w[1] for w in want]))


# ---------------------------------------------------------------------------------------------------------------------------
# (b) ep24_loss_finalize
FIN_NBLOCKS = [1, 2, 7, 8, 9, 15, 16, 17, 127, 128, 129, 137]
FIN_COUNTS = [1, 64, 256, 0]


def finalize_ref(partials, num_gt, state):
    """partials float32 [nblocks, 32], state float32 [26] -> (result float64 [64] with NaN where nothing is written, new state
    float64 [26], tol float64 [64], tol_state [26]).  The bound is the module docstring's."""
    p = partials.astype(np.float64)
    nb = p.shape[0]
    st = state.astype(np.float64)
    sums = p.sum(0)
    e_sums = nb * U * np.abs(p).sum(0)
    nfg_raw = sums[26]
    nfg = max(nfg_raw, 1.0)
    l = sums[:26] / nfg
    e_l = e_sums[:26] / nfg + U * np.abs(l)
    den0 = st + 1e-8
    q = l / den0
    r = np.clip(q, 0.0, 2.0)
    with np.errstate(all="ignore"):
        e_r = np.where(l != 0, np.abs(q) * (e_l / np.where(l != 0, np.abs(l), 1.0) + 3 * U), 0.0)
    e_r = np.where((q > 2.0 + e_r) | (q < -e_r), 0.0, np.minimum(e_r, 2.0))        # clamped well inside: exact
    e = np.exp(r / 20.0)
    e_e = e * (e_r / 20.0 + U * r / 20.0 + 6 * U)
    den = e.sum()
    e_den = e_e.sum() + 26 * U * den
    w = 26.0 * e / den
    e_w = w * (e_e / e + e_den / den + 2 * U)
    wl = w * l
    e_wl = np.abs(w) * e_l + np.abs(l) * e_w + U * np.abs(wl)
    l1 = sums[27] / nfg
    e_l1 = e_sums[27] / nfg + U * abs(l1)
    res = np.full(64, np.nan)
    tol = np.zeros(64)
    res[1:25], tol[1:25] = wl[:24], e_wl[:24]
    res[29:53], tol[29:53] = w[:24], e_w[:24]
    res[53], res[54], tol[53], tol[54] = w[24], w[25], e_w[24], e_w[25]
    res[0] = wl.sum() + l1
    tol[0] = e_wl.sum() + e_l1 + 27 * U * (np.abs(wl).sum() + abs(l1))
    res[25], res[26], tol[25], tol[26] = l[24], l[25], e_l[24], e_l[25]
    res[27], res[28], res[55] = nfg, float(np.sum(num_gt)), nfg_raw
    tol[55] = e_sums[26]
    tol[27] = e_sums[26]
    res[56], tol[56] = l1, e_l1
    new_state, tol_state = l, e_l * SECOND
    return res, new_state, tol * SECOND, tol_state


FIN_WRITTEN = np.array([i <= 56 for i in range(64)])
FIN_EXACT = [55, 27, 28, 25, 26, 56]


def finalize_partials(nblocks, count, seed=0):
    """Small distinct integers (every fold is exact in any order), columns 28 .. 31 zero as loss_terms leaves them, the count
    column summing to `count` with its last unit in the last row"""
    rng = np.random.default_rng(300 + seed)
    p = np.zeros((nblocks, NS), dtype=F32)
    perm = rng.permutation(nblocks * 28)
    p[:, :28] = (perm.reshape(nblocks, 28) % 4001 + 1).astype(F32)
    p[:, 26] = 0
    if count:
        p[nblocks - 1, 26] = 1
        p[0, 26] += count - 1
    return p


def finalize_general(nblocks, seed=0):
    rng = np.random.default_rng(400 + seed)
    p = np.zeros((nblocks, NS), dtype=F32)
    p[:, :28] = (rng.random((nblocks, 28)) * 3).astype(F32)
    p[:, 26] = rng.integers(0, 4, nblocks)
    return p


def finalize_fold(partials, drop_last_row=False, drop_tail=False):
    """float32 restatement of the kernel's fold (8 groups of ceil(nblocks / 8) rows, 16 loads at a time, then the 8 group sums),
    with the two planted faults of tests/test_assign_reference.py"""
    nb = partials.shape[0]
    per = (nb + 7) // 8
    sums = np.zeros(NS, dtype=F32)
    for g in range(8):
        lo, hi = g * per, min(nb, (g + 1) * per)
        if drop_last_row and hi > lo:
            hi -= 1
        if drop_tail and hi > lo:
            hi = lo + (hi - lo) // 16 * 16
        s = np.zeros(NS, dtype=F32)
        for i in range(lo, max(hi, lo)):
            s = (s + partials[i]).astype(F32)
        sums = (sums + s).astype(F32)
    return sums


def finalize_f32(partials, num_gt, state, sums=None):
    """float32 emulation of the kernel's arithmetic behind the fold, with numpy's own exp and another order of the sums (pairwise
    numpy sums): what the derived bound has to hold.  -> (result float32 [64], new state float32 [26])"""
    sums = partials.sum(0, dtype=F32) if sums is None else sums
    nfg = max(sums[26], F32(1.0))
    l = (sums[:26] / nfg).astype(F32)
    with np.errstate(all="ignore"):
        r = np.clip((l / (state.astype(F32) + F32(1e-8))).astype(F32), F32(0), F32(2))
    e = np.exp((r / F32(20.0)).astype(F32)).astype(F32)
    den = e.sum(dtype=F32)
    w = (F32(26.0) * e / den).astype(F32)
    res = np.zeros(64, dtype=F32)
    res[1:25], res[29:53], res[53], res[54] = (w * l)[:24], w[:24], w[24], w[25]
    l1 = F32(sums[27] / nfg)
    res[0] = F32((w * l).astype(F32).sum(dtype=F32) + l1)
    res[25], res[26], res[27], res[28], res[55], res[56] = l[24], l[25], nfg, F32(np.sum(num_gt)), sums[26], l1
    return res, l


# ---------------------------------------------------------------------------------------------------------------------------
# (c) ep24_assign_cost_range
def ray_ref(r1, r2, d, e1, e2, ed):
    """geom.h::ray_giou in float64 on arrays, with the bound of the module docstring.  e1, e2, ed: absolute errors of the inputs as
    the fp32 evaluation has them.  -> dict(giou, e_giou, inter, e_inter, branch 0 contained / 1 disjoint / 2 lens, margin: distance
    from the two branch boundaries over the larger radius, cmax: the larger |cosine| of a lens ray (0 elsewhere))"""
    r1, r2, d = np.broadcast_arrays(np.asarray(r1, dtype=np.float64), np.asarray(r2, dtype=np.float64), np.asarray(d, dtype=np.float64))
    e1, e2, ed = np.broadcast_to(e1, r1.shape), np.broadcast_to(e2, r1.shape), np.broadcast_to(ed, r1.shape)
    pi = PI32
    first = r1 <= r2
    rmin, rmax = np.where(first, r1, r2), np.where(first, r2, r1)
    emin, emax = np.where(first, e1, e2), np.where(first, e2, e1)
    rmin2, rmax2, d2 = rmin * rmin, rmax * rmax, d * d
    e_rmin2, e_rmax2, e_d2 = 2 * rmin * emin + U * rmin2, 2 * rmax * emax + U * rmax2, 2 * d * ed + U * d2
    contained = np.abs(r1 - r2) >= d
    disjoint = d >= r1 + r2
    lens = ~(contained | disjoint)
    with np.errstate(all="ignore"):
        margin = np.minimum(np.abs(np.abs(r1 - r2) - d), np.abs(r1 + r2 - d)) / np.maximum(rmax, 1e-300)
        n1, n2 = rmin2 + d2 - rmax2, rmax2 + d2 - rmin2
        e_n1 = e_rmin2 + e_d2 + e_rmax2 + U * (np.abs(rmin2 + d2) + np.abs(n1))
        e_n2 = e_rmin2 + e_d2 + e_rmax2 + U * (np.abs(rmax2 + d2) + np.abs(n2))
        den1, den2 = 2 * rmin * d + 1e-8, 2 * rmax * d + 1e-8
        e_den1, e_den2 = 2 * (rmin * ed + d * emin) + 2 * U * den1, 2 * (rmax * ed + d * emax) + 2 * U * den2
        c1r, c2r = n1 / den1, n2 / den2
        e_c1 = e_n1 / den1 + np.abs(c1r) * e_den1 / den1 + U * np.abs(c1r)
        e_c2 = e_n2 / den2 + np.abs(c2r) * e_den2 / den2 + U * np.abs(c2r)
        c1, c2 = np.clip(c1r, -0.99, 0.99), np.clip(c2r, -0.99, 0.99)
        a1, a2 = np.arccos(c1), np.arccos(c2)
        e_a1, e_a2 = e_c1 / np.sqrt(1 - c1 * c1) + 8 * U * a1, e_c2 / np.sqrt(1 - c2 * c2) + 8 * U * a2
        s1 = np.sin(a1)
        e_s1 = e_a1 + 8 * U
        t1, t2, t3 = a1 * rmin2, a2 * rmax2, rmin * d * s1
        e_t1, e_t2 = e_a1 * rmin2 + a1 * e_rmin2 + U * t1, e_a2 * rmax2 + a2 * e_rmax2 + U * t2
        e_t3 = (emin * d + rmin * ed) * s1 + rmin * d * e_s1 + 2 * U * t3
        lens_v = t1 + t2 - t3
        e_lens = e_t1 + e_t2 + e_t3 + U * (np.abs(t1 + t2) + np.abs(lens_v))
    inter = np.where(disjoint, 0.0, np.where(contained, pi * rmin2, np.where(lens, lens_v, 0.0)))
    e_inter = np.where(disjoint, 0.0, np.where(contained, pi * e_rmin2 + U * pi * rmin2, np.where(lens, e_lens, 0.0)))
    area1, area2 = pi * (r1 * r1), pi * (r2 * r2)
    e_ar1, e_ar2 = pi * (2 * r1 * e1 + U * r1 * r1) + U * area1, pi * (2 * r2 * e2 + U * r2 * r2) + U * area2
    uni = area1 + area2 - inter
    e_uni = e_ar1 + e_ar2 + e_inter + U * (area1 + area2 + np.abs(uni))
    ue = uni + 1e-6
    e_ue = e_uni + U * ue
    iou = inter / ue
    e_iou = e_inter / ue + np.abs(iou) * e_ue / ue + U * np.abs(iou)
    cl = np.where(contained, rmax, (r1 + r2 + d) / 2.0)
    e_cl = np.where(contained, emax, (e1 + e2 + ed + 2 * U * (r1 + r2 + d)) / 2.0)
    cs = pi * (cl * cl)
    e_cs = pi * (2 * cl * e_cl + U * cl * cl) + U * cs
    top = cs - uni
    e_top = e_cs + e_uni + U * np.abs(top)
    q = top / cs
    e_q = e_top / cs + np.abs(q) * e_cs / cs + U * np.abs(q)
    giou = iou - q
    e_giou = (e_iou + e_q + U * np.abs(giou)) * SECOND
    return dict(giou=giou, e_giou=e_giou, inter=inter, e_inter=e_inter * SECOND, branch=np.where(contained, 0, np.where(disjoint, 1, 2)),
                margin=margin, cmax=np.where(lens, np.maximum(np.abs(c1r), np.abs(c2r)), 0.0), uni=uni, cs=cs)


def label_geometry(lab):
    """labels float32 [G, 51] -> (class int [G], cx, cy float64 [G], r1 float64 [G, 24], e(r1)).  The fp32 form is
    sqrt(dx dx + dy dy) of dx = px - cx: three roundings under the root, one on it: 3 U relative."""
    lab = np.asarray(lab, dtype=np.float64)
    cx, cy = lab[:, 1], lab[:, 2]
    r1 = np.hypot(lab[:, 3::2] - cx[:, None], lab[:, 4::2] - cy[:, None])
    return lab[:, 0].astype(np.int64), cx, cy, r1, 3 * U * r1


def _sig(x):
    return 1.0 / (1.0 + np.exp(-x))


def class_terms_ref(cls_logit, obj_logit):
    """p = sqrt(sigmoid(cls) sigmoid(obj)) and the two BCE terms with their bounds: -> (t_neg, e_neg, t_pos, e_pos)"""
    p = np.sqrt(_sig(cls_logit) * _sig(obj_logit))
    e_p = 9.5 * U * p
    with np.errstate(all="ignore"):
        t_neg = -np.maximum(np.log1p(-p), -100.0)
        t_pos = -np.maximum(np.log(p), -100.0)
        e_neg = e_p / (1 - p) + 4 * U * np.abs(t_neg) + U * np.abs(p)
        e_pos = e_p / p + 6 * U * np.abs(t_pos)
    return t_neg, e_neg, t_pos, e_pos


def cost_ref(outputs, labels, in_box, in_ctr, num_gt, a_lo=0, a_hi=None):
    """One image.  outputs float32 [A, 27 + C] (decoded), labels float32 [50, 51], masks uint64 [A].  Everything [50, A] (rays:
    [50, A, 24]) in float64, NaN where the kernel writes nothing: dict(written, pw, tol_pw, cost, tol_cost, cls_cost, iou_cost,
    both_cost, branch, margin, cmax)"""
    o = np.asarray(outputs, dtype=np.float64)
    A = o.shape[0]
    a_hi = A if a_hi is None else a_hi
    ng = int(num_gt)
    cand = cand_of(in_box, in_ctr)
    cand = cand[(cand >= a_lo) & (cand < a_hi)]
    out = {k: np.full((G_MAX, A), np.nan) for k in ("pw", "tol_pw", "cost", "tol_cost", "cls_cost", "iou_cost", "both_cost")}
    out["written"] = np.zeros((G_MAX, A), dtype=bool)
    out["branch"] = np.full((G_MAX, A, 24), -1, dtype=np.int64)
    out["margin"], out["cmax"] = np.full((G_MAX, A, 24), np.inf), np.zeros((G_MAX, A, 24))
    if ng == 0 or cand.size == 0:
        return out
    gcls, gcx, gcy, r1, e1 = label_geometry(np.asarray(labels)[:ng])
    oc = o[cand]
    d = np.hypot(gcx[:, None] - oc[None, :, 0], gcy[:, None] - oc[None, :, 1])                  # [G, P]
    ray = ray_ref(r1[:, None, :], oc[None, :, 2:26], d[:, :, None], e1[:, None, :], 0.0, 3 * U * d[:, :, None])
    terms = 1.0 - ray["giou"]
    e_terms = ray["e_giou"] + U * np.abs(terms)
    pw = terms.sum(2) / 48.0
    tol_pw = ((e_terms.sum(2) + 24 * U * np.abs(terms).sum(2)) / 48.0 + U * np.abs(pw)) * SECOND
    t_neg, e_neg, t_pos, e_pos = class_terms_ref(oc[:, 27:], oc[:, 26:27])                     # [P, C]
    C = t_neg.shape[1]
    s0 = t_neg.sum(1)
    e_s0 = e_neg.sum(1) + C * U * np.abs(t_neg).sum(1)
    P = cand.size
    tn, tp = t_neg[np.arange(P)[None, :], gcls[:, None]], t_pos[np.arange(P)[None, :], gcls[:, None]]
    en, ep = e_neg[np.arange(P)[None, :], gcls[:, None]], e_pos[np.arange(P)[None, :], gcls[:, None]]
    cls_cost = s0[None, :] - tn + tp
    e_cls = e_s0[None, :] + en + ep + U * (np.abs(s0[None, :] - tn) + np.abs(cls_cost))
    nl = -np.log(pw + 1e-8)
    e_nl = (tol_pw + U * (pw + 1e-8)) / (pw + 1e-8) + 6 * U * np.abs(nl)
    iou_cost = 3.0 * nl
    e_iouc = 3.0 * e_nl + U * np.abs(iou_cost)
    both = ((np.asarray(in_box, dtype=np.uint64)[cand] & np.asarray(in_ctr, dtype=np.uint64)[cand])[None, :]
            >> np.arange(ng, dtype=np.uint64)[:, None]) & np.uint64(1)
    both_cost = 100000.0 * (1.0 - both.astype(np.float64))
    cost = cls_cost + iou_cost + both_cost
    tol_cost = (e_cls + e_iouc + U * (np.abs(cls_cost + iou_cost) + np.abs(cost))) * SECOND
    for k, v in (("pw", pw), ("tol_pw", tol_pw), ("cost", cost), ("tol_cost", tol_cost), ("cls_cost", cls_cost), ("iou_cost", iou_cost),
                 ("both_cost", both_cost)):
        out[k][:ng, cand] = v
    out["written"][:ng, cand] = True
    out["branch"][:ng, cand], out["margin"][:ng, cand], out["cmax"][:ng, cand] = ray["branch"], ray["margin"], ray["cmax"]
    return out


def ray_f32(r1, r2, d):
    """float32 emulation of ray_giou with numpy's own acos / sin (another library than the device's)"""
    r1, r2, d = np.broadcast_arrays(np.asarray(r1, dtype=F32), np.asarray(r2, dtype=F32), np.asarray(d, dtype=F32))
    pi = F32(PI32)
    rmin, rmax = np.minimum(r1, r2), np.maximum(r1, r2)
    rmin2, rmax2, d2 = rmin * rmin, rmax * rmax, d * d
    contained, disjoint = np.abs(r1 - r2) >= d, d >= r1 + r2
    with np.errstate(all="ignore"):
        c1 = np.clip((rmin2 + d2 - rmax2) / (F32(2) * rmin * d + F32(1e-8)), F32(-0.99), F32(0.99))
        c2 = np.clip((rmax2 + d2 - rmin2) / (F32(2) * rmax * d + F32(1e-8)), F32(-0.99), F32(0.99))
        a1, a2 = np.arccos(c1), np.arccos(c2)
        lens_v = a1 * rmin2 + a2 * rmax2 - rmin * d * np.sin(a1)
    inter = np.where(disjoint, F32(0), np.where(contained, pi * rmin2, lens_v)).astype(F32)
    uni = pi * (r1 * r1) + pi * (r2 * r2) - inter
    iou = inter / (uni + F32(1e-6))
    cl = np.where(contained, rmax, (r1 + r2 + d) / F32(2))
    cs = pi * (cl * cl)
    out = iou - (cs - uni) / cs
    assert out.dtype == F32
    return out, inter


def cost_f32(outputs, labels, in_box, in_ctr, num_gt):
    """float32 emulation of the cost kernel for every candidate of one image, pairwise numpy sums instead of the kernel's running
    ones: -> pw, cost float32 [50, A] (NaN where nothing is written)"""
    o = np.asarray(outputs, dtype=F32)
    lab = np.asarray(labels, dtype=F32)
    A, ng = o.shape[0], int(num_gt)
    cand = cand_of(in_box, in_ctr)
    pw_o, cost_o = np.full((G_MAX, A), np.nan, dtype=F32), np.full((G_MAX, A), np.nan, dtype=F32)
    if ng == 0 or cand.size == 0:
        return pw_o, cost_o
    lab = lab[:ng]
    dx, dy = lab[:, 3::2] - lab[:, 1:2], lab[:, 4::2] - lab[:, 2:3]
    r1 = np.sqrt(dx * dx + dy * dy)
    oc = o[cand]
    ddx, ddy = lab[:, 1][:, None] - oc[None, :, 0], lab[:, 2][:, None] - oc[None, :, 1]
    d = np.sqrt(ddx * ddx + ddy * ddy)
    giou, _ = ray_f32(r1[:, None, :], oc[None, :, 2:26], d[:, :, None])
    pw = ((F32(1) - giou).sum(2, dtype=F32) / F32(24) / F32(2)).astype(F32)
    sg = lambda x: F32(1) / (F32(1) + np.exp(-x))
    p = np.sqrt(sg(oc[:, 27:]) * sg(oc[:, 26:27]))
    with np.errstate(all="ignore"):
        t_neg, t_pos = -np.maximum(np.log1p(-p), F32(-100)), -np.maximum(np.log(p), F32(-100))
    gcls = lab[:, 0].astype(np.int64)
    ar = np.arange(cand.size)[None, :]
    cls_cost = t_neg.sum(1, dtype=F32)[None, :] - t_neg[ar, gcls[:, None]] + t_pos[ar, gcls[:, None]]
    both = ((np.asarray(in_box, dtype=np.uint64)[cand] & np.asarray(in_ctr, dtype=np.uint64)[cand])[None, :]
            >> np.arange(ng, dtype=np.uint64)[:, None]) & np.uint64(1)
    cost = cls_cost + F32(3) * (-np.log(pw + F32(1e-8))) + F32(100000) * (F32(1) - both.astype(F32))
    assert pw.dtype == F32 and cost.dtype == F32
    pw_o[:ng, cand], cost_o[:ng, cand] = pw, cost
    return pw_o, cost_o


# the launches: A = 5 full workgroups of 64 anchors and one of 37.  From a_lo = 0 the workgroups hold 64, 0, 1, 63, 64 and 37
# candidates; image b has COST_NUM_GT[b] labels: 64 x 4 pairs are exactly one batch of 256, 64 x 5 two, 64 x 50 thirteen.
COST_A = 5 * 64 + 37
COST_NUM_GT = [1, 4, 5, 50]
COST_C = [1, 3, 80, 96]
COST_RAYS = ["lens", "none", "mixed"]
COST_RANGES = [(0, COST_A), (13, 300), (64, 64), (168, 169)]


def cost_candidates():
    c = list(range(0, 64)) + [128 + 40] + list(range(192 + 1, 256)) + list(range(256, 320)) + list(range(320, COST_A))
    return np.array(c, dtype=np.int64)


@functools.lru_cache(maxsize=16)
def cost_case(C, rays, seed=0):
    """dict(outputs [4, A, 27 + C], labels [4, 50, 51] float32, in_box, in_ctr [4, A] uint64, num_gt).  Labels: centres in
    [100, 110]^2, radii 30 .. 40.  A prediction's rays are built into their branch against EVERY label:
      lens       centre in [130, 135] x [100, 110] (d in [20, 36.4]), radii 30 .. 40:  |r1 - r2| <= 10 < d < 60 <= r1 + r2
      contained  the same centre, radii 80 .. 90: |r1 - r2| >= 40 > d;  or a centre inside the labels' square (d <= 14.2), radii 2 .. 5
      disjoint   centre beyond (400, 400)
    'lens': every ray of every candidate a lens (the queue of a 64 x 4 batch is exactly full); 'none': no lens at all; 'mixed': the
    three kinds per ray and per candidate.  Non-candidates get rows of the same draw."""
    rng = np.random.default_rng(5000 + 10 * C + COST_RAYS.index(rays) + 100 * seed)
    A, B = COST_A, len(COST_NUM_GT)
    ang = np.arange(24) * (np.pi / 12)
    labels = np.zeros((B, G_MAX, LCOLS), dtype=F32)
    for b, ng in enumerate(COST_NUM_GT):
        cx, cy = 100 + 10 * rng.random(ng), 100 + 10 * rng.random(ng)
        r = 30 + 10 * rng.random((ng, 24))
        labels[b, :ng, 0] = rng.integers(0, C, ng)
        labels[b, :ng, 1], labels[b, :ng, 2] = cx, cy
        labels[b, :ng, 3::2], labels[b, :ng, 4::2] = cx[:, None] + r * np.cos(ang), cy[:, None] + r * np.sin(ang)
    out = np.zeros((B, A, 27 + C), dtype=F32)
    out[..., 26:] = np.clip(rng.standard_normal((B, A, 1 + C)) * 1.5, -3, 3)
    near = np.stack([130 + 5 * rng.random((B, A)), 100 + 10 * rng.random((B, A))], -1)
    inside = 100 + 10 * rng.random((B, A, 2))
    far = 400 + 200 * rng.random((B, A, 2))
    r_lens, r_big, r_small = 30 + 10 * rng.random((B, A, 24)), 80 + 10 * rng.random((B, A, 24)), 2 + 3 * rng.random((B, A, 24))
    if rays == "lens":
        out[..., :2], out[..., 2:26] = near, r_lens
    elif rays == "none":
        kind = rng.integers(0, 3, (B, A))
        out[..., :2] = np.where(kind[..., None] == 0, near, np.where(kind[..., None] == 1, inside, far))
        out[..., 2:26] = np.where(kind[..., None] == 0, r_big, np.where(kind[..., None] == 1, r_small, r_lens))
    else:
        kind = rng.integers(0, 4, (B, A))                                            # 0, 1: near with lens / contained rays drawn per ray
        out[..., :2] = np.where(kind[..., None] <= 1, near, np.where(kind[..., None] == 2, inside, far))
        per_ray = np.where(rng.integers(0, 2, (B, A, 24)) == 0, r_lens, r_big)
        out[..., 2:26] = np.where(kind[..., None] <= 1, per_ray, np.where(kind[..., None] == 2, r_small, r_lens))
    cand = cost_candidates()
    in_box, in_ctr = np.zeros((B, A), dtype=np.uint64), np.zeros((B, A), dtype=np.uint64)
    for b in range(B):
        in_box[b], in_ctr[b] = cand_masks(cand, A, rng)
        for a in cand[::3]:                                                          # in both for some labels: the 100000 term is absent
            both = np.uint64(rng.integers(1, 1 << 50))
            in_box[b, a] |= both
            in_ctr[b, a] |= both
    return dict(outputs=out, labels=labels, in_box=in_box, in_ctr=in_ctr, num_gt=np.array(COST_NUM_GT, dtype=np.int32), cand=cand)


# ---------------------------------------------------------------------------------------------------------------------------
# (d) ep24_assign_candidates
CAND_A = [1, 255, 256, 257, 1344]
CAND_SKIP_CAP = 1e-3


def candidates_ref(labels, xs, ys, strides):
    """labels float32 [50, 51]; xs, ys, strides float32 [A] -> dict(num_gt, deg [50, A], tol_deg, ctr [50, A]: the smallest of the
    four centre-square deltas, tol_ctr).  Rows g >= num_gt hold NaN.

    The fp32 evaluation (assign.hip::candidates_kernel) and what it can move, per edge with s = v_k - c, e = v_k+1 - c:
      xc = xs s + 0.5 s: U (|xs s| + |xc|) (zero for the integer shifts and power-of-two strides of the head: kept for the general
      case);  sx = vx - xc: e(xc) + U |sx|;  cross = sx ey - ex sy, dot = sx ex + sy ey: the product rule on the four differences,
      U per product, U on the result;  angle = atan2(|cross|, dot): since cross^2 + dot^2 = |s|^2 |e|^2 its two partial derivatives
      are at most 1 / (|s| |e|): (e(cross) + e(dot)) / (|s| |e|), + 12 U angle for the library's 6 ulp;  degrees: one more rounding;
      the sum of the 24: their errors + 24 U sum.  An anchor centre on a vertex has |s| = 0: the bound is infinite, the pair skipped.
      centre square: rad = 2.5 s: U rad;  gcx - rad: e(rad) + U |.|;  xc - (.): the two errors + U |.|; the min of four takes the
      largest of the four bounds."""
    lab = np.asarray(labels, dtype=np.float64)
    ng = int((lab.sum(1) > 0).sum())
    xs, ys, st = (np.asarray(v, dtype=np.float64) for v in (xs, ys, strides))
    A = xs.shape[0]
    xc, yc = xs * st + 0.5 * st, ys * st + 0.5 * st
    e_xc, e_yc = U * (np.abs(xs * st) + np.abs(xc)), U * (np.abs(ys * st) + np.abs(yc))
    e_xc, e_yc = np.where(np.float32(xs * st) == xs * st, 0.0, e_xc), np.where(np.float32(ys * st) == ys * st, 0.0, e_yc)
    e_xc, e_yc = e_xc + np.where(np.float32(xc) == xc, 0.0, U * np.abs(xc)), e_yc + np.where(np.float32(yc) == yc, 0.0, U * np.abs(yc))
    out = {k: np.full((G_MAX, A), np.nan) for k in ("deg", "tol_deg", "ctr", "tol_ctr")}
    out["num_gt"] = ng
    if ng == 0:
        return out
    vx, vy = lab[:ng, 3::2], lab[:ng, 4::2]                                                     # [G, 24]
    sx, sy = vx[:, None, :] - xc[None, :, None], vy[:, None, :] - yc[None, :, None]             # [G, A, 24]
    e_sx, e_sy = e_xc[None, :, None] + U * np.abs(sx), e_yc[None, :, None] + U * np.abs(sy)
    ex, ey, e_ex, e_ey = np.roll(sx, -1, 2), np.roll(sy, -1, 2), np.roll(e_sx, -1, 2), np.roll(e_sy, -1, 2)
    cross, dot = sx * ey - ex * sy, sx * ex + sy * ey
    e_cross = (e_sx * np.abs(ey) + np.abs(sx) * e_ey + e_ex * np.abs(sy) + np.abs(ex) * e_sy + U * (np.abs(sx * ey) + np.abs(ex * sy)) + U * np.abs(cross))
    e_dot = (e_sx * np.abs(ex) + np.abs(sx) * e_ex + e_sy * np.abs(ey) + np.abs(sy) * e_ey + U * (np.abs(sx * ex) + np.abs(sy * ey)) + U * np.abs(dot))
    ang = np.arctan2(np.abs(cross), dot)
    with np.errstate(all="ignore"):
        e_ang = (e_cross + e_dot) / (np.hypot(sx, sy) * np.hypot(ex, ey)) + 12 * U * ang
    k = 57.2957795130823208768
    degk = ang * k
    e_degk = e_ang * k + U * degk
    out["deg"][:ng] = degk.sum(2)
    out["tol_deg"][:ng] = np.nan_to_num((e_degk.sum(2) + 24 * U * degk.sum(2)) * SECOND, nan=np.inf)
    rad = 2.5 * st
    e_rad = np.where(np.float32(rad) == rad, 0.0, U * rad)
    gcx, gcy = lab[:ng, 1][:, None], lab[:ng, 2][:, None]
    deltas, tols = [], []
    for c, e_c, gc, sign in ((xc, e_xc, gcx, -1), (yc, e_yc, gcy, -1), (xc, e_xc, gcx, 1), (yc, e_yc, gcy, 1)):
        edge = gc + sign * rad[None, :]
        dl = (c[None, :] - edge) if sign < 0 else (edge - c[None, :])
        deltas.append(dl)
        tols.append(e_rad[None, :] + U * np.abs(edge) + e_c[None, :] + U * np.abs(dl))
    out["ctr"][:ng] = np.min(deltas, 0)
    out["tol_ctr"][:ng] = np.max(tols, 0) * SECOND
    return out


def candidates_expected(ref):
    """-> (in_box, in_ctr uint64 [A], decided_box, decided_ctr bool [50, A]: pairs outside the margin, the only ones compared)"""
    ng = ref["num_gt"]
    A = ref["deg"].shape[1]
    ib, ic = np.zeros(A, dtype=np.uint64), np.zeros(A, dtype=np.uint64)
    dec_b, dec_c = np.zeros((G_MAX, A), dtype=bool), np.zeros((G_MAX, A), dtype=bool)
    for g in range(ng):
        dec_b[g] = np.abs(ref["deg"][g] - 350.0) > ref["tol_deg"][g]
        dec_c[g] = np.abs(ref["ctr"][g]) > ref["tol_ctr"][g]
        ib |= (ref["deg"][g] >= 350.0).astype(np.uint64) << np.uint64(g)
        ic |= (ref["ctr"][g] > 0.0).astype(np.uint64) << np.uint64(g)
    return ib, ic, dec_b, dec_c


def candidates_f32(labels, xs, ys, strides):
    """float32 emulation of the kernel's two tests with numpy's atan2 and pairwise sums -> (deg, ctr float32 [ng, A])"""
    lab = np.asarray(labels, dtype=F32)
    ng = int((lab.astype(np.float64).sum(1) > 0).sum())
    xs, ys, st = (np.asarray(v, dtype=F32) for v in (xs, ys, strides))
    xc, yc = xs * st + F32(0.5) * st, ys * st + F32(0.5) * st
    vx, vy = lab[:ng, 3::2], lab[:ng, 4::2]
    sx, sy = vx[:, None, :] - xc[None, :, None], vy[:, None, :] - yc[None, :, None]
    ex, ey = np.roll(sx, -1, 2), np.roll(sy, -1, 2)
    deg = (np.arctan2(np.abs(sx * ey - ex * sy), sx * ex + sy * ey) * F32(57.2957795130823208768)).sum(2, dtype=F32)
    rad = F32(2.5) * st
    gcx, gcy = lab[:ng, 1][:, None], lab[:ng, 2][:, None]
    ctr = np.minimum(np.minimum(xc - (gcx - rad), yc - (gcy - rad)), np.minimum((gcx + rad) - xc, (gcy + rad) - yc))
    assert deg.dtype == F32 and ctr.dtype == F32
    return deg, ctr


CAND_SETS = [("convex", 50, 3), ("star", 50, 3), ("convex", 1, 4), ("star", 0, 5), ("hole", 50, 6)]


def candidate_inputs(synth, A, kind, ng, seed):
    """labels [50, 51] from synth.make_labels(size=256) (the caller passes the module: this file imports nothing of the package) and
    A anchors spread over the 1 344 of the 256-pixel grid.  'hole': 50 labels with row 24 zeroed - the count is 49 and the first 49
    rows are used, the zero row among them, as the reference model has it."""
    lab = synth.make_labels(1, ng, size=256, seed=seed, star=kind == "star")[0].numpy().astype(F32).copy()
    if kind == "hole":
        lab[24] = 0
    xs, ys, st = (v.numpy().astype(F32) for v in synth.anchor_grid(256))
    pick = np.unique(np.linspace(0, xs.shape[0] - 1, A).astype(np.int64)) if A > 1 else np.array([700])
    assert pick.size == A
    return lab, xs[pick].copy(), ys[pick].copy(), st[pick].copy()


# ---------------------------------------------------------------------------------------------------------------------------
# (e) ep24_loss_terms and ep24_loss_grad.  The gradient of a ray (geom.h::ray_loss_grad) is some sixty operations; its bound is the
# same first-order propagation, carried along mechanically: an Err is a float64 value with a bound on what the fp32 evaluation of
# the same expression can differ from it.  + - : the operands' bounds + U |result|;  x y: |x| e(y) + |y| e(x) + U |x y|;
# x / y: e(x) / |y| + |x / y| e(y) / |y| + U |x / y|;  f(x): |f'(x)| e(x) + 2 k U |f(x)| with k the library's ulp (sqrt: one
# rounding);  min, max, abs and a select on a float64 predicate do not enlarge a bound (the builders keep every predicate's
# operands apart).  The expressions below are written once and evaluated twice: on Err for the reference and its bound, on numpy
# float32 arrays for the emulation that the bound has to hold.
class Err:
    __array_priority__ = 1000

    def __init__(self, v, e=0.0):
        self.v = np.asarray(v, dtype=np.float64)
        self.e = np.broadcast_to(np.asarray(e, dtype=np.float64), self.v.shape)

    @staticmethod
    def lift(x):
        return x if isinstance(x, Err) else Err(x)

    def __add__(self, o):
        o = Err.lift(o)
        v = self.v + o.v
        return Err(v, self.e + o.e + U * np.abs(v))

    __radd__ = __add__

    def __neg__(self):
        return Err(-self.v, self.e)

    def __sub__(self, o):
        return self + (-Err.lift(o))

    def __rsub__(self, o):
        return Err.lift(o) + (-self)

    def __mul__(self, o):
        o = Err.lift(o)
        v = self.v * o.v
        return Err(v, np.abs(self.v) * o.e + np.abs(o.v) * self.e + U * np.abs(v))

    __rmul__ = __mul__

    def __truediv__(self, o):
        o = Err.lift(o)
        with np.errstate(all="ignore"):
            v = self.v / o.v
            return Err(v, np.nan_to_num(self.e / np.abs(o.v) + np.abs(v) * o.e / np.abs(o.v) + U * np.abs(v), nan=np.inf))

    def __rtruediv__(self, o):
        return Err.lift(o) / self

    def __getitem__(self, i):
        return Err(self.v[i], self.e[i])


def _fn(x, f, df, k):
    if not isinstance(x, Err):
        with np.errstate(all="ignore"):
            r = f(x)
        assert r.dtype == F32
        return r
    with np.errstate(all="ignore"):
        r = f(x.v)
        return Err(r, np.nan_to_num(np.abs(df(x.v)) * x.e + 2 * k * U * np.abs(r), nan=np.inf))


def m_sqrt(x): return _fn(x, np.sqrt, lambda v: 0.5 / np.sqrt(v), 0.5)
def m_acos(x): return _fn(x, np.arccos, lambda v: 1.0 / np.sqrt(1 - v * v), 4)
def m_sin(x): return _fn(x, np.sin, np.cos, 4)
def m_cos(x): return _fn(x, np.cos, np.sin, 4)
def m_exp(x): return _fn(x, np.exp, np.exp, 3)
def m_log(x): return _fn(x, np.log, lambda v: 1.0 / v, 3)
def m_log1p(x): return _fn(x, np.log1p, lambda v: 1.0 / (1 + v), 2)
def m_abs(x): return Err(np.abs(x.v), x.e) if isinstance(x, Err) else np.abs(x)
def val(x): return x.v if isinstance(x, Err) else x


def m_where(c, a, b):
    if isinstance(a, Err) or isinstance(b, Err):
        a, b = Err.lift(a), Err.lift(b)
        return Err(np.where(c, a.v, b.v), np.where(c, a.e, b.e))
    return np.where(c, a, b).astype(F32)


def m_const(like, c):
    return c if isinstance(like, Err) else F32(c)


def m_sum(x, axis):
    """A sum of the n terms along an axis: the terms' bounds + n U sum|terms| (float32: numpy's pairwise sum).
    Why n is enough: in any summation tree a term's error grows by U |partial sum| at each INEXACT addition it passes through, so
    the tree carries at most h U sum|terms| with h the largest number of such additions on one term's path; adding a zero is
    exact and does not count.  h <= n - 1 for the sequential and the pairwise order.  The kernels' trees (kernel_sum_depth):
      a lane's running sum over its share of the matched anchors of its wave (ceil(M / 4) of the block's M) and, for the classes,
      its ceil(C / 64) columns of each; then the butterfly over the lanes that hold something (ceil(log2(min(L, 64))) levels for L
      live lanes: 24 rays, 26 L1 columns, min(C, 64) classes, the block's anchors for the objectness), then the waves that hold
      something (at most 3 additions, M - 1 if fewer anchors).
    The nested class and L1 sums use n = C + M and 26 + M, the ray columns M, the objectness the anchors of the block; that each of
    these is at least the kernel's h is not obvious for the class sum (a lane's chain is ceil(M / 4) ceil(C / 64) long), so
    tests/test_assign_reference.py checks h <= n for every M <= 256 at every C the GPU file runs."""
    if not isinstance(x, Err):
        return x.sum(axis, dtype=F32)
    n = x.v.shape[axis]
    return Err(x.v.sum(axis), x.e.sum(axis) + n * U * np.abs(x.v).sum(axis))


def kernel_sum_depth(lane_terms, live_lanes, live_waves):
    """h of m_sum for one of loss_terms_kernel's sums: a lane adds lane_terms terms in a row, live_lanes lanes of a wave and
    live_waves waves of the block hold something"""
    return max(lane_terms - 1, 0) + int(np.ceil(np.log2(min(max(live_lanes, 1), 64)))) + min(3, max(live_waves - 1, 0))


def ray_loss_grad_expr(r1, r2, d):
    """geom.h::ray_loss_grad, expression by expression -> (loss term 1 - giou, g_r2, g_d)"""
    k = lambda c: m_const(r1, c)
    pi = k(PI32)
    pmin, pmax = val(r2) < val(r1), val(r2) > val(r1)
    rmin, rmax = m_where(pmin, r2, r1), m_where(pmax, r2, r1)
    drmin, drmax = m_where(pmin, k(1.0), k(0.0)), m_where(pmax, k(1.0), k(0.0))
    rmin2, rmax2, d2 = rmin * rmin, rmax * rmax, d * d
    contained = np.abs(val(r1) - val(r2)) >= val(d)
    disjoint = val(d) >= val(r1) + val(r2)
    den1, den2 = k(2.0) * rmin * d + k(1e-8), k(2.0) * rmax * d + k(1e-8)
    n1, n2 = rmin2 + d2 - rmax2, rmax2 + d2 - rmin2
    c1r, c2r = n1 / den1, n2 / den2
    in1, in2 = (val(c1r) >= -0.99) & (val(c1r) <= 0.99), (val(c2r) >= -0.99) & (val(c2r) <= 0.99)
    c1 = m_where(val(c1r) > 0.99, k(0.99), m_where(val(c1r) < -0.99, k(-0.99), c1r))
    c2 = m_where(val(c2r) > 0.99, k(0.99), m_where(val(c2r) < -0.99, k(-0.99), c2r))
    lens = ~(contained | disjoint)
    # outside the lens branch the cosines are not evaluated by the kernel: neutral values keep the float64 side finite
    c1, c2 = m_where(lens, c1, k(0.0)), m_where(lens, c2, k(0.0))
    a1, a2 = m_acos(c1), m_acos(c2)
    s1 = m_sin(a1)
    inter_l = a1 * rmin2 + a2 * rmax2 - rmin * d * s1
    dn1_r, dn1_d = k(2.0) * rmin * drmin - k(2.0) * rmax * drmax, k(2.0) * d
    dd1_r, dd1_d = k(2.0) * d * drmin, k(2.0) * rmin
    dn2_r, dn2_d = k(2.0) * rmax * drmax - k(2.0) * rmin * drmin, k(2.0) * d
    dd2_r, dd2_d = k(2.0) * d * drmax, k(2.0) * rmax
    zero = k(0.0)
    c1_r = m_where(in1, (dn1_r * den1 - n1 * dd1_r) / (den1 * den1), zero)
    c1_d = m_where(in1, (dn1_d * den1 - n1 * dd1_d) / (den1 * den1), zero)
    c2_r = m_where(in2, (dn2_r * den2 - n2 * dd2_r) / (den2 * den2), zero)
    c2_d = m_where(in2, (dn2_d * den2 - n2 * dd2_d) / (den2 * den2), zero)
    da1, da2 = k(-1.0) / m_sqrt(k(1.0) - c1 * c1), k(-1.0) / m_sqrt(k(1.0) - c2 * c2)
    a1_r, a1_d, a2_r, a2_d = da1 * c1_r, da1 * c1_d, da2 * c2_r, da2 * c2_d
    cos1 = m_cos(a1)
    i_r_l = (a1_r * rmin2 + a1 * k(2.0) * rmin * drmin + a2_r * rmax2 + a2 * k(2.0) * rmax * drmax
             - (drmin * d * s1 + rmin * d * cos1 * a1_r))
    i_d_l = a1_d * rmin2 + a2_d * rmax2 - (rmin * s1 + rmin * d * cos1 * a1_d)
    inter = m_where(disjoint, zero, m_where(contained, pi * rmin2, inter_l))
    i_r = m_where(disjoint, zero, m_where(contained, k(2.0) * pi * rmin * drmin, i_r_l))
    i_d = m_where(disjoint | contained, zero, i_d_l)
    area1, area2 = pi * (r1 * r1), pi * (r2 * r2)
    uni = area1 + area2 - inter
    u_r, u_d = k(2.0) * pi * r2 - i_r, -i_d
    ue = uni + k(1e-6)
    cl = m_where(contained, rmax, (r1 + r2 + d) / k(2.0))
    cl_r, cl_d = m_where(contained, drmax, k(0.5)), m_where(contained, zero, k(0.5))
    cs = pi * (cl * cl)
    cs_r, cs_d = k(2.0) * pi * cl * cl_r, k(2.0) * pi * cl * cl_d
    iou_r, iou_d = (i_r * ue - inter * u_r) / (ue * ue), (i_d * ue - inter * u_d) / (ue * ue)
    t = cs - uni
    q_r, q_d = ((cs_r - u_r) * cs - t * cs_r) / (cs * cs), ((cs_d - u_d) * cs - t * cs_d) / (cs * cs)
    loss = k(1.0) - (inter / ue - t / cs)
    return loss, -iou_r + q_r, -iou_d + q_d


def bce_expr(x, y):
    """loss.hip::bce_logits: max(x, 0) - x y + log1p(exp(-|x|)); x an input (exact)"""
    return m_where(val(x) > 0, x, m_const(x, 0.0)) - x * y + m_log1p(m_exp(-m_abs(x)))


def sigmoid_expr(x):
    return m_const(x, 1.0) / (m_const(x, 1.0) + m_exp(-x))


def l1_target_expr(lab, s, xsh, ysh):
    """loss.hip::l1_target for matched rows: lab [M, 51], s, xsh, ysh [M] (inputs) -> [M, 26]"""
    px, py = lab[:, 3::2], lab[:, 4::2]
    rad = m_log(m_sqrt(px * px + py * py) / s[:, None] + m_const(s, 1e-8))
    c0, c1 = lab[:, 1] / s - xsh, lab[:, 2] / s - ysh
    if isinstance(rad, Err):
        return Err(np.concatenate([c0.v[:, None], c1.v[:, None], rad.v], 1), np.concatenate([c0.e[:, None], c1.e[:, None], rad.e], 1))
    return np.concatenate([c0[:, None], c1[:, None], rad], 1)


def _wrap(x, f32):
    return np.asarray(x, dtype=F32) if f32 else Err(np.asarray(x, dtype=F32))


def _matched_geometry(o, lab, f32):
    """o [M, ncols], lab [M, 51] of the matched label -> r1 [M, 24], r2 [M, 24], d [M], ddx, ddy [M] as the kernels form them"""
    w = lambda x: _wrap(x, f32)
    gcx, gcy = w(lab[:, 1]), w(lab[:, 2])
    ddx, ddy = gcx - w(o[:, 0]), gcy - w(o[:, 1])
    d = m_sqrt(ddx * ddx + ddy * ddy)
    vx, vy = w(lab[:, 3::2]) - gcx[:, None], w(lab[:, 4::2]) - gcy[:, None]
    return m_sqrt(vx * vx + vy * vy), w(o[:, 2:26]), d, ddx, ddy


def terms_ref(case, l1, f32=False):
    """loss.hip::loss_terms_kernel: the partial rows [(b * blocks_per_image + block)][32].  f32 False: -> (float64 values, bounds),
    True: the float32 emulation (numpy's pairwise sums, its own transcendental functions) -> float32 values"""
    out, labels, mg, mi = case["outputs"], case["labels"], case["matched_gt"], case["matched_iou"]
    B, A, ncols = out.shape
    C = ncols - 27
    nblk = (A + 255) // 256
    w = lambda x: _wrap(x, f32)
    pv, pe = np.zeros((B * nblk, NS)), np.zeros((B * nblk, NS))
    for b in range(B):
        obj = bce_expr(w(out[b, :, 26]), w((mg[b] >= 0).astype(F32)))
        for blk in range(nblk):
            lo, hi = blk * 256, min(A, blk * 256 + 256)
            row = b * nblk + blk
            cols = {24: m_sum(obj[lo:hi], 0)}
            m = lo + np.flatnonzero(mg[b, lo:hi] >= 0)
            pv[row, 26] = m.size
            if m.size:
                o, lab = out[b, m], labels[b, mg[b, m]]
                r1, r2, d, _, _ = _matched_geometry(o, lab, f32)
                d = d[:, None] if not isinstance(d, Err) else Err(d.v[:, None], d.e[:, None])
                loss, _, _ = ray_loss_grad_expr(r1, r2, d)
                rays = m_sum(loss, 0)
                for k in range(24):
                    cols[k] = rays[k]
                tgt = np.zeros((m.size, C), dtype=F32)
                tgt[np.arange(m.size), lab[:, 0].astype(np.int64)] = mi[b, m]
                cols[25] = m_sum(m_sum(bce_expr(w(o[:, 27:]), w(tgt)), 1), 0)
                if l1:
                    t = l1_target_expr(w(lab), w(case["strides"][m]), w(case["xs"][m]), w(case["ys"][m]))
                    cols[27] = m_sum(m_sum(m_abs(w(case["origin"][b, m]) - t), 1), 0)
            for c, x in cols.items():
                pv[row, c], pe[row, c] = (x, 0.0) if f32 else (x.v, x.e)
    return pv.astype(F32) if f32 else (pv, pe * SECOND)


def grad_ref(case, result, grad_scale, l1, f32=False):
    """loss.hip::loss_grad_kernel -> dout [B, A, ncols] (and d_origin [B, A, 26] or None): float64 values and bounds, or the float32
    emulation.  result: the float32 [64] block of ep24_loss_finalize (an input); grad_scale: None or a float32 number."""
    out, labels, mg, mi = case["outputs"], case["labels"], case["matched_gt"], case["matched_iou"]
    B, A, ncols = out.shape
    w = lambda x: _wrap(x, f32)
    res = w(result)
    gs = w(np.float32(1.0 if grad_scale is None else grad_scale)) / res[27]
    dv, de = np.zeros((B, A, ncols)), np.zeros((B, A, ncols))
    ov, oe = (np.zeros((B, A, 26)), np.zeros((B, A, 26))) if l1 else (None, None)
    put = lambda av, ae, idx, x: (av.__setitem__(idx, x), None) if f32 else (av.__setitem__(idx, x.v), ae.__setitem__(idx, x.e))
    for b in range(B):
        so = sigmoid_expr(w(out[b, :, 26]))
        put(dv, de, (b, slice(None), 26), res[53] * gs * (so - w((mg[b] >= 0).astype(F32))))
        m = np.flatnonzero(mg[b] >= 0)
        if not m.size:
            continue
        o, lab = out[b, m], labels[b, mg[b, m]]
        r1, r2, d, ddx, ddy = _matched_geometry(o, lab, f32)
        d1 = d[:, None] if not isinstance(d, Err) else Err(d.v[:, None], d.e[:, None])
        _, g_r, g_d = ray_loss_grad_expr(r1, r2, d1)
        wk = res[29:53] * gs
        wk = wk[None, :] if not isinstance(wk, Err) else Err(wk.v[None, :], wk.e[None, :])
        put(dv, de, (b, m, slice(2, 26)), wk * g_r)
        gd = m_sum(wk * g_d, 1)
        put(dv, de, (b, m, 0), gd * (-ddx / d))
        put(dv, de, (b, m, 1), gd * (-ddy / d))
        tgt = np.zeros((m.size, ncols - 27), dtype=F32)
        tgt[np.arange(m.size), lab[:, 0].astype(np.int64)] = mi[b, m]
        put(dv, de, (b, m, slice(27, None)), (res[54] * gs) * (sigmoid_expr(w(o[:, 27:])) - w(tgt)))
        if l1:
            t = l1_target_expr(w(lab), w(case["strides"][m]), w(case["xs"][m]), w(case["ys"][m]))
            e = w(case["origin"][b, m]) - t
            ev, ee = (e, 0.0) if f32 else (e.v, e.e)
            assert f32 or bool(np.all(np.abs(ev) > 100 * ee)), "a sign of d_origin is not decided by construction"
            gv = val(gs)
            ov[b, m] = np.sign(ev) * gv
            if not f32:
                oe[b, m] = gs.e
    if f32:
        return dv.astype(F32), None if ov is None else ov.astype(F32)
    return dv, de * SECOND, ov, None if oe is None else oe * SECOND


LOSS_A = [1, 255, 256, 257, 513]
LOSS_C = [1, 3, 80, 101, 229, 230]
PATTERNS = ["all", "lanes", "one", "none", "random"]


@functools.lru_cache(maxsize=8)
def loss_case(A, C, shift, seed=0):
    """B = 4 images; block k of image b is matched by PATTERNS[(b + k + shift) % 5]: all its anchors, lanes 0 and 63 of each wave,
    one anchor, none, a random 1 %.  Labels and predictions as cost_case builds them (every ray in its branch against every label,
    a mix of lens, contained and disjoint rays); matched labels reach index 49; origin sits 0.01 .. 1 from the L1 target."""
    rng = np.random.default_rng(9000 + 1000 * shift + 10 * A + C + seed)
    B = 4
    ang = np.arange(24) * (np.pi / 12)
    labels = np.zeros((B, G_MAX, LCOLS), dtype=F32)
    cx, cy = 100 + 10 * rng.random((B, G_MAX)), 100 + 10 * rng.random((B, G_MAX))
    r = 30 + 10 * rng.random((B, G_MAX, 24))
    labels[..., 0] = rng.integers(0, C, (B, G_MAX))
    labels[..., 1], labels[..., 2] = cx, cy
    labels[..., 3::2], labels[..., 4::2] = cx[..., None] + r * np.cos(ang), cy[..., None] + r * np.sin(ang)
    out = np.zeros((B, A, 27 + C), dtype=F32)
    out[..., 26:] = np.clip(rng.standard_normal((B, A, 1 + C)) * 1.5, -3, 3)
    kind = rng.integers(0, 4, (B, A))[..., None]
    near = np.stack([130 + 5 * rng.random((B, A)), 100 + 10 * rng.random((B, A))], -1)
    inside, far = 100 + 10 * rng.random((B, A, 2)), 400 + 200 * rng.random((B, A, 2))
    r_lens, r_big, r_small = 30 + 10 * rng.random((B, A, 24)), 80 + 10 * rng.random((B, A, 24)), 2 + 3 * rng.random((B, A, 24))
    out[..., :2] = np.where(kind <= 1, near, np.where(kind == 2, inside, far))
    per_ray = np.where(rng.integers(0, 2, (B, A, 24)) == 0, r_lens, r_big)
    out[..., 2:26] = np.where(kind <= 1, per_ray, np.where(kind == 2, r_small, r_lens))
    mg = np.full((B, A), -1, dtype=np.int32)
    pats = {}
    for b in range(B):
        for blk in range((A + 255) // 256):
            lo, hi = blk * 256, min(A, blk * 256 + 256)
            p = PATTERNS[(b + blk + shift) % 5]
            pats[(b, blk)] = p
            t = np.arange(hi - lo)
            sel = {"all": t >= 0, "lanes": (t % 64 == 0) | (t % 64 == 63), "one": t == (hi - lo) // 2, "none": t < 0,
                   "random": rng.random(hi - lo) < 0.01}[p]
            g = rng.integers(0, G_MAX, hi - lo)
            g[::7] = 49
            mg[b, lo:hi] = np.where(sel, g, -1)
    mi = rng.random((B, A)).astype(F32)
    xs, ys = rng.integers(0, 32, A).astype(F32), rng.integers(0, 32, A).astype(F32)
    st = np.array([8.0, 16.0, 32.0], dtype=F32)[rng.integers(0, 3, A)]
    c = dict(outputs=out, labels=labels, matched_gt=mg, matched_iou=mi, xs=xs, ys=ys, strides=st, patterns=pats)
    lab_m = labels[np.arange(B)[:, None], np.maximum(mg, 0)].reshape(B * A, LCOLS).astype(np.float64)
    t = l1_target_expr(Err(lab_m), Err(np.tile(st, B)), Err(np.tile(xs, B)), Err(np.tile(ys, B))).v.reshape(B, A, 26)
    off = (0.01 + 0.99 * rng.random((B, A, 26))) * np.where(rng.integers(0, 2, (B, A, 26)) == 0, -1.0, 1.0)
    c["origin"] = (t + off).astype(F32)
    return c


def loss_result(seed=0):
    """a result block as ep24_loss_finalize leaves it, for the gradient's tests: weights near 1, num_fg a power of two"""
    rng = np.random.default_rng(700 + seed)
    res = np.zeros(64, dtype=F32)
    res[29:55] = (0.9 + 0.2 * rng.random(26)).astype(F32)
    res[27] = res[55] = 64.0
    return res


# ---------------------------------------------------------------------------------------------------------------------------
# (f) the comparison both test files use
def check_bound(got_bits, want, tol, what):
    """got_bits: uint32 patterns of fp32 results; want, tol float64.  Where tol == 0 the pattern must be the one of float32(want)
    (+0 for a zero); elsewhere |got - want| <= tol.  -> the largest err / tol (the caller prints it, then asserts <= 1)"""
    got_bits, want, tol = np.asarray(got_bits, dtype=np.uint32).reshape(-1), np.asarray(want).reshape(-1), np.asarray(tol).reshape(-1)
    exact = tol == 0
    assert_same(got_bits[exact], bits32(want[exact].astype(F32)), what + " (exact part)")
    if exact.all():
        return 0.0
    return err_ratio(from_bits32(got_bits[~exact]), want[~exact], tol[~exact])


def u64(a):
    return np.ascontiguousarray(a, dtype=np.uint64).view(np.int64)
