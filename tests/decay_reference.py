"""References of the weight update with weight decay by parameter group (ep24_sgd_nesterov_decay, ep24_sgd_nesterov_decay_hp_range_pack,
ep24_set_hparams_decay).  A helper, not a test module: tests/test_decay_reference.py checks it on the CPU (the formula against
torch.optim.SGD, the float32 emulation within the bound, three mutants rejected, the dyadic draws exact), tests/test_gpu_decay_exact.py
runs the kernels against it.  Bit patterns, sentinels, layouts and the draws without decay come from tests/update_reference.py; like
that file this one never imports the package under test.

The update (include/ep24.h, a11), g scaled first, the decay product formed only for a decaying group:
    gs = g*s     d = decays ? gs + w*p : gs     b' = first ? d : m*b + d     p' = p - lr*(d + m*b')
decay_grp[e >> 6] != 0: element e of the flat buffer decays (one byte per 64 elements; segments start at multiples of 64).
"""
import functools

import numpy as np

import update_reference as R

U = R.U
# The bound's only constant: second-order terms (a rounding acts on the computed, not the exact, operand).  The same value as
# update_reference.SECOND, for the same reason; every other factor below is U times the magnitude of a float64 intermediate.
SECOND = 1.0 + 2.0 ** -20


def sgd_decay_ref(p, g, b, first, lr, m, s, w, dec):
    """float64 in, float64 out: (p', b', intermediates).  dec: bool [n].  With first the momentum buffer is not read."""
    gs = g * s
    wp = np.where(dec, w * p, 0.0)
    d = np.where(dec, gs + wp, gs)
    mb = None if first else m * b
    b2 = d if first else mb + d
    mb2 = m * b2
    t = d + mb2
    lt = lr * t
    p2 = p - lt
    return p2, b2, dict(gs=gs, wp=wp, d=d, mb=mb, b2=b2, mb2=mb2, t=t, lt=lt, p2=p2)


def sgd_decay_f32(p, g, b, first, lr, m, s, w, dec):
    """The same, op by op in float32 (every product and sum rounded on its own, as -ffp-contract=off compiles it)."""
    f = np.float32
    p, g = np.asarray(p, dtype=f), np.asarray(g, dtype=f)
    lr, m, s, w = f(lr), f(m), f(s), f(w)
    with np.errstate(all="ignore"):
        gs = g * s
        d = np.where(dec, gs + w * p, gs).astype(f)
        b2 = d if first else (m * np.asarray(b, dtype=f) + d).astype(f)
        p2 = (p - lr * (d + m * b2)).astype(f)
    return p2, b2


def decay_tol(mid, first, lr, m, dec):
    """Per-element bounds (tol p', tol b') of an fp32 evaluation against float64, built like update_reference.general_tol: every
    rounding contributes at most U times the magnitude of the value it rounds, an error entering a product is scaled by its constant.
    One more term than there: the decay product and the sum that takes it in (decaying elements only; p itself is an input, exact).
        d(gs) = U |gs|        d(wp) = U |w p|        d(d) = decays ? d(gs) + d(wp) + U |d| : d(gs)
        d(b') = first ? d(d) : d(d) + U |m b| + U |b'|
        d(mb') = m d(b') + U |m b'|      d(t) = d(d) + d(mb') + U |t|      d(lt) = lr d(t) + U |lr t|      d(p') = d(lt) + U |p'|
    """
    a = {k: (None if v is None else np.abs(v)) for k, v in mid.items()}
    d_gs = U * a["gs"]
    d_d = np.where(dec, d_gs + U * a["wp"] + U * a["d"], d_gs)
    d_b = d_d if first else d_d + U * a["mb"] + U * a["b2"]
    d_mb2 = m * d_b + U * a["mb2"]
    d_t = d_d + d_mb2 + U * a["t"]
    d_lt = lr * d_t + U * a["lt"]
    d_p = d_lt + U * a["p2"]
    return d_p * SECOND, d_b * SECOND


# ---------------------------------------------------------------------------------------------------------------------------
# mutants of the formula (float64), each rejected by the comparison with torch.optim.SGD in tests/test_decay_reference.py
def mutant_decoupled(p, g, b, first, lr, m, s, w, dec):
    """AdamW-style: the decay leaves the momentum alone, p -= lr*w*p beside the update"""
    p2, b2, _ = sgd_decay_ref(p, g, b, first, lr, m, s, 0.0, dec)
    return p2 - np.where(dec, lr * w * p, 0.0), b2, None


def mutant_before_scale(p, g, b, first, lr, m, s, w, dec):
    """the decay added to the raw gradient, so that grad_scale scales it too"""
    return sgd_decay_ref(p, g + np.where(dec, w * p, 0.0), b, first, lr, m, s, 0.0, dec)


def mutant_every_group(p, g, b, first, lr, m, s, w, dec):
    """the table ignored: every group decays"""
    return sgd_decay_ref(p, g, b, first, lr, m, s, w, np.ones_like(dec))


MUTANTS = {"decoupled": mutant_decoupled, "before_scale": mutant_before_scale, "every_group": mutant_every_group}


# ---------------------------------------------------------------------------------------------------------------------------
# the table, from the header's text: one byte per 64 flat elements, non-zero = the group decays
def table_from_layout(L, decaying=None):
    """uint8 [max(L.numel / 64, 1)] of an update_reference layout: the conv segments whose index is in `decaying` (default: all of
    them) decay with their alignment padding, vectors never do."""
    tab = np.zeros(max(L.numel // 64, 1), dtype=np.uint8)
    for i, s in enumerate(L.segs):
        if decaying is None or i in decaying:
            tab[s["off"] // 64:R.r64(s["off"] + s["numel"]) // 64] = 1
    return tab


def alternating_table(n_total):
    """1, 0, 1, 0, ... over ceil(n_total / 64) groups: a launch of more than 64 elements crosses both kinds"""
    k = (n_total + 63) // 64
    return (1 - np.arange(k) % 2).astype(np.uint8)


def elements(table, n_total):
    """bool [n_total]: does element e decay"""
    return np.asarray(table)[np.arange(n_total) >> 6] != 0


# ---------------------------------------------------------------------------------------------------------------------------
# dyadic draws.  lr, m, s and w are powers of two, so a product only moves the exponent; what grows is the grid.  p = k/2 (|k| <= 32),
# g = k (|k| <= 8), b = k (|k| <= 8), lr = w = 1/4, m = s = 1/2:  gs on 2^-1, w*p on 2^-3, d on 2^-3, t on 2^-4, p' on 2^-6 after
# the first step; 2^-11 after the second (d on 2^-8, t on 2^-9), 2^-16 after the third (d 2^-13, t 2^-14), all below 32 in
# magnitude: at most 21 significant bits.  tests/test_decay_reference.py asserts that every intermediate is an fp32 number.
HP_DYADIC = (0.25, 0.5, 0.5)          # lr, momentum, grad_scale
W_DYADIC = 0.25
STEPS = 3
HP_GENERAL = R.HP_GENERAL
W_GENERAL = R.f32(5e-4)
LENGTHS = [1, 3, 4, 5, 63, 64, 65, 194]
STARTS = [0, 4, 64, 68]
CAP_N = 2048 * 1024 + 1024 + 3        # just above the grid cap of the update: 2048 workgroups x 256 lanes x 4 elements


def dyadic_draw(n, seed):
    """-> p [n], b [n], g [STEPS][n] float64, e [n] float32"""
    rng = np.random.default_rng(3000 + seed)
    p = rng.integers(-32, 33, n).astype(np.float64) / 2.0
    b = rng.integers(-8, 9, n).astype(np.float64)
    g = [rng.integers(-8, 9, n).astype(np.float64) for _ in range(STEPS)]
    e = rng.standard_normal(n).astype(np.float32)
    return p, b, g, e


def run_steps(p, b, g, e, hp, w, dec, first=True):
    """Consecutive steps from (p, b, e): -> [(p', b', e', intermediates)], float64 / float64 / float32; `first` holds for the first."""
    lr, m, s = hp
    out = []
    for k, gk in enumerate(g):
        p, b, mid = sgd_decay_ref(p, gk, b, first and k == 0, lr, m, s, w, dec)
        e = None if e is None else R.ema_ref(e, p.astype(np.float32), R.EMA_D, R.EMA_OMD)
        out.append((p, b, e, mid))
    return out


@functools.lru_cache(maxsize=8)
def dyadic_case(n_total, first=True, seed=0):
    """Inputs and expected bit patterns of the dyadic steps over a flat buffer of n_total elements under the alternating table
    (shared by the tests that run it; treat as read-only).  first: the first step ignores the buffer; otherwise it reads b0.
    -> dict(table, p0, b0, e0: patterns [n_total]; g: [patterns] * STEPS; want: [(p, b, e) patterns] * STEPS)"""
    p, b, g, e = dyadic_draw(n_total, seed)
    table = alternating_table(n_total)
    steps = run_steps(p, b, g, e, HP_DYADIC, W_DYADIC, elements(table, n_total), first)
    return dict(table=table, p0=R.bits32(p), b0=R.bits32(b), e0=R.bits32(e), g=[R.bits32(x) for x in g],
                want=[(R.bits32(q), R.bits32(c), R.bits32(f)) for q, c, f, _ in steps], mids=[mid for _, _, _, mid in steps])


@functools.lru_cache(maxsize=4)
def general_case(n, first=False, seed=0):
    """Normal draws (update_reference.general_draw), lr = 0.0123, m = 0.9, s = 0.5, w = 5e-4 as fp32 numbers, the alternating table:
    float64 results, their bounds, and the float32 emulation's patterns."""
    p, g, b = R.general_draw(n, seed)
    table = alternating_table(n)
    dec = elements(table, n)
    lr, m, s = HP_GENERAL
    p2, b2, mid = sgd_decay_ref(p.astype(np.float64), g.astype(np.float64), b.astype(np.float64), first, lr, m, s, W_GENERAL, dec)
    tp, tb = decay_tol(mid, first, lr, m, dec)
    ep, eb = sgd_decay_f32(p, g, b, first, lr, m, s, W_GENERAL, dec)
    return dict(table=table, dec=dec, p0=R.bits32(p), g=R.bits32(g), b0=R.bits32(b), p=p2, b=b2, tol_p=tp, tol_b=tb,
                emu_p=R.bits32(ep), emu_b=R.bits32(eb))
