"""References, draws, layouts and sentinel buffers of the weight-update and packing kernels (ep24_sgd_nesterov, _hp, _hp_range,
_hp_range_pack, ep24_pack_weights, ep24_pack_weights_batched, ep24_cast_f32_bf16, ep24_cast_bf16_f32, ep24_memset_zero).  A helper, not
a test module: tests/test_update_reference.py checks it on the CPU (the formulas against torch.optim.SGD and the oracle, the exactness
of every dyadic case, the general bound against two float32 emulations, every table against the header's definition, and that each
mutant is rejected), and tests/test_gpu_update_exact.py runs the kernels against it.  It never imports the package under test: the
layouts are built from the text of include/ep24.h alone.

Everything that is compared bit for bit travels as raw bit patterns (numpy uint32 for fp32, uint16 for bf16); NaN equals NaN whatever
its payload, every other pattern only itself.

The update (include/ep24.h, a11), g scaled first:
    b' = first ? g*s : m*b + g*s          p' = p - lr*(g*s + m*b')          e' = fl32(fl32(e*d) + fl32((1-d)*p'))
wf_delta[e >> 6] = (offset of element e's segment in w_fwd) - (its offset in the flat buffer), INT32_MIN for a group without a copy;
the update writes bf16(p'[e]) to w_fwd[e + wf_delta[e >> 6]] for every element e of its range whose group has one.
"""
import functools

import numpy as np
import torch

U = 2.0 ** -24                    # unit roundoff of fp32
GUARD = 64                        # elements of sentinel before and after every buffer (>= 128 bytes: alignment is kept)
SENT32 = 0xFFA5A5A5               # a negative NaN with a payload no kernel here produces (they propagate or make 0x7FC00000)
SENT16 = 0xFFA5
SENT8 = 0xA5
NAN32 = 0x7FC00000
INT32_MIN = -2 ** 31
SENT64 = 0xFFF5A5A5A5A5A5A5       # the float64 twin of SENT32: a negative NaN with a payload
_NP = {"f32": np.uint32, "bf16": np.uint16, "u8": np.uint8, "i32": np.int32, "i64": np.int64, "f64": np.uint64}
_SENT = {"f32": SENT32, "bf16": SENT16, "u8": SENT8, "i32": 0x5A5A5A5A, "i64": 0x5A5A5A5A5A5A, "f64": SENT64}
_TORCH = {"f32": (np.int32, torch.float32), "bf16": (np.int16, torch.bfloat16), "u8": (np.uint8, torch.uint8),
          "i32": (np.int32, torch.int32), "i64": (np.int64, torch.int64), "f64": (np.int64, torch.float64)}


def r8(v):
    return (v + 7) // 8 * 8


def r64(v):
    return (v + 63) // 64 * 64


def f32(x):
    """A float argument as the C ABI receives it."""
    return float(np.float32(x))


# ---------------------------------------------------------------------------------------------------------------------------
# (a) bit patterns and bf16 rounding
def bits32(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def from_bits32(b):
    return np.ascontiguousarray(b, dtype=np.uint32).view(np.float32)


def is_nan32(b):
    return (np.asarray(b, dtype=np.uint32) & np.uint32(0x7FFFFFFF)) > np.uint32(0x7F800000)


def is_nan16(b):
    return (np.asarray(b, dtype=np.uint16) & np.uint16(0x7FFF)) > np.uint16(0x7F80)


def bf16_rne(b32):
    """fp32 bit patterns -> bf16 bit patterns, round to nearest even on the integer pattern; every NaN becomes 0x7FC0 (a payload is
    not part of the contract: compare with same_bits, which takes NaN for NaN)."""
    u = np.asarray(b32, dtype=np.uint32).astype(np.uint64)
    r = (((u + 0x7FFF + ((u >> 16) & 1)) >> 16) & 0xFFFF).astype(np.uint16)
    r[is_nan32(b32)] = 0x7FC0
    return r


def bf16_widen(b16):
    return np.asarray(b16, dtype=np.uint16).astype(np.uint32) << np.uint32(16)


def mismatches(got, want):
    """Indices where two arrays of bit patterns differ; for uint32 / uint16 patterns NaN equals NaN."""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (got.shape, want.shape, got.dtype, want.dtype)
    bad = got != want
    if got.dtype == np.uint32:
        bad &= ~(is_nan32(got) & is_nan32(want))
    elif got.dtype == np.uint16:
        bad &= ~(is_nan16(got) & is_nan16(want))
    return np.flatnonzero(bad.reshape(-1))


def same_bits(got, want):
    return mismatches(got, want).size == 0


def assert_same(got, want, what):
    bad = mismatches(got, want)
    if bad.size:
        i = int(bad[0])
        g, w = np.asarray(got).reshape(-1)[i], np.asarray(want).reshape(-1)[i]
        raise AssertionError("%s: %d of %d elements differ, first at %d: got 0x%X, want 0x%X" % (what, bad.size, np.asarray(got).size, i, int(g), int(w)))


# (b) fp32 patterns at the edges of the rounding, with the bf16 pattern each must give (written out by hand, not by bf16_rne).
# No denormals: whether they are flushed is a compile mode, not a contract of these kernels.
SPECIAL = [
    (0x3F808000, 0x3F80), (0x3F818000, 0x3F82), (0xBF808000, 0xBF80), (0xBF818000, 0xBF82),      # ties: to the even neighbour
    (0x3F807FFF, 0x3F80), (0x3F808001, 0x3F81), (0x3F817FFF, 0x3F81), (0x3F818001, 0x3F82),      # one below / above the tie
    (0x00000000, 0x0000), (0x80000000, 0x8000), (0x7F800000, 0x7F80), (0xFF800000, 0xFF80),      # zeros, infinities
    (0x7FC00000, 0x7FC0),                                                                         # NaN (isnan only)
    (0x7F7FFFFF, 0x7F80), (0xFF7FFFFF, 0xFF80), (0x7F7F8000, 0x7F80),                            # the largest numbers round to inf
    (0x00800000, 0x0080), (0x80800000, 0x8080),                                                  # the smallest normal number
]
SPECIAL32 = np.array([a for a, _ in SPECIAL], dtype=np.uint32)
SPECIAL16 = np.array([b for _, b in SPECIAL], dtype=np.uint16)


def random_bits(n, seed):
    """n fp32 patterns: random sign, exponent field 1 .. 254 (no zero, denormal, inf, NaN), random mantissa, with the patterns of (b)
    at the front, in the middle and at the very end as far as n allows."""
    rng = np.random.default_rng(seed)
    b = rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
    e = rng.integers(1, 255, n, dtype=np.uint64).astype(np.uint32)
    b = (b & np.uint32(0x807FFFFF)) | (e << np.uint32(23))
    k = SPECIAL32.size
    for at in (0, n // 2 + 1, n - k):
        if 0 <= at and at + k <= n:
            b[at:at + k] = SPECIAL32
    return b


# ---------------------------------------------------------------------------------------------------------------------------
# (c) the update in float64, with every intermediate
def sgd_ref(p, g, b, first, lr, m, s):
    """float64 in, float64 out: (p', b', intermediates).  With first the momentum buffer is not read."""
    gs = g * s
    mb = None if first else m * b
    b2 = gs if first else mb + gs
    mb2 = m * b2
    t = gs + mb2
    lt = lr * t
    p2 = p - lt
    return p2, b2, dict(gs=gs, mb=mb, b2=b2, mb2=mb2, t=t, lt=lt, p2=p2)


def ema_ref(e, p, d, omd):
    """float32 arrays in, float32 out: two rounded products and a rounded sum (ModelEMA.update: v *= d; v += (1 - d) * p)."""
    e, p = np.asarray(e, dtype=np.float32), np.asarray(p, dtype=np.float32)
    with np.errstate(all="ignore"):
        return (e * np.float32(d)).astype(np.float32) + (np.float32(omd) * p).astype(np.float32)


EMA_D = 0.99871
EMA_OMD = 1.0 - EMA_D            # formed in double on the host and rounded by the call, as ep24.ema does

# (d) dyadic draws: p = k 2^-6 (|k| <= 1024), g and b = k 2^-4 (|k| <= 64), lr = 2^-5, momentum = 3/4, grad_scale = 1/2.  b' is a
# multiple of 2^-6 after one step, p' of 2^-13, 2^-15, 2^-17 after one, two, three steps with |p'| < 32: 18, 20, 22 significant bits
# (the fourth step reaches 24).  Every product and sum is an fp32 number, so fused or separate multiply-adds give the same bits.
HP_DYADIC = (2.0 ** -5, 0.75, 0.5)
STEPS = 3
SGD_N = [1, 3, 4, 5, 1023, 1024, 1025, 4100, 1 << 21, (1 << 21) + 4, (1 << 21) + 1027]


def dyadic_draw(n, seed, steps=STEPS):
    """-> p [n], b [n], g [steps][n] float64 (b is what the buffer would hold: the first step must not read it), e [n] float32"""
    rng = np.random.default_rng(1000 + seed)
    p = rng.integers(-1024, 1025, n).astype(np.float64) / 64.0
    b = rng.integers(-64, 65, n).astype(np.float64) / 16.0
    g = [rng.integers(-64, 65, n).astype(np.float64) / 16.0 for _ in range(steps)]
    e = rng.standard_normal(n).astype(np.float32) + np.float32(2.0) * (rng.integers(0, 2, n).astype(np.float32) - np.float32(0.5))
    return p, b, g, e


def run_steps(p, b, g, e, hp, first=True, mask=None):
    """Consecutive steps of (c) from (p, b, e): -> [(p', b', e', intermediates)] per step, float64 / float64 / float32.  `first`
    holds for the first of them.  mask (bool [n]): elements outside it hold zeros in p, g and b (alignment padding)."""
    lr, m, s = hp
    if mask is not None:
        p, b, g = np.where(mask, p, 0.0), np.where(mask, b, 0.0), [np.where(mask, x, 0.0) for x in g]
    out = []
    for k, gk in enumerate(g):
        p, b, mid = sgd_ref(p, gk, b, first and k == 0, lr, m, s)
        e = None if e is None else ema_ref(e, p.astype(np.float32), EMA_D, EMA_OMD)
        out.append((p, b, e, mid))
    return out


def exact32(x):
    return bool(np.all(x.astype(np.float32).astype(np.float64) == x))


@functools.lru_cache(maxsize=4)
def dyadic_case(n, seed=0):
    """Inputs and expected bit patterns of the three dyadic steps at size n (shared by the tests that run it; treat as read-only).
    -> dict(p0, b0, e0: uint32 [n]; g: [uint32 [n]] * 3; want: [(p, b, e) uint32] * 3)"""
    p, b, g, e = dyadic_draw(n, seed)
    steps = run_steps(p, b, g, e, HP_DYADIC)
    return dict(p0=bits32(p), b0=bits32(b), e0=bits32(e), g=[bits32(x) for x in g],
                want=[(bits32(q), bits32(c), bits32(f)) for q, c, f, _ in steps])


# (f) the general draw: normal p, g, b; lr = 0.0123, m = 0.9, s = 0.5, as fp32 numbers
HP_GENERAL = (f32(0.0123), f32(0.9), f32(0.5))
GENERAL_N = [4100, (1 << 21) + 1027]
SECOND = 1.0 + 2.0 ** -20         # the second-order terms (a rounding acts on the computed, not the exact, operand)


def general_draw(n, seed=0):
    rng = np.random.default_rng(2000 + seed)
    return tuple(rng.standard_normal(n).astype(np.float32) * np.float32(sc) for sc in (1.0, 0.3, 0.5))     # p, g, b


def general_tol(mid, first, hp):
    """Per-element bounds (tol p', tol b') of an fp32 evaluation of (c) against float64, from the float64 intermediates `mid`: each
    fp32 rounding on the path contributes at most U = 2^-24 times the magnitude of the value it rounds, and an error that enters a
    later product is scaled by that product's constant.  A fused multiply-add only drops the product's term.
        d(gs) = U |gs|                         d(mb) = U |m b|             d(b') = d(gs) + d(mb) + U |b'|      (first: d(b') = d(gs))
        d(mb') = m d(b') + U |m b'|            d(t)  = d(gs) + d(mb') + U |t|
        d(lt)  = lr d(t) + U |lr t|            d(p') = d(lt) + U |p'|
    """
    lr, m, _ = hp
    a = {k: (None if v is None else np.abs(v)) for k, v in mid.items()}
    d_gs = U * a["gs"]
    d_b = d_gs if first else d_gs + U * a["mb"] + U * a["b2"]
    d_mb2 = m * d_b + U * a["mb2"]
    d_t = d_gs + d_mb2 + U * a["t"]
    d_lt = lr * d_t + U * a["lt"]
    d_p = d_lt + U * a["p2"]
    return d_p * SECOND, d_b * SECOND


@functools.lru_cache(maxsize=2)
def general_case(n, seed=0):
    p, g, b = general_draw(n, seed)
    p2, b2, mid = sgd_ref(p.astype(np.float64), g.astype(np.float64), b.astype(np.float64), False, *HP_GENERAL)
    tp, tb = general_tol(mid, False, HP_GENERAL)
    return dict(p0=bits32(p), g=bits32(g), b0=bits32(b), p=p2, b=b2, tol_p=tp, tol_b=tb)


def err_ratio(got32, want64, tol):
    """Largest |got - want| / tol; inf where got is not finite."""
    got = np.asarray(got32, dtype=np.float32).astype(np.float64)
    with np.errstate(all="ignore"):
        r = np.abs(got - want64) / np.maximum(tol, 1e-300)
    r[~np.isfinite(got)] = np.inf
    return float(r.max())


# ---------------------------------------------------------------------------------------------------------------------------
# (g) pack references: real positions only.  `image` is the bit image (uint16) of the whole destination buffer, prefilled by the
# caller with what the kernel must leave alone; master is a uint32 image of the fp32 source.
def master_rows(master, off, Cout, T, Cin, ld_w=None):
    """-> uint32 [Cout][T][Cin] of a master stored at element `off`, rows ld_w apart (default T * Cin: flat)"""
    ld_w = T * Cin if ld_w is None else ld_w
    if ld_w == T * Cin:
        return master[off:off + Cout * T * Cin].reshape(Cout, T, Cin)
    idx = off + np.arange(Cout)[:, None] * ld_w + np.arange(T * Cin)[None, :]
    return master[idx].reshape(Cout, T, Cin)


def pack_fwd_into(image, wf_off, w, Cin_pad):
    """forward copy [Cout][T][Cin_pad] at element wf_off of image <- bf16(w [Cout][T][Cin])"""
    Cout, T, Cin = w.shape
    image[wf_off:wf_off + Cout * T * Cin_pad].reshape(Cout, T, Cin_pad)[:, :, :Cin] = bf16_rne(w)


def pack_dgrad_into(image, wd_off, w, Cout_pad):
    """transposed copy [Cin][T][Cout_pad] at element wd_off of image <- bf16(w [Cout][T][Cin])"""
    Cout, T, Cin = w.shape
    image[wd_off:wd_off + Cin * T * Cout_pad].reshape(Cin, T, Cout_pad)[:, :, :Cout] = bf16_rne(w).transpose(2, 1, 0)


PACK_SHAPES = [(27, 1, 64, 64, 32, 64), (32, 1, 108, 112, 32, 108), (65, 9, 36, 40, 72, 9 * 36 + 5), (130, 9, 451, 456, 136, 9 * 451)]


# ---------------------------------------------------------------------------------------------------------------------------
# (h) layouts, from include/ep24.h:
#   desc [n_seg][8] = {master offset, w_fwd offset, w_dgrad offset or -1, Cout, T, Cin, Cin_pad, Cout_pad}
#   prefix [n_seg + 1] = running sum of Cout*T*Cin;  tile_prefix [n_seg + 1] = running sum of T*ceil(Cout/64)*ceil(Cin/64)
#   chunk_seg [ceil(total/4096)] = segment of element 4096 c;  tile_seg [total_tiles] = segment of tile t
#   wf_delta [flat / 64]: segments start at multiples of 64 in the flat buffer; a conv whose Cin is a multiple of 8 has its packed
#   layout in the flat buffer already and gets (w_fwd offset) - (flat offset) in each of its groups, everything else INT32_MIN
class Layout:
    pass


def build_layout(items, shifts=None):
    """items: (Cout, T, Cin, need_dgrad) for a conv segment, ("vec", numel) for flat elements without a packed copy.  The flat buffer
    and w_fwd advance in multiples of 64 elements, w_dgrad by Cin*T*Cout_pad.  shifts: {item index: dict(off=, wf=, wd=)} adds to
    that segment's computed offsets (what follows starts at the next multiple of 64 behind it); a shifted segment gets no
    wf_delta entries."""
    shifts = shifts or {}
    L = Layout()
    L.segs, L.vecs = [], []
    n = wf = wd = 0
    for i, it in enumerate(items):
        sh = shifts.get(i, {})
        if it[0] == "vec":
            L.vecs.append((n, it[1]))
            n += r64(it[1])
            continue
        Cout, T, Cin, need = it
        s = dict(cout=Cout, taps=T, cin=Cin, need_dgrad=bool(need), cin_pad=r8(Cin), cout_pad=r8(Cout), numel=Cout * T * Cin,
                 off=n + sh.get("off", 0), wf_off=wf + sh.get("wf", 0), wd_off=(wd + sh.get("wd", 0)) if need else -1, shifted=bool(sh))
        s["wf_numel"], s["wd_numel"] = Cout * T * s["cin_pad"], (Cin * T * s["cout_pad"] if need else 0)
        n = r64(s["off"] + s["numel"])
        wf = r64(s["wf_off"] + s["wf_numel"])
        if need:
            wd = s["wd_off"] + s["wd_numel"]
            if "wd" in sh:
                wd = r64(wd)
        L.segs.append(s)
    L.numel, L.wf_numel, L.wd_numel, L.n_seg = n, max(wf, 8), max(wd, 8), len(L.segs)
    L.desc = np.array([[s["off"], s["wf_off"], s["wd_off"], s["cout"], s["taps"], s["cin"], s["cin_pad"], s["cout_pad"]] for s in L.segs],
                      dtype=np.int64).reshape(-1, 8)
    L.prefix = np.concatenate([[0], np.cumsum([s["numel"] for s in L.segs])]).astype(np.int64)
    L.tile_prefix = np.concatenate([[0], np.cumsum([s["taps"] * (-(-s["cout"] // 64)) * (-(-s["cin"] // 64)) for s in L.segs])]).astype(np.int64)
    L.total, L.total_tiles = int(L.prefix[-1]), int(L.tile_prefix[-1])
    L.chunk_seg = (np.searchsorted(L.prefix, np.arange(-(-L.total // 4096), dtype=np.int64) * 4096, side="right") - 1).astype(np.int32)
    L.tile_seg = np.repeat(np.arange(L.n_seg), np.diff(L.tile_prefix)).astype(np.int32)
    L.wf_delta = np.full(max(n // 64, 1), INT32_MIN, dtype=np.int64)
    for s in L.segs:
        s["mapped"] = s["cin"] == s["cin_pad"] and not s["shifted"]
        if s["mapped"]:
            L.wf_delta[s["off"] // 64:r64(s["off"] + s["numel"]) // 64] = s["wf_off"] - s["off"]
    assert np.all((L.wf_delta >= INT32_MIN) & (L.wf_delta < 2 ** 31))
    L.wf_delta = L.wf_delta.astype(np.int32)
    return L


def real_mask(L, n=None):
    """bool [n]: flat elements that belong to a segment or a vector (False: the alignment padding behind one)"""
    m = np.zeros(L.numel, dtype=bool)
    for s in L.segs:
        m[s["off"]:s["off"] + s["numel"]] = True
    for off, k in L.vecs:
        m[off:off + k] = True
    return m[:L.numel if n is None else n]


def update_into(image, L, pnew, lo, hi):
    """What the fused update leaves in w_fwd for flat elements [lo, hi): bf16(p') at e + wf_delta[e >> 6] for every e whose group
    has a copy (the alignment padding of a mapped segment included: its zeros land in that copy's own padding)."""
    e = np.arange(lo, hi)
    d = L.wf_delta[e >> 6].astype(np.int64)
    keep = d != INT32_MIN
    image[(e + d)[keep]] = bf16_rne(pnew[lo:hi])[keep]


def pack_layout_into(wf_image, wd_image, L, master, which=0):
    for s in L.segs:
        w = master_rows(master, s["off"], s["cout"], s["taps"], s["cin"])
        if which != 2:
            pack_fwd_into(wf_image, s["wf_off"], w, s["cin_pad"])
        if which != 1 and s["need_dgrad"]:
            pack_dgrad_into(wd_image, s["wd_off"], w, s["cout_pad"])


def wd_prefill(L, n=None):
    """The transposed buffer as the engine allocates it, seen through sentinels: real positions hold the sentinel (they must be
    written), the Cout padding columns +0 (they may be rewritten with +0 only), the gaps between segments the sentinel."""
    img = np.full(L.wd_numel if n is None else n, SENT16, dtype=np.uint16)
    for s in L.segs:
        if s["need_dgrad"]:
            img[s["wd_off"]:s["wd_off"] + s["wd_numel"]].reshape(s["cin"], s["taps"], s["cout_pad"])[:, :, s["cout"]:] = 0
    return img


# the table of the batched packing test: Cin != Cin_pad and Cin = 1 without a transposed copy; 21 elements that misalign the 4-element
# groups of all that follows and force the scalar transpose; Cout = 27 / 80 / 65 / 130 against the 64-wide tiles; 9 taps; 74 880
# elements across 4096-element chunks; a master offset that is no multiple of 4 (scalar tile load although Cin % 4 == 0) and a
# transposed offset that is no multiple of 8 (scalar tile store although Cout_pad % 8 == 0)
BATCH_ITEMS = [(32, 1, 108, False), (64, 9, 1, False), (7, 1, 3, True), (27, 1, 64, True), (80, 1, 64, True), (64, 9, 32, True),
               (65, 9, 36, True), (130, 9, 64, True), (24, 1, 16, True), (40, 9, 8, True)]
BATCH_SHIFTS = {8: dict(off=3), 9: dict(wd=4)}
CAP_ITEMS = {"chunks": [(4100, 1, 4096, True)], "tiles": [(1, 1, 64 * 8200, True)]}


def batch_layout(aligned=False):
    """aligned: the same table without the 21-element segment, so that the 16-byte paths of the forward copy run as well"""
    if not aligned:
        return build_layout(BATCH_ITEMS, BATCH_SHIFTS)
    return build_layout(BATCH_ITEMS[:2] + BATCH_ITEMS[3:], {k - 1: v for k, v in BATCH_SHIFTS.items()})


# the layouts of the fused update + pack: deltas zero (first segment), INT32_MIN (a padded-Cin conv, vectors), positive (behind the
# padded-Cin conv, whose packed copy is larger than its master), negative (behind vectors); (7, 9, 8) has 504 elements - not a
# multiple of 64 - and n ends inside the last mapped group at an odd element.  "big" reaches the second trip of the grid-stride loop.
UPDATE_ITEMS = {
    "small": [(16, 1, 64, True), (32, 1, 108, False), (27, 1, 64, True), ("vec", 300), (7, 9, 8, True), ("vec", 100), (5, 1, 24, True)],
    "big": [(16, 1, 64, True), (2, 1, 108, False), ("vec", 100), (513, 1, 4096, False), ("vec", 70), (9, 1, 40, True)],
}


def update_layout(name):
    L = build_layout(UPDATE_ITEMS[name])
    last = L.segs[-1]
    L.n = last["off"] + last["numel"] - 3                       # ends inside the last mapped group, n % 4 == 1
    if name == "small":
        L.cuts = [4, 68, 1028, 5000, L.segs[3]["off"] + 200, L.n]       # 5000: inside (27, 1, 64); then inside (7, 9, 8)
    else:
        L.cuts = [4, 68, 1028, L.segs[2]["off"] + 100 * 4096 + 36, (1 << 21) + 4, L.n]
    return L


@functools.lru_cache(maxsize=4)
def update_case(name, draw):
    """-> dict(L, p0, b0, g [steps], want [(p, b)] per step, wf [image per step]); draw 'dyadic': three steps of (d) with zeros in the
    alignment padding; 'pass': (e) one first step with g = 0, p the patterns of (b) and random bits - p' = p bit for bit, b' = +0."""
    L = update_layout(name)
    n = L.n
    mask = real_mask(L, n)
    if draw == "dyadic":
        p, b, g, _ = dyadic_draw(n, 7)
        steps = run_steps(p, b, g, None, HP_DYADIC, mask=mask)
        p0, b0, gs = bits32(np.where(mask, p, 0.0)), bits32(np.where(mask, b, 0.0)), [bits32(np.where(mask, x, 0.0)) for x in g]
        want = [(bits32(q), bits32(c)) for q, c, _, _ in steps]
    else:
        p0 = random_bits(n, 11) * mask.astype(np.uint32)
        b0, gs = np.full(n, NAN32, dtype=np.uint32), [np.zeros(n, dtype=np.uint32)]
        want = [(p0, np.zeros(n, dtype=np.uint32))]
    images = []
    for q, _ in want:
        img = np.full(L.wf_numel, SENT16, dtype=np.uint16)
        update_into(img, L, q, 0, n)
        images.append(img)
    return dict(L=L, p0=p0, b0=b0, g=gs, want=want, wf=images)


# ---------------------------------------------------------------------------------------------------------------------------
# (i) sentinel buffers
class Guarded:
    """n elements between two guards of GUARD elements, all holding the kind's sentinel until `fill` (bit patterns) is given; `dev`
    is where the kernels see it.  The window starts on a 16-byte boundary."""

    def __init__(self, n, kind, dev="cpu", fill=None, sentinel=None):
        self.n, self.kind = n, kind
        self.sent = _SENT[kind] if sentinel is None else sentinel
        self.host = np.full(n + 2 * GUARD, self.sent, dtype=_NP[kind])
        if fill is not None:
            self.host[GUARD:GUARD + n] = fill
        view, tdt = _TORCH[kind]
        self.dev = torch.from_numpy(self.host.view(view)).view(tdt).to(dev)
        self.itemsize = self.host.itemsize

    def ptr(self, off=0, byte_shift=0):
        return self.dev.data_ptr() + (GUARD + off) * self.itemsize + byte_shift

    def tensor(self):
        """the window as a tensor on the device (a view)"""
        return self.dev[GUARD:GUARD + self.n]

    def read(self):
        """-> (window, whole buffer) as bit patterns"""
        view, _ = _TORCH[self.kind]
        whole = self.dev.cpu().view({np.int32: torch.int32, np.int16: torch.int16, np.uint8: torch.uint8, np.int64: torch.int64}[view]).numpy().view(_NP[self.kind])
        return whole[GUARD:GUARD + self.n], whole

    def check(self, want, what):
        """The window equals `want` (NaN for NaN) and both guards still hold the sentinel bit for bit.  -> the window"""
        win, whole = self.read()
        g = np.concatenate([whole[:GUARD], whole[GUARD + self.n:]])
        assert bool(np.all(g == np.array(self.sent).astype(_NP[self.kind]))), "%s: a guard element was written" % what
        assert_same(win, np.asarray(want, dtype=_NP[self.kind]), what)
        return win
