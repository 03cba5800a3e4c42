"""The weight-update, packing, cast and clearing kernels (csrc/elementwise.hip) against tests/update_reference.py, through the C ABI.

Bit for bit: the four SGD entry points on dyadic draws over three steps (every product and sum is an fp32 number, so the result does
not depend on where a multiply-add is fused), the EMA copy (its two products and its sum are rounded by contract), the packed bf16
forward copy the update keeps current (round to nearest even of the new p, also for the patterns of update_reference.SPECIAL carried
through a step with g = 0), both packing entry points, both casts and ep24_memset_zero.  Against float64 under a derived bound
(update_reference.general_tol): one step of the update on normal draws.  tests/test_update_reference.py shows without a GPU that the
references equal torch.optim.SGD, the oracle and torch's bf16 rounding, that a float32 emulation stays inside the bound and that nine
mutants are rejected on these inputs.

Every buffer sits between two guards of 64 sentinel elements (a NaN pattern no kernel produces), whole buffers are compared, and a
buffer a call must not write is compared as well.  NaN equals NaN; every other pattern only itself.

The sizes come from the constants of csrc/elementwise.hip:
  MAX_BLOCKS = 2048 workgroups of 256 lanes: the update moves 4 elements per lane, so its second grid-stride trip starts at element
      2048 * 1024 = 2^21; ep24_pack_weights moves one, so (130, 9, 451) with 527 670 > 2048 * 256 elements loops; the casts loop
      beyond 2^21 elements as well
  ep24_pack_weights_batched: at most 4096 workgroups of 4096 elements (forward copy), at most 8192 workgroups of one 64 x 64 tile
      (transposed copy)
  ep24_memset_zero: at most 8192 workgroups of 256 lanes, 4 stores of 16 bytes per lane on an aligned base

The general draw's largest err / tol (1.0 is the bound; the last rounding alone reaches 1.0 for a result just above a power of two):
the float32 emulations of tests/test_update_reference.py give 0.994 for p' and 0.968 for b' at n = 2^21 + 1027 and 0.952 / 0.826 at
n = 4100.  NOT YET MEASURED on an MI355X: the test prints the figures (UPD-ERR) before it asserts.
"""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import update_reference as R  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
E_ARG = -1


def _abi():
    from ep24._lib import call, lib, ptr, stream_ptr
    return call, ptr, stream_ptr, lib()


def G(n, kind, fill=None):
    return R.Guarded(n, kind, DEV, fill)


def sync():
    torch.cuda.synchronize()


def make_hp(hp3, with_ema=True):
    """The device block of ep24_set_hparams between guards: hp[0..4] written, hp[5..7] left alone."""
    call, _, sp, _ = _abi()
    hp = G(8, "f32")
    d, omd = (R.EMA_D, R.EMA_OMD) if with_ema else (0.0, 0.0)
    call("set_hparams", hp.ptr(), hp3[0], hp3[1], hp3[2], d, omd, sp())
    sync()
    want = np.full(8, R.SENT32, dtype=np.uint32)
    want[:5] = R.bits32(np.array([hp3[0], hp3[1], hp3[2], d, omd], dtype=np.float32))
    hp.check(want, "hp")
    return hp


class Sgd:
    """p, buf (and ema) of one run between guards, the first-step flag between two guard words."""

    def __init__(self, n, p0, b0, e0=None, flag=1):
        self.n = n
        self.p, self.b = G(n, "f32", p0), G(n, "f32", b0)
        self.e = None if e0 is None else G(n, "f32", e0)
        self.flag = G(1, "i32", [flag])

    def call(self, form, g, hp3, hp, lo=0, hi=None, last=1, delta=None, wf=None):
        call, _, sp, _ = _abi()
        hi = self.n if hi is None else hi
        e = None if self.e is None else self.e.ptr()
        if form == "plain":
            assert lo == 0 and hi == self.n and e is None
            call("sgd_nesterov", self.p.ptr(), g.ptr(), self.b.ptr(), self.n, hp3[0], hp3[1], hp3[2], self.flag.ptr(), sp())
        elif form == "hp":
            assert lo == 0 and hi == self.n
            call("sgd_nesterov_hp", self.p.ptr(), g.ptr(), self.b.ptr(), self.n, hp.ptr(), self.flag.ptr(), e, sp())
        elif form == "range":
            call("sgd_nesterov_hp_range", self.p.ptr(), g.ptr(), self.b.ptr(), lo, hi - lo, hp.ptr(), self.flag.ptr(), e, last, sp())
        else:
            call("sgd_nesterov_hp_range_pack", self.p.ptr(), g.ptr(), self.b.ptr(), lo, hi - lo, hp.ptr(), self.flag.ptr(), e, last,
                 delta.ptr(), wf.ptr(), sp())
        sync()


FORMS = [("plain", False), ("hp", False), ("hp", True), ("range", True), ("range_pack", True)]


# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form,ema", FORMS, ids=["%s%s" % (f, "-ema" if e else "") for f, e in FORMS])
@pytest.mark.parametrize("n", R.SGD_N)
def test_sgd_entry_points_exact(n, form, ema):
    """Three steps.  The first runs with first_flag = 1 over a buffer full of NaN: no NaN may come out, and the flag reads 0 afterwards;
    the others find 0 and leave 0.  g and every guard are unchanged.  The _range_pack form gets a table of INT32_MIN groups here: its
    packed buffer stays untouched."""
    c = R.dyadic_case(n)
    hp = None if form == "plain" else make_hp(R.HP_DYADIC, ema)
    st = Sgd(n, c["p0"], np.full(n, R.NAN32, dtype=np.uint32), c["e0"] if ema else None, flag=1)
    delta = wf = None
    if form == "range_pack":
        delta, wf = G((n + 63) // 64, "i32", np.full((n + 63) // 64, R.INT32_MIN, dtype=np.int32)), G(64, "bf16")
    for k in range(R.STEPS):
        g = G(n, "f32", c["g"][k])
        st.call(form, g, R.HP_DYADIC, hp, delta=delta, wf=wf)
        wp, wb, we = c["want"][k]
        got_p = st.p.check(wp, "p' step %d" % k)
        got_b = st.b.check(wb, "buf' step %d" % k)
        assert not R.is_nan32(got_p).any() and not R.is_nan32(got_b).any()
        if ema:
            st.e.check(we, "ema' step %d" % k)
        g.check(c["g"][k], "g")
        st.flag.check([0], "first_flag after step %d" % k)
        if wf is not None:
            wf.check(np.full(64, R.SENT16, dtype=np.uint16), "w_fwd")
            delta.check(np.full((n + 63) // 64, R.INT32_MIN, dtype=np.int32), "wf_delta")


@pytest.mark.parametrize("n", [5, 1025, 4100, (1 << 21) + 1027])
def test_sgd_ranges_exact(n):
    """[0, n) cut at 4, 68, 1028 and 2^21 + 4: after every call the elements of the ranges done so far hold the step's result and every
    other element what it held before, bit for bit (on the first step: the NaN the buffer was filled with).  Only the call with
    last = 1 clears the flag, so the later ranges of a first step still ignore the buffer."""
    c = R.dyadic_case(n)
    cuts = [x for x in (4, 68, 1028, (1 << 21) + 4) if x < n] + [n]
    hp = make_hp(R.HP_DYADIC)
    st = Sgd(n, c["p0"], np.full(n, R.NAN32, dtype=np.uint32), c["e0"], flag=1)
    cur = [c["p0"].copy(), np.full(n, R.NAN32, dtype=np.uint32), c["e0"].copy()]
    for k in range(R.STEPS):
        g = G(n, "f32", c["g"][k])
        lo = 0
        for hi in cuts:
            st.call("range", g, R.HP_DYADIC, hp, lo, hi, last=int(hi == n))
            for buf, have, want, what in zip((st.p, st.b, st.e), cur, c["want"][k], ("p'", "buf'", "ema'")):
                have[lo:hi] = want[lo:hi]
                buf.check(have, "%s step %d after [%d, %d)" % (what, k, lo, hi))
            st.flag.check([0 if hi == n or k > 0 else 1], "first_flag step %d after [%d, %d)" % (k, lo, hi))
            lo = hi
        g.check(c["g"][k], "g")
        for have, want in zip(cur, c["want"][k]):                  # the ranges together are the one-call result
            assert R.same_bits(have, want)


@pytest.mark.parametrize("draw", ["dyadic", "pass"])
@pytest.mark.parametrize("name", list(R.UPDATE_ITEMS))
def test_update_keeps_the_forward_copy(name, draw):
    """ep24_sgd_nesterov_hp_range_pack over a synthetic layout (deltas zero, positive, negative and INT32_MIN; a 504-element segment
    whose alignment padding lands in its own copy's padding; n ends inside a mapped group at n % 4 == 1), in ranges cut inside mapped
    segments.  w_fwd starts full of the sentinel; after every call it holds bf16(p') at e + wf_delta[e >> 6] for every element done
    so far and the sentinel everywhere else.  'pass': g = 0 on a first step carries the special patterns through p' = p."""
    c = R.update_case(name, draw)
    L = c["L"]
    n = L.n
    hp = make_hp(R.HP_DYADIC, with_ema=False)
    nan = np.full(n, R.NAN32, dtype=np.uint32)
    st = Sgd(n, c["p0"], nan, None, flag=1)
    delta, wf = G(L.wf_delta.size, "i32", L.wf_delta), G(L.wf_numel, "bf16")
    cur = [c["p0"].copy(), nan.copy()]
    img = np.full(L.wf_numel, R.SENT16, dtype=np.uint16)
    for k, gk in enumerate(c["g"]):
        g = G(n, "f32", gk)
        lo = 0
        for hi in L.cuts:
            st.call("range_pack", g, R.HP_DYADIC, hp, lo, hi, last=int(hi == n), delta=delta, wf=wf)
            for buf, have, want, what in zip((st.p, st.b), cur, c["want"][k], ("p'", "buf'")):
                have[lo:hi] = want[lo:hi]
                buf.check(have, "%s step %d after [%d, %d)" % (what, k, lo, hi))
            R.update_into(img, L, c["want"][k][0], lo, hi)
            wf.check(img, "w_fwd step %d after [%d, %d)" % (k, lo, hi))
            st.flag.check([0 if hi == n or k > 0 else 1], "first_flag")
            lo = hi
        assert R.same_bits(img, c["wf"][k])
        g.check(gk, "g")
    delta.check(L.wf_delta, "wf_delta")


@pytest.mark.parametrize("n", R.GENERAL_N)
def test_sgd_general_draw_within_the_derived_bound(n):
    c = R.general_case(n)
    hp = make_hp(R.HP_GENERAL)
    worst = {}
    for form in ("plain", "hp"):
        st = Sgd(n, c["p0"], c["b0"], None, flag=0)
        g = G(n, "f32", c["g"])
        st.call(form, g, R.HP_GENERAL, hp)
        p, _ = st.p.read()
        b, _ = st.b.read()
        worst[form] = (R.err_ratio(R.from_bits32(p), c["p"], c["tol_p"]), R.err_ratio(R.from_bits32(b), c["b"], c["tol_b"]))
        st.p.check(p, "p guards")
        st.b.check(b, "buf guards")
        g.check(c["g"], "g")
    print("UPD-ERR general n %d: %s" % (n, ", ".join("%s p %.3g b %.3g" % (f, a, b) for f, (a, b) in worst.items())))
    assert all(a <= 1.0 and b <= 1.0 for a, b in worst.values()), worst


def test_sgd_refusals():
    """EP24_E_ARG before any launch: every buffer is unchanged afterwards."""
    _, _, sp, lib = _abi()
    n = 64
    c = R.dyadic_case(n)
    hp = make_hp(R.HP_DYADIC)
    st = Sgd(n, c["p0"], c["b0"], c["e0"], flag=1)
    g = G(n, "f32", c["g"][0])
    delta, wf = G(1, "i32", [0]), G(n, "bf16")
    lr, m, s = R.HP_DYADIC
    P, Gp, B, E, H, F, D, W = st.p.ptr(), g.ptr(), st.b.ptr(), st.e.ptr(), hp.ptr(), st.flag.ptr(), delta.ptr(), wf.ptr()
    good = {
        "ep24_sgd_nesterov": [P, Gp, B, n, lr, m, s, F, sp()],
        "ep24_sgd_nesterov_hp": [P, Gp, B, n, H, F, E, sp()],
        "ep24_sgd_nesterov_hp_range": [P, Gp, B, 0, n, H, F, E, 1, sp()],
        "ep24_sgd_nesterov_hp_range_pack": [P, Gp, B, 0, n, H, F, E, 1, D, W, sp()],
    }
    refused = 0
    for name, args in good.items():
        names = [a for _, a in lib.protos[name][1]]
        bad = [(k, None) for k in ("p", "g", "buf", "first_flag")] + [("n", 0), ("p", P + 4), ("g", Gp + 4), ("buf", B + 4)]
        if "hp" in names:
            bad += [("hp", None), ("ema", E + 4)]
        if "first" in names:
            bad += [("first", 2), ("first", -4), ("first", -1)]
        if "wf" in names:
            bad += [("wf", W + 8), ("wf", None), ("wf_delta", None)]
        for key, val in bad:
            a = list(args)
            a[names.index(key)] = val
            assert lib.fn[name](*a) == E_ARG, (name, key, val)
            refused += 1
    assert refused == 8 + 10 + 13 + 16
    sync()
    st.p.check(c["p0"], "p")
    st.b.check(c["b0"], "buf")
    st.e.check(c["e0"], "ema")
    g.check(c["g"][0], "g")
    st.flag.check([1], "first_flag")
    wf.check(np.full(n, R.SENT16, dtype=np.uint16), "w_fwd")


# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("outs", ["both", "fwd", "dgrad"])
@pytest.mark.parametrize("Cout,T,Cin,Cin_pad,Cout_pad,ld_w", R.PACK_SHAPES, ids=["%dx%dx%d" % s[:3] for s in R.PACK_SHAPES])
def test_pack_weights_exact(Cout, T, Cin, Cin_pad, Cout_pad, ld_w, outs):
    """Real positions bit for bit; every padding position, the copy that is not asked for and the guards untouched."""
    call, _, sp, _ = _abi()
    src = R.random_bits(Cout * ld_w, Cout)
    src.reshape(Cout, ld_w)[:, T * Cin:] = R.SENT32                 # between the rows: never read
    master = G(Cout * ld_w, "f32", src)
    wf, wd = G(Cout * T * Cin_pad, "bf16"), G(Cin * T * Cout_pad, "bf16")
    call("pack_weights", master.ptr(), ld_w, wf.ptr() if outs != "dgrad" else None, wd.ptr() if outs != "fwd" else None, Cout, T, Cin,
         Cin_pad, Cout_pad, sp())
    sync()
    w = R.master_rows(src, 0, Cout, T, Cin, ld_w)
    fi, di = np.full(wf.n, R.SENT16, dtype=np.uint16), np.full(wd.n, R.SENT16, dtype=np.uint16)
    if outs != "dgrad":
        R.pack_fwd_into(fi, 0, w, Cin_pad)
    if outs != "fwd":
        R.pack_dgrad_into(di, 0, w, Cout_pad)
    wf.check(fi, "w_fwd")
    wd.check(di, "w_dgrad")
    master.check(src, "master")


def _run_batched(L, which, tables, seed):
    call, _, sp, _ = _abi()
    src = R.random_bits(L.numel, seed)
    master = G(L.numel, "f32", src)
    wf, wd = G(L.wf_numel, "bf16"), G(L.wd_numel, "bf16", R.wd_prefill(L))
    desc, pre, tpre = G(L.desc.size, "i64", L.desc.reshape(-1)), G(L.prefix.size, "i64", L.prefix), G(L.tile_prefix.size, "i64", L.tile_prefix)
    cs, ts = G(L.chunk_seg.size, "i32", L.chunk_seg), G(L.tile_seg.size, "i32", L.tile_seg)
    call("pack_weights_batched", master.ptr(), desc.ptr(), pre.ptr(), tpre.ptr(), L.n_seg, wf.ptr(), wd.ptr(), L.total, L.total_tiles,
         cs.ptr() if tables else None, ts.ptr() if tables else None, which, sp())
    sync()
    fi, di = np.full(L.wf_numel, R.SENT16, dtype=np.uint16), R.wd_prefill(L)
    R.pack_layout_into(fi, di, L, src, which)
    wf.check(fi, "w_fwd")                        # real positions; Cin padding, the 64-element steps' gaps and the guards untouched
    wd.check(di, "w_dgrad")                      # real positions; Cout padding columns still +0; gaps and guards untouched
    master.check(src, "master")
    for t, want, what in ((desc, L.desc.reshape(-1), "desc"), (pre, L.prefix, "prefix"), (tpre, L.tile_prefix, "tile_prefix"),
                          (cs, L.chunk_seg, "chunk_seg"), (ts, L.tile_seg, "tile_seg")):
        t.check(want, what)


@pytest.mark.parametrize("which", [0, 1, 2])
@pytest.mark.parametrize("tables", [True, False], ids=["tables", "bisect"])
@pytest.mark.parametrize("aligned", [False, True], ids=["misaligned", "aligned"])
def test_pack_weights_batched_exact(aligned, tables, which):
    """update_reference.BATCH_ITEMS.  The copy that `which` excludes is wholly untouched."""
    _run_batched(R.batch_layout(aligned), which, tables, 40 + which)


@pytest.mark.parametrize("cap", list(R.CAP_ITEMS))
def test_pack_weights_batched_beyond_the_grid_caps(cap):
    """One segment of more than 4096 * 4096 elements; one of more than 8192 tiles."""
    L = R.build_layout(R.CAP_ITEMS[cap])
    assert L.total > 4096 * 4096 if cap == "chunks" else L.total_tiles > 8192
    _run_batched(L, 0, True, 50)


# ---------------------------------------------------------------------------------------------------------------------------
def test_cast_bf16_f32_every_pattern():
    call, _, sp, _ = _abi()
    pat = np.arange(65536, dtype=np.uint16)
    src, dst = G(65536, "bf16", pat), G(65536, "f32")
    call("cast_bf16_f32", src.ptr(), dst.ptr(), 65536, sp())
    sync()
    got = dst.check(R.bf16_widen(pat), "fp32")
    assert np.array_equal(R.is_nan32(got), R.is_nan16(pat))
    src.check(pat, "bf16 source")


@pytest.mark.parametrize("n", [0, 4, 1028, (1 << 21) + 4])
def test_cast_f32_bf16_exact(n):
    call, _, sp, _ = _abi()
    bits = R.random_bits(max(n, 4), 21)
    src, dst = G(max(n, 4), "f32", bits), G(max(n, 4), "bf16")
    call("cast_f32_bf16", src.ptr(), dst.ptr(), n, sp())
    sync()
    want = np.full(max(n, 4), R.SENT16, dtype=np.uint16)
    want[:n] = R.bf16_rne(bits[:n])
    dst.check(want, "bf16")
    src.check(bits, "fp32 source")
    if n == 1028:                                                 # ... and back: the widening is exact
        back = G(n, "f32")
        call("cast_bf16_f32", dst.ptr(), back.ptr(), n, sp())
        sync()
        back.check(R.bf16_widen(want), "fp32 again")


def test_cast_refusals():
    """n % 4 != 0, a NULL pointer, the fp32 side off its 16-byte or the bf16 side off its 8-byte boundary: EP24_E_ARG, nothing written."""
    _, _, sp, lib = _abi()
    bits = R.random_bits(64, 22)
    f, h = G(64, "f32", bits), G(64, "bf16", R.bf16_rne(bits))
    to_bf, to_f = lib.fn["ep24_cast_f32_bf16"], lib.fn["ep24_cast_bf16_f32"]
    for n in (1, 6, 63, -4):
        assert to_bf(f.ptr(), h.ptr(), n, sp()) == E_ARG and to_f(h.ptr(), f.ptr(), n, sp()) == E_ARG, n
    for shift in (4, 8, 12):
        assert to_bf(f.ptr(0, shift), h.ptr(), 8, sp()) == E_ARG and to_f(h.ptr(), f.ptr(0, shift), 8, sp()) == E_ARG, shift
    for shift in (2, 4, 6):
        assert to_bf(f.ptr(), h.ptr(0, shift), 8, sp()) == E_ARG and to_f(h.ptr(0, shift), f.ptr(), 8, sp()) == E_ARG, shift
    assert to_bf(None, h.ptr(), 8, sp()) == E_ARG and to_bf(f.ptr(), None, 8, sp()) == E_ARG
    assert to_f(None, f.ptr(), 8, sp()) == E_ARG and to_f(h.ptr(), None, 8, sp()) == E_ARG
    assert "aligned" in lib.last_error() or "cast" in lib.last_error()
    sync()
    f.check(bits, "fp32")
    h.check(R.bf16_rne(bits), "bf16")
    # the boundaries themselves are accepted: 16 bytes on the fp32 side go with 8 on the bf16 side (4 elements)
    assert to_bf(f.ptr(4), h.ptr(4), 8, sp()) == 0
    sync()
    h.check(R.bf16_rne(bits), "bf16 from an offset of 4 elements")


# ---------------------------------------------------------------------------------------------------------------------------
MEMSET_BYTES = [0, 1, 8, 15, 16, 17, 4096 + 7, 16 * 1024 * 8192 + 16 + 5]


@pytest.mark.parametrize("nbytes", MEMSET_BYTES)
def test_memset_zero_exact(nbytes):
    """Exactly the requested bytes become zero, on a 16-byte aligned base (16-byte stores and a byte tail) and on bases off by 1 and
    by 8 bytes (byte stores); 8 bytes is the barrier slot, the last count is beyond the grid cap."""
    call, _, sp, _ = _abi()
    pad = 256
    t = torch.empty(nbytes + 2 * pad, dtype=torch.uint8, device=DEV)
    assert t.data_ptr() % 16 == 0
    for shift in (0, 1, 8):
        t.fill_(R.SENT8)
        lo = pad + shift
        call("memset_zero", t.data_ptr() + lo, nbytes, sp())
        sync()
        assert bool((t[:lo] == R.SENT8).all()) and bool((t[lo + nbytes:] == R.SENT8).all()), (nbytes, shift)
        assert bool((t[lo:lo + nbytes] == 0).all()), (nbytes, shift)
    _, _, _, lib = _abi()
    assert lib.fn["ep24_memset_zero"](None, 16, sp()) == E_ARG and lib.fn["ep24_memset_zero"](t.data_ptr(), -1, sp()) == E_ARG


# ---------------------------------------------------------------------------------------------------------------------------
def _bits(t):
    t = t.detach().contiguous().cpu()
    if t.dtype == torch.float32:
        return t.view(torch.int32).numpy().view(np.uint32).reshape(-1)
    return t.view(torch.int16).numpy().view(np.uint16).reshape(-1)


def _module_weights(seg):
    """uint32 [Cout][T][Cin] from the modules' own weight tensors (logical [Cout, Cin, kh, kw]; a merged segment stacks its modules)"""
    w = torch.cat([p.detach() for p in seg.params], 0).permute(0, 2, 3, 1).contiguous()
    assert w.numel() == seg.cout * seg.taps * seg.cin
    return _bits(w.float()).reshape(seg.cout, seg.taps, seg.cin)


def test_engine_layout_and_packed_copies():
    """The real layout (test_gpu_engine.tiny_model): the tables against the header's definitions, a full pack against the reference
    pack of the modules' own weight tensors (merged CSP pairs and the reg + obj head segment included), and one fused update in two
    ranges on dyadic p and g against bf16(p')."""
    import test_gpu_engine as TE
    from ep24.engine import param_home
    call, ptr, sp, _ = _abi()
    torch.manual_seed(0)
    model = TE.tiny_model()
    home = param_home(model)
    segs = home.convs
    assert any(len(s.params) == 2 and s.taps == 1 and s.cout == 27 for s in segs) and any(len(s.params) == 2 and s.cout != 27 for s in segs)
    assert home.pack_rest and len(home.pack_rest) < len(segs)
    # ---- tables
    delta = home.wf_delta.cpu().numpy().astype(np.int64)
    assert bool(np.all((delta == R.INT32_MIN) | (delta % 4 == 0))) and delta.size == home.numel // 64
    assert all(s.off % 64 == 0 for s in home.order) and all(s.wf_off % 64 == 0 for s in segs)
    want_delta = np.full(home.numel // 64, R.INT32_MIN, dtype=np.int64)
    spans = []
    for s in segs:
        if s not in home.pack_rest:
            assert s.cin % 8 == 0
            want_delta[s.off // 64:R.r64(s.off + s.numel) // 64] = s.wf_off - s.off
            spans.append((s.wf_off, s.wf_off + R.r64(s.numel)))           # what the update may write: the copy and its own padding
        else:
            spans.append((s.wf_off, s.wf_off + s.cout * s.taps * s.cin_pad))
    assert np.array_equal(delta, want_delta)
    spans.sort()
    assert all(a[1] <= b[0] for a, b in zip(spans, spans[1:])) and spans[0][0] >= 0 and spans[-1][1] <= home.wf.numel()
    pref = home.pack_prefix.cpu().numpy()
    tpref = home.pack_tprefix.cpu().numpy()
    desc = home.pack_desc.cpu().numpy()
    assert np.array_equal(pref, np.concatenate([[0], np.cumsum([s.numel for s in segs])]))
    assert np.array_equal(tpref, np.concatenate([[0], np.cumsum([s.taps * ((s.cout + 63) // 64) * ((s.cin + 63) // 64) for s in segs])]))
    assert home.pack_total == pref[-1] and home.pack_tiles == tpref[-1]
    for i, s in enumerate(segs):
        assert list(desc[i]) == [s.off, s.wf_off, s.wd_off if s.need_dgrad else -1, s.cout, s.taps, s.cin, s.cin_pad, s.cout_pad]
    cseg, tseg = home.pack_chunk_seg.cpu().numpy(), home.pack_tile_seg.cpu().numpy()
    assert cseg.size == (pref[-1] + 4095) // 4096 and tseg.size == tpref[-1]
    assert all(pref[sg] <= 4096 * c < pref[sg + 1] for c, sg in enumerate(cseg))
    assert all(tpref[sg] <= t < tpref[sg + 1] for t, sg in enumerate(tseg))
    # ---- a full pack against the modules' own tensors
    home.wf.view(torch.int16).fill_(R.SENT16 - 65536)
    wd_img = np.full(home.wd.numel(), R.SENT16, dtype=np.uint16)
    for s in segs:
        if s.need_dgrad:
            wd_img[s.wd_off:s.wd_off + s.cin * s.taps * s.cout_pad].reshape(s.cin, s.taps, s.cout_pad)[:, :, s.cout:] = 0
    home.wd.copy_(torch.from_numpy(wd_img.view(np.int16)).view(torch.bfloat16))
    home.pack(0)
    sync()
    wf_img = np.full(home.wf.numel(), R.SENT16, dtype=np.uint16)
    for s in segs:
        w = _module_weights(s)
        R.assert_same(_bits(home.flat[s.off:s.off + s.numel]).reshape(w.shape), w, "the flat master of segment %d" % s.off)
        R.pack_fwd_into(wf_img, s.wf_off, w, s.cin_pad)
        if s.need_dgrad:
            R.pack_dgrad_into(wd_img, s.wd_off, w, s.cout_pad)
    R.assert_same(_bits(home.wf), wf_img, "w_fwd after pack(0)")
    R.assert_same(_bits(home.wd), wd_img, "w_dgrad after pack(0)")
    # ---- one fused update in two ranges, dyadic p and g (zeros in the alignment padding), first step over a buffer full of NaN
    n = home.numel
    mask = np.zeros(n, dtype=bool)
    for s in home.order:
        mask[s.off:s.off + s.numel] = True
    p, _, g, _ = R.dyadic_draw(n, 9, steps=1)
    p, g = np.where(mask, p, 0.0), np.where(mask, g[0], 0.0)
    (p2, b2, _, _), = R.run_steps(p, np.zeros(n), [g], None, R.HP_DYADIC)
    f32t = lambda a: torch.from_numpy(a.astype(np.float32)).to(DEV)
    home.flat.copy_(f32t(p))
    home.gflat.copy_(f32t(g))
    home.mflat.fill_(float("nan"))
    home.first_flag.fill_(1)
    home.wf.view(torch.int16).fill_(R.SENT16 - 65536)
    hp = make_hp(R.HP_DYADIC, with_ema=False)
    mapped = [s for s in segs if s not in home.pack_rest and s.numel > 256]
    cut = mapped[len(mapped) // 2].off + 132                     # inside a mapped segment, in the middle of a 64-element group
    home.sgd_hp(hp.tensor(), lo=cut, hi=n, last=False)           # backward completes the buffer from its tail
    sync()
    assert int(home.first_flag) == 1
    home.sgd_hp(hp.tensor(), lo=0, hi=cut, last=True)
    sync()
    assert int(home.first_flag) == 0
    R.assert_same(_bits(home.flat), R.bits32(p2), "p'")
    R.assert_same(_bits(home.mflat), R.bits32(b2), "buf'")
    R.assert_same(_bits(home.gflat), R.bits32(g), "g")
    got = _bits(home.wf)
    want = np.full(home.wf.numel(), R.SENT16, dtype=np.uint16)
    e = np.arange(n)
    d = want_delta[e >> 6]
    want[(e + d)[d != R.INT32_MIN]] = R.bf16_rne(R.bits32(p2))[d != R.INT32_MIN]
    R.assert_same(got, want, "w_fwd after the update")
    for s in segs:
        if s not in home.pack_rest:
            w = R.bits32(p2[s.off:s.off + s.numel]).reshape(s.cout, s.taps, s.cin)
            assert R.same_bits(got[s.wf_off:s.wf_off + s.numel], R.bf16_rne(w).reshape(-1)), s.off
