"""tests/update_reference.py without a GPU: (a) its update equals torch.optim.SGD(momentum, nesterov=True) and the oracle's step in
float64 and fp32 torch's EMA bit for bit, its bf16 rounding equals torch's, its pack references equal permutes in torch; (b) every
exactness precondition holds for every dyadic case tests/test_gpu_update_exact.py runs; (c) the general draw's bound holds two float32
emulations of the kernel's expression (not too tight); (d) the layout tables satisfy the definitions of include/ep24.h; (e) each
mutant - `first` ignored, plain momentum, grad_scale twice, EMA from the old p, truncation, the neighbouring group's wf_delta, the
last tail element skipped, ci and co swapped, a padding column written - is rejected by the comparison the GPU tests use, on their
inputs (not too loose)."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import update_reference as R  # noqa: E402

BF = torch.bfloat16
SMALL_N = [n for n in R.SGD_N if n <= 4100]


def test_helper_never_imports_the_package():
    src = open(R.__file__.replace(".pyc", ".py")).read()
    assert "import ep24" not in src and "from ep24" not in src


# ------------------------------------------------------------------------------------------------------------- (a)
def _three_steps(n=333):
    rng = np.random.default_rng(3)
    p, b = rng.standard_normal(n), rng.standard_normal(n)
    g = [rng.standard_normal(n) for _ in range(3)]
    return p, b, g


def test_sgd_equals_torch_optim_and_the_oracle():
    from oracle.model import sgd_nesterov_step
    p0, b0, g = _three_steps()
    lr, m, s = 0.0123, 0.9, 0.5
    hp = (lr, m, s)
    mine = R.run_steps(p0, b0, g, None, hp, first=True)
    tp = torch.nn.Parameter(torch.tensor(p0, dtype=torch.float64))
    opt = torch.optim.SGD([tp], lr=lr, momentum=m, nesterov=True)
    op = torch.tensor(p0, dtype=torch.float64)
    obuf = [None]
    for k in range(3):
        tp.grad = torch.tensor(g[k] * s, dtype=torch.float64)
        opt.step()
        op.grad = torch.tensor(g[k] * s, dtype=torch.float64)
        sgd_nesterov_step([op], obuf, lr, m)
        assert float((torch.tensor(mine[k][0]) - tp.detach()).abs().max()) < 1e-12
        assert float((torch.tensor(mine[k][1]) - opt.state[tp]["momentum_buffer"]).abs().max()) < 1e-12
        assert float((torch.tensor(mine[k][0]) - op).abs().max()) < 1e-12
        assert float((torch.tensor(mine[k][1]) - obuf[0]).abs().max()) < 1e-12
    # a later step reads the buffer: the same against the optimizer's state carried over
    again = R.run_steps(mine[0][0], mine[0][1], g[1:], None, hp, first=False)
    assert np.array_equal(again[1][0], mine[2][0])


def test_ema_equals_fp32_torch_bit_for_bit():
    rng = np.random.default_rng(4)
    e, p = rng.standard_normal(5000).astype(np.float32), rng.standard_normal(5000).astype(np.float32)
    d, omd = R.EMA_D, R.EMA_OMD
    v = torch.from_numpy(e.copy())
    v *= d                                                       # utils/ema.py: v *= d; v += (1 - d) * model_v
    v += omd * torch.from_numpy(p)
    assert R.same_bits(R.bits32(R.ema_ref(e, p, d, omd)), R.bits32(v.numpy()))
    assert omd == 1.0 - 0.99871 and np.float32(omd) != np.float32(1.0) - np.float32(d)       # the host forms 1 - d in double


def _torch_bf16_bits(b32):
    t = torch.from_numpy(np.ascontiguousarray(b32).view(np.int32)).view(torch.float32).to(BF)
    return t.view(torch.int16).numpy().view(np.uint16)


def test_bf16_rounding_equals_torch_and_the_hand_written_patterns():
    assert R.same_bits(R.bf16_rne(R.SPECIAL32), R.SPECIAL16)
    nan = R.is_nan32(R.SPECIAL32)
    assert nan.sum() == 1 and bool(np.all(R.is_nan16(R.SPECIAL16) == nan))
    assert R.same_bits(_torch_bf16_bits(R.SPECIAL32), R.SPECIAL16)
    b = np.random.default_rng(5).integers(0, 1 << 32, 1 << 20, dtype=np.uint64).astype(np.uint32)
    got, want = R.bf16_rne(b), _torch_bf16_bits(b)
    assert bool(np.all(R.is_nan16(want) == R.is_nan32(b))) and R.same_bits(got, want)
    assert bool(np.all(got[~R.is_nan32(b)] == want[~R.is_nan32(b)]))
    r = R.random_bits(4100, 6)                                    # what the GPU tests feed: no zero / denormal / inf / NaN but (b)'s
    ex = (r >> np.uint32(23)) & np.uint32(0xFF)
    assert int(((ex == 0) & (r << np.uint32(1) != 0)).sum()) == 0 and int(R.is_nan32(r).sum()) == 3
    assert R.same_bits(R.bf16_widen(R.bf16_rne(R.bf16_widen(np.arange(65536, dtype=np.uint16)))), R.bf16_widen(np.arange(65536, dtype=np.uint16)))


@pytest.mark.parametrize("Cout,T,Cin,Cin_pad,Cout_pad,ld_w", R.PACK_SHAPES[:3] + [(5, 4, 3, 8, 8, 12)])
def test_pack_references_equal_permutes(Cout, T, Cin, Cin_pad, Cout_pad, ld_w):
    rng = np.random.default_rng(Cout)
    master = R.bits32(rng.standard_normal(Cout * ld_w + 7).astype(np.float32))
    w = R.master_rows(master, 3, Cout, T, Cin, ld_w)
    tw = torch.from_numpy(master.view(np.int32)).view(torch.float32)[3:3 + Cout * ld_w].view(Cout, ld_w)[:, :T * Cin].reshape(Cout, T, Cin)
    assert np.array_equal(R.from_bits32(w), tw.numpy())
    wf = np.full(Cout * T * Cin_pad + 10, R.SENT16, dtype=np.uint16)
    wd = np.full(Cin * T * Cout_pad + 10, R.SENT16, dtype=np.uint16)
    R.pack_fwd_into(wf, 5, w, Cin_pad)
    R.pack_dgrad_into(wd, 2, w, Cout_pad)
    sent = torch.tensor([R.SENT16 - 65536], dtype=torch.int16).view(BF)
    tf = sent.repeat(Cout, T, Cin_pad).clone()
    tf[:, :, :Cin] = tw.to(BF)
    td = sent.repeat(Cin, T, Cout_pad).clone()
    td[:, :, :Cout] = tw.to(BF).permute(2, 1, 0)
    assert np.array_equal(wf[5:-5], tf.reshape(-1).view(torch.int16).numpy().view(np.uint16)) and bool(np.all(wf[:5] == R.SENT16)) and bool(np.all(wf[-5:] == R.SENT16))
    assert np.array_equal(wd[2:-8], td.reshape(-1).view(torch.int16).numpy().view(np.uint16)) and bool(np.all(wd[:2] == R.SENT16)) and bool(np.all(wd[-8:] == R.SENT16))


# ------------------------------------------------------------------------------------------------------------- (b)
@pytest.mark.parametrize("n", SMALL_N + [1 << 21])
def test_every_dyadic_intermediate_is_an_fp32_number(n):
    p, b, g, e = R.dyadic_draw(n, 0)
    for k, (_, _, _, mid) in enumerate(R.run_steps(p, b, g, e, R.HP_DYADIC)):
        for name, v in mid.items():
            assert v is None or R.exact32(v), (n, k, name)
    assert all(R.f32(h) == h for h in R.HP_DYADIC)


@pytest.mark.parametrize("name", list(R.UPDATE_ITEMS))
def test_every_dyadic_intermediate_of_the_pack_cases_is_an_fp32_number(name):
    L = R.update_layout(name)
    p, b, g, _ = R.dyadic_draw(L.n, 7)
    for k, (_, _, _, mid) in enumerate(R.run_steps(p, b, g, None, R.HP_DYADIC, mask=R.real_mask(L, L.n))):
        assert all(v is None or R.exact32(v) for v in mid.values()), (name, k)
    c = R.update_case(name, "pass")
    assert R.same_bits(c["want"][0][0], c["p0"]) and int(R.is_nan32(c["p0"]).sum()) >= 1


# ------------------------------------------------------------------------------------------------------------- (c)
def _emulate32(p, g, b, hp, fused):
    """The kernel's expression in float32: every operation rounded, or each multiply-add rounded once (the product of two fp32
    numbers is exact in float64; the sum is then rounded to float64 and to float32, the second rounding being the one that counts)."""
    lr, m, s = (np.float32(h) for h in hp)
    gs = g * s
    if fused:
        fma = lambda a, x, c: (a.astype(np.float64) * np.float64(x) + c.astype(np.float64)).astype(np.float32)
        b2 = fma(b, m, gs)
        t = fma(b2, m, gs)
        return fma(t, -lr, p), b2
    b2 = m * b + gs
    return p - lr * (gs + m * b2), b2


@pytest.mark.parametrize("fused", [False, True])
@pytest.mark.parametrize("n", R.GENERAL_N)
def test_general_bound_holds_a_float32_emulation(n, fused):
    c = R.general_case(n)
    p2, b2 = _emulate32(R.from_bits32(c["p0"]), R.from_bits32(c["g"]), R.from_bits32(c["b0"]), R.HP_GENERAL, fused)
    rp, rb = R.err_ratio(p2, c["p"], c["tol_p"]), R.err_ratio(b2, c["b"], c["tol_b"])
    print("UPD-ERR emulation n %d fused %d: p %.3g, b %.3g" % (n, fused, rp, rb))
    assert rp <= 1.0 and rb <= 1.0
    assert rp > 0.05 and rb > 0.05                                # ... and is no more than 20 times the largest error met
    assert float(c["tol_p"].max()) < 1e-6 and float(c["tol_b"].max()) < 1e-6


# ------------------------------------------------------------------------------------------------------------- (d)
def _check_tables(L):
    numel = [s["cout"] * s["taps"] * s["cin"] for s in L.segs]
    tiles = [s["taps"] * ((s["cout"] + 63) // 64) * ((s["cin"] + 63) // 64) for s in L.segs]
    assert L.desc.shape == (L.n_seg, 8) and L.prefix.shape == (L.n_seg + 1,) and L.tile_prefix.shape == (L.n_seg + 1,)
    for i, s in enumerate(L.segs):
        assert list(L.desc[i]) == [s["off"], s["wf_off"], s["wd_off"] if s["need_dgrad"] else -1, s["cout"], s["taps"], s["cin"], s["cin_pad"], s["cout_pad"]]
        assert L.prefix[i + 1] - L.prefix[i] == numel[i] and L.tile_prefix[i + 1] - L.tile_prefix[i] == tiles[i]
        assert s["cin_pad"] >= s["cin"] and s["cout_pad"] >= s["cout"] and s["cin_pad"] % 8 == 0 and s["cout_pad"] % 8 == 0
    assert L.prefix[0] == 0 and L.tile_prefix[0] == 0 and L.total == sum(numel) and L.total_tiles == sum(tiles)
    assert L.chunk_seg.shape == ((L.total + 4095) // 4096,) and L.tile_seg.shape == (L.total_tiles,)
    for c, sg in enumerate(L.chunk_seg):
        assert L.prefix[sg] <= 4096 * c < L.prefix[sg + 1]
    for t, sg in enumerate(L.tile_seg):
        assert L.tile_prefix[sg] <= t < L.tile_prefix[sg + 1]
    # nothing overlaps: masters in the flat buffer, forward copies, transposed copies
    for key, size in (("off", "numel"), ("wf_off", "wf_numel"), ("wd_off", "wd_numel")):
        spans = sorted((s[key], s[key] + s[size]) for s in L.segs if s[size] and s[key] >= 0)
        assert all(a[1] <= b[0] for a, b in zip(spans, spans[1:])), key
    assert max(s["off"] + s["numel"] for s in L.segs) <= L.numel and max(s["wf_off"] + s["wf_numel"] for s in L.segs) <= L.wf_numel
    assert max(s["wd_off"] + s["wd_numel"] for s in L.segs) <= L.wd_numel


def _check_delta(L):
    assert L.wf_delta.dtype == np.int32 and L.wf_delta.shape == (L.numel // 64,)
    want = np.full(L.numel // 64, R.INT32_MIN, dtype=np.int64)
    for s in L.segs:
        if s["cin"] % 8 == 0 and not s["shifted"]:
            assert s["off"] % 64 == 0 and s["wf_off"] % 64 == 0
            for e in range(s["off"], s["off"] + s["numel"], 64):
                want[e >> 6] = s["wf_off"] - s["off"]
            # the alignment padding behind the master maps into this copy's own 64-element step, not into a neighbour
            assert R.r64(s["numel"]) == R.r64(s["wf_numel"])
    assert np.array_equal(L.wf_delta.astype(np.int64), want)
    assert bool(np.all((want == R.INT32_MIN) | (want % 4 == 0)))


def test_batch_tables_satisfy_the_header():
    for aligned in (False, True):
        L = R.batch_layout(aligned)
        _check_tables(L)
        assert (L.prefix[3] % 4 != 0) == (not aligned)            # the 21 elements misalign every later 4-element group
        assert any(s["off"] % 4 for s in L.segs) and any(s["wd_off"] % 8 for s in L.segs if s["need_dgrad"])
        big = [i for i, s in enumerate(L.segs) if s["numel"] > 2 * 4096][-1]
        assert len(set(L.chunk_seg)) < len(L.chunk_seg) and int((L.chunk_seg == big).sum()) >= 2        # a segment across chunks
    for name, items in R.CAP_ITEMS.items():
        L = R.build_layout(items)
        _check_tables(L)
        assert L.total > 4096 * 4096 if name == "chunks" else L.total_tiles > 8192       # the grid caps of ep24_pack_weights_batched


def test_update_layouts_satisfy_the_header():
    for name in R.UPDATE_ITEMS:
        L = R.update_layout(name)
        _check_tables(L)
        _check_delta(L)
        d = set(L.wf_delta.tolist())
        assert R.INT32_MIN in d and 0 in d and any(R.INT32_MIN < v < 0 for v in d)
        assert L.n % 4 == 1 and L.wf_delta[(L.n - 1) >> 6] != R.INT32_MIN and L.cuts[-1] == L.n
        assert all(c % 4 == 0 for c in L.cuts[:-1]) and L.cuts == sorted(L.cuts)
        assert any(s["mapped"] and s["off"] < c < s["off"] + s["numel"] and c % 64 for c in L.cuts[:-1] for s in L.segs)
    d = set(R.update_layout("small").wf_delta.tolist())
    assert any(v > 0 for v in d)
    assert any(s["mapped"] and s["numel"] % 64 for s in R.update_layout("small").segs)
    assert R.update_layout("big").n > (1 << 21) + 4                # the second trip of the grid-stride loop, with a copy to write


# ------------------------------------------------------------------------------------------------------------- (e)
def _mutant_sgd(p, g, b, first, hp, kind):
    lr, m, s = hp
    gs = g * s * (s if kind == "scale_twice" else 1.0)
    b2 = gs if (first and kind != "first_ignored") else m * b + gs
    return p - lr * (b2 if kind == "plain_momentum" else gs + m * b2), b2


@pytest.mark.parametrize("kind", ["first_ignored", "plain_momentum", "scale_twice"])
@pytest.mark.parametrize("n", SMALL_N)
def test_update_mutants_are_rejected_by_the_exact_cases(n, kind):
    """On the inputs of the exact tests: the first step runs with the buffer full of NaN, the later ones with what the step before left."""
    c = R.dyadic_case(n)
    p, g = R.from_bits32(c["p0"]).astype(np.float64), [R.from_bits32(x).astype(np.float64) for x in c["g"]]
    b = np.full(n, np.nan)
    caught = False
    for k in range(R.STEPS):
        p2, b2 = _mutant_sgd(p, g[k], b, k == 0, R.HP_DYADIC, kind)
        wp, wb, _ = c["want"][k]
        caught = caught or not (R.same_bits(R.bits32(p2), wp) and R.same_bits(R.bits32(b2), wb))
        p, b = R.from_bits32(wp).astype(np.float64), R.from_bits32(wb).astype(np.float64)     # the test checks every step from the true state
    assert caught


@pytest.mark.parametrize("kind", ["first_ignored", "plain_momentum", "scale_twice"])
def test_update_mutants_are_rejected_by_the_general_bound(kind):
    c = R.general_case(R.GENERAL_N[0])
    a = [R.from_bits32(c[k]).astype(np.float64) for k in ("p0", "g", "b0")]
    first = kind == "first_ignored"                               # the general step is no first step: the opposite slip, b not read
    p2, b2 = _mutant_sgd(a[0], a[1], a[2], first, R.HP_GENERAL, "" if first else kind)
    assert max(R.err_ratio(p2.astype(np.float32), c["p"], c["tol_p"]), R.err_ratio(b2.astype(np.float32), c["b"], c["tol_b"])) > 1.0


@pytest.mark.parametrize("n", SMALL_N)
def test_ema_from_the_old_p_is_rejected(n):
    c = R.dyadic_case(n)
    e = R.ema_ref(R.from_bits32(c["e0"]), R.from_bits32(c["p0"]), R.EMA_D, R.EMA_OMD)
    assert not R.same_bits(R.bits32(e), c["want"][0][2])


def test_truncation_is_rejected():
    trunc = lambda b: (np.asarray(b, dtype=np.uint32) >> np.uint32(16)).astype(np.uint16)
    assert not R.same_bits(trunc(R.SPECIAL32), R.SPECIAL16)
    for name in R.UPDATE_ITEMS:
        for draw in ("dyadic", "pass"):
            c = R.update_case(name, draw)
            for (p, _), img in zip(c["want"], c["wf"]):
                mut = np.full_like(img, R.SENT16)
                e = np.arange(c["L"].n)
                d = c["L"].wf_delta[e >> 6].astype(np.int64)
                mut[(e + d)[d != R.INT32_MIN]] = trunc(p)[d != R.INT32_MIN]
                assert not R.same_bits(mut, img), (name, draw)
    for n in (4, 1028):
        assert not R.same_bits(trunc(R.random_bits(n, 21)), R.bf16_rne(R.random_bits(n, 21)))       # the cast test's inputs


@pytest.mark.parametrize("draw", ["dyadic", "pass"])
@pytest.mark.parametrize("name", list(R.UPDATE_ITEMS))
def test_wrong_group_and_skipped_tail_are_rejected(name, draw):
    c = R.update_case(name, draw)
    L, p, img = c["L"], c["want"][0][0], c["wf"][0]
    e = np.arange(L.n)
    # the delta of the next group: wrong wherever the neighbour belongs to another segment
    d = L.wf_delta[np.minimum((e >> 6) + 1, L.wf_delta.size - 1)].astype(np.int64)
    mut = np.full_like(img, R.SENT16)
    mut[(e + d)[d != R.INT32_MIN]] = R.bf16_rne(p)[d != R.INT32_MIN]
    assert not R.same_bits(mut, img)
    # the last element of the scalar tail never converted
    mut = np.full_like(img, R.SENT16)
    R.update_into(mut, L, p, 0, L.n - 1)
    assert not R.same_bits(mut, img)
    # ... nor updated
    assert c["want"][0][0][L.n - 1] != c["p0"][L.n - 1] or draw == "pass"


def test_skipped_tail_is_rejected_by_the_plain_cases():
    for n in SMALL_N:
        c = R.dyadic_case(n)
        assert c["want"][0][0][n - 1] != c["p0"][n - 1] or c["want"][0][1][n - 1] != R.NAN32


@pytest.mark.parametrize("aligned", [False, True])
def test_pack_mutants_are_rejected(aligned):
    L = R.batch_layout(aligned)
    master = R.random_bits(L.numel, 31)
    wf, wd = np.full(L.wf_numel, R.SENT16, dtype=np.uint16), R.wd_prefill(L)
    R.pack_layout_into(wf, wd, L, master)
    assert not bool(np.any(wd[np.concatenate([np.arange(s["wd_off"], s["wd_off"] + s["wd_numel"]).reshape(s["cin"], s["taps"], s["cout_pad"])[:, :, :s["cout"]].reshape(-1)
                                              for s in L.segs if s["need_dgrad"]])] == R.SENT16))           # every real position was written
    for s in L.segs:
        w = R.master_rows(master, s["off"], s["cout"], s["taps"], s["cin"])
        if s["need_dgrad"] and s["cin"] > 1:
            # ci and co swapped: w[ci][t][co] written where w[co][t][ci] belongs (the part of the block where both exist)
            mut = wd.copy()
            blk = mut[s["wd_off"]:s["wd_off"] + s["wd_numel"]].reshape(s["cin"], s["taps"], s["cout_pad"])
            k = min(s["cin"], s["cout"])
            blk[:k, :, :k] = R.bf16_rne(w)[:k, :, :k]
            assert not R.same_bits(mut, wd), s
        if s["need_dgrad"] and s["cout_pad"] > s["cout"]:
            mut = wd.copy()
            mut[s["wd_off"]:s["wd_off"] + s["wd_numel"]].reshape(s["cin"], s["taps"], s["cout_pad"])[:, :, s["cout"]] = R.bf16_rne(w)[0].transpose(1, 0)
            assert not R.same_bits(mut, wd), s
        if s["cin_pad"] > s["cin"]:
            mut = wf.copy()
            mut[s["wf_off"]:s["wf_off"] + s["wf_numel"]].reshape(s["cout"], s["taps"], s["cin_pad"])[:, :, s["cin"]] = R.bf16_rne(w)[:, :, 0]
            assert not R.same_bits(mut, wf), s
