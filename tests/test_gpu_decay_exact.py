"""Weight decay by parameter group in the fused update (csrc/elementwise.hip sgd_kernel<true>; ep24_sgd_nesterov_decay,
ep24_sgd_nesterov_decay_hp_range_pack, ep24_set_hparams_decay) against tests/decay_reference.py, through the C ABI and through
ParamHome / SGD / TrainStep / train_24p.py.

Kernel level, every buffer between two guards of 64 sentinel elements: dyadic draws (every product and sum an fp32 number; lr, m, s
and the decay powers of two) bit for bit over three steps - the first with first_flag set over a buffer full of NaN - at the lengths
1 .. 194 from the range starts 0, 4, 64, 68 under a table that alternates 1, 0, 1, and once just above the grid cap (MAX_BLOCKS =
2048 workgroups x 256 lanes x 4 elements, so the grid-stride loop wraps at 2^21); normal draws within the derived bound of the
float64 formula (decay_reference.decay_tol); decay 0 and the non-decaying groups bit-identical to ep24_sgd_nesterov_hp_range_pack.

Model level (test_gpu_engine.tiny_model, B = 2, 64 x 64): the captured step against the eager loop with stock YOLOX's three groups,
one step against torch.optim.SGD, the switch-over rules of TrainStep.set_weight_decay, the entry point with --weight-decay.

The general draw's largest err / tol (1.0 is the bound), measured on an MI355X: 0.966 for p' and 0.826 for b' from a filled buffer,
0.975 / 0.482 on a first step, and the op-by-op float32 emulation matched bit for bit in all four (recorded, not asserted: the test
prints the figures, DECAY-ERR, before it asserts).  The captured and the eager loop differed by 0 in every element (DECAY-STEP).
"""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import decay_reference as D  # noqa: E402
import update_reference as R  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
E_ARG = -1
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
Y24 = os.path.join(ROOT, "exploration-of-potential_amd", "yolox_24p")


def _abi():
    from ep24._lib import call, lib, ptr, stream_ptr
    return call, ptr, stream_ptr, lib()


def G(n, kind, fill=None):
    return R.Guarded(n, kind, DEV, fill)


def sync():
    torch.cuda.synchronize()


def make_hp(hp3, w, with_ema=True):
    """The device block of ep24_set_hparams_decay between guards: hp[0..5] written, hp[6..7] left alone."""
    call, _, sp, _ = _abi()
    hp = G(8, "f32")
    d, omd = (R.EMA_D, R.EMA_OMD) if with_ema else (0.0, 0.0)
    call("set_hparams_decay", hp.ptr(), hp3[0], hp3[1], hp3[2], d, omd, w, sp())
    sync()
    want = np.full(8, R.SENT32, dtype=np.uint32)
    want[:6] = R.bits32(np.array([hp3[0], hp3[1], hp3[2], d, omd, w], dtype=np.float32))
    hp.check(want, "hp")
    return hp


class Flat:
    """p, buf, ema and the packed copy of one flat buffer of N elements between guards, its decay table (and a wf_delta table of
    zeros: the copy of element e is wf[e]) and the first-step flag between two guard words."""

    def __init__(self, N, p0, b0, e0, table, flag, pack=True):
        self.N = N
        self.p, self.b = G(N, "f32", p0), G(N, "f32", b0)
        self.e = None if e0 is None else G(N, "f32", e0)
        self.table_host = np.asarray(table, dtype=np.uint8)
        assert self.table_host.size >= (N + 63) // 64                 # the kernel reads table[(first + i) >> 6] for i < n
        self.table = G(self.table_host.size, "u8", self.table_host)
        self.flag = G(1, "i32", [flag])
        self.delta = G((N + 63) // 64, "i32", np.zeros((N + 63) // 64, dtype=np.int32)) if pack else None
        self.wf = G(R.r64(N), "bf16") if pack else None
        self.wf_img = np.full(R.r64(N), R.SENT16, dtype=np.uint16)

    def decay(self, g, hp, lo=0, n=None, last=1):
        call, _, sp, _ = _abi()
        n = self.N - lo if n is None else n
        assert 0 <= lo and lo + n <= self.N
        call("sgd_nesterov_decay_hp_range_pack", self.p.ptr(), g.ptr(), self.b.ptr(), lo, n, hp.ptr(), self.flag.ptr(),
             None if self.e is None else self.e.ptr(), last, None if self.delta is None else self.delta.ptr(),
             None if self.wf is None else self.wf.ptr(), self.table.ptr(), sp())
        sync()

    def plain(self, g, hp, lo=0, n=None, last=1):
        """the entry point from before the decay, on the same buffers"""
        call, _, sp, _ = _abi()
        n = self.N - lo if n is None else n
        call("sgd_nesterov_hp_range_pack", self.p.ptr(), g.ptr(), self.b.ptr(), lo, n, hp.ptr(), self.flag.ptr(),
             None if self.e is None else self.e.ptr(), last, self.delta.ptr(), self.wf.ptr(), sp())
        sync()

    def check_tables(self):
        self.table.check(self.table_host, "decay_grp")
        if self.delta is not None:
            self.delta.check(np.zeros(self.delta.n, dtype=np.int32), "wf_delta")


def _dyadic_steps(N, lo, n, flag):
    """Three steps on [lo, lo + n) of a flat buffer of N elements: inside the range the step's result, outside it what was there."""
    c = D.dyadic_case(N, bool(flag))
    nan = np.full(N, R.NAN32, dtype=np.uint32)
    b0 = nan if flag else c["b0"]
    st = Flat(N, c["p0"], b0, c["e0"], c["table"], flag)
    hp = make_hp(D.HP_DYADIC, D.W_DYADIC)
    cur = [c["p0"].copy(), b0.copy(), c["e0"].copy()]
    for k in range(D.STEPS):
        g = G(N, "f32", c["g"][k])
        st.decay(g, hp, lo, n, last=1)
        for buf, have, want, what in zip((st.p, st.b, st.e), cur, c["want"][k], ("p'", "buf'", "ema'")):
            have[lo:lo + n] = want[lo:lo + n]
            got = buf.check(have, "%s step %d of [%d, %d) in %d, flag %d" % (what, k, lo, lo + n, N, flag))
            assert not R.is_nan32(got[lo:lo + n]).any()
        st.wf_img[lo:lo + n] = R.bf16_rne(c["want"][k][0][lo:lo + n])
        st.wf.check(st.wf_img, "w_fwd step %d" % k)
        g.check(c["g"][k], "g")
        st.flag.check([0], "first_flag")
    st.check_tables()
    hp.check(hp.read()[0], "hp guards")
    return c


@pytest.mark.parametrize("first", D.STARTS)
@pytest.mark.parametrize("n", D.LENGTHS)
def test_decay_lengths_and_range_starts_exact(n, first):
    """The vector body, the scalar tail and a group boundary next to a 4-element step, from range starts inside and at the head of a
    group; the table alternates, so from 65 elements on one launch crosses decaying and non-decaying groups.  With first_flag set
    (the buffer full of NaN is not read) and clear."""
    for flag in (1, 0):
        _dyadic_steps(first + n, first, n, flag)


def test_decay_beyond_the_grid_cap():
    c = _dyadic_steps(D.CAP_N, 0, D.CAP_N, 1)
    assert D.CAP_N > 2048 * 1024 and D.CAP_N % 4 == 3
    dec = D.elements(c["table"], D.CAP_N)
    assert dec[2048 * 1024] and not dec[2048 * 1024 - 1]              # the wrap of the grid-stride loop is a group boundary of both kinds


@pytest.mark.parametrize("flag", [0, 1])
def test_decay_general_draw_within_the_derived_bound(flag):
    n = 4100
    c = D.general_case(n, bool(flag))
    st = Flat(n, c["p0"], c["b0"], None, c["table"], flag, pack=False)
    hp = make_hp(D.HP_GENERAL, D.W_GENERAL)
    g = G(n, "f32", c["g"])
    st.decay(g, hp)
    p, _ = st.p.read()
    b, _ = st.b.read()
    rp, rb = R.err_ratio(R.from_bits32(p), c["p"], c["tol_p"]), R.err_ratio(R.from_bits32(b), c["b"], c["tol_b"])
    print("DECAY-ERR general n %d first %d: p %.3g b %.3g of the bound; float32 emulation bit for bit: p %s (%d differ) b %s (%d differ)"
          % (n, flag, rp, rb, R.same_bits(p, c["emu_p"]), R.mismatches(p, c["emu_p"]).size, R.same_bits(b, c["emu_b"]),
             R.mismatches(b, c["emu_b"]).size))
    st.p.check(p, "p guards")
    st.b.check(b, "buf guards")
    g.check(c["g"], "g")
    assert rp <= 1.0 and rb <= 1.0, (rp, rb)


def _general_flat(n, table, flag=0):
    p, g, b = R.general_draw(n, 3)
    e = np.random.default_rng(77).standard_normal(n).astype(np.float32)
    return Flat(n, R.bits32(p), R.bits32(b), R.bits32(e), table, flag), G(n, "f32", R.bits32(g))


def _read(st):
    return [x.read()[0].copy() for x in (st.p, st.b, st.e, st.wf)]


def test_zero_decay_and_non_decaying_groups_equal_the_plain_kernel():
    """Normal draws at n = 4099 (a scalar tail) in two ranges.  (1) decay = 0 with a table of ones: p, buf, ema and w_fwd bit-identical
    to ep24_sgd_nesterov_hp_range_pack on the same inputs.  (2) decay != 0 under the alternating table: the elements of the
    non-decaying groups are bit-identical to it, and the decaying ones are not."""
    call, _, sp, _ = _abi()
    n, cut = 4099, 132
    groups = (n + 63) // 64
    ref, g = _general_flat(n, np.ones(groups, dtype=np.uint8))
    hp_plain = G(8, "f32")
    call("set_hparams", hp_plain.ptr(), *D.HP_GENERAL, R.EMA_D, R.EMA_OMD, sp())
    ref.plain(g, hp_plain, cut, n - cut, last=0)
    ref.plain(g, hp_plain, 0, cut, last=1)
    want = _read(ref)
    zero, g0 = _general_flat(n, np.ones(groups, dtype=np.uint8))
    hp0 = make_hp(D.HP_GENERAL, 0.0)
    zero.decay(g0, hp0, cut, n - cut, last=0)
    zero.decay(g0, hp0, 0, cut, last=1)
    for got, w, what in zip(_read(zero), want, ("p'", "buf'", "ema'", "w_fwd")):
        R.assert_same(got, w, "decay 0: " + what)
    for x in (zero.p, zero.b, zero.e, zero.wf):
        x.check(x.read()[0], "guards")
    table = D.alternating_table(n)
    some, g1 = _general_flat(n, table)
    hp1 = make_hp(D.HP_GENERAL, D.W_GENERAL)
    some.decay(g1, hp1, cut, n - cut, last=0)
    some.decay(g1, hp1, 0, cut, last=1)
    dec = D.elements(table, n)
    got = _read(some)
    for a, w, what in zip(got[:3], want[:3], ("p'", "buf'", "ema'")):
        R.assert_same(a[~dec], w[~dec], "non-decaying groups: " + what)
    R.assert_same(got[3][:n][~dec], want[3][:n][~dec], "non-decaying groups: w_fwd")
    assert (got[1][dec] != want[1][dec]).mean() > 0.9 and (got[0][dec] != want[0][dec]).any()
    for x in (some.p, some.b, some.e, some.wf):
        x.check(x.read()[0], "guards")
    some.check_tables()


def test_flag_handling_and_the_by_value_form():
    """last = 0 leaves first_flag, last = 1 clears it; ep24_sgd_nesterov_decay (by value, whole buffer, clears the flag) gives the bits
    of the device-block form."""
    call, _, sp, _ = _abi()
    n = 194
    c = D.general_case(4100, True)
    sl = lambda a: a[:n].copy()
    nan = np.full(n, R.NAN32, dtype=np.uint32)
    table = c["table"][:(n + 63) // 64]
    a = Flat(n, sl(c["p0"]), nan, None, table, 1, pack=False)
    hp = make_hp(D.HP_GENERAL, D.W_GENERAL, with_ema=False)
    g = G(n, "f32", sl(c["g"]))
    a.decay(g, hp, 64, n - 64, last=0)
    a.flag.check([1], "first_flag after last = 0")
    a.decay(g, hp, 0, 64, last=1)
    a.flag.check([0], "first_flag after last = 1")
    b = Flat(n, sl(c["p0"]), nan, None, table, 1, pack=False)
    lr, m, s = D.HP_GENERAL
    for step in range(2):                                            # the first step and one that reads the buffer
        if step:
            a.decay(g, hp)
        call("sgd_nesterov_decay", b.p.ptr(), g.ptr(), b.b.ptr(), n, lr, m, s, D.W_GENERAL, b.table.ptr(), b.flag.ptr(), sp())
        sync()
        b.flag.check([0], "first_flag after the by-value form")
        b.p.check(a.p.read()[0], "by value: p' step %d" % step)
        b.b.check(a.b.read()[0], "by value: buf' step %d" % step)
    assert not R.is_nan32(b.p.read()[0]).any() and not R.is_nan32(b.b.read()[0]).any()


def test_decay_refusals():
    """EP24_E_ARG before any launch - a null table above all - and every buffer unchanged afterwards."""
    _, _, sp, lib = _abi()
    n = 64
    c = D.dyadic_case(n, False)
    st = Flat(n, c["p0"], c["b0"], c["e0"], c["table"], 1)
    hp = make_hp(D.HP_DYADIC, D.W_DYADIC)
    g = G(n, "f32", c["g"][0])
    lr, m, s = D.HP_DYADIC
    P, Gp, B, E, H, F, T, Dl, W = (st.p.ptr(), g.ptr(), st.b.ptr(), st.e.ptr(), hp.ptr(), st.flag.ptr(), st.table.ptr(), st.delta.ptr(),
                                   st.wf.ptr())
    good = {"ep24_sgd_nesterov_decay": [P, Gp, B, n, lr, m, s, D.W_DYADIC, T, F, sp()],
            "ep24_sgd_nesterov_decay_hp_range_pack": [P, Gp, B, 0, n, H, F, E, 1, Dl, W, T, sp()]}
    refused = 0
    for name, args in good.items():
        names = [a for _, a in lib.protos[name][1]]
        bad = [(k, None) for k in ("decay_grp", "p", "g", "buf", "first_flag")] + [("n", 0), ("p", P + 4), ("g", Gp + 4), ("buf", B + 4)]
        if "hp" in names:
            bad += [("hp", None), ("ema", E + 4), ("first", 2), ("first", -4), ("wf", W + 8), ("wf", None), ("wf_delta", None)]
        for key, val in bad:
            a = list(args)
            a[names.index(key)] = val
            assert lib.fn[name](*a) == E_ARG, (name, key, val)
            refused += 1
    assert refused == 9 + 16
    assert lib.fn["ep24_set_hparams_decay"](None, lr, m, s, 0.0, 0.0, D.W_DYADIC, sp()) == E_ARG
    sync()
    st.p.check(c["p0"], "p")
    st.b.check(c["b0"], "buf")
    st.e.check(c["e0"], "ema")
    g.check(c["g"][0], "g")
    st.flag.check([1], "first_flag")
    st.wf.check(st.wf_img, "w_fwd")
    # ema and the packed copy are optional together with their table: the _hp and _hp_range forms
    args = list(good["ep24_sgd_nesterov_decay_hp_range_pack"])
    args[7] = args[9] = args[10] = None
    assert lib.fn["ep24_sgd_nesterov_decay_hp_range_pack"](*args) == 0
    sync()
    st.p.check(D.dyadic_case(n, True)["want"][0][0], "p' without ema and packed copy")
    st.e.check(c["e0"], "ema")
    st.wf.check(st.wf_img, "w_fwd")


# ---------------------------------------------------------------------------------------------------------------------------
B, S, LR, MOM, WDEC = 2, 64, 0.01, 0.9, 5e-4


def _batch():
    from ep24 import synth
    return synth.make_images(B, S, seed=1).to(DEV), synth.make_labels(B, [2, 1], size=S, seed=2).to(DEV)


def _model():
    import test_gpu_engine as TE
    torch.manual_seed(0)
    m = TE.tiny_model()
    m.head.initialize_biases(1e-2)
    return m


def _eager_steps(m, opt, steps):
    from ep24 import loss as eloss
    lf = eloss.Loss_Function(80)
    lf.draw = False
    images, labels = _batch()
    for _ in range(steps):
        opt.zero_grad()
        lf(m(images, train=True), labels)[0].backward()
        opt.step()
    sync()


def test_default_table_is_the_stock_decay_group():
    """pg1 of ep24.train.yolox_param_groups = the parameters of the home's conv segments; the table marks exactly their groups,
    alignment padding included."""
    from ep24.engine import param_home
    from ep24.train import yolox_param_groups
    m = _model()
    home = param_home(m)
    pg = yolox_param_groups(m, WDEC)
    assert {id(p) for p in pg[1]["params"]} == {id(p) for s in home.convs for p in s.params}
    assert {id(p) for p in pg[0]["params"] + pg[2]["params"]} == {id(p) for s in home.vecs for p in s.params}
    want = np.zeros(home.numel // 64, dtype=np.uint8)
    for s in home.convs:
        want[s.off // 64:R.r64(s.off + s.numel) // 64] = 1
    assert np.array_equal(home.decay_grp.cpu().numpy(), want) and 0 < want.sum() < want.size
    # parameters that share a segment decay together or not at all
    from ep24._lib import Ep24Error
    shared = next(s for s in home.convs if len(s.params) == 2)
    with pytest.raises(Ep24Error, match="share"):
        home.set_decay_params([shared.params[0]])
    assert np.array_equal(home.decay_grp.cpu().numpy(), want)
    home.set_decay_params([])
    assert int(home.decay_grp.sum()) == 0
    home.set_decay_params(pg[1]["params"])
    assert np.array_equal(home.decay_grp.cpu().numpy(), want)


@pytest.mark.parametrize("graph_backward", [False, True])
def test_captured_step_equals_the_eager_loop_with_three_groups(graph_backward):
    """(a) three steps each: home.flat and home.mflat torch.equal."""
    from ep24 import loss as eloss, train as etrain
    from ep24.engine import param_home
    ma, mb = _model(), _model()
    mb.load_state_dict(ma.state_dict())
    opt = etrain.SGD(etrain.yolox_param_groups(ma, WDEC), lr=LR, momentum=MOM, nesterov=True, model=ma)
    _eager_steps(ma, opt, 3)
    ts = etrain.TrainStep(mb, eloss.Loss_Function(80), lr=LR, momentum=MOM, batch=B, size=S, graph_backward=graph_backward, weight_decay=WDEC)
    images, labels = _batch()
    for _ in range(3):
        ts.step(images, labels)
    sync()
    ha, hb = param_home(ma), ts.home
    print("DECAY-STEP graph_backward %s: max |flat a - b| %.3g, max |mflat a - b| %.3g" %
          (graph_backward, float((ha.flat - hb.flat).abs().max()), float((ha.mflat - hb.mflat).abs().max())))
    assert torch.equal(ha.flat, hb.flat) and torch.equal(ha.mflat, hb.mflat)


def test_one_eager_step_against_torch_sgd():
    """(b) the gradients are copied off the device before the update; torch.optim.SGD runs in float64 on the CPU from the same p and
    g (lr, momentum and decay the fp32 numbers the kernel receives), and every parameter stays within decay_reference.decay_tol of
    it.  Against the update without decay on the same p and g: every conv weight moved differently, BatchNorm vectors and biases bit
    for bit the same; the alignment padding is still zero."""
    from ep24 import train as etrain
    from ep24.engine import param_home
    m = _model()
    opt = etrain.SGD(etrain.yolox_param_groups(m, WDEC), lr=LR, momentum=MOM, nesterov=True, model=m)
    home = param_home(m)
    from ep24 import loss as eloss
    lf = eloss.Loss_Function(80)
    lf.draw = False
    images, labels = _batch()
    opt.zero_grad()
    lf(m(images, train=True), labels)[0].backward()
    sync()
    names = [n for n, _ in m.named_parameters()]
    p0 = {n: p.detach().cpu().clone() for n, p in m.named_parameters()}
    g0 = {n: p.grad.detach().cpu().clone() for n, p in m.named_parameters()}
    flat0, gflat0 = home.flat.clone(), home.gflat.clone()
    assert int(home.first_flag) == 1
    opt.step()
    sync()
    flat_decay = home.flat.clone()
    got = {n: p.detach().cpu().clone() for n, p in m.named_parameters()}
    # torch, float64
    ref = {n: torch.nn.Parameter(p0[n].double()) for n in names}
    by_id = {id(p): n for n, p in m.named_parameters()}
    groups = [{"params": [ref[by_id[id(p)]] for p in grp["params"]], "weight_decay": R.f32(grp["weight_decay"])} for grp in opt.param_groups]
    topt = torch.optim.SGD(groups, lr=R.f32(LR), momentum=R.f32(MOM), nesterov=True)
    for n in names:
        ref[n].grad = g0[n].double()
    topt.step()
    decaying = {by_id[id(p)] for p in opt.param_groups[1]["params"]}
    worst = 0.0
    for n in names:
        p, g = p0[n].double().numpy().reshape(-1), g0[n].double().numpy().reshape(-1)
        dec = np.full(p.size, n in decaying)
        p2, _, mid = D.sgd_decay_ref(p, g, None, True, R.f32(LR), R.f32(MOM), 1.0, R.f32(WDEC), dec)
        tol, _ = D.decay_tol(mid, True, R.f32(LR), R.f32(MOM), dec)
        want = ref[n].detach().numpy().reshape(-1)
        assert float(np.abs(want - p2).max()) <= 1e-12 * float(np.abs(p2).max())        # torch float64 is the formula
        r = R.err_ratio(got[n].numpy().reshape(-1), want, tol)
        worst = max(worst, r)
        assert r <= 1.0, (n, r)
    print("DECAY-ERR model: largest |p' - torch float64| / bound %.3g" % worst)
    # the same p and g without decay
    with torch.no_grad():
        home.flat.copy_(flat0)
        home.gflat.copy_(gflat0)
        home.mflat.zero_()
        home.first_flag.fill_(1)
    home.sgd(LR, MOM, 1.0)
    sync()
    plain = {n: p.detach().cpu().clone() for n, p in m.named_parameters()}
    for n in names:
        if n in decaying:
            assert not torch.equal(plain[n], got[n]), n
        else:
            assert torch.equal(plain[n], got[n]), n
    assert len(decaying) == sum(len(s.params) for s in home.convs)
    mask = torch.zeros(home.numel, dtype=torch.bool)
    for s in home.order:
        mask[s.off:s.off + s.numel] = True
    assert bool((~mask).any()) and float(flat_decay.cpu()[~mask].abs().max()) == 0.0 and float(home.mflat.cpu()[~mask].abs().max()) == 0.0


def test_zero_decay_is_the_step_without_the_argument():
    """(c) two steps, bit for bit; the update's launches are the ones from before the decay."""
    from ep24 import loss as eloss, train as etrain
    out = []
    for kw in ({}, {"weight_decay": 0.0}):
        m = _model()
        ts = etrain.TrainStep(m, eloss.Loss_Function(80), lr=LR, momentum=MOM, batch=B, size=S, **kw)
        images, labels = _batch()
        for _ in range(2):
            ts.step(images, labels)
        sync()
        out.append((ts.home.flat.clone(), ts.home.mflat.clone(), float(ts.hp[5])))
    assert torch.equal(out[0][0], out[1][0]) and torch.equal(out[0][1], out[1][1])
    assert out[0][2] == out[1][2] == 0.0


def test_set_weight_decay_recaptures_only_across_zero():
    """(d)"""
    from ep24 import loss as eloss, train as etrain
    m = _model()
    ts = etrain.TrainStep(m, eloss.Loss_Function(80), lr=LR, momentum=MOM, batch=B, size=S)
    images, labels = _batch()
    ts.step(images, labels)
    g0 = ts.g_upd
    ts.set_weight_decay(WDEC)
    ts.step(images, labels)
    g1 = ts.g_upd
    sync()
    assert g1 is not g0 and float(ts.hp[5]) == R.f32(WDEC)
    ts.set_weight_decay(1e-4)
    before = ts.home.flat.clone()
    ts.step(images, labels)
    sync()
    assert ts.g_upd is g1 and float(ts.hp[5]) == R.f32(1e-4) and not torch.equal(before, ts.home.flat)
    ts.set_weight_decay(1e-4)
    ts.step(images, labels)
    assert ts.g_upd is g1
    ts.set_weight_decay(0.0)
    ts.step(images, labels)
    sync()
    assert ts.g_upd is not g1
    with pytest.raises(ValueError):
        ts.set_weight_decay(-1.0)


def test_trainer_weight_decay_flag_checkpoint_and_resume(tmp_path):
    """(e) train_24p.py --synthetic --steps 3 --weight-decay on a tiny Exp: three optimizer groups with decays [0, 5e-4, 0] in the
    checkpoint; --resume from it runs (also without a value behind the flag: the checkpoint's decay is restored); --resume from a
    checkpoint written without the flag stops with both layouts in the message."""
    sys.path.insert(0, Y24)
    try:
        import importlib
        mod = importlib.import_module("train_24p")
        from exp import get_exp

        def run(out, *extra):
            exp = get_exp(os.path.join(Y24, "load_train", "yolox_24p_train.py"))
            exp.width, exp.input_size, exp.synthetic_len, exp.synthetic_gts = 0.125, (64, 64), 8, 2
            args = mod.make_parser().parse_args(["-b", "2", "-l", "0.01", "--synthetic", "--log-interval", "1", "--loader-workers", "0",
                                                 "--output-dir", str(tmp_path / out)] + list(extra))
            tr = mod.main(exp, args)
            torch.cuda.synchronize()
            return tr, os.path.join(str(tmp_path / out), "yolox_24p", "last_epoch_ckpt.pth")

        tr, path = run("a", "--steps", "3", "--weight-decay")
        assert tr.run_steps == 3
        ck = torch.load(path, map_location="cpu")
        assert [g["weight_decay"] for g in ck["optimizer"]["param_groups"]] == [0.0, 5e-4, 0.0]
        sizes = [len(g["params"]) for g in ck["optimizer"]["param_groups"]]
        assert len(ck["optimizer"]["state"]) == sum(sizes) == len(list(tr.model.parameters()))
        tr2, path2 = run("b", "--steps", "1", "-c", path, "--resume", "--weight-decay", "1e-4")
        assert tr2.run_steps == 1 and tr2.current_step == 4
        assert tr2.optimizer.weight_decay == 5e-4                    # the checkpoint's, not the flag's
        ck2 = torch.load(path2, map_location="cpu")
        assert [g["weight_decay"] for g in ck2["optimizer"]["param_groups"]] == [0.0, 5e-4, 0.0]
        m1, m2 = ck["optimizer"]["state"][sizes[0]]["momentum_buffer"], ck2["optimizer"]["state"][sizes[0]]["momentum_buffer"]
        assert m1.shape == m2.shape and float(m2.abs().max()) > 0 and not torch.equal(m1, m2)
        _, plain = run("c", "--steps", "1")
        assert len(torch.load(plain, map_location="cpu")["optimizer"]["param_groups"]) == 1
        with pytest.raises(ValueError, match=r"\[%d\].*\[%d, %d, %d\]" % (sum(sizes), sizes[0], sizes[1], sizes[2])):
            run("d", "--steps", "1", "-c", plain, "--resume", "--weight-decay")
        with pytest.raises(ValueError, match=r"\[%d, %d, %d\].*\[%d\]" % (sizes[0], sizes[1], sizes[2], sum(sizes))):
            run("e", "--steps", "1", "-c", path, "--resume")
    finally:
        sys.path.remove(Y24)
