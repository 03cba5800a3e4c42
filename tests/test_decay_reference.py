"""CPU checks of tests/decay_reference.py and of the host side of weight decay by parameter group: the float64 formula against
torch.optim.SGD(nesterov=True, weight_decay) with a decaying and a non-decaying group over three steps, the float32 emulation within
the derived bound, three mutants rejected by the same comparison, the dyadic draws exact in fp32; ep24.train.yolox_param_groups
against an independent restatement of stock YOLOX's rule (default backbone and resnet); the --weight-decay flag; what ep24.train.SGD
refuses before it touches a device."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import decay_reference as D  # noqa: E402
import update_reference as R  # noqa: E402

N = 257                                      # four groups and one element; the alternating table: groups 0, 2, 4 decay
LR, MOM, S, W = 0.0123, 0.9, 0.5, 5e-4


def _torch_steps(p, gs, dec, dtype, w=W):
    """Three steps of torch.optim.SGD on two parameter groups (the decaying elements, the others); g arrives scaled: torch has no
    grad_scale, and the formula scales g before anything else.  -> [(p', b')] per step"""
    td = torch.from_numpy
    a, c = torch.nn.Parameter(td(p[dec]).to(dtype)), torch.nn.Parameter(td(p[~dec]).to(dtype))
    opt = torch.optim.SGD([{"params": [a], "weight_decay": w}, {"params": [c], "weight_decay": 0.0}], lr=LR, momentum=MOM, nesterov=True)
    out = []
    for g in gs:
        a.grad, c.grad = td(g[dec]).to(dtype), td(g[~dec]).to(dtype)
        opt.step()
        q, b = np.empty(p.size), np.empty(p.size)
        q[dec], q[~dec] = a.detach().double().numpy(), c.detach().double().numpy()
        b[dec], b[~dec] = opt.state[a]["momentum_buffer"].double().numpy(), opt.state[c]["momentum_buffer"].double().numpy()
        out.append((q, b))
    return out


def _draw():
    rng = np.random.default_rng(5)
    p = rng.standard_normal(N).astype(np.float32).astype(np.float64)
    g = [(rng.standard_normal(N) * 0.3).astype(np.float32).astype(np.float64) for _ in range(3)]
    return p, g, D.elements(D.alternating_table(N), N)


def _formula_steps(fn, p, g, dec):
    b, out = np.zeros(N), []
    for k, gk in enumerate(g):
        p, b = fn(p, gk, b, k == 0, LR, MOM, S, W, dec)[:2]
        out.append((p, b))
    return out


def _worst_rel(got, want):
    return max(float(np.max(np.abs(a - b) / np.maximum(np.abs(b), 1e-30))) for x, y in zip(got, want) for a, b in zip(x, y))


def test_float64_formula_equals_torch_sgd():
    p, g, dec = _draw()
    assert dec.any() and (~dec).any()
    want = _torch_steps(p, [x * S for x in g], dec, torch.float64)
    assert _worst_rel(_formula_steps(D.sgd_decay_ref, p, g, dec), want) <= 1e-12


@pytest.mark.parametrize("name", list(D.MUTANTS))
def test_mutants_are_rejected(name):
    p, g, dec = _draw()
    want = _torch_steps(p, [x * S for x in g], dec, torch.float64)
    assert _worst_rel(_formula_steps(D.MUTANTS[name], p, g, dec), want) > 1e-6


def test_float32_emulation_within_the_bound_of_float64_and_torch():
    """One step from a filled momentum buffer and one first step: the emulation and torch's float32 optimizer (whose decay and
    momentum are fused multiply-adds or not, as it likes) both stay inside the bound around the float64 formula."""
    for first in (False, True):
        c = D.general_case(4100, first)
        assert R.err_ratio(R.from_bits32(c["emu_p"]), c["p"], c["tol_p"]) <= 1.0
        assert R.err_ratio(R.from_bits32(c["emu_b"]), c["b"], c["tol_b"]) <= 1.0
    # torch float32, first step (its buffer cannot be preset without reaching into its state): s = 1 here, g as drawn
    p, g, _ = R.general_draw(4100)
    dec = D.elements(D.alternating_table(4100), 4100)
    lr, m, _ = D.HP_GENERAL
    td = torch.from_numpy
    a, c2 = torch.nn.Parameter(td(p[dec].copy())), torch.nn.Parameter(td(p[~dec].copy()))
    opt = torch.optim.SGD([{"params": [a], "weight_decay": D.W_GENERAL}, {"params": [c2]}], lr=lr, momentum=m, nesterov=True)
    a.grad, c2.grad = td(g[dec].copy()), td(g[~dec].copy())
    opt.step()
    got = np.empty(4100, dtype=np.float32)
    got[dec], got[~dec] = a.detach().numpy(), c2.detach().numpy()
    p2, _, mid = D.sgd_decay_ref(p.astype(np.float64), g.astype(np.float64), None, True, lr, m, 1.0, D.W_GENERAL, dec)
    tp, _ = D.decay_tol(mid, True, lr, m, dec)
    assert R.err_ratio(got, p2, tp) <= 1.0
    # the bound tells the mutants apart at this size too: a decoupled decay lies far outside it
    q, _, _ = D.mutant_decoupled(p.astype(np.float64), g.astype(np.float64), None, True, lr, m, 1.0, D.W_GENERAL, dec)
    assert R.err_ratio(q.astype(np.float32), p2, tp) > 10.0


@pytest.mark.parametrize("first", [True, False])
def test_dyadic_draws_are_exact(first):
    """Every intermediate of the three steps is an fp32 number, so the kernel's result does not depend on how it rounds."""
    c = D.dyadic_case(D.CAP_N if first else 194 + 68, first)
    for k, mid in enumerate(c["mids"]):
        for name, v in mid.items():
            assert v is None or R.exact32(v), (k, name)
    dec = D.elements(c["table"], c["p0"].size)
    assert not R.same_bits(c["want"][0][0][dec], c["p0"][dec])
    # ... and the float32 emulation gives the same bits
    lr, m, s = D.HP_DYADIC
    p, b = R.from_bits32(c["p0"]), R.from_bits32(c["b0"])
    for k in range(D.STEPS):
        p, b = D.sgd_decay_f32(p, R.from_bits32(c["g"][k]), b, first and k == 0, lr, m, s, D.W_DYADIC, dec)
        assert R.same_bits(R.bits32(p), c["want"][k][0]) and R.same_bits(R.bits32(b), c["want"][k][1])


def test_table_from_a_layout():
    L = R.update_layout("small")
    tab = D.table_from_layout(L)
    assert tab.size == L.numel // 64
    e = D.elements(tab, L.numel)
    for s in L.segs:
        assert e[s["off"]:R.r64(s["off"] + s["numel"])].all()
    for off, k in L.vecs:
        assert not e[off:R.r64(off + k)].any()
    assert not D.elements(D.table_from_layout(L, {0}), L.numel)[L.segs[1]["off"]:].any()


# ---------------------------------------------------------------------------------------------------------------------------
def _stock_rule(model):
    """Stock YOLOX's grouping as sets of parameter names, from its description: a module's bias goes to pg2; its weight to pg0 if the
    module is a BatchNorm2d or has "bn" in its name, else to pg1."""
    names = {id(p): n for n, p in model.named_parameters()}
    pg = [set(), set(), set()]
    for k, v in model.named_modules():
        if isinstance(getattr(v, "bias", None), torch.nn.Parameter):
            pg[2].add(names[id(v.bias)])
        if isinstance(getattr(v, "weight", None), torch.nn.Parameter):
            pg[0 if isinstance(v, torch.nn.BatchNorm2d) or "bn" in k else 1].add(names[id(v.weight)])
    return pg


@pytest.mark.parametrize("backbone", ["darknet", "resnet"])
def test_param_groups_follow_the_stock_rule(backbone):
    from ep24 import nn as enn
    from ep24.train import yolox_param_groups
    width = 0.125 if backbone == "darknet" else 1.0
    model = enn.YOLOX(enn.YOLOPAFPN(0.33, width, backbone_type=backbone), enn.YOLOXHead(80, width))
    groups = yolox_param_groups(model, 5e-4)
    assert [g["weight_decay"] for g in groups] == [0.0, 5e-4, 0.0]
    names = {id(p): n for n, p in model.named_parameters()}
    got = [[names[id(p)] for p in g["params"]] for g in groups]
    assert [set(x) for x in got] == _stock_rule(model)
    flat = [n for x in got for n in x]
    assert len(flat) == len(set(flat)) and set(flat) == set(names.values())          # nobody missing, nobody twice
    assert all(n.endswith("bias") for n in got[2]) and all(n.endswith("weight") for n in got[0] + got[1])
    bn = {id(m.weight) for m in model.modules() if isinstance(m, torch.nn.BatchNorm2d)}
    assert {id(p) for p in groups[0]["params"]} == bn and all(p.dim() >= 2 for p in groups[1]["params"])


def test_weight_decay_flag():
    y24 = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "exploration-of-potential_amd", "yolox_24p")
    sys.path.insert(0, y24)
    try:
        import importlib
        T = importlib.import_module("train_24p")
        from exp import get_exp
        exp = get_exp(os.path.join(y24, "load_train", "yolox_24p_train.py"))
        assert exp.weight_decay == 5e-4
        parse = T.make_parser().parse_args
        assert T.weight_decay_arg(parse([]), exp) is None
        assert T.weight_decay_arg(parse(["--weight-decay"]), exp) == 5e-4
        assert T.weight_decay_arg(parse(["--weight-decay", "--ema"]), exp) == 5e-4
        assert T.weight_decay_arg(parse(["--weight-decay", "1e-4"]), exp) == 1e-4
        exp.weight_decay = 1e-3
        assert T.weight_decay_arg(parse(["--weight-decay"]), exp) == 1e-3
        with pytest.raises(SystemExit):
            T.weight_decay_arg(parse(["--weight-decay", "-1"]), exp)
    finally:
        sys.path.remove(y24)


def _tiny():
    from ep24 import nn as enn
    return enn.YOLOX(enn.YOLOPAFPN(0.33, 0.125), enn.YOLOXHead(80, 0.125))


def test_sgd_refuses_two_decays_and_a_foreign_group_layout():
    from ep24.train import SGD, yolox_param_groups
    model = _tiny()
    groups = yolox_param_groups(model, 5e-4)
    groups[2]["weight_decay"] = 1e-4
    with pytest.raises(NotImplementedError, match="ONE weight decay"):
        SGD(groups, lr=0.01, model=model)
    with pytest.raises(ValueError):
        SGD(model.parameters(), lr=0.01, model=model, weight_decay=-1.0)
    three = SGD(yolox_param_groups(model, 5e-4), lr=0.01, model=model)
    assert [g["weight_decay"] for g in three.param_groups] == [0.0, 5e-4, 0.0] and three.weight_decay == 5e-4
    one = SGD(model.parameters(), lr=0.01, model=model)
    assert len(one.param_groups) == 1 and one.weight_decay == 0.0
    three.param_groups[1]["lr"] = 0.02                               # one launch, one lr: refused before anything runs
    with pytest.raises(ValueError, match="one lr and one momentum"):
        three.step()
    three.param_groups[1]["lr"] = 0.01
    n = [len(g["params"]) for g in three.param_groups]
    # a one-group checkpoint into the three groups (and back): refused before any momentum is written, both layouts named
    sd_one = {"state": {}, "param_groups": [{"lr": 0.01, "momentum": 0.9, "weight_decay": 0.0, "params": list(range(sum(n)))}]}
    with pytest.raises(ValueError, match=r"\[%d\].*\[%d, %d, %d\]" % (sum(n), n[0], n[1], n[2])):
        three.load_state_dict(sd_one)
    sd_three, at = {"state": {}, "param_groups": []}, 0
    for k, w in zip(n, (0.0, 5e-4, 0.0)):
        sd_three["param_groups"].append({"lr": 0.01, "momentum": 0.9, "weight_decay": w, "params": list(range(at, at + k))})
        at += k
    with pytest.raises(ValueError, match=r"\[%d, %d, %d\].*\[%d\]" % (n[0], n[1], n[2], sum(n))):
        one.load_state_dict(sd_three)
