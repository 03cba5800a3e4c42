"""GPU box helper: the five BatchNorm + activation entry points (ep24_bn_act_fwd, _bwd_reduce, _bwd_apply, _bwd_apply_acc, _bwd_fused) on
seeded inputs, one SHA-256 per output buffer.  Run once per library (EP24_LIB=...) on one box: two builds compute the same bits exactly
when their listings are identical (`diff`).  Shapes: the nine (M, C) the flagship step runs these kernels at, and the shapes of
tests/test_gpu_bn_pipeline.py (three and four batches per thread, partial last batches, the forward's moving-group path), those also
in a slice layout (every operand with a stride and a channel offset of its own) and with every activation."""
import hashlib
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "exploration-of-potential_amd"))
import torch  # noqa: E402
from ep24._lib import call, lib, ptr, stream_ptr  # noqa: E402

DEV = "cuda:0"
BF = torch.bfloat16
FLAGSHIP = [(32000, 256), (128000, 128), (8000, 512), (512000, 64), (128000, 256), (32000, 512), (512000, 128), (2048000, 64), (8000, 1024)]
EDGES = [(4200000, 8), (1400000, 24), (8200, 2048), (270000, 64), (5003, 2048), (1600003, 8)]
REPS = 8
# (ld - C, channel offset) per operand
DENSE = dict(z=(0, 0), y=(0, 0), res=(0, 0), dy=(0, 0), dz=(0, 0))
SLICE = dict(z=(24, 8), y=(40, 16), res=(56, 24), dy=(40, 24), dz=(56, 16))


def digest(t):
    t = t.contiguous()
    raw = t.view(torch.int16) if t.dtype == BF else t
    return hashlib.sha256(raw.cpu().numpy().tobytes()).hexdigest()[:20]


class Op:
    """An [M, ld] buffer and the [M, C] window the kernels see; the whole buffer is hashed (a write outside the window shows too)."""

    def __init__(self, M, C, lay, fill):
        self.ld, self.off = C + lay[0], lay[1]
        self.t = torch.full((M, self.ld), -7.0, dtype=BF, device=DEV)
        if fill is not None:
            self.t[:, self.off:self.off + C] = fill

    def p(self):
        return self.t.data_ptr() + self.off * 2


def run(M, C, act, lay, name):
    g = torch.Generator(device=DEV).manual_seed(M * 131 + C + act)
    gc = torch.Generator().manual_seed(M * 137 + C)
    mean, std = torch.randn(C, generator=gc).double(), (0.25 + 1.75 * torch.rand(C, generator=gc)).double()
    gamma, beta = (torch.rand(C, generator=gc) + 0.5).to(DEV), (torch.rand(C, generator=gc) - 0.5).to(DEV)
    rnd = lambda: torch.randn(M, C, generator=g, device=DEV)
    z = Op(M, C, lay["z"], (rnd() * std.float().to(DEV) + mean.float().to(DEV)).to(BF))
    res, dy, old = Op(M, C, lay["res"], rnd().to(BF)), Op(M, C, lay["dy"], rnd().to(BF)), rnd().to(BF)
    # the statistics: the channel's moments as 2^-20 fixed point, split over the replicas with cancelling parts
    total = torch.stack([(M * mean * 2 ** 20).round().long(), (M * (std * std + mean * mean) * 2 ** 20).round().long()])
    parts = torch.randint(-(1 << 40), 1 << 40, (REPS, 2, C), generator=gc, dtype=torch.int64)
    parts[REPS - 1] = total - parts[:REPS - 1].sum(0)
    stats = parts.to(DEV)
    out = []
    save = torch.zeros(2, C, device=DEV)
    for with_res in (False, True):
        y = Op(M, C, lay["y"], None)
        rm, rv, nb = torch.zeros(C, device=DEV), torch.ones(C, device=DEV), torch.zeros(2, dtype=torch.int64, device=DEV)
        call("bn_act_fwd", z.p(), z.ld, ptr(stats), REPS, ptr(gamma), ptr(beta), ptr(rm), ptr(rv), ptr(nb), nb.data_ptr() + 8, ptr(save), y.p(), y.ld,
             res.p() if with_res else None, res.ld if with_res else 0, M, C, 1e-3, 0.03, act, stream_ptr())
        out += [("fwd%s.y" % ("+res" if with_res else ""), y.t), ("fwd%s.save" % ("+res" if with_res else ""), save.clone()),
                ("fwd%s.running" % ("+res" if with_res else ""), torch.cat([rm, rv]))]
    sums = torch.zeros(REPS, 2, C, dtype=torch.int64, device=DEV)
    bwd = (dy.p(), dy.ld, z.p(), z.ld, ptr(save), ptr(gamma), ptr(beta))
    call("bn_act_bwd_reduce", *bwd, ptr(sums), sums.data_ptr() + C * 8, M, C, act, REPS, stream_ptr())
    out.append(("reduce.sums", sums))
    for entry in ("bn_act_bwd_apply", "bn_act_bwd_apply_acc"):
        dz = Op(M, C, lay["dz"], old if entry.endswith("acc") else None)
        gg = torch.ones(2, C, device=DEV)
        call(entry, *bwd, ptr(sums), sums.data_ptr() + C * 8, ptr(gg), gg.data_ptr() + C * 4, dz.p(), dz.ld, M, C, act, REPS, stream_ptr())
        out += [(entry[len("bn_act_bwd_"):] + ".dz", dz.t), (entry[len("bn_act_bwd_"):] + ".grads", gg)]
    if C <= 2048:
        fsums, gg, bar = torch.zeros_like(sums), torch.ones(2, C, device=DEV), torch.zeros(2, dtype=torch.int32, device=DEV)
        dz = Op(M, C, lay["dz"], None)
        call("bn_act_bwd_fused", *bwd, ptr(fsums), fsums.data_ptr() + C * 8, ptr(gg), gg.data_ptr() + C * 4, dz.p(), dz.ld, M, C, act, REPS, ptr(bar), stream_ptr())
        out += [("fused.sums", fsums), ("fused.dz", dz.t), ("fused.grads", gg)]
    torch.cuda.synchronize()
    for what, t in out:
        print("%-22s act %d %-5s %-18s %s" % ("%d,%d" % (M, C), act, name, what, digest(t)), flush=True)


def main():
    for M, C in FLAGSHIP:
        run(M, C, 1, DENSE, "dense")
    for M, C in EDGES:
        for act in (0, 1, 2, 3):
            run(M, C, act, DENSE, "dense")
        run(M, C, 1, SLICE, "slice")
    assert lib().fn["ep24_conv_ring_timeouts"]() == 0, "a bounded wait gave up"


main()
