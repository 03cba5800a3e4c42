"""GPU box helper: the launch plan of an engine in a canonical text form, one entry of fwd / bwd / fwd_eval per line, so that two
checkouts can be compared with cmp.  Pointers are written relative to the engine's and the home's named buffers (anything else is
P), the rows of the plan's own descriptor tables are written out, and the cut indices and scratch sizes follow.
usage: plan_dump.py OUT_DIR [config ...]     (no config: all of CONFIGS; one file OUT_DIR/<config>.txt each)"""
import os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "exploration-of-potential_amd")):
    sys.path.insert(0, p)
import torch
from ep24 import loss as eloss, nn as enn, train as etrain
from ep24.engine import Dyn, SubEngine
from ep24.options import PlanOptions, set_options
DEV = torch.device("cuda", 0)
B, S = 4, 256
ENG_BUFS = ("slab", "dzbuf", "stats", "bnsums", "outputs", "images", "fold_w", "fold_b")
HOME_BUFS = ("flat", "gflat", "mflat", "wf", "wd", "bflat")
PLANS = {"nogroup": "group_wgrad=0", "nostream": "fuse_bn_stream=0,fuse_bn_dgrad=0,fuse_bn_reduce_stream=0", "bnreduce": "fuse_bn_reduce=1",
         "bnbwd": "fuse_bn_bwd=1", "nomerge": "merge_csp=0,merge_head=0", "noparhead": "parallel_head=0", "nolossdecode": "fuse_loss_decode=0"}
NETS = {"tiny": (0.33, 0.125, {}), "w25": (0.67, 0.25, {}), "w50": (0.67, 0.5, {}), "dw": (0.33, 0.125, dict(depthwise=True)),
        "resnet": (0.33, 1.0, dict(backbone_type="resnet")), "densenet": (0.33, 1.0, dict(backbone_type="densenet")),
        "vgg": (0.33, 1.0, dict(backbone_type="vgg"))}      # the swapped backbones emit 256 / 512 / 1024 channels: width 1.0
SUBS = {"csp": (lambda: enn.CSPLayer(16, 16, n=2), [(16, 32, 32)]), "spp": (lambda: enn.SPPBottleneck(16, 16), [(16, 32, 32)]),
        "bottleneck": (lambda: enn.Bottleneck(16, 16, True, 1.0), [(16, 32, 32)]),
        "head": (lambda: enn.YOLOXHead(80, 0.125), [(32, 32, 32), (64, 16, 16), (128, 8, 8)]),
        "resblock": (lambda: enn.ResBottleneck(64, 16), [(64, 16, 16)]), "denseblock": (lambda: enn.DenseBlock(3, 64, drop_rate=0.3), [(64, 16, 16)])}
CONFIGS = list(NETS) + ["f32"] + list(PLANS) + ["sub_" + k for k in SUBS]


def build(cfg):
    """-> (engine, TrainStep or None)"""
    torch.manual_seed(0)
    if cfg.startswith("sub_"):
        make, shapes = SUBS[cfg[4:]]
        return SubEngine(make().to(DEV), cfg[4:], shapes, B), None
    depth, width, kw = NETS.get(cfg, NETS["tiny"])
    m = enn.YOLOX(enn.YOLOPAFPN(depth, width, **kw), enn.YOLOXHead(80, width, depthwise=kw.get("depthwise", False))).to(DEV)
    if cfg == "f32":
        return m.engine(B, S, torch.float32), None
    set_options(m, PlanOptions.parse(PLANS.get(cfg, "")))
    ts = etrain.TrainStep(m, eloss.Loss_Function(80), lr=0.0, momentum=0.9, batch=B, size=S)
    return ts.eng, ts


def dump(eng, ts, out):
    home = eng.home
    bufs = [(n, getattr(o, n)) for o, names in ((eng, ENG_BUFS), (home, HOME_BUFS)) for n in names if getattr(o, n, None) is not None]
    ranges = [(n, t.data_ptr(), t.numel() * t.element_size()) for n, t in bufs]
    tables = {t.data_ptr(): t for t in eng._keep if t.dtype == torch.int64}      # descriptor tables of the grouped launches and reduces

    def canon(a, depth=0):
        if isinstance(a, Dyn):
            return "D:%s" % a.key
        if not isinstance(a, int) or isinstance(a, bool) or abs(a) < 1 << 32:
            return repr(a)
        for n, p0, nb in ranges:
            if p0 <= a < p0 + nb:
                return "%s+%d" % (n, a - p0)
        if a in tables and depth == 0:
            return "T[%s]" % ";".join(",".join(canon(v, 1) for v in row) for row in tables[a].cpu().tolist())
        return "P"

    for lname in ("fwd", "bwd", "fwd_eval"):
        for i, (name, args) in enumerate(getattr(eng, lname)):
            out.write("%s %d %s %s\n" % (lname, i, name, " ".join(canon(a) for a in args)))
    out.write("bwd_writes %r\n" % (eng.bwd_writes,))
    for n in ("fwd_fork", "fwd_fork1", "fwd_head0", "fwd_head1", "bwd_tail_cut", "bwd_join", "bwd_par_end"):
        out.write("%s %r\n" % (n, getattr(eng, n, None)))
    out.write("sizes %r home.numel %d\n" % ([(n, getattr(eng, n).numel()) for n in ("slab", "dzbuf", "stats", "bnsums")], home.numel))
    if ts is not None:
        segs, ready = ts._segments()
        early = ts._early_update_cut(segs)
        chunks = ts._update_chunks(segs, early[1]) if early is not None and ts.chunked_update else ({}, None)
        out.write("segments %r %r\nearly %r update_chunks %r\n" % (segs, ready, early, chunks))


if __name__ == "__main__":
    os.makedirs(sys.argv[1], exist_ok=True)
    for cfg in sys.argv[2:] or CONFIGS:
        eng, ts = build(cfg)
        with open(os.path.join(sys.argv[1], cfg + ".txt"), "w") as f:
            dump(eng, ts, f)
        print(cfg, len(eng.fwd), len(eng.bwd), len(eng.fwd_eval), flush=True)
        del eng, ts
