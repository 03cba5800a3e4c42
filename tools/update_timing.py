"""The fused weight update on YOLOX-l's flat layout (54.2 M parameters + alignment padding, the real wf_delta and decay_grp tables of
ep24.engine.ParamHome): ep24_sgd_nesterov_hp_range_pack as it was, against ep24_sgd_nesterov_decay_hp_range_pack (weight decay by
parameter group), each with and without the EMA buffer, for a kernel trace.

    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -o kt -- python tools/update_timing.py --manifest OUT/manifest.json
    python tools/update_timing.py --summarize OUT/<host>/kt_kernel_trace.csv OUT/manifest.json

in a run of its own (no counters, no other tracing beside it).  The four variants alternate launch by launch, so drift of the box
hits them alike; the manifest lists which variant every timed launch was, and --summarize matches it against the trace's update
kernels in dispatch order: median / min / max per variant, the spread of the unchanged kernel over its repeats, and bytes over time
(p, g, buf read and p, buf written, + the EMA read and written, + 2 bytes per packed weight, + the tables).  Without a trace the JSON
line of the first form still carries GPU-event times of the same launches for orientation.
"""
import argparse
import csv
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "exploration-of-potential_amd"))

VARIANTS = ["plain", "decay", "plain+ema", "decay+ema"]
WARMUP = 3                                                # launches of every variant before the timed ones


def bytes_moved(numel, mapped, variant):
    n = 5 * 4 * numel + 2 * mapped + 4 * (numel // 64)    # p, g, buf in; p, buf out; the packed copy; wf_delta
    if "ema" in variant:
        n += 2 * 4 * numel
    if "decay" in variant:
        n += numel // 64
    return n


def run(args):
    import torch
    from ep24 import nn as enn
    from ep24._lib import call, ptr, stream_ptr
    from ep24.engine import param_home
    dev = "cuda:0"
    torch.manual_seed(0)
    model = enn.YOLOX(enn.YOLOPAFPN(1.0, 1.0), enn.YOLOXHead(80, 1.0)).to(dev)
    home = param_home(model)
    n = home.numel
    home.gflat.normal_(0.0, 0.01)
    ema = home.flat.clone()
    hp = torch.zeros(8, dtype=torch.float32, device=dev)
    # lr 0: the parameters stay what they are however many launches run, the kernels do all their work
    call("set_hparams_decay", ptr(hp), 0.0, 0.9, 1.0, 0.9998, 1.0 - 0.9998, 5e-4, stream_ptr())
    home.first_flag.zero_()

    def launch(variant):
        e = ptr(ema) if "ema" in variant else None
        if "decay" in variant:
            call("sgd_nesterov_decay_hp_range_pack", ptr(home.flat), ptr(home.gflat), ptr(home.mflat), 0, n, ptr(hp), ptr(home.first_flag),
                 e, 1, ptr(home.wf_delta), ptr(home.wf), ptr(home.decay_grp), stream_ptr())
        else:
            call("sgd_nesterov_hp_range_pack", ptr(home.flat), ptr(home.gflat), ptr(home.mflat), 0, n, ptr(hp), ptr(home.first_flag),
                 e, 1, ptr(home.wf_delta), ptr(home.wf), stream_ptr())

    order = [v for _ in range(WARMUP) for v in VARIANTS]
    for v in order:
        launch(v)
    torch.cuda.synchronize()
    timed, events = [], []
    for _ in range(args.reps):
        for v in VARIANTS:
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            launch(v)
            t1.record()
            timed.append(v)
            events.append((t0, t1))
    torch.cuda.synchronize()
    ms = {v: [a.elapsed_time(b) for w, (a, b) in zip(timed, events) if w == v] for v in VARIANTS}
    mapped = sum(s.numel for s in home.convs if s not in home.pack_rest)
    out = {"numel": n, "parameters": sum(p.numel() for p in model.parameters()), "mapped": mapped,
           "decaying_groups": int(home.decay_grp.sum()), "groups": int(home.decay_grp.numel()), "reps": args.reps,
           "event_ms_median": {v: round(statistics.median(x), 4) for v, x in ms.items()},
           "bytes": {v: bytes_moved(n, mapped, v) for v in VARIANTS}}
    if args.manifest:
        with open(args.manifest, "w") as fh:
            json.dump(dict(out, warmup=order, timed=timed), fh)
    print(json.dumps(out))


def summarize(trace, manifest):
    man = json.load(open(manifest))
    rows = [r for r in csv.DictReader(open(trace)) if "sgd_kernel" in r["Kernel_Name"]]
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    labels = man["warmup"] + man["timed"]
    assert len(rows) == len(labels), "the trace holds %d update kernels, the manifest %d launches" % (len(rows), len(labels))
    for r, v in zip(rows, labels):                            # the decayed form is the template's other instantiation
        assert ("true" in r["Kernel_Name"] or "ILb1" in r["Kernel_Name"]) == ("decay" in v), (r["Kernel_Name"], v)
    us = {v: [] for v in VARIANTS}
    for r, v in list(zip(rows, labels))[len(man["warmup"]):]:
        us[v].append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3)
    out = {}
    for v, x in us.items():
        med = statistics.median(x)
        out[v] = {"median_us": round(med, 2), "min_us": round(min(x), 2), "max_us": round(max(x), 2), "n": len(x),
                  "TB_per_s": round(man["bytes"][v] / med / 1e6, 3)}
    for a, b in (("plain", "decay"), ("plain+ema", "decay+ema")):
        out["%s - %s" % (b, a)] = {"median_us": round(out[b]["median_us"] - out[a]["median_us"], 2),
                                   "spread_of_%s_us" % a: round(out[a]["max_us"] - out[a]["min_us"], 2)}
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--manifest", default=None, help="write the launch order here (read back by --summarize)")
    ap.add_argument("--summarize", nargs=2, metavar=("TRACE_CSV", "MANIFEST"), default=None)
    a = ap.parse_args()
    if a.summarize:
        summarize(*a.summarize)
    else:
        run(a)


if __name__ == "__main__":
    main()
