"""Launch the four feature-map kernels (csrc/featmap.hip) on fixed workloads, for a kernel trace.

    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -o kt -- python tools/featmap_timing.py [--reps 20]

in a run of its own (no counters, no other tracing beside it).  The kernel times come from the trace's statistics; the JSON line
this prints carries the workload sizes, GPU-event times of the same launches, the mean kernel's achieved (M * C * 2 + M * 4) / t and
the time of the only route to the same maps without the kernel, ``_from_act(act).mean(1)`` (an NCHW fp32 copy, then torch).

* ``featmap_mean``: the three neck outputs of the -l model at B = 20, 640 x 640 (80 x 80 x 256, 40 x 40 x 512, 20 x 20 x 1024) and at
  B = 8, 1280 x 1280 (160 x 160 x 256, 80 x 80 x 512, 40 x 40 x 1024).  Every repetition reads another buffer of a ring that is
  larger than the 256 MiB Infinity Cache, so the rate is an HBM rate; in the study the maps follow the forward pass that wrote them.
* ``featmap_range`` / ``featmap_render`` over the network input at stride 8 / ``featmap_response`` (50 labels per image, both
  regions) on the stride-8 maps of both sizes.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "exploration-of-potential_amd"))

import torch  # noqa: E402

from ep24 import featmap as F, synth  # noqa: E402
from ep24.engine import Act, Buf, _from_act  # noqa: E402

DEV = "cuda:0"
RING_BYTES = 512 << 20                                     # twice the Infinity Cache
NECK = {640: (20, ((80, 256), (40, 512), (20, 1024))), 1280: (8, ((160, 256), (80, 512), (40, 1024)))}


def timed(fn, reps):
    fn(0)                                                  # warm-up: allocations, code objects
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    t0.record()
    for i in range(reps):
        fn(i)
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) / reps


def ring(B, S, C):
    """Acts [B, S, S, C] with random contents, enough of them to exceed RING_BYTES."""
    n = max(2, RING_BYTES // (B * S * S * C * 2) + 1)
    acts = []
    g = torch.Generator(device=DEV).manual_seed(C)
    for _ in range(n):
        a = Act(Buf(DEV, B * S * S, C), 0, C, B, S, S)
        a.buf.t.copy_(torch.randn(a.buf.t.numel(), device=DEV, generator=g).to(torch.bfloat16))
        acts.append(a)
    return acts


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    a = ap.parse_args()
    out = {"reps": a.reps, "mean": [], "range": [], "render": [], "response": []}
    for size, (B, levels) in NECK.items():
        for S, C in levels:
            acts = ring(B, S, C)
            M = B * S * S
            dst = torch.empty(B, S, S, dtype=torch.float32, device=DEV)
            ms = timed(lambda i: F.channel_mean(acts[i % len(acts)], out=dst), a.reps)
            ms_torch = timed(lambda i: _from_act(acts[i % len(acts)]).mean(1), a.reps)
            nbytes = M * C * 2 + M * 4
            out["mean"].append({"input": size, "B": B, "HW": S, "C": C, "M": M, "bytes": nbytes, "ring_buffers": len(acts),
                                "ms": round(ms, 4), "GBps": round(nbytes / ms / 1e6, 1), "from_act_mean_ms": round(ms_torch, 4)})
            del acts
        S8 = size // 8
        maps = torch.randn(B, S8, S8, device=DEV)
        base = synth.make_images(B, size, seed=1).to(DEV)
        heat = torch.empty(B, size, size, 3, dtype=torch.uint8, device=DEV)
        rng = F.value_range(maps)
        out["range"].append({"input": size, "N": B, "cells": S8 * S8, "ms": round(timed(lambda i: F.value_range(maps), a.reps), 4)})
        for with_base in (False, True):
            # explicit limits: the render launch alone (the default form adds one featmap_range launch)
            ms = timed(lambda i: F.render(maps, 8, base=base if with_base else None, vmin=-3.0, vmax=3.0, out=heat), a.reps)
            out["render"].append({"input": size, "N": B, "HW": S8, "scale": 8, "base": with_base, "bytes_out": heat.numel(),
                                  "ms": round(ms, 4)})
        labels = synth.make_labels(B, 50, size=size, seed=2).to(DEV)
        for region in ("rect", "poly24"):
            r = F.response([maps], labels, strides=(8,), region=region)
            out["response"].append({"input": size, "B": B, "L": 50, "HW": S8, "region": region,
                                    "mean_cells": round(float(r.count.float().mean()), 1),
                                    "ms": round(timed(lambda i: F.response([maps], labels, strides=(8,), region=region), a.reps), 4)})
        del rng
    print(json.dumps(out))


if __name__ == "__main__":
    main()
