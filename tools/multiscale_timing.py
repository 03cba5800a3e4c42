"""Launch the multiscale resize kernel (csrc/preproc.hip, ep24_resize_bilinear_f32) at full size, for a kernel trace.

    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -o kt -- python tools/multiscale_timing.py [--reps 20]

in a run of its own (no counters, no other tracing beside it).  The kernel times come from the trace's statistics; the JSON line
this prints carries the bytes moved and GPU-event times of the same launches for orientation.

A batch of 20 fp32 canvases at 640 x 640 goes to 480 x 480, 800 x 800 and 640 x 640 (``--batch`` / ``--base`` / ``--sizes`` change
that).  Beside every launch of the kernel, ATen's ``F.interpolate(mode="bilinear", align_corners=False)`` runs on the same tensors:
the kernel ``Exp.preprocess`` would otherwise launch, and the reference of this measurement (same memory traffic).  The label kernel
(ep24_scale_labels, 51 000 floats) is launched too.  Rates are bytes read + bytes written over time, to be read against the
6.3 TB/s a float4 copy reaches on an MI355X.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "exploration-of-potential_amd"))

import torch  # noqa: E402

from ep24 import multiscale, synth  # noqa: E402

DEV = "cuda:0"


def timed(fn, reps):
    fn()                                                  # warm-up: code object load, allocations
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    t0.record()
    for _ in range(reps):
        fn()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--batch", type=int, default=20)
    ap.add_argument("--base", type=int, default=640)
    ap.add_argument("--sizes", type=int, nargs="+", default=[480, 800, 640])
    a = ap.parse_args()
    out = {"reps": a.reps, "batch": a.batch, "base": a.base, "shapes": []}
    images = torch.rand(a.batch, 3, a.base, a.base, device=DEV) * 255.0
    labels = synth.make_labels(a.batch, 10, size=a.base, seed=2).to(DEV)
    for s in a.sizes:
        dst = torch.empty(a.batch, 3, s, s, device=DEV)
        dst_l = torch.empty_like(labels)
        moved = images.numel() * 4 + dst.numel() * 4
        ms_ep24 = timed(lambda: multiscale.resize_batch(images, labels, (s, s), out_images=dst, out_labels=dst_l), a.reps)
        ms_aten = timed(lambda: torch.nn.functional.interpolate(images, size=(s, s), mode="bilinear", align_corners=False), a.reps)
        ref = torch.nn.functional.interpolate(images, size=(s, s), mode="bilinear", align_corners=False)
        out["shapes"].append({"to": s, "bytes_moved": moved, "ep24_pair_ms": round(ms_ep24, 4), "aten_ms": round(ms_aten, 4),
                              "ep24_pair_TBps": round(moved / ms_ep24 * 1e-9, 3), "aten_TBps": round(moved / ms_aten * 1e-9, 3),
                              "max_abs_diff_to_aten": float((dst - ref).abs().max())})
    print(json.dumps(out))


if __name__ == "__main__":
    main()
