"""Launch the COCO mask decode kernels (csrc/cocomask.hip) and ep24_ray24 on one fixed batch, for a kernel trace.

    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -o kt -- python tools/cocomask_timing.py [--reps 10]

in a run of its own (no counters, no other tracing beside it).  The kernel times come from the trace's statistics
(``poly_xor_kernel``, ``poly_scan_kernel``, ``rle_kernel``, ``ray24_kernel``, and the fill kernel that zeroes the buffer);
the JSON line this prints carries the batch's sizes, the host's planning time and GPU-event times of the same calls for
orientation.

The batch is ``--copies`` (1 024) times the polygon of tests/golden/coco_ann_130566.json (30 vertices, 427 x 640, 32 513
pixels), each copy a mask of its own, decoded by ``ep24.cocomask.decode_batch`` and cast by ``labels24.rays_from_buffer``
from the same device buffer.  ``--rle`` adds the same masks once more as uncompressed RLE (the runs of the decoded polygon).
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "exploration-of-potential_amd"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from ep24 import cocomask, labels24  # noqa: E402

FIXTURE = os.path.join(ROOT, "tests", "golden", "coco_ann_130566.json")


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
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--copies", type=int, default=1024)
    ap.add_argument("--rle", action="store_true")
    a = ap.parse_args()
    with open(FIXTURE) as f:
        d = json.load(f)
    an, h, w = d["annotations"][0], d["images"][0]["height"], d["images"][0]["width"]
    n = a.copies
    segs, sizes = [an["segmentation"]] * n, [(h, w)] * n
    centres = [[an["bbox"][0] + an["bbox"][2] / 2, an["bbox"][1] + an["bbox"][3] / 2]] * n
    t = time.perf_counter()
    plan = cocomask._plan(segs, sizes)
    plan_ms = (time.perf_counter() - t) * 1e3
    out = {"reps": a.reps, "annotations": n, "h": h, "w": w, "mask_bytes": plan["nbytes"], "edges": int(len(plan["edges"])),
           "dense_points": int(plan["start"][-1]), "host_plan_ms": round(plan_ms, 3)}
    buf, desc = cocomask.decode_batch(segs, sizes)
    one = buf[: h * w].view(h, w)
    out["pixels_per_mask"] = int(one.sum())
    out["copies_equal"] = bool((buf[: n * h * w].view(n, h * w) == one.reshape(1, -1)).all())
    decode_ms = timed(lambda: cocomask.decode_batch(segs, sizes, out=buf), a.reps)
    rays_ms = timed(lambda: labels24.rays_from_buffer(buf, desc, centres), a.reps)
    out.update(decode_call_ms=round(decode_ms, 4), decode_call_us_per_annotation=round(decode_ms * 1e3 / n, 3),
               ray24_call_ms=round(rays_ms, 4), ray24_call_us_per_annotation=round(rays_ms * 1e3 / n, 3))
    if a.rle:
        col = one.t().contiguous().reshape(-1).cpu().numpy()                          # column-major, as the runs are
        change = np.flatnonzero(col[1:] != col[:-1]) + 1
        counts = np.diff(np.concatenate([[0], change, [col.size]])).tolist()
        if col[0]:
            counts = [0] + counts
        rle = [{"size": [h, w], "counts": counts}] * n
        rbuf, _ = cocomask.decode_batch(rle, sizes)
        out["rle_runs"] = len(counts)
        out["rle_equal"] = bool(torch.equal(rbuf, buf))
        rle_ms = timed(lambda: cocomask.decode_batch(rle, sizes, out=rbuf), a.reps)
        out.update(rle_call_ms=round(rle_ms, 4), rle_call_us_per_annotation=round(rle_ms * 1e3 / n, 3))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
