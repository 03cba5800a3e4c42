"""Launch the mask -> COCO RLE kernels (csrc/rle.hip) on one fixed batch, for a kernel trace.

    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -o kt -- python tools/rle_timing.py [--reps 10]

in a run of its own (no counters, no other tracing beside it).  The kernel times come from the trace's statistics
(``rle_count_kernel``, ``rle_colscan_kernel``, ``rle_offsets_kernel``, ``rle_emit_kernel``, ``rle_counts_kernel``, and
``rle_pack_bytes_kernel`` for the byte buffer; ``mask_unpack_kernel`` over the same masks stands beside them: a byte per pixel is
the first step of the only other way out).  The JSON line this prints carries the batch's sizes and GPU-event times of the same
calls for orientation.

The batch is ``--copies`` (1 024) times the polygon of tests/golden/coco_ann_130566.json (427 x 640, 32 513 pixels, 1 131 runs),
decoded by ``ep24.cocomask.decode_batch``, packed by ``ep24.masks.pack`` and encoded by ``ep24.cocomask.encode``; the same
buffer also goes through ``encode_buffer``.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "exploration-of-potential_amd"))

import torch  # noqa: E402

from ep24 import cocomask, masks  # noqa: E402

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
    a = ap.parse_args()
    with open(FIXTURE) as f:
        d = json.load(f)
    an, h, w = d["annotations"][0], d["images"][0]["height"], d["images"][0]["width"]
    n = a.copies
    buf, desc = cocomask.decode_batch([an["segmentation"]] * n, [(h, w)] * n)
    pm = masks.pack(buf[: n * h * w].view(n, h, w))
    rl = cocomask.encode(pm)
    off = rl.offsets.cpu()
    out = {"reps": a.reps, "masks": n, "h": h, "w": w, "packed_bytes": int(pm.bits.numel() * 4), "mask_bytes": n * h * w,
           "runs_per_mask": int(off[1]), "runs": int(off[-1]), "pixels_per_mask": int(pm.area[0]),
           "copies_equal": bool((rl.counts.view(n, -1) == rl.counts[: int(off[1])]).all())}
    rb = cocomask.encode_buffer(buf, desc)
    out["buffer_equal"] = bool(torch.equal(rb.counts, rl.counts) and torch.equal(rb.offsets, rl.offsets))
    hold = (torch.empty_like(rl.offsets), torch.empty_like(rl.counts))
    for name, fn in (("encode", lambda: cocomask.encode(pm, out=hold)), ("encode_buffer", lambda: cocomask.encode_buffer(buf, desc, out=hold)),
                     ("pack", lambda: masks.pack(buf[: n * h * w].view(n, h, w))), ("unpack", lambda: masks.unpack(pm))):
        ms = timed(fn, a.reps)
        out.update({name + "_call_ms": round(ms, 4), name + "_call_us_per_mask": round(ms * 1e3 / n, 3)})
    t = time.perf_counter()
    coco = rl.to_coco()
    out["to_coco_host_ms"] = round((time.perf_counter() - t) * 1e3, 3)
    out["string_chars_per_mask"] = len(coco[0]["counts"])
    print(json.dumps(out))


if __name__ == "__main__":
    main()
