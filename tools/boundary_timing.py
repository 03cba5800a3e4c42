"""Launch the boundary-band kernel of Boundary IoU (csrc/boundary.hip) beside ``ep24_segm_mask_stats`` and ``ep24_segm_iou`` on
the same packed masks, for a kernel trace.

    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -o kt -- python tools/boundary_timing.py [--reps 5] [--d 15]

in a run of its own (no counters, no other tracing beside it).  The kernel times come from the trace (``mask_boundary_kernel``,
``segm_mask_stats_kernel``, ``segm_iou_kernel``).  One radius per run keeps the statistics of ``mask_boundary_kernel`` apart; with
several (the default: 15 and 38, the radii of a 427 x 640 image at dilation ratios 0.02 and 0.05) every repetition launches
statistics, IoU and then the band kernel once per radius in the order given, so the trace's dispatches of ``mask_boundary_kernel``
belong to the radii in turn.  The JSON line this prints carries the workload's sizes, the bytes the band kernel has to move
(one read and one write of the packed words: 2 x H x ceil(W / 32) x 4 per mask) and, for orientation, GPU-event times of ``--burst``
back-to-back launches of each kernel with the rate those give against the 6.3 TB/s the project counts as achievable from HBM.
``--uniform`` adds the form without a table (one size and one radius for all masks: the grid has no idle workgroup).

The workload is that of tools/segmeval_timing.py: ``--groups`` (1 024) images of 427 x 640, every GT and result mask of it
decoded and packed once.
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "exploration-of-potential_amd"))

import torch  # noqa: E402

from ep24 import cocomask  # noqa: E402
from ep24._lib import call, ptr, stream_ptr  # noqa: E402
from ep24.segmeval import build_plan, load_gt  # noqa: E402
from segmeval_timing import workload  # noqa: E402

HBM_TBS = 6.3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--burst", type=int, default=20)
    ap.add_argument("--groups", type=int, default=1024)
    ap.add_argument("--dets", type=int, default=8)
    ap.add_argument("--d", type=int, nargs="+", default=[15, 38])
    ap.add_argument("--uniform", action="store_true", help="also launch the form without a table (one size, one radius)")
    a = ap.parse_args()
    gt_doc, res = workload(a.groups, a.dets)
    gt = load_gt(gt_doc)
    plan = build_plan(gt, res, 100)
    dev = torch.device("cuda:0")
    s = stream_ptr()
    # the masks: every group's GTs, then every group's results, as SegmEvaluator._chunk lays a chunk out
    G, D = plan["G"], plan["D"]
    nG, nD, J = int(G.sum()), int(D.sum()), len(G)
    n = nG + nD
    segs = [gt["seg"][k] for k in plan["gt_ann"]] + [res[r]["segmentation"] for r in plan["dt_res"]]
    hw = gt["sizes"][np.concatenate([np.repeat(plan["groups"][:, 0], G), np.repeat(plan["groups"][:, 0], D)])]
    H, W = int(hw[:, 0].max()), int(hw[:, 1].max())
    words = np.concatenate([[0], np.cumsum(hw[:, 0] * ((hw[:, 1] + 31) // 32))])
    bits = torch.empty(int(words[-1]), dtype=torch.int32, device=dev)
    tabs = {}
    for d in [0] + a.d:
        tabs[d] = torch.from_numpy(np.ascontiguousarray(np.stack([words[:-1], hw[:, 0], hw[:, 1], np.full(n, d, dtype=np.int64)], 1))).to(dev)
    for k0 in range(0, n, 1024):                              # decoded a thousand masks at a time (one byte per pixel)
        k1 = min(k0 + 1024, n)
        buf, desc = cocomask.decode_batch(segs[k0:k1], hw[k0:k1], dev)
        call("rle_pack_bytes", ptr(buf), buf.numel(), ptr(desc), ptr(tabs[0], 4 * k0), k1 - k0, H, ptr(bits), s)
        torch.cuda.synchronize()
    gfirst, dfirst = np.concatenate([[0], np.cumsum(G)]), np.concatenate([[0], np.cumsum(D)])
    ioff = np.concatenate([[0], np.cumsum(G * D)])
    pairs = int(ioff[-1])
    gh = gt["sizes"][plan["groups"][:, 0]]
    grp = torch.from_numpy(np.ascontiguousarray(np.stack([gh[:, 0], gh[:, 1], gfirst[:-1], G, nG + dfirst[:-1], D, ioff[:-1], np.zeros(J, dtype=np.int64)], 1))).to(dev)
    crowd = np.zeros(n, dtype=np.uint8)
    crowd[:nG] = gt["crowd"][plan["gt_ann"]]
    crowd = torch.from_numpy(crowd).to(dev)
    bbox = torch.empty(n, 4, dtype=torch.int32, device=dev)
    area = torch.empty(n, dtype=torch.int32, device=dev)
    iou = torch.empty(max(pairs, 1), dtype=torch.float64, device=dev)
    band = torch.empty_like(bits)

    launches = {"segm_mask_stats": lambda: call("segm_mask_stats", ptr(bits), ptr(tabs[0]), n, ptr(bbox), ptr(area), s),
                "segm_iou": lambda: call("segm_iou", ptr(bits), ptr(tabs[0]), n, ptr(bbox), ptr(area), ptr(crowd), ptr(grp), J, pairs, ptr(iou), None, s)}
    for d in a.d:
        launches["mask_boundary_d%d" % d] = lambda d=d: call("mask_boundary", ptr(bits), ptr(tabs[d]), n, H, W, 0, ptr(band), s)
    if a.uniform:                                             # all masks have one size: the form without a table (an exact grid)
        for d in a.d:
            launches["mask_boundary_uniform_d%d" % d] = lambda d=d: call("mask_boundary", ptr(bits), None, n, H, W, d, ptr(band), s)
    for _ in range(1 + a.reps):                               # the first round is the warm-up; these are the trace's dispatches
        for f in launches.values():
            f()
    torch.cuda.synchronize()
    band_bytes = 2 * 4 * int(words[-1])
    out = {"reps": a.reps, "burst": a.burst, "masks": n, "h": H, "w": W, "pairs": pairs, "packed_bytes": 4 * int(words[-1]), "band_kernel_bytes": band_bytes,
           "event_us": {}, "event_tbs": {}}
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for name, f in launches.items():
        t0.record()
        for _ in range(a.burst):
            f()
        t1.record()
        torch.cuda.synchronize()
        us = 1e3 * t0.elapsed_time(t1) / a.burst
        out["event_us"][name] = round(us, 2)
        if name.startswith("mask_boundary"):
            out["event_tbs"][name] = round(band_bytes / us / 1e6, 3)
        elif name == "segm_mask_stats":
            out["event_tbs"][name] = round(band_bytes / 2 / us / 1e6, 3)
    out["hbm_tbs"] = HBM_TBS
    print(json.dumps(out))


if __name__ == "__main__":
    main()
