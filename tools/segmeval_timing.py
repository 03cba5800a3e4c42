"""Launch the COCO "segm" evaluation kernels (csrc/segmeval.hip) on one fixed synthetic workload, for a kernel trace.

    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -o kt -- python tools/segmeval_timing.py [--reps 5]

in a run of its own (no counters, no other tracing beside it).  The kernel times come from the trace's statistics
(``segm_mask_stats_kernel``, ``segm_iou_kernel``, ``segm_match_kernel``, ``accumulate_kernel``, beside ``rle_pack_bytes_kernel``,
the cocomask decode kernels and the radix sort of ``ep24_eval_sort``).  The JSON line this prints carries the workload's sizes,
the 12 numbers and the GPU-event time of whole ``evaluate()`` calls for orientation (host planning and JSON parsing included).

The workload is ``--groups`` (1 024) images of 427 x 640, each with one (image, category) group built from the polygon of
tests/golden/coco_ann_130566.json: the GT is the polygon, plus a crowd copy shifted down in every fourth image; the results are
``--dets`` (8) copies of it shifted by 3 k pixels and scaled by 1 - 0.02 k, with scores falling in k.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "exploration-of-potential_amd"))

import torch  # noqa: E402

from ep24.segmeval import SegmEvaluator  # noqa: E402

FIXTURE = os.path.join(ROOT, "tests", "golden", "coco_ann_130566.json")


def moved(poly, dx, dy, s):
    return [(v * s + (dx if i % 2 == 0 else dy)) for i, v in enumerate(poly)]


def workload(groups, dets):
    with open(FIXTURE) as f:
        d = json.load(f)
    an, im = d["annotations"][0], d["images"][0]
    poly = an["segmentation"][0]
    gt = {"images": [], "annotations": [], "categories": [{"id": an["category_id"]}]}
    res = []
    for i in range(groups):
        gt["images"].append({"id": i + 1, "height": im["height"], "width": im["width"]})
        gt["annotations"].append({"id": len(gt["annotations"]) + 1, "image_id": i + 1, "category_id": an["category_id"],
                                  "segmentation": [poly], "area": an["area"], "iscrowd": 0})
        if i % 4 == 0:
            gt["annotations"].append({"id": len(gt["annotations"]) + 1, "image_id": i + 1, "category_id": an["category_id"],
                                      "segmentation": [moved(poly, 0.0, 90.0, 1.0)], "area": an["area"], "iscrowd": 1})
        for k in range(dets):
            res.append({"image_id": i + 1, "category_id": an["category_id"], "score": 0.95 - 0.9 * k / max(dets, 1) - 1e-4 * (i % 7),
                        "segmentation": [moved(poly, 3.0 * k, 2.0 * k + (60.0 if k % 3 == 2 else 0.0), 1.0 - 0.02 * k)]})
    return gt, res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--groups", type=int, default=1024)
    ap.add_argument("--dets", type=int, default=8)
    a = ap.parse_args()
    gt, res = workload(a.groups, a.dets)
    ev = SegmEvaluator(gt)
    ev.add_results(res)
    st = ev.evaluate()                                    # warm-up: code object load, allocations
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    t0.record()
    for _ in range(a.reps):
        st = ev.evaluate()
    t1.record()
    torch.cuda.synchronize()
    print(json.dumps({"reps": a.reps, "groups": a.groups, "gt_masks": len(gt["annotations"]), "results": len(res), "h": 427, "w": 640,
                      "pairs": int((ev.plan["G"] * ev.plan["D"]).sum()), "records": st["records"], "chunks": st["chunks"],
                      "evaluate_call_ms": round(t0.elapsed_time(t1) / a.reps, 3), "stats": [round(s, 6) for s in st["stats"]]}))


if __name__ == "__main__":
    main()
