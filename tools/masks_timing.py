"""Launch the polygon kernels (csrc/mask.hip, the poly24 IoU type of csrc/evaluate.hip) on fixed workloads, for a kernel trace.

    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -o kt -- python tools/masks_timing.py [--reps 20]

in a run of its own (no counters, no other tracing beside it).  The kernel times come from the trace's statistics; the JSON line
this prints carries the workload sizes and GPU-event times of the same launches for orientation.

* ``poly24_raster``: 100 detections per image x 20 images rasterised at 640 x 640 (2 000 masks of 51 KB each per repetition).
* ``mask_iou``: 50 x 100 masks per image at 640 x 640.
* ``eval_match`` with ``"poly24"`` beside ``"circle24"`` on the same 64-image scene (50 GTs and ~120 detections per image).
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "exploration-of-potential_amd"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from ep24 import evaluate as E, masks as M, synth  # noqa: E402

DEV = "cuda:0"


def timed(fn, reps):
    fn()                                                  # warm-up: allocations, constants
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    t0.record()
    for _ in range(reps):
        fn()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) / reps


def detections(n, size, seed):
    """n rows [cx, cy, 24 radii]: centres over the image, radii 10 .. 60 px with 20 % ray-to-ray variation."""
    rng = np.random.default_rng(seed)
    c = rng.uniform(0.1 * size, 0.9 * size, (n, 2))
    r = rng.uniform(10.0, 60.0, (n, 1)) * rng.uniform(0.8, 1.2, (n, 24))
    return torch.from_numpy(np.concatenate([c, r], 1).astype(np.float32)).to(DEV)


def scene(n_img, seed):
    """labels [n, 50, 51] with 50 GTs each and per image detections [k, 29]: two jittered copies of the GTs plus 20 random rows."""
    rng = np.random.default_rng(seed)
    labels = synth.make_labels(n_img, 50, size=640, seed=seed, num_classes=80)
    dets = []
    for i in range(n_img):
        g = labels[i, :, 1:].numpy()
        vx, vy = g[:, 2::2] - g[:, 0:1], g[:, 3::2] - g[:, 1:2]
        base = np.concatenate([g[:, :2], np.sqrt(vx * vx + vy * vy)], 1).astype(np.float32)
        rows = []
        for rep in range(2):
            j = base.copy()
            j[:, :2] += rng.normal(0.0, 2.0 + 4.0 * rep, (50, 2)).astype(np.float32)
            j[:, 2:] *= (1.0 + rng.normal(0.0, 0.08, (50, 24))).astype(np.float32)
            rows.append(np.concatenate([j, np.ones((50, 2), np.float32), labels[i, :, 0:1].numpy()], 1))
        fp = np.concatenate([detections(20, 640, seed * 100 + i).cpu().numpy(), np.ones((20, 2), np.float32),
                             rng.integers(0, 80, (20, 1)).astype(np.float32)], 1)
        rows.append(fp)
        r = np.concatenate(rows, 0)
        r[:, 26] = rng.uniform(0.1, 1.0, len(r)).astype(np.float32)
        dets.append(torch.from_numpy(r).to(DEV))
    return labels.to(DEV), dets


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    a = ap.parse_args()
    out = {"reps": a.reps}

    S, images, per_image = 640, 20, 100
    polys = M.detection_polygons(detections(images * per_image, S, 1))
    pm = M.rasterize(polys, (S, S))
    out["raster_masks"] = len(pm)
    out["raster_bytes_written"] = int(pm.bits.numel() * 4)
    out["raster_mean_area_px"] = float(pm.area.float().mean())
    out["raster_ms"] = round(timed(lambda: M.rasterize(polys, (S, S), out=pm), a.reps), 4)

    ga = M.rasterize(M.detection_polygons(detections(50, S, 2)), (S, S))
    db = M.rasterize(M.detection_polygons(detections(100, S, 3)), (S, S))
    inter, _ = M.mask_iou(ga, db)
    out["mask_iou_pairs"] = int(inter.numel())
    out["mask_iou_overlapping_pairs"] = int((inter > 0).sum())
    out["mask_iou_ms"] = round(timed(lambda: M.mask_iou(ga, db), a.reps), 4)

    labels, dets = scene(64, 5)
    for iou_type in ("circle24", "poly24"):
        ev = E.Evaluator24(80, iou_type=iou_type)

        def run():
            ev.reset()
            ev.update_detections(dets, labels)            # one eval_match launch over the 64 images (+ the count read)
        out["update_detections_ms_" + iou_type] = round(timed(run, max(a.reps // 4, 1)), 4)
        out["AP_" + iou_type] = round(ev.summarize()["AP"], 4)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
