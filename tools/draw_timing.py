"""Launch the drawing kernels (csrc/draw.hip) on a fixed workload, for a kernel trace.

    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -o kt -- python tools/draw_timing.py

in a run of its own (no counters, no other tracing beside it).  The kernel times come from the trace's statistics; the JSON line
this prints carries the workload and the GPU-event time of the same calls for orientation.

One 1280 x 960 image, 100 detections of radius 20 .. 150 px, 21 calls of ``draw_detections`` (the first one also uploads the font,
the palette and the label table), outline only and with ``fill_alpha = 96``.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "exploration-of-potential_amd"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from ep24 import draw  # noqa: E402

DEV = "cuda:0"


def detections(n, H, W, seed):
    """n rows [cx, cy, 24 radii, obj, class_conf, class]: centres over the image, radii 20 .. 150 px with 20 % ray-to-ray variation."""
    rng = np.random.default_rng(seed)
    c = np.stack([rng.uniform(0, W, n), rng.uniform(0, H, n)], 1)
    r = rng.uniform(20.0, 150.0, (n, 1)) * rng.uniform(0.8, 1.2, (n, 24))
    tail = np.stack([rng.uniform(0.3, 1.0, n), rng.uniform(0.3, 1.0, n), rng.integers(0, 80, n).astype(np.float64)], 1)
    return torch.from_numpy(np.concatenate([c, r, tail], 1).astype(np.float32)).to(DEV)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=21)
    a = ap.parse_args()
    H, W, n = 960, 1280, 100
    image = torch.from_numpy(np.random.default_rng(0).integers(0, 256, (H, W, 3), dtype=np.uint8)).to(DEV)
    dets = detections(n, H, W, 1)
    out = {"image": [H, W], "detections": n, "calls": a.calls}
    for name, alpha in (("outline", 0), ("fill96", 96)):
        dst = torch.empty_like(image)
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        draw.draw_detections(image, dets, fill_alpha=alpha, show_scores=True, out=dst)        # call 1: uploads, scratch
        torch.cuda.synchronize()
        t0.record()
        for _ in range(a.calls - 1):
            draw.draw_detections(image, dets, fill_alpha=alpha, show_scores=True, out=dst)
        t1.record()
        torch.cuda.synchronize()
        out[name + "_ms_per_call"] = round(t0.elapsed_time(t1) / max(a.calls - 1, 1), 4)       # copy + prepare + paint
        out[name + "_pixels_changed"] = int((dst != image).any(dim=2).sum())
    print(json.dumps(out))


if __name__ == "__main__":
    main()
