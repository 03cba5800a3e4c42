"""Launch the label warp (csrc/sector.hip: ep24_sector_labels, ep24_sector_points) on fixed workloads, for a kernel trace.

    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -o kt -- python tools/fisheye_labels_timing.py [--reps 20]

in a run of its own (no counters, no other tracing beside it).  The kernel times come from the trace's statistics; the JSON line
this prints carries the workload sizes and GPU-event times of the same calls (upload of the one parameter / row table included) for
orientation.

* ``config5``: 8 images of 1280 x 1280 with 50 labels each, angles 30 .. 90, letterboxed to 1280 x 1280.
* ``config2``: 20 images of 640 x 640 with 10 labels each, angles 30 .. 90, letterboxed to 640 x 640.
* ``points``: 100 000 points of one 1280 x 1280 geometry through ``map_points``.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "exploration-of-potential_amd"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from ep24 import fisheye  # noqa: E402
from ep24.sector import Image_Distortion  # noqa: E402

DEV = "cuda:0"


def timed(fn, reps):
    fn()                                                  # warm-up: allocations, the ray table
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    t0.record()
    for _ in range(reps):
        fn()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) / reps


def rows(rng, k, size):
    """k label rows on a size x size image: 24 vertices on rays around a centre, radii 3 % .. 12 % of the side."""
    phi = np.arange(24) * 15 * np.pi / 180
    out = np.zeros((k, 51))
    for i in range(k):
        r = rng.uniform(0.03, 0.12) * size * rng.uniform(0.8, 1.2, 24)
        cx, cy = rng.uniform(0.15 * size, 0.85 * size, 2)
        out[i, 0] = rng.randint(0, 80)
        out[i, 1], out[i, 2] = cx / size, cy / size
        out[i, 3::2], out[i, 4::2] = (cx + r * np.cos(phi)) / size, (cy + r * np.sin(phi)) / size
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    a = ap.parse_args()
    out = {"reps": a.reps}
    rng = np.random.RandomState(0)
    for name, n, size, k in (("config5", 8, 1280, 50), ("config2", 20, 640, 10)):
        targets = [rows(rng, k, size) for _ in range(n)]
        sizes = [(size, size)] * n
        thetas = [int(rng.randint(30, 91)) for _ in range(n)]
        buf = torch.empty(n, 50, 51, dtype=torch.float32, device=DEV)
        _, counts, flags = fisheye.warp_labels(targets, sizes, thetas, (size, size), 50, out=buf)
        out[name + "_rows"] = n * k
        out[name + "_survivors"] = int(counts.sum())
        out[name + "_fell_back"] = int(flags.sum())
        out[name + "_ms"] = round(timed(lambda: fisheye.warp_labels(targets, sizes, thetas, (size, size), 50, out=buf), a.reps), 4)
    dist = Image_Distortion(DEV)
    pts = torch.from_numpy(rng.uniform(0.0, 1279.0, (100000, 2))).to(DEV)
    out["points"] = int(pts.shape[0])
    out["points_ms"] = round(timed(lambda: dist.map_points(pts, 60, 1280, 1280), a.reps), 4)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
