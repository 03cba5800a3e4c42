"""``ep24.jpeg.encode`` with its Huffman stage on the host against the same call with the stage on the GPU (csrc/jpeg_huffenc.hip), on
the workload of tools/jpeg_encode_timing.py: wall time and device-to-host bytes of both, on the same batch, in the same process.

    python tools/jpeg_encode_device_timing.py [--images 1024] [--reps 7]
    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -o kt -- python tools/jpeg_encode_device_timing.py --reps 3

the second in a run of its own (no counters, no other tracing beside it): the trace's statistics then hold the kernel times of
jpeg_sample_kernel and jpeg_fdct_kernel beside the seven launches of the device Huffman stage.  Wall times under the profiler are
not the ones to quote.

The batch: ``--images`` images of 480 x 640 (the decode of the 240 x 320 scene fixture tiled 2 x 2, every image its own memory),
quality 95 at 4:2:0.  One warm-up call of each path, then ``--reps`` calls of each, alternating; median, minimum and maximum are
printed.  Checked: both paths return the same bytes for every image.
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "exploration-of-potential_amd"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from ep24 import _lib, jpeg  # noqa: E402

FIXTURES = os.path.join(ROOT, "tests", "golden", "jpeg")


def one(images, entropy):
    torch.cuda.synchronize()
    before, t0 = jpeg.stats["d2h_bytes"], time.perf_counter()
    out = jpeg.encode(images, quality=95, subsampling="4:2:0", bgr=False, entropy=entropy)
    return out, time.perf_counter() - t0, jpeg.stats["d2h_bytes"] - before


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=7)
    a = ap.parse_args()
    _lib.require_gpu()
    rgb = np.tile(np.load(os.path.join(FIXTURES, "scene_420.rgb.npy")), (2, 2, 1))
    H, W = rgb.shape[:2]
    batch = torch.from_numpy(rgb).cuda().unsqueeze(0).repeat(a.images, 1, 1, 1).contiguous()
    images = [batch[i] for i in range(a.images)]
    ref, _, host_bytes = one(images, "host")                # warm-up of both paths, and the check
    got, _, dev_bytes = one(images, "device")
    ok = got == ref
    times = {"host": [], "device": []}
    for _ in range(a.reps):
        for entropy in ("host", "device"):
            times[entropy].append(one(images, entropy)[1])
    res = {"images": a.images, "height": H, "width": W, "sampling": "4:2:0", "quality": 95, "reps": a.reps,
           "file_bytes_total": sum(len(d) for d in ref), "same_bytes": bool(ok),
           "host_d2h_bytes": host_bytes, "device_d2h_bytes": dev_bytes}
    for k, v in times.items():
        res[k + "_wall_s_median"] = round(statistics.median(v), 4)
        res[k + "_wall_s_min"] = round(min(v), 4)
        res[k + "_wall_s_max"] = round(max(v), 4)
        res[k + "_images_per_s_median"] = round(a.images / statistics.median(v), 1)
    print(json.dumps(res))
    if not ok:
        sys.exit(1)


if __name__ == "__main__":
    main()
