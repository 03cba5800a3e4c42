"""Kernel time of the device Huffman stage (csrc/jpeg_huff.hip: jpeg_huff_kernel, jpeg_dc_kernel) beside the two arithmetic kernels
(csrc/jpeg.hip), for a kernel trace.

    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -o kt -- python tools/jpeg_device_timing.py [--images 1024] [--reps 5]

in a run of its own (no counters, no other tracing beside it).  The kernel times come from the trace's statistics; the JSON lines this
prints carry what the times are divided into: the scan bytes of the batch, its coefficients, GPU-event times of the same launches for
orientation, and the largest number of rounds a tile needed (from the host emulation of one file: the batch is copies of it).

Two batches, ``--images`` files each: the file ``jpeg.entropy_encode`` writes from the coefficient-tiled scene of tools/jpeg_timing.py
(480 x 640, 4:2:0, Annex K tables), and the photo fixture (640 x 427, 4:4:4, optimised tables, 1.1 bytes per pixel).  The bytes are
uploaded once, outside the timed launches; every repetition runs the memset, jpeg_huff_kernel, jpeg_dc_kernel, jpeg_idct_kernel and
jpeg_color_kernel.  The first and the last image's coefficients are checked against ``jpeg.entropy_decode``.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "exploration-of-potential_amd"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from ep24 import _lib, jpeg  # noqa: E402
from jpeg_timing import FIXTURES, tiled_scene, timed  # noqa: E402


def run(name, data, images, reps, S, tile):
    want = jpeg.entropy_decode(data).coef
    _, rounds = jpeg.selfsync_emulate(data, S, tile)
    item = jpeg.scan(data)
    P = jpeg.pack([item] * images, subseq_bytes=S, tile=tile)
    buf = jpeg.upload(P, torch.device("cuda"))
    planes = torch.empty(64 * P.blocks, dtype=torch.uint8, device="cuda")
    out = torch.empty(P.out_bytes, dtype=torch.uint8, device="cuda")
    status = torch.empty(P.n_scan, dtype=torch.int32, device="cuda")
    ms_entropy = timed(lambda: jpeg.launch_entropy(P, buf, status), reps)
    ms_all = timed(lambda: jpeg.launch(P, buf, planes, out, True, status), reps)
    coef = buf[:P.gap].view(torch.int16)
    n = item.header.ncoef
    ok = not bool(status.any()) and np.array_equal(coef[:n].cpu().numpy(), want) and np.array_equal(coef[-n:].cpu().numpy(), want)
    scan_bytes = images * item.data.size
    print(json.dumps({"batch": name, "images": images, "height": item.header.height, "width": item.header.width, "reps": reps,
                      "subseq_bytes": S, "tile": tile, "scan_bytes": scan_bytes, "coef_bytes": P.gap, "subsequences_per_image": -(-item.data.size // S),
                      "max_rounds_per_tile": rounds, "entropy_event_ms": round(ms_entropy, 3), "all_event_ms": round(ms_all, 3),
                      "entropy_event_scan_GBps": round(scan_bytes / ms_entropy / 1e6, 2), "equals_entropy_decode": ok}), flush=True)
    return ok


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--subseq-bytes", type=int, default=jpeg.SUBSEQ_BYTES)
    ap.add_argument("--tile", type=int, default=jpeg.TILE)
    a = ap.parse_args()
    _lib.require_gpu()
    scene = jpeg.entropy_encode(tiled_scene())
    with open(os.path.join(FIXTURES, "photo_000000130566.jpg"), "rb") as fh:
        photo = fh.read()
    ok = run("scene_480x640_420", scene, a.images, a.reps, a.subseq_bytes, a.tile)
    ok = run("photo_640x427_444", photo, a.images, a.reps, a.subseq_bytes, a.tile) and ok
    if not ok:
        sys.exit(1)


if __name__ == "__main__":
    main()
