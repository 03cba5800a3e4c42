"""Host entropy stage (ep24.jpeg.entropy_decode: marker parser + Huffman decoder of libep24jpeg.so) in images/s on one core, beside
Pillow's FULL decode of the same file where Pillow is installed.  No GPU involved.

    python tools/jpeg_host_timing.py [--file tests/golden/jpeg/photo_000000130566.jpg] [--seconds 2]

A report, not a gate: the host stage is what a loader process spends per image; Pillow's figure is the whole decode it replaces.
"""
import argparse
import io
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "exploration-of-potential_amd"))

from ep24 import jpeg  # noqa: E402


def rate(fn, seconds):
    fn()
    n, t0 = 0, time.perf_counter()
    while time.perf_counter() - t0 < seconds:
        fn()
        n += 1
    return n / (time.perf_counter() - t0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--file", default=os.path.join(ROOT, "tests", "golden", "jpeg", "photo_000000130566.jpg"))
    ap.add_argument("--seconds", type=float, default=2.0)
    a = ap.parse_args()
    with open(a.file, "rb") as fh:
        data = fh.read()
    hd = jpeg.parse(data)
    rec = {"file": os.path.basename(a.file), "bytes": len(data), "height": hd.height, "width": hd.width,
           "sampling": "%dx%d" % (hd.h[0], hd.v[0]), "entropy_stage_images_per_s_per_core": round(rate(lambda: jpeg.entropy_decode(data), a.seconds), 1)}
    try:
        from PIL import Image
        import numpy as np
        rec["pillow_full_decode_images_per_s_per_core"] = round(rate(lambda: np.asarray(Image.open(io.BytesIO(data)).convert("RGB")), a.seconds), 1)
    except ImportError:
        rec["pillow_full_decode_images_per_s_per_core"] = None
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
