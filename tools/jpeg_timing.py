"""Kernel time of the two JPEG kernels (csrc/jpeg.hip: jpeg_idct_kernel, jpeg_color_kernel), for a kernel trace.

    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -o kt -- python tools/jpeg_timing.py [--images 1024] [--reps 10]

in a run of its own (no counters, no other tracing beside it).  The kernel times come from the trace's statistics; the JSON line this
prints carries the bytes each kernel moves, computed from the shapes, and GPU-event times of the same launches for orientation
(bytes / kernel time = the achieved bytes/s).

The batch: ``--images`` images of 480 x 640, 4:2:0, built by tiling the MCU grid of the 240 x 320 scene fixture 2 x 2 at the coefficient
level (no encoder needed); the coefficients are uploaded once, outside the timed launches.  The decode of the tiled image is checked
against the fixture's decode tiled the same way, away from the seams (chroma upsampling looks one sample across them).
"""
import argparse
import copy
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "exploration-of-potential_amd"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from ep24 import _lib, jpeg  # noqa: E402

FIXTURES = os.path.join(ROOT, "tests", "golden", "jpeg")


def tiled_scene(ty=2, tx=2):
    with open(os.path.join(FIXTURES, "scene_420.jpg"), "rb") as fh:
        it = jpeg.entropy_decode(fh.read())
    hd = copy.deepcopy(it.header)
    assert hd.width % (8 * max(hd.h)) == 0 and hd.height % (8 * max(hd.v)) == 0     # whole MCUs: tiles meet without padding
    parts, off = [], 0
    for c in range(hd.ncomp):
        blk = it.coef[off:off + 64 * hd.nblocks[c]].reshape(hd.blocks_h[c], hd.blocks_w[c], 64)
        off += 64 * hd.nblocks[c]
        parts.append(np.tile(blk, (ty, tx, 1)).reshape(-1))
        hd.blocks_h[c], hd.blocks_w[c] = hd.blocks_h[c] * ty, hd.blocks_w[c] * tx
        hd.nblocks[c] = hd.blocks_h[c] * hd.blocks_w[c]
    hd.height, hd.width = hd.height * ty, hd.width * tx
    hd.ncoef = 64 * sum(hd.nblocks)
    return jpeg.JpegCoefficients(hd, np.ascontiguousarray(np.concatenate(parts)))


def timed(fn, reps):
    fn()
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
    ap.add_argument("--images", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=10)
    a = ap.parse_args()
    _lib.require_gpu()
    item = tiled_scene()
    H, W = item.header.height, item.header.width
    P = jpeg.pack([item] * a.images)
    buf = torch.from_numpy(P.host).cuda()
    planes = torch.empty(64 * P.blocks, dtype=torch.uint8, device="cuda")
    out = torch.empty(P.out_bytes, dtype=torch.uint8, device="cuda")
    base, s = buf.data_ptr(), _lib.stream_ptr()

    def idct():
        _lib.call("jpeg_idct", base, base + P.o_qt, P.n_qt, base + P.o_pd, P.n_planes, P.blocks, _lib.ptr(planes), s)

    def color():
        _lib.call("jpeg_color", _lib.ptr(planes), base + P.o_id, P.n_images, P.groups, _lib.ptr(out), P.out_bytes, 1, s)

    ms_idct, ms_color = timed(idct, a.reps), timed(color, a.reps)
    # the result: first and last image against the fixture's decode, tiled, away from the seams
    want = np.load(os.path.join(FIXTURES, "scene_420.rgb.npy"))[:, :, ::-1]
    want = np.tile(want, (2, 2, 1))
    keep = np.ones((H, W), bool)
    keep[H // 2 - 2:H // 2 + 2] = False
    keep[:, W // 2 - 2:W // 2 + 2] = False
    ok = True
    for o, h, w in (P.shapes[0], P.shapes[-1]):
        got = out[o:o + h * w * 3].view(h, w, 3).cpu().numpy()
        ok = ok and bool(np.array_equal(got[keep], want[keep]))
    idct_bytes = P.blocks * 128 + P.blocks * 64                      # int16 coefficients read, uint8 planes written (tables: 128 B each, cached)
    color_bytes = P.blocks * 64 + a.images * H * W * 3               # planes read, HWC written
    print(json.dumps({"images": a.images, "height": H, "width": W, "sampling": "4:2:0", "reps": a.reps, "blocks": P.blocks,
                      "idct_bytes": idct_bytes, "color_bytes": color_bytes, "idct_event_ms": round(ms_idct, 4),
                      "color_event_ms": round(ms_color, 4), "idct_event_GBps": round(idct_bytes / ms_idct / 1e6, 1),
                      "color_event_GBps": round(color_bytes / ms_color / 1e6, 1), "equals_fixture_away_from_seams": ok}))
    if not ok:
        sys.exit(1)


if __name__ == "__main__":
    main()
