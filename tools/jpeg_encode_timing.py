"""Kernel time of the two JPEG encode kernels (csrc/jpeg_encode.hip: jpeg_sample_kernel, jpeg_fdct_kernel), for a kernel trace, and
the host stage (ep24.jpeg.entropy_encode) in images/s on one core.

    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -o kt -- python tools/jpeg_encode_timing.py [--images 1024] [--reps 10]

in a run of its own (no counters, no other tracing beside it).  The kernel times come from the trace's statistics; the JSON line this
prints carries the bytes each kernel moves, computed from the shapes, and GPU-event times of the same launches for orientation
(bytes / kernel time = the achieved bytes/s).

The batch: ``--images`` images of 480 x 640 (the decode of the 240 x 320 scene fixture tiled 2 x 2, every image its own memory),
quality 95 at 4:2:0 - the workload of tools/jpeg_timing.py, backwards.  The descriptors are uploaded once, outside the timed launches.
Checked: the first and the last image give the coefficients of the image encoded alone, and the project's decoder reads the written
file back at more than 30 dB PSNR against the pixels that went in.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "exploration-of-potential_amd"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from ep24 import _lib, jpeg  # noqa: E402

FIXTURES = os.path.join(ROOT, "tests", "golden", "jpeg")


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
    ap.add_argument("--seconds", type=float, default=2.0, help="how long the host stage is timed")
    a = ap.parse_args()
    _lib.require_gpu()
    rgb = np.tile(np.load(os.path.join(FIXTURES, "scene_420.rgb.npy")), (2, 2, 1))
    H, W = rgb.shape[:2]
    batch = torch.from_numpy(rgb).cuda().unsqueeze(0).repeat(a.images, 1, 1, 1).contiguous()
    qt = jpeg.quality_tables(95)
    gr = jpeg._grids(H, W, 3)
    groups_i = 8 * gr[0][2] * gr[0][3] + 8 * gr[1][2] * gr[1][3]
    plane_i = 64 * sum(g[2] * g[3] for g in gr)
    blocks_i = sum(g[4] * g[5] for g in gr)
    idesc, pdesc = [], []
    for i in range(a.images):
        idesc.append([i * groups_i, batch[i].data_ptr(), W * 3, H, W, 3, i * plane_i, 0])
        b, p = i * blocks_i, i * plane_i
        for c, (hc, _, wb, hb, bw, bh) in enumerate(gr):
            pdesc.append([b, bw, min(c, 1), p, wb, hb, hc, 0])
            b, p = b + bw * bh, p + 64 * wb * hb
    idesc.append([a.images * groups_i] + [0] * 7)
    pdesc.append([a.images * blocks_i] + [0] * 7)
    d_qt = torch.from_numpy(qt.astype(np.int16)).cuda()
    d_id = torch.from_numpy(np.asarray(idesc, dtype=np.int64)).cuda()
    d_pd = torch.from_numpy(np.asarray(pdesc, dtype=np.int64)).cuda()
    planes = torch.empty(a.images * plane_i, dtype=torch.uint8, device="cuda")
    coef = torch.empty(a.images * blocks_i * 64, dtype=torch.int16, device="cuda")
    s = _lib.stream_ptr()

    def sample():
        _lib.call("jpeg_sample", _lib.ptr(d_id), a.images, a.images * groups_i, _lib.ptr(planes), planes.numel(), s)

    def fdct():
        _lib.call("jpeg_fdct", _lib.ptr(planes), planes.numel(), _lib.ptr(d_qt), 2, _lib.ptr(d_pd), len(pdesc) - 1, a.images * blocks_i,
                  _lib.ptr(coef), s)

    ms_sample, ms_fdct = timed(sample, a.reps), timed(fdct, a.reps)
    alone = jpeg.forward([batch[0]], quality=95, subsampling="4:2:0", bgr=False)[0]
    n = blocks_i * 64
    ok = all(np.array_equal(coef[i * n:(i + 1) * n].cpu().numpy(), alone.coef) for i in (0, a.images - 1))
    data = jpeg.entropy_encode(alone)
    back = jpeg.decode([data], bgr=False)[0].cpu().numpy().astype(np.float64)
    psnr = 10 * np.log10(255.0 ** 2 / max(float(((back - rgb) ** 2).mean()), 1e-9))
    ok = ok and psnr > 30.0
    n_host, t0 = 0, time.perf_counter()
    while time.perf_counter() - t0 < a.seconds:
        jpeg.entropy_encode(alone)
        n_host += 1
    host_rate = n_host / (time.perf_counter() - t0)
    sample_bytes = a.images * (2 * H * W * 3 + plane_i)               # the pixels are read once for Y and once for Cb / Cr; planes written
    fdct_bytes = a.images * (plane_i + blocks_i * 128)                # planes read, int16 coefficients written
    print(json.dumps({"images": a.images, "height": H, "width": W, "sampling": "4:2:0", "quality": 95, "reps": a.reps,
                      "blocks": a.images * blocks_i, "sample_bytes": sample_bytes, "fdct_bytes": fdct_bytes,
                      "sample_event_ms": round(ms_sample, 4), "fdct_event_ms": round(ms_fdct, 4),
                      "sample_event_GBps": round(sample_bytes / ms_sample / 1e6, 1), "fdct_event_GBps": round(fdct_bytes / ms_fdct / 1e6, 1),
                      "file_bytes": len(data), "psnr_db": round(psnr, 2), "host_stage_images_per_s_per_core": round(host_rate, 1),
                      "batch_equals_single": bool(ok)}))
    if not ok:
        sys.exit(1)


if __name__ == "__main__":
    main()
