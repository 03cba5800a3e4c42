"""Launch the rectangle NMS and the polygon NMS (csrc/polynms.hip) on the same predictions, for a kernel trace.

    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -o kt -- python tools/polynms_timing.py [--reps 5]

in a run of its own (no counters, no other tracing beside it).  The kernel times come from the trace's statistics
(``nms_kernel`` against ``polynms_sort_kernel``, ``polynms_geometry_kernel``, ``polynms_matrix_kernel``, ``polynms_scan_kernel``);
the JSON line this prints carries the workload and GPU-event times of the same launches for orientation.

Workload: the ``synth`` head at 640 x 640, B = 20, ``conf_thre`` 0.01, ``nms_thre`` 0.65 (the evaluator's settings).  Printed with it:
the candidates per image and the share of the candidate pairs (j > i) that pass the class and box tests and reach ``poly24_iou``.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "exploration-of-potential_amd"))

import torch  # noqa: E402

from ep24 import infer, synth  # noqa: E402
from ep24._lib import call, ptr, stream_ptr  # noqa: E402

DEV = "cuda:0"


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


def pair_share(ps, B, K):
    """(pairs j > i among the candidates, pairs of them with equal classes and overlapping vertex boxes), from the geometry the
    kernels left in the scratch."""
    n_cand = ps.n_cand.tolist()
    box, cls = ps.vbox.view(B, K, 4), ps.vcls.view(B, K)
    total = live = 0
    for b, n in enumerate(n_cand):
        total += n * (n - 1) // 2
        for lo in range(0, n, 1024):                      # row blocks: the [n, n] tables stay small
            a, q = box[b, lo:lo + 1024][:n - lo], box[b, :n]
            w = torch.minimum(a[:, None, 2], q[None, :, 2]).double() - torch.maximum(a[:, None, 0], q[None, :, 0]).double()
            h = torch.minimum(a[:, None, 3], q[None, :, 3]).double() - torch.maximum(a[:, None, 1], q[None, :, 1]).double()
            ok = (w > 0) & (h > 0) & (cls[b, lo:lo + 1024][:n - lo, None] == cls[b, None, :n])
            ok &= torch.arange(n, device=DEV)[None, :] > (lo + torch.arange(a.shape[0], device=DEV))[:, None]
            live += int(ok.sum())
    return n_cand, total, live


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--batch", type=int, default=20)
    ap.add_argument("--size", type=int, default=640)
    ap.add_argument("--max-candidates", type=int, default=None)
    a = ap.parse_args()
    B, S, C, conf, thr = a.batch, a.size, 80, 0.01, 0.65
    pred = synth.decode_head(synth.make_raw_head(B, S, seed=3, num_classes=C), S)
    pred[..., 26:] = torch.sigmoid(pred[..., 26:])
    pred = pred.to(DEV).contiguous()
    A, ncols = pred.shape[1], pred.shape[2]
    ws = infer._scratch[(B, A, str(pred.device))] = infer._Scratch(B, A, pred.device)
    s = stream_ptr()
    call("post_prepare", ptr(pred), ncols, C, B * A, conf, ptr(ws.ray), ptr(ws.score), ptr(ws.conf), ptr(ws.cls), ptr(ws.rect), s)

    def rect():
        call("post_nms", ptr(ws.score), ptr(ws.cls), ptr(ws.rect), B, A, thr, 0, ptr(ws.skey), ptr(ws.sidx), ptr(ws.dead), ptr(ws.keep),
             ptr(ws.count), ws.P, s)

    def poly():
        infer.nms_poly24(ws, pred, ncols, B, A, thr, False, a.max_candidates, s)

    out = {"reps": a.reps, "B": B, "A": A, "conf_thre": conf, "nms_thre": thr, "max_candidates": a.max_candidates}
    out["rect_nms_ms"] = round(timed(rect, a.reps), 4)
    out["rect_kept"] = ws.count.tolist()
    out["poly24_nms_ms"] = round(timed(poly, a.reps), 4)
    out["poly24_kept"] = ws.count.tolist()
    K = A if a.max_candidates is None else min(a.max_candidates, A)
    n_cand, total, live = pair_share(ws.poly(K), B, K)
    out["candidates_per_image"] = n_cand
    out["pairs"] = total
    out["pairs_reaching_poly24_iou"] = live
    out["share_reaching_poly24_iou"] = round(live / max(total, 1), 5)
    out["matrix_bytes_per_image"] = K * ((K + 63) // 64) * 8
    print(json.dumps(out))


if __name__ == "__main__":
    main()
