"""Time the evaluator's kernels (csrc/evaluate.hip) on synthetic eval-mode predictions.

    python tools/eval24_timing.py [--batch 20] [--size 640] [--images 5000]

Prints one JSON line: the match kernel per batch (post_prepare + post_nms excluded), update() per batch (post_prepare + NMS +
match + the one count read) and summarize() for --images images (the same batch fed images / batch times), GPU event timed.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "exploration-of-potential_amd"))

import torch  # noqa: E402

from ep24 import evaluate as E, infer, synth  # noqa: E402
from ep24._lib import call, ptr, stream_ptr  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=20)
    ap.add_argument("--size", type=int, default=640)
    ap.add_argument("--images", type=int, default=5000)
    ap.add_argument("--iou-type", default="circle24")
    a = ap.parse_args()
    B, S, C = a.batch, a.size, 80
    pred = synth.decode_head(synth.make_raw_head(B, S, seed=3, num_classes=C), S)
    pred[..., 26:] = torch.sigmoid(pred[..., 26:])
    pred = pred.cuda()
    labels = synth.make_labels(B, 10, size=S, seed=4).cuda()
    ev = E.Evaluator24(C, iou_type=a.iou_type)
    ev.update(pred, labels)                               # warm-up: scratch, constants
    ws = infer._scratch[(B, pred.shape[1], str(pred.device))]
    ms = next(iter(E._match_scratch.values()))
    dets_per_image = ws.count.float().mean().item()
    row_off = next(iter(E._row_offs.values()))
    cs, thr, _ = E._device_consts(pred.device)
    A = pred.shape[1]

    def match():
        ms.count.zero_()                                  # as Evaluator24._match: records are appended at *rec_count, the buffers hold one batch's
        call("eval_match", ptr(labels), labels.shape[1], B, ptr(pred), pred.shape[2], ptr(row_off), ptr(ws.keep), A, ptr(ws.count),
             ptr(ws.conf), ptr(ws.cls), C, ev._t, ptr(cs), ptr(thr), ev.max_dets, 0, ptr(ms.sort), E._pow2(A), ptr(ms.key), ptr(ms.cls),
             ptr(ms.p), ptr(ms.tp), ptr(ms.count), ptr(ev._npig), ptr(ev._err), stream_ptr())

    def timed(fn, reps):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        t0.record()
        for _ in range(reps):
            fn()
        t1.record()
        torch.cuda.synchronize()
        return t0.elapsed_time(t1) / reps

    match_ms = timed(match, 20)
    ev.reset()
    nb = max(a.images // B, 1)
    update_ms = timed(lambda: ev.update(pred, labels), nb)
    summarize_ms = timed(ev.summarize, 1)
    print(json.dumps({"batch": B, "size": S, "anchors": A, "iou_type": a.iou_type, "kept_dets_per_image": round(dets_per_image, 1),
                      "match_ms_per_batch": round(match_ms, 3), "update_ms_per_batch": round(update_ms, 3), "images": nb * B,
                      "records": ev.n_records, "summarize_ms": round(summarize_ms, 3), "AP": ev.stats["AP"]}))


if __name__ == "__main__":
    main()
