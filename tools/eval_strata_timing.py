"""Launch the match kernel's instance with strata (csrc/evalgeom.h) beside the single-range one on one fixed batch, for

    rocprofv3 --kernel-trace --stats -- python tools/eval_strata_timing.py

B = 20 images, 50 GTs each, 8 400 anchors at conf 0.01 (synthetic eval-mode predictions through post_prepare + post_nms, as
``Evaluator24.update`` runs them).  ``eval_match_kernel<GW, false>``, ``eval_match_kernel<GW, true>`` at NA = 1 and at NA = 8 (the four COCO area
rows and four lens zones) are launched ``--reps`` times each on the same buffers; the trace tells the three apart by their order.
Prints one JSON line with GPU-event times per launch, for a run without the profiler.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "exploration-of-potential_amd"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from ep24 import evaluate as E, infer, synth  # noqa: E402
from ep24._lib import call, ptr, stream_ptr  # noqa: E402
from ep24.lens import LensModel  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=21)
    ap.add_argument("--iou-type", default="circle24")
    a = ap.parse_args()
    B, S, C, G = 20, 640, 80, 50
    pred = synth.decode_head(synth.make_raw_head(B, S, seed=3, num_classes=C), S)
    pred[..., 26:] = torch.sigmoid(pred[..., 26:])
    pred = pred.cuda()
    labels = synth.make_labels(B, G, size=S, seed=4).cuda()
    lens = LensModel.equidistant((S, S), (S, S), 170.0)
    configs = {"NA=1": [E.Stratum("all")], "NA=8": E.coco_area_strata() + E.zone_strata([0, 20, 40, 60, 90], "deg")}
    zones = E.lens_zones([lens] * B)
    ev = E.Evaluator24(C, iou_type=a.iou_type, conf_thre=0.01)
    ev.update(pred, labels)                               # post_prepare + post_nms: their outputs stay in the scratch
    A = pred.shape[1]
    ws = infer._scratch[(B, A, str(pred.device))]
    row_off = next(iter(E._row_offs.values()))
    cs, thr, _ = E._device_consts(pred.device)
    kept = float(ws.count.float().mean().item())
    cap, P = B * A, E._pow2(A)
    ms = E._MatchScratch(B, P, cap, pred.device, 8)
    sc, zt = torch.ones(B, dtype=torch.float64, device=pred.device), torch.from_numpy(zones).to(pred.device)
    npig = torch.zeros(C * 8, dtype=torch.int32, device=pred.device)
    err = torch.zeros(1, dtype=torch.int32, device=pred.device)

    def plain():
        ms.count.zero_()
        call("eval_match", ptr(labels), labels.shape[1], B, ptr(pred), pred.shape[2], ptr(row_off), ptr(ws.keep), A, ptr(ws.count),
             ptr(ws.conf), ptr(ws.cls), C, ev._t, ptr(cs), ptr(thr), 100, 0, ptr(ms.sort), P, ptr(ms.key), ptr(ms.cls), ptr(ms.p),
             ptr(ms.tp), ptr(ms.count), ptr(npig), ptr(err), stream_ptr())

    def strata(rows):
        def run():
            ms.count.zero_()
            call("eval_match_strata", ptr(labels), labels.shape[1], B, ptr(pred), pred.shape[2], ptr(row_off), ptr(ws.keep), A,
                 ptr(ws.count), ptr(ws.conf), ptr(ws.cls), C, ev._t, ptr(cs), ptr(thr), 100, 0, ptr(ms.sort), P, ptr(sc), ptr(zt),
                 rows.ctypes.data, len(rows), ptr(ms.key), ptr(ms.cls), ptr(ms.p), ptr(ms.tp), ptr(ms.val), ptr(ms.count), ptr(npig),
                 ptr(err), stream_ptr())
        return run

    def timed(fn):
        fn()
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        t0.record()
        for _ in range(a.reps):
            fn()
        t1.record()
        torch.cuda.synchronize()
        return round(t0.elapsed_time(t1) / a.reps * 1000.0, 1)

    out = {"batch": B, "gts_per_image": G, "anchors": A, "iou_type": a.iou_type, "kept_dets_per_image": round(kept, 1),
           "eval_match_us": timed(plain)}
    for name, st in configs.items():
        rows = np.array([s.row() for s in st], dtype=np.float64)
        out["eval_match_strata_%s_us" % name] = timed(strata(rows))
    out["records"] = int(ms.count.item())
    assert int(err.item()) == 0
    print(json.dumps(out))


if __name__ == "__main__":
    main()
