"""Launch the test-time augmentation kernels (csrc/tta.hip) beside the polygon NMS on one merged table, for a kernel trace.

    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -o kt -- python tools/tta_timing.py [--reps 5]

in a run of its own (no counters, no other tracing beside it).  The kernel times come from the trace's statistics
(``mirror_kernel``, ``unmap_kernel`` and ``vote_kernel`` against ``polynms_matrix_kernel``); the JSON line this prints carries the
workload and GPU-event times of the same launches for orientation.

Workload: B = 20 images at 640 x 640 and six views' worth of candidates - the ``synth`` head at 640, 544 and 448, each with two
seeds standing for the plain and the mirrored view, brought into one frame by ``ep24_tta_unmap`` (37 170 rows per image) - at
``conf_thre`` 0.01, ``nms_thre`` 0.65 (the evaluator's settings), ``vote_thre`` = ``nms_thre``, and the canonical view's 8 400
anchors as ``max_candidates``, as the entry points set it.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "exploration-of-potential_amd"))

import torch  # noqa: E402

from ep24 import infer, synth, tta  # noqa: E402
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--batch", type=int, default=20)
    ap.add_argument("--size", type=int, default=640)
    ap.add_argument("--vote", type=float, default=0.65)
    ap.add_argument("--max-candidates", type=int, default=None, help="default: the canonical view's anchor count")
    a = ap.parse_args()
    B, S, C, conf, thr = a.batch, a.size, 80, 0.01, 0.65
    views = tta.views_for(S)
    anchors = [tta.anchors_for(v[:2]) for v in views]
    A, ncols = sum(anchors), 27 + C
    K = anchors[0] if a.max_candidates is None else min(a.max_candidates, A)
    s = stream_ptr()
    heads = []
    for i, (h, w, _) in enumerate(views):
        p = synth.decode_head(synth.make_raw_head(B, h, seed=3 + i, num_classes=C), h)
        p[..., 26:] = torch.sigmoid(p[..., 26:])
        heads.append(p.to(DEV).contiguous())
    merged = torch.empty(B, A, ncols, dtype=torch.float32, device=DEV)

    def unmap():
        off = 0
        for (h, w, mir), p, n in zip(views, heads, anchors):
            call("tta_unmap", ptr(p), B, n, ncols, w, S / w, 1 if mir else 0, ptr(merged), A, off, s)
            off += n

    images = synth.make_images(B, S, seed=1).to(DEV).contiguous()
    flipped = torch.empty_like(images)

    def mirror():
        call("mirror_f32", ptr(images), B * 3, S, S, ptr(flipped), s)

    out = {"reps": a.reps, "B": B, "views": [list(v) for v in views], "A": A, "conf_thre": conf, "nms_thre": thr, "vote_thre": a.vote,
           "max_candidates": K}
    out["mirror_ms"] = round(timed(mirror, a.reps), 4)
    out["unmap_all_views_ms"] = round(timed(unmap, a.reps), 4)
    ws = infer._scratch[(B, A, str(merged.device))] = infer._Scratch(B, A, merged.device)
    call("post_prepare", ptr(merged), ncols, C, B * A, conf, ptr(ws.ray), ptr(ws.score), ptr(ws.conf), ptr(ws.cls), ptr(ws.rect), s)

    def nms():
        infer.nms_poly24(ws, merged, ncols, B, A, thr, False, K, s)

    def vote():
        infer.vote_poly24(ws, merged, ncols, B, A, a.vote, False, K, s)

    out["poly24_nms_ms"] = round(timed(nms, a.reps), 4)
    out["vote_ms"] = round(timed(vote, a.reps), 4)
    ps = ws.poly(K)
    kept = ws.count.tolist()
    out["candidates_per_image"] = ps.n_cand.tolist()
    out["kept_per_image"] = kept
    nv = ps.n_voters.view(B, A)
    out["voters_per_kept_mean"] = round(sum(float(nv[b, :k].sum()) for b, k in enumerate(kept)) / max(sum(kept), 1), 3)
    out["voters_per_kept_max"] = max((int(nv[b, :k].max()) for b, k in enumerate(kept) if k), default=0)
    out["matrix_bytes_per_image"] = K * ((K + 63) // 64) * 8
    print(json.dumps(out))


if __name__ == "__main__":
    main()
