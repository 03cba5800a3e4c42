"""Launch the two tracking kernels (csrc/track.hip) over a synthetic sequence, and the polygon NMS on the same number of candidates,
for a kernel trace.

    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -o kt -- python tools/track_timing.py

in a run of its own (no counters, no other tracing beside it).  The kernel times come from the trace's statistics
(``track_cost_kernel`` and ``track_step_kernel`` against ``polynms_matrix_kernel``); the JSON line this prints carries the workload,
GPU-event times of the same launches for orientation, and the rounds of mutual best the association needed, recomputed on the host
from the IoU matrices the cost kernel left (a second pass over the same sequence, outside the timed one).

Workload: S = 8 streams, T = 256 slots, 100 detections per stream and frame, 50 frames: objects of radius 15..40 px drifting over a
1280 x 720 frame with 1 px centre noise and 3 % radial noise, four classes, a fifth of the scores between low and high.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "exploration-of-potential_amd"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from ep24 import infer, track  # noqa: E402
from ep24._lib import call, ptr, stream_ptr  # noqa: E402

DEV = "cuda:0"


def sequence(S, n, frames, seed=0):
    """-> list of det [S, n, 29] float32"""
    rng = np.random.default_rng(seed)
    c = np.stack([rng.uniform(40, 1240, (S, n)), rng.uniform(40, 680, (S, n))], -1)
    v = rng.uniform(-3, 3, (S, n, 2))
    r = rng.uniform(15, 40, (S, n, 1)) * (1 + 0.2 * rng.uniform(-1, 1, (S, n, 24)))
    cls = rng.integers(0, 4, (S, n)).astype(np.float64)
    out = []
    for _ in range(frames):
        c = c + v
        det = np.zeros((S, n, 29))
        det[..., :2] = c + rng.uniform(-1, 1, (S, n, 2))
        det[..., 2:26] = r * (1 + 0.03 * rng.uniform(-1, 1, (S, n, 24)))
        low = rng.uniform(size=(S, n)) < 0.2
        det[..., 26] = np.where(low, 0.6, 0.95)
        det[..., 27] = np.where(low, 0.5, rng.uniform(0.8, 1.0, (S, n)))
        det[..., 28] = cls
        order = rng.permuted(np.tile(np.arange(n), (S, 1)), axis=1)                 # the rows of a frame come in any order
        out.append(np.take_along_axis(det, order[..., None], 1).astype(np.float32))
    return out


def rounds(M, thr, slot_ok, row_ok):
    """Rounds of mutual best on one stream's matrix -> (matched slots, matched rows, matching rounds)."""
    adm = (M > thr) & slot_ok[:, None] & row_ok[None, :]
    ms, mr, n = np.zeros(M.shape[0], bool), np.zeros(M.shape[1], bool), 0
    while adm.any():
        X = np.where(adm, M, -1.0)
        d = X.argmax(1)
        t = np.nonzero(adm.any(1) & (X.argmax(0)[d] == np.arange(M.shape[0])))[0]
        n += 1
        ms[t], mr[d[t]] = True, True
        adm[t, :] = False
        adm[:, d[t]] = False
    return ms, mr, n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=8)
    ap.add_argument("--tracks", type=int, default=256)
    ap.add_argument("--dets", type=int, default=100)
    ap.add_argument("--frames", type=int, default=50)
    a = ap.parse_args()
    S, T, n, F = a.streams, a.tracks, a.dets, a.frames
    seq = [torch.from_numpy(d).to(DEV) for d in sequence(S, n, F)]
    count = torch.full((S,), n, dtype=torch.int32, device=DEV)
    trk = track.Tracker24(streams=S, max_tracks=T, max_dets=n, device=DEV)
    trk.update_padded(seq[0], count)                                              # warm-up
    trk.reset()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    t0.record()
    for det in seq:
        trk.update_padded(det, count)
    t1.record()
    torch.cuda.synchronize()
    out = {"S": S, "T": T, "dets_per_frame": n, "frames": F, "frame_ms": round(t0.elapsed_time(t1) / F, 4),
           "live_after": trk.hdr[:, 3].tolist(), "next_id": trk.hdr[:, 0].tolist(), "dropped": trk.hdr[:, 2].tolist()}
    # the rounds, on the host, from the kernel's own matrices
    trk.reset()
    hist1, hist2, pairs = {}, {}, 0
    for det in seq:
        before = trk.trk_i.cpu().numpy()
        trk.update_padded(det, count)
        M, sc = trk.iou.cpu().numpy(), trk.dscore.cpu().numpy()
        pairs += int((M > 0).sum())
        for s in range(S):
            live = before[s, :, 0] != 0
            high = sc[s] >= np.float32(trk.high_thre)
            ms, _, r1 = rounds(M[s], float(np.float32(trk.match_thre)), live, high)
            second = live & ~ms & (before[s, :, 2] == 2) & (before[s, :, 4] == 0)
            _, _, r2 = rounds(M[s], float(np.float32(trk.match_low_thre)), second, ~np.isnan(sc[s]) & ~high)
            hist1[r1] = hist1.get(r1, 0) + 1
            hist2[r2] = hist2.get(r2, 0) + 1
    out["rounds_stage1"] = {str(k): hist1[k] for k in sorted(hist1)}
    out["rounds_stage2"] = {str(k): hist2[k] for k in sorted(hist2)}
    out["pairs_reaching_poly24_iou_per_frame_and_stream"] = round(pairs / (F * S), 1)
    # the polygon NMS on the same number of candidates: B = S images of n rows, the last frame's
    C = 4
    pred = torch.zeros(S, n, 27 + C, device=DEV)
    pred[..., :27] = seq[-1][..., :27]
    pred[..., 27:] = 0.01
    pred.view(-1, 27 + C)[torch.arange(S * n, device=DEV), 27 + seq[-1][..., 28].reshape(-1).long()] = seq[-1][..., 27].reshape(-1)
    ws = infer._Scratch(S, n, pred.device)
    s = stream_ptr()
    call("post_prepare", ptr(pred), 27 + C, C, S * n, 0.01, ptr(ws.ray), ptr(ws.score), ptr(ws.conf), ptr(ws.cls), ptr(ws.rect), s)
    for _ in range(3):
        infer.nms_poly24(ws, pred, 27 + C, S, n, 0.65, False, None, s)
    torch.cuda.synchronize()
    out["poly24_nms_kept"] = ws.count.tolist()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
