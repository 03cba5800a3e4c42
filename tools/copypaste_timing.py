"""Kernel time of the copy-paste post-pass (csrc/paste.hip) beside its two yardsticks, for a kernel trace.

    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -o kt -- python tools/copypaste_timing.py [--reps 20]

in a run of its own (no counters, no other tracing beside it).  The kernel times come from the trace's statistics
(paste_u8_kernel<true>, paste_labels_kernel, augment_u8_kernel<false>, augment_labels_kernel<false>, and the elementwise copy kernel
of ``Tensor.copy_``); the JSON line this prints carries GPU-event times of the same launches for orientation.

A batch of 20 raw 640 x 480 images with 10 label rows each goes through ``augment_u8`` + ``augment_labels`` (default YOLOX parameters)
to 640 x 640; then every image pastes from a partner (``sample_paste`` at probability 1): ``paste_labels`` + ``paste_u8`` on the
resident batch.  ``paste_u8`` reads and writes the fp32 batch once (2 x 98.3 MB), so its yardstick is a plain device ``copy_`` of the
same tensor, launched beside it; the yardstick of ``paste_labels`` is ``augment_labels``.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "exploration-of-potential_amd"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from ep24 import augment as aug, synth  # noqa: E402


def timed(fn, reps):
    fn()                                                  # warm-up: code object load, allocations
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
    ap.add_argument("--batch", type=int, default=20)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--size", type=int, default=640)
    a = ap.parse_args()
    n, S, h, w = a.batch, (a.size, a.size), 480, 640
    rs = np.random.RandomState(0)
    images = [torch.from_numpy(rs.randint(0, 256, (h, w, 3)).astype(np.uint8)).cuda() for _ in range(n)]
    targets = []
    for i in range(n):
        lab = synth.make_labels(1, [10], size=(h, w), seed=10 + i)[0][:10].double().numpy()
        lab[:, 1::2] /= w
        lab[:, 2::2] /= h
        targets.append(lab)
    sizes = [(h, w)] * n
    params = aug.sample_params(aug.position_rng(0, 0, 0), sizes, S)
    pre_i = torch.empty(n, 3, *S, dtype=torch.float32, device="cuda")
    pre_l = torch.empty(n, 50, 51, dtype=torch.float32, device="cuda")
    state = {}

    def augmented():
        state["pre_c"] = aug.mosaic_batch(images, targets, params, S, 50, pre_i, pre_l)[2]

    augmented()
    pasting = aug.sample_paste(aug.paste_rng(0, 0, 0), aug.AugParams(n), n, S, 1.0)
    desc = aug.paste_descriptors(pasting)
    out_i, out_l = torch.empty_like(pre_i), torch.empty_like(pre_l)
    counts = torch.empty(n, dtype=torch.int32, device="cuda")

    def pasted():
        state["ranges"] = aug.paste_batch(pre_i, pre_l, state["pre_c"], desc, out_images=out_i, out_labels=out_l, counts=counts)[3]

    def copied():
        out_i.copy_(pre_i)

    ms_aug, ms_copy, ms_paste = timed(augmented, a.reps), timed(copied, a.reps), timed(pasted, a.reps)
    ranges = state["ranges"].cpu().numpy()
    changed = int((out_i != pre_i).any(1).sum())
    print(json.dumps({"batch": n, "input_size": list(S), "reps": a.reps, "bytes_moved_by_paste_u8": 2 * pre_i.numel() * 4,
                      "augment_pair_ms_incl_host": round(ms_aug, 4), "copy_ms": round(ms_copy, 4),
                      "paste_pair_ms_incl_host": round(ms_paste, 4), "rows_before": state["pre_c"].tolist(),
                      "rows_pasted": (ranges[:, 1] - ranges[:, 0]).tolist(), "pixels_changed": changed}))


if __name__ == "__main__":
    main()
