"""Kernel time of the augmentation pair, without and with mixup, beside the plain pair on the same inputs.

    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/augment_timing.py [--batch 20] [--reps 20]

Uploads --batch raw 640x480 uint8 images with 10 labels each once, then launches ``preproc_u8`` + ``preproc_labels``,
``augment_u8`` + ``augment_labels`` (default YOLOX parameters: mosaic, affine, mirror, HSV) and ``augment_mix_u8`` +
``augment_mix_labels`` (the same parameters plus ``sample_mixup``'s defaults: a partner on every image) --reps times each on the
resident buffers, alternated.  The kernel times are read from the profiler's statistics (augment_u8_kernel<false> / <true>,
augment_labels_kernel<false> / <true>, preproc_u8_kernel, preproc_labels_kernel); the script itself prints one JSON line with
GPU-event times of the three pairs (host work and launch overhead included) and the survivors per image.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "exploration-of-potential_amd"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from ep24 import augment as aug, input as ein, synth  # noqa: E402


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
    out_i = torch.empty(n, 3, *S, dtype=torch.float32, device="cuda")
    out_l = torch.empty(n, 50, 51, dtype=torch.float32, device="cuda")
    sizes = [(h, w)] * n
    params = aug.sample_params(aug.position_rng(0, 0, 0), sizes, S)

    def plain():
        _, r = ein.preproc_batch(images, S, out=out_i)
        ein.labels_batch(targets, sizes, r, 50, out=out_l)

    counts = []

    def augmented():
        counts.append(aug.mosaic_batch(images, targets, params, S, 50, out_i, out_l)[2])

    mixed = aug.sample_mixup(aug.mixup_rng(0, 0, 0), aug.sample_params(aug.position_rng(0, 0, 0), sizes, S), sizes,
                             [len(t) for t in targets], S)
    mix_counts = []

    def with_mixup():
        mix_counts.append(aug.mosaic_batch(images, targets, mixed, S, 50, out_i, out_l)[2])

    def timed(fn):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        t0.record()
        fn()
        t1.record()
        torch.cuda.synchronize()
        return t0.elapsed_time(t1)

    plain(), augmented(), with_mixup()                       # warm-up
    tp, ta, tm = [], [], []
    for _ in range(a.reps):
        tp.append(timed(plain))
        ta.append(timed(augmented))
        tm.append(timed(with_mixup))
    print(json.dumps({"batch": n, "source": [h, w], "input_size": list(S), "reps": a.reps,
                      "plain_pair_ms_median_incl_host": round(float(np.median(tp)), 3),
                      "augment_pair_ms_median_incl_host": round(float(np.median(ta)), 3),
                      "mixup_pair_ms_median_incl_host": round(float(np.median(tm)), 3),
                      "survivors_per_image": counts[-1].tolist(), "mixup_images": int(mixed.mixup.sum()),
                      "survivors_per_image_with_mixup": mix_counts[-1].tolist()}))


if __name__ == "__main__":
    main()
