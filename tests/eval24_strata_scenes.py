"""Seeded scenes for the stratified 24-point evaluation, shared by tests/test_eval24_strata_oracle.py (CPU: the oracle alone) and
tests/test_gpu_eval24_strata.py (the kernels against the oracle).  numpy only.

``make_scene()`` builds five images on a 640 x 640 canvas; ``B`` / ``L`` cut it down (the first B images, the first L label rows):

  0  random GTs of four classes with jittered detections and false positives, plus two hand-made pairs: a DUPLICATED GT row with a
     detection on it (an equal-IoU tie between two non-ignored GTs), and a regular 24-gon of radius 17 (area 898: small) inside one
     of radius 20 (area 1 242: medium) with a detection equal to the small one (in "medium" the ignored GT has the larger IoU and the
     non-ignored one wins)
  1  256 GT rows of class 0 on a grid (exactly EV_MAX_L rows of one class) and 150 detections of class 0 (more than 128 in a segment)
  2  70 GTs of class 1 (more than 64: a lane holds two) and 10 of class 3, no detections
  3  no GTs, 37 detections
  4  random GTs, one of them centred at (25, 28): beyond the field of either lens
"""
import numpy as np

import eval24_oracle as O
import eval24_strata_oracle as SO
from ep24 import evaluate as E
from ep24.lens import LensModel

S = 640
SIZES = [(480, 640), (1280, 960), (800, 800), (640, 640), (512, 400)]       # raw (h, w): letterbox ratios 1, 0.5, 0.8, 1, 1.25
LENS_A = LensModel((200.0, 200.0, 319.5, 319.5), (200.0, 200.0, 319.5, 319.5), (0.02, -0.003, 0.0, 0.0), 160.0, (S, S))
LENS_B = LensModel((230.0, 210.0, 300.0, 330.0), (230.0, 210.0, 300.0, 330.0), (-0.01, 0.002, 0.0, 0.0), 150.0, (S, S))    # fx != fy
F = np.float32


def gt_row(cls, cx, cy, r, rng=None, noise=0.08):
    c, s = O.ray_cos_sin()
    rad = np.full(24, r, dtype=np.float64)
    if rng is not None:
        rad = np.maximum(rad * (1.0 + noise * rng.randn(24)), 2.0)
    rad = rad.astype(np.float32)
    row = np.zeros(51, dtype=np.float32)
    row[0], row[1], row[2] = cls, cx, cy
    row[3::2] = F(cx) + rad * c
    row[4::2] = F(cy) + rad * s
    return row


def det_of(row, rng=None, dc=0.0, dr=0.0, cls=None):
    """A detection row [29] on the GT ``row``: its centre and radii, jittered."""
    vx, vy = row[3::2] - row[1], row[4::2] - row[2]
    d = np.zeros(29, dtype=np.float32)
    d[0:2] = row[1:3]
    d[2:26] = np.sqrt(vx * vx + vy * vy)
    if rng is not None:
        d[0:2] += (rng.randn(2) * dc).astype(np.float32)
        d[2:26] *= (1.0 + rng.randn(24) * dr).astype(np.float32)
    d[28] = row[0] if cls is None else cls
    return d


def false_positives(n, classes, rng):
    d = np.zeros((n, 29), dtype=np.float32)
    d[:, 0:2] = rng.uniform(20, S - 20, (n, 2))
    d[:, 2:26] = (rng.uniform(6, 70, (n, 1)) * (1.0 + 0.1 * rng.randn(n, 24))).clip(2.0)
    d[:, 28] = rng.choice(classes, n)
    return d


def random_gts(n, classes, rng):
    return [gt_row(rng.choice(classes), rng.uniform(40, S - 40), rng.uniform(40, S - 40), rng.uniform(8, 75), rng) for _ in range(n)]


def make_scene(B=5, L=256, seed=0):
    rng = np.random.RandomState(seed)
    gts, dets = [], []
    # image 0
    g = random_gts(22, [0, 1, 2, 3], rng)
    dup = gt_row(1, 200.0, 420.0, 30.0, rng)
    small, medium = gt_row(2, 450.0, 150.0, 17.0), gt_row(2, 450.0, 150.0, 20.0)
    g = [dup, dup.copy(), small, medium] + g
    d = [det_of(dup), det_of(dup, rng, 1.0, 0.02), det_of(small), det_of(medium, rng, 1.5, 0.03)]
    d += [det_of(r, rng, 3.0, 0.06) for r in g[4:]] + [det_of(r, rng, 8.0, 0.12) for r in g[4:16]]
    gts.append(g)
    dets.append(np.concatenate([np.stack(d), false_positives(25, [0, 1, 2, 3], rng)]))
    # image 1: a 16 x 16 grid of class 0
    g = [gt_row(0, 30.0 + 38.0 * (i % 16), 30.0 + 38.0 * (i // 16), 8.0 + 22.0 * rng.rand(), rng) for i in range(256)]
    gts.append(g)
    dets.append(np.concatenate([np.stack([det_of(r, rng, 1.5, 0.05) for r in g[:140]]), false_positives(10, [0], rng),
                                false_positives(7, [1, 2], rng)]))
    # image 2: no detections
    gts.append(random_gts(70, [1], rng) + random_gts(10, [3], rng))
    dets.append(None)
    # image 3: no GTs
    gts.append([])
    dets.append(false_positives(37, [0, 1, 2, 3], rng))
    # image 4
    g = [gt_row(2, 25.0, 28.0, 14.0, rng)] + random_gts(30, [0, 1, 2, 3], rng)
    gts.append(g)
    dets.append(np.concatenate([np.stack([det_of(r, rng, 2.5, 0.05) for r in g]), false_positives(13, [0, 1, 2, 3], rng)]))
    labels = np.zeros((5, L, 51), dtype=np.float32)
    for i, g in enumerate(gts):
        for r, row in enumerate(g[:L]):
            labels[i, r] = row
    for d in dets:
        if d is not None:
            d[:, 26] = (rng.randint(1, 11, len(d)) / 10.0).astype(np.float32)           # quantised scores: ties
            d[:, 27] = np.where(rng.rand(len(d)) < 0.5, 1.0, 0.5).astype(np.float32)
            d[:] = d[rng.permutation(len(d))]
    sizes = SIZES[:B]
    return {"labels": labels[:B], "dets": dets[:B], "sizes": sizes, "scales": E.letterbox_scales(sizes, (S, S)),
            "lenses": [LENS_A if i % 2 == 0 else LENS_B for i in range(B)]}


CONFIGS = ("all", "coco+lens", "radius3")


def config(scene, name):
    """-> (strata, zones [B, 16]) of a named configuration: NA = 1, 4 COCO areas + 4 lens zones = 8, 3 radius zones."""
    B = len(scene["sizes"])
    if name == "all":
        return [E.Stratum("all")], E.no_zones(B)
    if name == "coco":
        return E.coco_area_strata(), E.no_zones(B)
    if name == "coco+lens":
        return E.coco_area_strata() + E.zone_strata([0, 20, 40, 60, 90], "deg"), E.lens_zones(scene["lenses"])
    if name == "radius3":
        return E.zone_strata([0, 1 / 3, 2 / 3, float("inf")], "r"), E.radius_zones(scene["sizes"], (S, S))
    raise KeyError(name)


def oracle_images(scene, zones, iou_fn):
    """The oracle's image dicts: measures from the oracle, ``iou_fn(gt50 [G, 50], det26 [D, 26]) -> [G, D] float64``."""
    imgs = []
    for i, d in enumerate(scene["dets"]):
        lab = scene["labels"][i]
        n = O.num_gt(lab)
        gt = lab[:n]
        if d is None:
            d = np.zeros((0, 29), dtype=np.float32)
        gm = SO.measure_labels(gt, np.full(n, i), scene["scales"], zones)
        dm = SO.measure_dets(d, np.full(len(d), i), scene["scales"], zones)
        iou = iou_fn(gt[:, 1:], d[:, :26]) if n and len(d) else np.zeros((n, len(d)))
        imgs.append({"gt_cls": gt[:, 0].astype(np.int64), "gt_area": gm[:, 0], "gt_zone": gm[:, 1], "det_cls": d[:, 28].astype(np.int64),
                     "det_score": d[:, 26] * d[:, 27], "det_area": dm[:, 0], "det_zone": dm[:, 1], "iou": iou})
    return imgs


def strata_rows(strata):
    return [s.row() for s in strata]
