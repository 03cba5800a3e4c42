"""A dataset folder for ``train_24p.py --data-dir OUT/images --label-dir OUT/COCO_24p_label`` from the committed JPEG fixtures
(tests/golden/jpeg), with seeded synthetic label rows - for machines that have neither COCO nor a JPEG encoder.

    python tools/make_jpeg_dataset.py OUT --copies 8 [--fixtures scene_420,photo_000000130566] [--seed 0] [--max-objects 6]

Writes ``OUT/images/<12-digit id>.jpg`` (copies of the fixtures, in turn) and ``OUT/COCO_24p_label/<id>.txt`` (rows of a class and
50 coordinates normalised by width / height: centre, then 24 points every 15 degrees - the format ``labels_create_24p.py`` writes).
Every fifth label file is empty: an image without objects.
"""
import argparse
import json
import math
import os
import shutil
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURES = os.path.join(ROOT, "tests", "golden", "jpeg")
DEFAULT = ("scene_420", "scene_420_rst", "q90_444_33x50", "q90_422_33x50", "q90_420_17x23", "grey_q80_33x50", "flat_q100_420_24x40",
           "q75rst_420_33x50")


def label_rows(rs, count, h, w, num_classes=80):
    rows = np.zeros((count, 51), dtype=np.float64)
    ang = np.arange(24) * (15.0 * math.pi / 180.0)
    for i in range(count):
        cx, cy = rs.uniform(0.25, 0.75) * w, rs.uniform(0.25, 0.75) * h
        r = rs.uniform(0.05, 0.2, 24) * min(h, w)
        rows[i, 0] = rs.randint(0, num_classes)
        rows[i, 1], rows[i, 2] = cx / w, cy / h
        rows[i, 3::2] = np.clip((cx + r * np.cos(ang)) / w, 0.0, 1.0)
        rows[i, 4::2] = np.clip((cy + r * np.sin(ang)) / h, 0.0, 1.0)
    return rows


def make(out, copies, names=DEFAULT, seed=0, max_objects=6, fixtures=FIXTURES):
    """-> list of (id, fixture name, label rows)"""
    with open(os.path.join(fixtures, "cases.json")) as fh:
        cases = {c["name"]: c for c in json.load(fh)}
    img_dir, lab_dir = os.path.join(out, "images"), os.path.join(out, "COCO_24p_label")
    os.makedirs(img_dir, exist_ok=True)
    os.makedirs(lab_dir, exist_ok=True)
    rs = np.random.RandomState(seed)
    made = []
    for k in range(copies):
        name = names[k % len(names)]
        c = cases[name]
        stem = "%012d" % (k + 1)
        shutil.copyfile(os.path.join(fixtures, name + ".jpg"), os.path.join(img_dir, stem + ".jpg"))
        count = 0 if k % 5 == 4 else int(rs.randint(1, max_objects + 1))
        rows = label_rows(rs, count, c["height"], c["width"])
        with open(os.path.join(lab_dir, stem + ".txt"), "w") as fh:
            for row in rows:
                fh.write(" ".join(["%d" % row[0]] + ["%.17g" % v for v in row[1:]]) + "\n")
        made.append((k + 1, name, rows))
    return made


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("out")
    ap.add_argument("--copies", type=int, default=8)
    ap.add_argument("--fixtures", default=",".join(DEFAULT), help="comma-separated fixture names of tests/golden/jpeg/cases.json")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--max-objects", type=int, default=6)
    a = ap.parse_args()
    m = make(a.out, a.copies, tuple(a.fixtures.split(",")), a.seed, a.max_objects)
    print("%d images in %s" % (len(m), a.out))
    sys.exit(0)
