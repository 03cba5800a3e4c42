"""tests/segmeval_oracle.py against the reference's own COCOevalEvaluateImages / COCOevalAccumulate on a recorded scene.

tests/golden/segmeval_scene.json holds the scene (3 classes, 6 images, built once from a fixed seed: GT and detection ids from 1,
the IoU blocks of rectangles as the oracle's ``mask_iou`` gives them) and, under ``reference_evaluations``, what the reference's
EvaluateImages returned for it per (class, area range, image); segmeval_ref_precision.npy / segmeval_ref_recall.npy are its
Accumulate tables.  The scene holds a crowd GT matched by several detections, a GT with ``ignore``, GT areas exactly at 32^2 and
96^2, two GTs with equal IoU to one detection, equal scores inside a group and across images, two scores that differ only below
fp32 resolution, an unmatched detection outside each area range, a class without GT, an image without detections and a group of
101 detections.

Matches, ignore flags and recall are compared bit for bit.  Precision: the reference forms ``tp / (tp + fp)`` (0 for 0 / 0), the
COCO API and the kernels ``tp / (fp + tp + eps)``.  The two are the same double except where tp + fp == 1, so the oracle is
compared twice: in the reference's form (``eps=None``) the whole table is bit-equal, and in the API's form every entry is
bit-equal except those the reference gives as exactly 1.0, which the API's form gives as 1 / (1 + eps)."""
import functools
import json
import os

import numpy as np

import segmeval_oracle as ora

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@functools.lru_cache(maxsize=None)
def scene():
    with open(os.path.join(GOLDEN, "segmeval_scene.json")) as f:
        return json.load(f)


@functools.lru_cache(maxsize=None)
def scene_groups():
    """The scene as oracle groups (detections in score order, cut at the largest maxDets) -> (groups, gt ids, dt ids per group)."""
    sc = scene()
    cut = max(sc["max_dets"])
    groups, gt_ids, dt_ids = [], [], []
    for g in sc["groups"]:
        order = sorted(range(len(g["dt"])), key=lambda j: -g["dt"][j]["score"])[:cut]          # stable: input order on ties
        G = len(g["gt"])
        groups.append({"cls": g["cls"], "seq": g["img"], "iou": np.array(g["iou"], dtype=np.float64).reshape(len(order), G),
                       "gt_crowd": [int(o["iscrowd"]) for o in g["gt"]],
                       "gt_ignore0": [int(bool(o["ignore"]) or bool(o["iscrowd"])) for o in g["gt"]],
                       "gt_area": [float(o["area"]) for o in g["gt"]],
                       "dt_area": [float(g["dt"][j]["area"]) for j in order],
                       "dt_score": [float(g["dt"][j]["score"]) for j in order]})
        gt_ids.append([o["id"] for o in g["gt"]])
        dt_ids.append([g["dt"][j]["id"] for j in order])
    return groups, gt_ids, dt_ids


@functools.lru_cache(maxsize=None)
def scene_records():
    """The oracle's records and tables of the scene, computed once and shared: (records, precision, recall)."""
    sc = scene()
    groups, _, _ = scene_groups()
    rec = ora.records(groups, sc["num_classes"], [tuple(r) for r in sc["area_ranges"]])
    precision, recall = ora.accumulate(rec, sc["num_classes"], tuple(sc["max_dets"]))
    return rec, precision, recall


def test_scene_holds_the_cases():
    sc = scene()
    groups, _, _ = scene_groups()
    assert sc["num_classes"] == 3 and sc["num_images"] == 6 and sc["max_dets"] == [1, 10, 100]
    assert min(o["id"] for g in sc["groups"] for o in g["gt"] + g["dt"]) == 1
    assert any(sum(g["gt_crowd"]) for g in groups) and any(o["ignore"] for g in sc["groups"] for o in g["gt"])
    areas = [a for g in groups for a in g["gt_area"]]
    assert 32.0 ** 2 in areas and 96.0 ** 2 in areas
    assert any(len(g["dt"]) == 101 for g in sc["groups"]) and max(len(g["dt_score"]) for g in groups) == 100
    assert not any(g["cls"] == 2 and g["gt_area"] for g in groups) and any(g["cls"] == 2 and g["dt_area"] for g in groups)
    assert not any(g["seq"] == 5 and g["dt_area"] for g in groups) and any(g["seq"] == 5 for g in groups)
    assert any(np.any((row[:, None] == row[None, :]) & (row[:, None] >= 0.5) & ~np.eye(len(row), dtype=bool))
               for g in groups for row in g["iou"])                                            # two GTs, one IoU
    scores = np.array([s for g in groups for s in g["dt_score"]])
    assert len(np.unique(scores)) < len(scores)                                               # equal scores
    assert len(np.unique(scores)) > len(np.unique(scores.astype(np.float32)))                 # apart in float64 only
    # a crowd GT matched by several detections
    e = ora.evaluate_img(groups[0], tuple(sc["area_ranges"][0]))
    crowd = groups[0]["gt_crowd"].index(1)
    assert int((e["dt_match"][0] == crowd).sum()) >= 3
    # an unmatched detection outside each range
    for a, r in enumerate(sc["area_ranges"]):
        assert any(np.any((ora.evaluate_img(g, tuple(r))["dt_match"][0] < 0) & ora.evaluate_img(g, tuple(r))["dt_ignore"][0])
                   for g in groups if g["seq"] == 1), a


def test_evaluate_img_equals_the_reference():
    sc = scene()
    groups, gt_ids, dt_ids = scene_groups()
    at = {(g["cls"], g["seq"]): n for n, g in enumerate(groups)}
    seen = 0
    for e in sc["reference_evaluations"]:
        n = at.get((e["cls"], e["img"]))
        if n is None:
            assert e["detection_matches"] == [] and e["ground_truth_ignores"] == [] and e["detection_scores"] == []
            continue
        g = groups[n]
        got = ora.evaluate_img(g, tuple(sc["area_ranges"][e["area"]]))
        ids = np.array(gt_ids[n] + [0])                                                       # -1 -> 0: the reference's "unmatched"
        assert ids[got["dt_match"]].reshape(-1).tolist() == e["detection_matches"], (e["cls"], e["area"], e["img"])
        assert got["dt_ignore"].reshape(-1).tolist() == e["detection_ignores"], (e["cls"], e["area"], e["img"])
        assert list(got["gt_ignore"]) == e["ground_truth_ignores"]
        assert [float(s) for s in g["dt_score"]] == e["detection_scores"]
        seen += 1
    assert seen == len(groups) * len(sc["area_ranges"])


def test_accumulate_equals_the_reference():
    sc = scene()
    rec, precision, recall = scene_records()
    want_p = np.load(os.path.join(GOLDEN, "segmeval_ref_precision.npy"))
    want_r = np.load(os.path.join(GOLDEN, "segmeval_ref_recall.npy"))
    assert precision.shape == want_p.shape == (10, 101, 3, 4, 3) and recall.shape == want_r.shape == (10, 3, 4, 3)
    assert np.array_equal(recall.view(np.int64), want_r.view(np.int64))
    # the reference's own precision expression: the whole table, bit for bit
    p0, r0 = ora.accumulate(rec, sc["num_classes"], tuple(sc["max_dets"]), eps=None)
    assert np.array_equal(p0.view(np.int64), want_p.view(np.int64)) and np.array_equal(r0.view(np.int64), want_r.view(np.int64))
    # the COCO API's expression: bit-equal except 1 / (1 + eps) where the reference holds exactly 1.0 (tp = 1, fp = 0)
    diff = precision.view(np.int64) != want_p.view(np.int64)
    assert diff.any() and np.all(want_p[diff] == 1.0) and np.all(precision[diff] == 1.0 / (1.0 + ora.EPS))
    assert (want_p == -1).any() and (want_p == 0).any() and ((want_p > 0) & (want_p < 1)).any()
    assert np.all(want_p[:, :, 2] == -1) and np.all(want_r[:, 2] == -1)                       # the class without GT


def test_summarize_lines():
    _, precision, recall = scene_records()
    stats, lines = ora.summarize(precision, recall)
    assert len(stats) == len(lines) == 12
    assert lines[0].startswith(" Average Precision  (AP) @[ IoU=0.50:0.95 | area=   all | maxDets=100 ] = ")
    assert lines[1].startswith(" Average Precision  (AP) @[ IoU=0.50      | area=   all | maxDets=100 ] = ")
    assert lines[6].startswith(" Average Recall     (AR) @[ IoU=0.50:0.95 | area=   all | maxDets=  1 ] = ")
    assert lines[11].startswith(" Average Recall     (AR) @[ IoU=0.50:0.95 | area= large | maxDets=100 ] = ")
    assert stats[0] == float(np.mean(precision[:, :, :, 0, 2][precision[:, :, :, 0, 2] > -1]))
    assert stats[1] == float(np.mean(precision[0, :, :, 0, 2][precision[0, :, :, 0, 2] > -1]))
    assert all(-1 <= s <= 1 for s in stats)
