"""Hand-computed cases that pin the evaluation oracle (tests/eval24_oracle.py) to the pycocotools semantics."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import eval24_oracle as O  # noqa: E402


def img(gt_cls, det_cls, det_score, iou):
    return {"gt_cls": np.array(gt_cls, dtype=np.int64), "det_cls": np.array(det_cls, dtype=np.int64),
            "det_score": np.array(det_score, dtype=np.float32), "iou": np.array(iou, dtype=np.float64).reshape(len(gt_cls), len(det_cls))}


def ap(res, k=None):
    s = O.summarize(res["precision"], res["recall"])
    return s["AP"] if k is None else s["per_class_AP"][k]


def test_one_perfect_detection():
    r = O.evaluate([img([0], [0], [0.9], [[1.0]])], 1)
    assert abs(ap(r) - 1.0) < 1e-12                       # pr = 1 / (1 + eps): pycocotools' 0.9999999999999998
    assert r["records"][0][-1] == 0x3FF


def test_fp_above_tp_is_exactly_half():
    r = O.evaluate([img([0], [0, 0], [0.9, 0.8], [[0.0, 1.0]])], 1)
    assert ap(r) == 0.5
    assert np.all(r["precision"] == 0.5)


def test_one_tp_two_gts():
    r = O.evaluate([img([0, 0], [0], [0.9], [[1.0], [0.0]])], 1)
    assert abs(ap(r) - 51 / 101) < 1e-12
    assert np.all(r["recall"] == 0.5)


def test_class_with_gt_and_no_detection_is_zero_and_class_without_gt_is_excluded():
    r = O.evaluate([img([0], [1], [0.9], [[0.0]])], 3)
    assert ap(r, 0) == 0.0 and np.all(r["recall"][:, 0] == 0)
    assert ap(r, 1) == -1.0 and np.all(r["precision"][:, :, 1] == -1) and np.all(r["recall"][:, 1] == -1)
    assert ap(r, 2) == -1.0
    assert ap(r) == 0.0


def test_detection_beyond_max_dets_is_ignored():
    # 100 FPs above the one TP: the TP is the 101st detection of its class and never counts
    D = 101
    iou = np.zeros((1, D))
    iou[0, D - 1] = 1.0
    scores = np.linspace(0.99, 0.5, D).astype(np.float32)
    r = O.evaluate([img([0], [0] * D, scores, iou)], 1)
    assert len(r["records"]) == 100 and ap(r) == 0.0
    r = O.evaluate([img([0], [0] * D, scores, iou)], 1, max_dets=101)
    assert ap(r) > 0.0


def test_iou_exactly_at_the_threshold_counts():
    r = O.evaluate([img([0], [0], [0.9], [[0.75]])], 1)
    assert r["records"][0][-1] == 0b111111                 # thresholds 0.50 .. 0.75 (np.linspace value of 0.75 is exact)
    r = O.evaluate([img([0], [0], [0.9], [[np.nextafter(0.75, 0)]])], 1)
    assert r["records"][0][-1] == 0b11111


def test_equal_iou_goes_to_the_later_gt():
    # the first detection has IoU 0.72 with both GTs: it takes GT 1 (the later row) at 0.50 .. 0.70; the second detection
    # overlaps GT 1 only (0.92), so it finds GT 1 taken there and matches at 0.75 .. 0.90.  Had GT 0 won the tie, the second
    # detection would match at 0.50 .. 0.90.
    iou = [[0.72, 0.0], [0.72, 0.92]]
    r = O.evaluate([img([0, 0], [0, 0], [0.9, 0.8], iou)], 1)
    assert [rec[-1] for rec in r["records"]] == [0b0000011111, 0b0111100000]


def test_score_ties_keep_image_then_p_order():
    a = img([0], [0, 0], [0.5, 0.5], [[0.0, 1.0]])          # p 0 is the FP, p 1 the TP
    b = img([0], [0], [0.5], [[1.0]])
    r = O.evaluate([a, b], 1)
    order = [(rec[2], rec[3]) for rec in r["records"]]     # (seq, p)
    assert order == [(0, 0), (0, 1), (1, 0)]
    # FP first, then two TPs: pr = 0, 1/2, 2/3 -> envelope 2/3 everywhere up to recall 1
    assert abs(r["precision"][0, 0, 0] - 2 / 3) < 1e-15
    r2 = O.evaluate([b, a], 1)
    assert [(rec[2], rec[3]) for rec in r2["records"]] == [(0, 0), (1, 0), (1, 1)]
    assert abs(r2["precision"][0, 0, 0] - 1.0) < 1e-15


def test_oracle_ious():
    from ep24 import synth
    lab = synth.make_labels(1, 4, size=320, seed=5)[0, :4].numpy()
    gt50 = lab[:, 1:]
    r = O._gt_radii(gt50)
    det = np.concatenate([gt50[:, :2], r], 1)
    ci = O.iou_circle24(gt50, det)
    assert np.all(np.abs(np.diag(ci) - 1.0) < 1e-5)
    ri = O.iou_rect(gt50, det)
    assert ri.dtype == np.float64 and np.all(np.diag(ri) > 0.9)
    assert np.all((ci >= 0) & (ci <= 1.0 + 1e-6))
