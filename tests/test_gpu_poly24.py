"""The "poly24" IoU type of the evaluator (csrc/poly24.h in csrc/evaluate.hip) against the numpy oracle
(tests/poly24_oracle.py): the IoU matrix to 1e-9, and matching / accumulation bit-equal to tests/eval24_oracle.py fed with
the kernel's own matrices, as tests/test_gpu_eval24.py does for the other two types."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import eval24_oracle as O  # noqa: E402
import poly24_oracle as P  # noqa: E402
import test_gpu_eval24 as T  # noqa: E402
from ep24 import evaluate as E, infer, synth  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _gt_row(poly, cx, cy):
    return np.concatenate([[cx, cy], np.asarray(poly, dtype=np.float32).reshape(-1)]).astype(np.float32)


def _det_row(cx, cy, r):
    return np.concatenate([[cx, cy], np.broadcast_to(np.asarray(r, dtype=np.float64), (24,))]).astype(np.float32)


def _pairwise_inputs():
    """50 GT rows x 200 detections as test_pairwise_iou_against_the_oracle builds them (jittered copies of the GTs plus random
    rows), the last rows replaced by the analytic cases."""
    lab = synth.make_labels(2, 25, size=640, seed=11).reshape(-1, 51)[:, 1:].numpy()
    gt50 = lab[:50].copy()
    det = synth.decode_head(synth.make_raw_head(1, 640, seed=12))[0, :200, :26].numpy().copy()
    det[:50] = T._det26_from_gt(gt50) * np.float32(1.02)
    det[:50, :2] = gt50[:, :2] + 3.0
    # analytic GTs: a regular 24-gon, three squares, a duplicate's original
    gt50[45] = _gt_row(P.regular(300.0, 200.0, 40.0), 300.0, 200.0)
    gt50[46] = _gt_row(P.regular(100.0, 500.0, P.square_radii(16.0)), 100.0, 500.0)
    gt50[47] = _gt_row(P.square64(400.0, 420.0, 8.0), 400.0, 420.0)              # vertices exactly on the square
    dup = _det_row(520.25, 310.5, np.random.default_rng(7).uniform(10.0, 30.0, 24))
    gt50[48] = _gt_row(P.det_polygons(dup[None])[0], dup[0], dup[1])
    gt50[49] = _gt_row(P.regular(50.0, 50.0, 12.0)[::-1], 50.0, 50.0)            # clockwise
    det[190] = _det_row(300.0, 200.0, 10.0)                                      # concentric in gt 45: (10 / 40)^2
    det[191] = _det_row(300.0, 200.0, 80.0)                                      # around it: (40 / 80)^2
    det[192] = _det_row(110.0, 505.0, P.square_radii(16.0))                      # squares: the rectangle formula
    det[193] = _det_row(416.0, 420.0, P.square_radii(8.0))                       # shares (to fp32 rounding) the edge x = 408 of gt 47
    det[194] = _det_row(440.0, 420.0, P.square_radii(8.0))                       # disjoint from it
    det[195] = dup                                                               # exact duplicate of gt 48
    det[196] = dup
    det[196, 7] = np.nan                                                         # a NaN radius
    det[197] = _det_row(50.0, 50.0, 12.0)                                        # gt 49 in the other orientation
    det[198] = _det_row(300.0, 200.0, 0.0)                                       # a point
    return gt50, det


def test_pairwise_poly24_against_the_oracle():
    gt50, det = _pairwise_inputs()
    got = E.pairwise_iou(torch.from_numpy(gt50).to(DEV), torch.from_numpy(det).to(DEV), "poly24").cpu().numpy()
    want = P.iou_poly24(gt50, det)
    assert got.shape == want.shape == (50, 200) and got.dtype == np.float64
    nan = np.isnan(want)
    assert nan[:, 196].all() and nan.sum() == 50
    assert np.array_equal(np.isnan(got), nan)
    diff = float(np.abs(got - want)[~nan].max())
    print("poly24 pairwise_iou vs oracle: max |diff| = %.3e over %d pairs, %d of them overlapping" % (diff, (~nan).sum(), (want > 0).sum()))
    assert diff <= 1e-9
    # pairs whose vertex boxes do not overlap are exactly 0.0
    gb, db = O.gt_boxes(gt50).astype(np.float64), O.det_boxes(det).astype(np.float64)
    w = np.minimum(gb[:, None, 2], db[None, :, 2]) - np.maximum(gb[:, None, 0], db[None, :, 0])
    h = np.minimum(gb[:, None, 3], db[None, :, 3]) - np.maximum(gb[:, None, 1], db[None, :, 1])
    disjoint = ~((w > 0) & (h > 0)) & ~nan
    assert disjoint.sum() > 1000 and np.all(got[disjoint] == 0.0)
    assert got[47, 194] == 0.0 and got[45, 198] == 0.0
    # the analytic cases (fp32 vertices: the closed forms hold to fp32 rounding, the oracle to 1e-9)
    assert abs(got[45, 190] - (10.0 / 40.0) ** 2) <= 1e-6 and abs(got[45, 191] - (40.0 / 80.0) ** 2) <= 1e-6
    assert abs(got[46, 192] - P.rect_iou((84.0, 484.0, 116.0, 516.0), (94.0, 489.0, 126.0, 521.0))) <= 1e-5
    assert got[47, 193] <= 1e-6
    assert abs(got[48, 195] - 1.0) <= 1e-9 and abs(got[49, 197] - 1.0) <= 1e-9
    assert float(np.nanmax(got)) <= 1.0 and float(np.nanmin(got)) >= 0.0
    assert (got[:25, :25].diagonal() > 0.5).all()                                # the 25 real GT rows against their jittered copies


def test_pairwise_poly24_empty_sides():
    g = torch.zeros(0, 50, device=DEV)
    d = torch.rand(3, 26, device=DEV)
    assert tuple(E.pairwise_iou(g, d, "poly24").shape) == (0, 3)
    assert tuple(E.pairwise_iou(torch.rand(2, 50, device=DEV), d[:0], "poly24").shape) == (2, 0)


def test_random_scenes_poly24_bit_equal_to_the_oracle():
    C = 80
    labels, dets = T.make_scenes(16, C, seed=31)
    ev, st = T.run_gpu(labels, dets, C, "poly24", [16])
    want = O.evaluate(T.oracle_images(labels, dets, "poly24"), C)
    T.check_against_oracle(ev, st, want, C)
    assert 0.0 < st["AP"] < 1.0 and st["AP50"] > st["AP"]
    _, st4 = T.run_gpu(labels, dets, C, "poly24", [4, 4, 4, 4])
    assert np.array_equal(st4["precision"], st["precision"]) and np.array_equal(st4["recall"], st["recall"])


@pytest.mark.parametrize("iou_type", ["circle24", "rect"])
def test_other_types_undisturbed_by_the_wider_geometry(iou_type):
    C = 80
    labels, dets = T.make_scenes(16, C, seed=31)
    ev, st = T.run_gpu(labels, dets, C, iou_type, [16])
    T.check_against_oracle(ev, st, O.evaluate(T.oracle_images(labels, dets, iou_type), C), C)
    _, st4 = T.run_gpu(labels, dets, C, iou_type, [4, 4, 4, 4])
    assert np.array_equal(st4["precision"], st["precision"]) and np.array_equal(st4["recall"], st["recall"])


def test_update_equals_update_detections_of_postprocess_poly24():
    B, S, C = 2, 320, 80
    pred = synth.decode_head(synth.make_raw_head(B, S, seed=21, num_classes=C), S)
    pred[..., 26:] = torch.sigmoid(pred[..., 26:])
    pred = pred.to(DEV)
    labels = synth.make_labels(B, [6, 12], size=S, seed=22).to(DEV)
    a = E.Evaluator24(C, iou_type="poly24")
    a.update(pred, labels)
    b = E.Evaluator24(C, iou_type="poly24")
    b.update_detections(infer.postprocess(pred, C, conf_thre=0.01, nms_thre=0.65), labels)
    sa, sb = a.summarize(), b.summarize()
    assert a.n_records == b.n_records > 0
    ra, rb = a.records(), b.records()
    for k in ra:
        assert np.array_equal(ra[k], rb[k]), k
    assert np.array_equal(sa["precision"], sb["precision"]) and np.array_equal(sa["recall"], sb["recall"])
    assert sa["iou_type"] == "poly24"


def test_exp_eval_poly24_equals_the_decomposed_path():
    from ep24.input import TrainTransform
    exp = T._small_exp()
    exp.eval_iou_type = "poly24"
    torch.manual_seed(0)
    model = exp.get_model().to(DEV)
    ev = exp.get_evaluator(4)
    assert ev.iou_type == "poly24"
    ap, ap50, summary = exp.eval(model, ev, False)
    assert model.training and "Average Precision" in summary
    ref = E.Evaluator24(exp.num_classes, iou_type="poly24", conf_thre=exp.test_conf, nms_thre=exp.nmsthre)
    model.eval()
    tt = TrainTransform(max_labels=50)
    with torch.no_grad():
        for images, targets, _, _ in exp.get_eval_loader(4):
            imgs, labs = tt.batch(images, targets, (320, 320))
            eng = model.engine(imgs.shape[0], 320)
            ref.update(eng.forward_eval(imgs), labs)
    st = ref.summarize()
    model.train()
    assert ref.seq == 10 and ev.seq == 10
    assert np.all(np.isfinite(ev.stats["precision"])) and np.all(np.isfinite(ev.stats["recall"]))
    assert np.array_equal(st["precision"], ev.stats["precision"]) and np.array_equal(st["recall"], ev.stats["recall"])
    assert (ap, ap50) == (st["AP"], st["AP50"]) and np.isfinite(ap) and np.isfinite(ap50)
