"""ep24.segmeval without a GPU: the grouping plan (group order, the cut at the largest maxDets, score_rank, dropped foreign ids,
chunks on image boundaries), the ValueErrors of malformed files and records, the summary's format, and the ABI: include/ep24.h
declares every ep24_segm_* entry point and ep24._lib binds it (tests/test_abi.py then checks declared against exported)."""
import json

import numpy as np
import pytest

import segmeval_oracle as ora
from ep24 import _lib, segmeval

ENTRY_POINTS = ("ep24_segm_mask_stats", "ep24_segm_iou", "ep24_segm_match", "ep24_segm_accumulate")


def rle(h, w, runs):
    assert sum(runs) == h * w
    return {"size": [h, w], "counts": list(runs)}


def tiny_gt():
    """Images 30 (8 x 6), 10 (4 x 4), 20 (5 x 7) - out of order on purpose - and categories 9, 3."""
    return {"images": [{"id": 30, "height": 8, "width": 6}, {"id": 10, "height": 4, "width": 4}, {"id": 20, "height": 5, "width": 7}],
            "categories": [{"id": 9}, {"id": 3}],
            "annotations": [{"id": 1, "image_id": 30, "category_id": 3, "segmentation": rle(8, 6, [4, 10, 34]), "area": 10.0, "iscrowd": 0},
                            {"id": 2, "image_id": 10, "category_id": 9, "segmentation": rle(4, 4, [0, 16]), "area": 16.0, "iscrowd": 1},
                            {"id": 3, "image_id": 30, "category_id": 3, "segmentation": [[0, 0, 3, 0, 3, 3, 0, 3]], "area": 9.0, "ignore": 1},
                            {"id": 4, "image_id": 10, "category_id": 3, "segmentation": rle(4, 4, [5, 3, 8]), "area": 3.0}]}


def res(image_id, category_id, score, h, w):
    return {"image_id": image_id, "category_id": category_id, "score": score, "segmentation": rle(h, w, [1, 2, h * w - 3])}


def test_load_gt_tables():
    t = segmeval.load_gt(tiny_gt())
    assert t["img_ids"] == [10, 20, 30] and t["cat_ids"] == [3, 9]
    assert t["sizes"].tolist() == [[4, 4], [5, 7], [8, 6]]
    assert t["img"].tolist() == [2, 0, 2, 0] and t["cat"].tolist() == [0, 1, 0, 0]
    assert t["crowd"].tolist() == [0, 1, 0, 0] and t["ignore0"].tolist() == [0, 1, 1, 0]            # ignore OR iscrowd
    assert t["area"].tolist() == [10.0, 16.0, 9.0, 3.0]


def test_plan_group_order_cut_rank_and_drops(tmp_path):
    gt = segmeval.load_gt(tiny_gt())
    results = [res(30, 3, 0.5, 8, 6), res(99, 3, 0.9, 8, 6), res(20, 9, 0.25, 5, 7), res(30, 3, 0.75, 8, 6), res(30, 77, 0.9, 8, 6),
               res(30, 3, 0.5, 8, 6), res(20, 9, 0.25 + 1e-12, 5, 7), res(30, 3, 0.125, 8, 6)]
    p = segmeval.build_plan(gt, results, 3)
    # groups: image-major in the order of the sorted ids, then category; every pair with a GT or a kept result
    assert p["groups"].tolist() == [[0, 0], [0, 1], [1, 1], [2, 0]]
    assert p["G"].tolist() == [1, 1, 0, 2] and p["D"].tolist() == [0, 0, 2, 3]
    assert p["gt_ann"].tolist() == [3, 1, 0, 2] and p["gt_first"].tolist() == [0, 1, 2, 2]
    # results: score descending, input order on ties, cut at 3 (the 0.125 goes); the foreign image 99 and category 77 are dropped
    assert p["dt_res"].tolist() == [6, 2, 3, 0, 5] and p["dt_first"].tolist() == [0, 0, 0, 2]
    assert p["dropped"] == 2
    # dense ranks of the float64 scores: 0.75 -> 0, 0.5 -> 1 (twice), 0.25 + 1e-12 -> 2, 0.25 -> 3, though fp32 cannot tell the last two apart
    assert p["score_rank"].tolist() == [2, 3, 0, 1, 1] and p["score_rank"].dtype == np.int32
    assert np.float32(0.25 + 1e-12) == np.float32(0.25)
    assert p["score_rank"].tolist() == ora.score_ranks(p["score"]).tolist()
    # the cut at 100 of the default maxDets
    many = [res(20, 9, 1.0 - 0.001 * k, 5, 7) for k in range(130)]
    p = segmeval.build_plan(gt, many, 100)
    assert p["D"].tolist() == [0, 0, 100, 0] and p["dt_res"].tolist() == list(range(100))
    # an evaluator takes a list, a path and an object with .records, and adds them up
    ev = segmeval.SegmEvaluator(tiny_gt())
    path = tmp_path / "dt.json"
    path.write_text(json.dumps(results))

    class Holder:
        records = results
    assert ev.add_results(results) == 8 and ev.add_results(str(path)) == 8 and ev.add_results(Holder()) == 8
    assert len(ev.results) == 24


def test_chunks_end_on_image_boundaries():
    gt = segmeval.load_gt(tiny_gt())
    results = [res(30, 3, 0.5, 8, 6), res(20, 9, 0.25, 5, 7), res(10, 9, 0.75, 4, 4)]
    p = segmeval.build_plan(gt, results, 100)
    assert p["groups"].tolist() == [[0, 0], [0, 1], [1, 1], [2, 0]]
    sizes = gt["sizes"]                                    # bytes per image: 3 * 16, 1 * 35, 3 * 48
    assert segmeval.plan_chunks(p, sizes, 1 << 30) == [(0, 4)]
    assert segmeval.plan_chunks(p, sizes, 1) == [(0, 2), (2, 3), (3, 4)]
    assert segmeval.plan_chunks(p, sizes, 48 + 35) == [(0, 3), (3, 4)]
    assert segmeval.plan_chunks(p, sizes, 48 + 34) == [(0, 2), (2, 3), (3, 4)]
    assert segmeval.plan_chunks(segmeval.build_plan(gt, [], 100), sizes, 1 << 30) == [(0, 3)]          # GT-only groups still count


def test_value_errors(tmp_path):
    gt = tiny_gt()
    for key in ("images", "annotations", "categories"):
        bad = {k: v for k, v in gt.items() if k != key}
        with pytest.raises(ValueError):
            segmeval.SegmEvaluator(bad)
    for key in ("image_id", "category_id", "segmentation", "area"):
        bad = json.loads(json.dumps(gt))
        del bad["annotations"][0][key]
        with pytest.raises(ValueError):
            segmeval.SegmEvaluator(bad)
    bad = json.loads(json.dumps(gt))
    bad["annotations"][0]["segmentation"]["size"] = [6, 8]                  # not the image's 8 x 6
    with pytest.raises(ValueError):
        segmeval.SegmEvaluator(bad)
    bad = json.loads(json.dumps(gt))
    bad["annotations"][0]["image_id"] = 12345
    with pytest.raises(ValueError):
        segmeval.SegmEvaluator(bad)
    path = tmp_path / "broken.json"
    path.write_text("{not json")
    with pytest.raises(ValueError):
        segmeval.SegmEvaluator(str(path))
    ev = segmeval.SegmEvaluator(gt)
    for key in ("image_id", "category_id", "segmentation", "score"):
        r = res(30, 3, 0.5, 8, 6)
        del r[key]
        with pytest.raises(ValueError):
            ev.add_results([r])
    with pytest.raises(ValueError):
        ev.add_results([res(30, 3, 0.5, 6, 8)])                             # a segmentation whose size is not the image's
    with pytest.raises(ValueError):
        ev.add_results([res(30, 3, float("nan"), 8, 6)])
    with pytest.raises(ValueError):
        ev.add_results({"image_id": 30})
    assert ev.results == []                                                 # a refused batch leaves nothing behind
    assert ev.add_results([res(99, 3, 0.5, 1, 1)]) == 1                     # a foreign image is dropped later, not an error
    with pytest.raises(_lib.Ep24Error):
        segmeval.SegmEvaluator(gt, max_dets=(1, 10, 129))
    with pytest.raises(_lib.Ep24Error):
        segmeval.SegmEvaluator(gt, max_dets=(1, 2, 3, 4, 5))
    with pytest.raises(_lib.Ep24Error):
        segmeval.SegmEvaluator(gt, area_ranges=[(0, 1)] * 5)


def test_no_cpu_fallback():
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    ev = segmeval.SegmEvaluator(tiny_gt())
    ev.add_results([res(30, 3, 0.5, 8, 6)])
    with pytest.raises(_lib.Ep24Error):
        ev.evaluate()


def test_summary_format_equals_the_oracle():
    rng = np.random.RandomState(3)
    precision = rng.rand(10, 101, 3, 4, 3)
    recall = rng.rand(10, 3, 4, 3)
    precision[:, :, 1] = -1
    recall[:, 1] = -1
    precision[:, :, :, 1] = -1                                              # no small objects at all: -1.000
    recall[:, :, 1] = -1
    stats, lines = segmeval.summarize_tables(precision, recall, [1, 10, 100])
    want_stats, want_lines = ora.summarize(precision, recall)
    assert stats == want_stats and lines == want_lines and len(lines) == 12
    assert lines[3] == " Average Precision  (AP) @[ IoU=0.50:0.95 | area= small | maxDets=100 ] = -1.000"
    assert np.array_equal(segmeval.IOU_THRS, ora.IOU_THRS) and np.array_equal(segmeval.REC_THRS, ora.REC_THRS)
    assert np.array_equal(np.array(segmeval.AREA_RANGES, dtype=np.float64), np.array(ora.AREA_RANGES, dtype=np.float64))


def test_header_declares_and_lib_binds_the_entry_points():
    protos = _lib.parse_header()
    for name in ENTRY_POINTS:
        assert name in protos, name
    assert [t for t, _ in protos["ep24_segm_mask_stats"][1]] == ["const uint32_t*", "const int64_t*", "int", "int32_t*", "int32_t*", "void*"]
    assert [n for _, n in protos["ep24_segm_iou"][1]] == ["bits", "tab", "N", "bbox", "area", "gt_crowd", "grp", "J", "pairs", "iou", "inter",
                                                          "stream"]
    assert len(protos["ep24_segm_match"][1]) == 18 and len(protos["ep24_segm_accumulate"][1]) == 17
    L = _lib.lib()
    for name in ENTRY_POINTS:
        assert name in L.fn and len(L.fn[name].argtypes) == len(protos[name][1]), name
    assert L.fn["ep24_abi_version"]() == 3                                  # entry points were only added
