"""Pins tests/boundary_oracle.py, the numpy restatement of Boundary IoU that ep24_mask_boundary and
``SegmEvaluator(iou_type="boundary")`` are tested against: the iterated 3 x 3 erosion against the square-window definition and
against scipy, hand cases, the radius formula, and the evaluation of the segm evaluator's own scene with the boundary IoU."""
import functools

import numpy as np
import pytest

import boundary_oracle as bo
import cocomask_oracle as cmo
import segmeval_oracle as ora


def window_erode(m, d):
    """The definition: pixel (x, y) iff every pixel of its (2d + 1) x (2d + 1) neighbourhood is set, outside the image unset."""
    H, W = m.shape
    out = np.zeros((H, W), dtype=bool)
    for y in range(H):
        for x in range(W):
            ok = True
            for yy in range(y - d, y + d + 1):
                for xx in range(x - d, x + d + 1):
                    if yy < 0 or yy >= H or xx < 0 or xx >= W or not m[yy, xx]:
                        ok = False
            out[y, x] = ok
    return out


def random_masks():
    rng = np.random.RandomState(3)
    return [rng.rand(H, W) < p for (H, W) in ((1, 1), (7, 9), (12, 33), (20, 17)) for p in (0.5, 0.9, 0.98, 1.0)]


@pytest.mark.parametrize("d", (1, 2, 5))
def test_erode_equals_the_window_definition(d):
    nonempty = 0
    for m in random_masks():
        got = bo.erode(m, d)
        assert np.array_equal(got, window_erode(m, d)), (m.shape, d)
        nonempty += int(got.any())
    assert nonempty > 0 or d == 5
    assert bo.erode(np.ones((20, 17), dtype=bool), d).sum() == (20 - 2 * d) * (17 - 2 * d)


def test_erode_equals_scipy():
    ndimage = pytest.importorskip("scipy.ndimage")
    for m in random_masks():
        for d in (1, 2, 5):
            want = ndimage.binary_erosion(m, np.ones((3, 3), dtype=bool), iterations=d, border_value=0)
            assert np.array_equal(bo.erode(m, d), want), (m.shape, d)


def test_hand_cases():
    full = np.ones((5, 7), dtype=bool)
    frame = full.copy()
    frame[1:4, 1:6] = False
    assert np.array_equal(bo.boundary(full, 1), frame)
    for d in (3, 4, 100):
        assert np.array_equal(bo.boundary(full, d), full)
    assert bo.boundary(full, 2).sum() == 35 - 3                                     # the middle row's three inner pixels survive d = 2
    one = np.zeros((5, 7), dtype=bool)
    one[2, 3] = True
    assert np.array_equal(bo.boundary(one, 1), one)
    assert not bo.boundary(np.zeros((5, 7), dtype=bool), 1).any()
    for m in random_masks():
        b = bo.boundary(m, 2)
        assert not (b & ~m).any()


def test_dilation_formula():
    assert bo.dilation(427, 640, 0.02) == 15
    assert bo.dilation(427, 640, 0.05) == 38
    assert bo.dilation(33, 31, 0.02) == 1
    assert bo.dilation(64, 65, 0.02) == 2
    assert bo.dilation(427, 640) == 15
    assert bo.dilation(3, 4, 0.5) == 2                                              # 2.5 rounds half to even


# ------------------------------------------------------------------------------------------------- the evaluator's scene
@functools.lru_cache(maxsize=None)
def dataset_masks():
    """``dataset()`` of tests/test_gpu_segmeval.py with its grouping repeated and the masks kept: (gt, res, want of "segm",
    groups = [(image height, width, oracle group without "iou", detection masks, GT masks)])."""
    from test_gpu_segmeval import dataset
    gt, res, want = dataset()
    sizes = {im["id"]: (im["height"], im["width"]) for im in gt["images"]}
    img_ids, cat_ids = sorted(sizes), sorted(c["id"] for c in gt["categories"])
    mask = lambda seg, i: np.array(cmo.ann_to_mask(seg, *sizes[i]), dtype=bool)
    groups = []
    for seq, i in enumerate(img_ids):
        for k, c in enumerate(cat_ids):
            G = [a for a in gt["annotations"] if a["image_id"] == i and a["category_id"] == c]
            D = [r for r in res if r["image_id"] == i and r["category_id"] == c]
            if not G and not D:
                continue
            D = sorted(D, key=lambda r: -r["score"])[:100]
            dm, gm = [mask(r["segmentation"], i) for r in D], [mask(a["segmentation"], i) for a in G]
            crowd = [int(a.get("iscrowd", 0)) for a in G]
            groups.append((sizes[i][0], sizes[i][1],
                           {"cls": k, "seq": seq, "gt_crowd": crowd,
                            "gt_ignore0": [int(bool(a.get("ignore", 0)) or bool(a.get("iscrowd", 0))) for a in G],
                            "gt_area": [float(a["area"]) for a in G], "dt_area": [float(m.sum()) for m in dm],
                            "dt_score": [r["score"] for r in D]}, dm, gm))
    return gt, res, want, groups


@functools.lru_cache(maxsize=None)
def boundary_want(ratio):
    """-> (the oracle's evaluation with the boundary IoU at ``ratio``, [(mask IoU, boundary IoU) per group])."""
    gt, res, want, groups = dataset_masks()
    out, ious = [], []
    for h, w, g, dm, gm in groups:
        _, iou_mask = ora.mask_iou(dm, gm, g["gt_crowd"])
        iou = bo.boundary_iou(dm, gm, g["gt_crowd"], bo.dilation(h, w, ratio))
        out.append(dict(g, iou=iou))
        ious.append((iou_mask, iou))
    return ora.evaluate(out, len(gt["categories"])), ious


def test_the_scene_scores_lower_by_its_boundaries():
    gt, res, want, groups = dataset_masks()
    # the grouping repeated here is dataset()'s: with the mask IoU it gives dataset()'s tables
    segm = ora.evaluate([dict(g, iou=ora.mask_iou(dm, gm, g["gt_crowd"])[1]) for _, _, g, dm, gm in groups], len(gt["categories"]))
    assert segm[0] == want[0] and np.array_equal(segm[2], want[2]) and np.array_equal(segm[3], want[3])
    (stats, lines, precision, recall, _), ious = boundary_want(0.02)
    assert len(stats) == 12 and all(a != b for a, b in zip(stats, want[0]))
    assert 0 < stats[0] < want[0][0]
    assert round(stats[0], 4) == 0.3386 and round(want[0][0], 4) == 0.8442
    assert all((b <= m).all() for m, b in ious)
    # the min matters in both directions: somewhere the band IoU alone is above the mask IoU
    above = 0
    for h, w, g, dm, gm in groups:
        d = bo.dilation(h, w, 0.05)
        _, iou_mask = ora.mask_iou(dm, gm, g["gt_crowd"])
        _, iou_band = ora.mask_iou([bo.boundary(m, d) for m in dm], [bo.boundary(m, d) for m in gm], g["gt_crowd"])
        above += int((iou_band > iou_mask).sum())
    assert above > 0
