"""The oracle of the stratified 24-point evaluation (tests/eval24_strata_oracle.py) against the two oracles it generalises, the
coverage of the shared scenes (tests/eval24_strata_scenes.py) asserted from the oracle alone, and the host API's argument errors.
No GPU."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import eval24_oracle as O  # noqa: E402
import eval24_strata_oracle as SO  # noqa: E402
import eval24_strata_scenes as SC  # noqa: E402
import segmeval_oracle as SEG  # noqa: E402
from ep24 import evaluate as E  # noqa: E402
from ep24._lib import Ep24Error  # noqa: E402

C = 120
_cache = {}


def scene_images(cfg):
    if cfg not in _cache:
        scene = SC.make_scene()
        strata, zones = SC.config(scene, cfg)
        _cache[cfg] = (scene, strata, SC.oracle_images(scene, zones, O.iou_rect))
    return _cache[cfg]


def test_one_stratum_equals_the_single_range_oracle():
    scene, strata, imgs = scene_images("all")
    got = SO.evaluate(imgs, C, SC.strata_rows(strata), (100,))
    want = O.evaluate(imgs, C, 100)
    rec, wr = got["records"], want["records"]
    assert len(wr) == len(rec["cls"]) > 200
    assert np.array_equal(rec["cls"], [r[0] for r in wr])
    assert np.array_equal(rec["score"].view(np.uint32), np.array([r[1] for r in wr], dtype=np.float32).view(np.uint32))
    assert np.array_equal(rec["seq"], [r[2] for r in wr]) and np.array_equal(rec["p"], [r[3] for r in wr])
    assert np.array_equal(rec["rank"], [r[4] for r in wr])
    assert np.array_equal(rec["m"][:, 0], [r[5] for r in wr])                  # no ignore bit anywhere: the word is the TP mask
    assert np.array_equal(got["npig"][:, 0], want["npig"])
    assert np.array_equal(got["precision"][:, :, :, 0, 0], want["precision"])
    assert np.array_equal(got["recall"][:, :, 0, 0], want["recall"])
    assert ((want["precision"] > 0) & (want["precision"] < 1)).any()


def test_coco_area_strata_equal_the_segm_oracle():
    scene, strata, imgs = scene_images("coco")
    rows = SC.strata_rows(strata)
    md = (1, 10, 100)
    got = SO.evaluate(imgs, C, rows, md)
    groups = []
    for seq, img in enumerate(imgs):
        for c in sorted(set(img["gt_cls"].tolist()) | set(img["det_cls"].tolist())):
            gs = np.nonzero(img["gt_cls"] == c)[0]
            ds = SO.class_dets(img, c, 100)
            groups.append({"cls": c, "seq": seq, "iou": img["iou"][np.ix_(gs, ds)].T.reshape(len(ds), len(gs)), "gt_crowd": [0] * len(gs),
                           "gt_ignore0": [0] * len(gs), "gt_area": img["gt_area"][gs], "dt_area": img["det_area"][ds],
                           "dt_score": img["det_score"][ds].astype(np.float64)})
    rng = [(r[0], r[1]) for r in rows]
    want = SEG.records(groups, C, rng)
    # the segm oracle's records stand in group order; the stratified oracle's in the sorted order: compare on (cls, seq, rank)
    rec = got["records"]
    key = lambda r: np.lexsort((r["rank"], r["seq"], r["cls"]))               # noqa: E731
    ka, kb = key(rec), key(want)
    assert len(ka) == len(kb) > 200
    for f in ("cls", "seq", "rank"):
        assert np.array_equal(rec[f][ka], want[f][kb]), f
    assert np.array_equal(rec["m"][ka], want["m"][kb])
    assert np.array_equal(rec["npig"], want["npig"])
    wp, wr = SEG.accumulate(want, C, md)
    assert np.array_equal(got["precision"], wp) and np.array_equal(got["recall"], wr)
    assert (rec["m"] >> 16).any() and all((wp[:, :, :, a, :] > 0).any() for a in range(4))


@pytest.mark.parametrize("cfg", SC.CONFIGS)
def test_scenes_cover_what_the_gpu_test_relies_on(cfg):
    scene, strata, imgs = scene_images(cfg)
    stats = {}
    rec = SO.records(imgs, C, SC.strata_rows(strata), 100, stats)
    per_stratum = (rec["npig"] > 0).sum(0)
    print(cfg, "classes with non-ignored GTs per stratum", per_stratum.tolist(), "npig", rec["npig"].sum(0).tolist(), stats)
    assert (per_stratum >= 2).all()
    if cfg != "all":
        assert stats["to_ignored"] > 0 and stats["unmatched_outside"] > 0
    assert stats["tie_non_ignored"] > 0
    if cfg == "coco+lens":
        assert stats["ignored_larger_iou"] > 0
        assert np.isinf(np.concatenate([i["gt_zone"] for i in imgs])).sum() >= 1          # a GT centre beyond the lens field
    gt_per_class = [np.bincount(i["gt_cls"], minlength=4) for i in imgs]
    assert any(64 < n.max() < 256 for n in gt_per_class) and any(n.max() == 256 for n in gt_per_class)
    assert max(np.bincount(i["det_cls"], minlength=4).max() for i in imgs) > 128
    assert any(len(i["det_cls"]) == 0 and len(i["gt_cls"]) for i in imgs)
    assert any(len(i["gt_cls"]) == 0 and len(i["det_cls"]) for i in imgs)
    n_det = [len(i["det_cls"]) for i in imgs]
    assert any(n and n & (n - 1) for n in n_det)                               # a detection count that is no power of two


def test_argument_errors_name_the_argument():
    with pytest.raises(ValueError, match="area"):
        E.Stratum("x", area=(5.0, 1.0))
    with pytest.raises(ValueError, match="zone"):
        E.Stratum("x", zone=(2.0, 1.0))
    with pytest.raises(ValueError, match="edges"):
        E.zone_strata([0, 2, 1])
    with pytest.raises(Ep24Error, match="strata"):
        E.Evaluator24(3, strata=E.zone_strata(range(10)))                     # 9 strata
    with pytest.raises(Ep24Error, match="max_dets"):
        E.Evaluator24(3, max_dets=(10, 1))
    with pytest.raises(Ep24Error, match="max_dets"):
        E.Evaluator24(3, max_dets=(1, 10, 100, 120, 128))
    with pytest.raises(Ep24Error, match="max_dets"):
        E.Evaluator24(3, max_dets=(1, 129))
    with pytest.raises(ValueError, match="scales"):
        E._check_tables(2, [1.0, 0.0], None)
    with pytest.raises(ValueError, match="scales"):
        E._check_tables(2, [1.0], None)
    zt = E.no_zones(2)
    zt[1, 0] = 3.0
    with pytest.raises(ValueError, match="zones.*kind"):
        E._check_tables(2, None, zt)
    with pytest.raises(ValueError, match="zones"):
        E._check_tables(2, None, np.zeros((2, 5)))
    ev = E.Evaluator24(3)
    with pytest.raises(ValueError, match="scales / zones"):
        ev._tables(2, [1.0, 1.0], None)
    sc, zt = E._check_tables(3, None, None)
    assert np.array_equal(sc, np.ones(3)) and zt.shape == (3, 16) and not zt.any()


def test_zone_tables():
    zt = E.radius_zones([(480, 640), (1280, 960)], (640, 640))
    assert zt[0, :5].tolist() == [1.0, 400.0, 400.0, 319.5, 239.5]
    assert zt[1, :5].tolist() == [1.0, 400.0, 400.0, 239.5, 319.5]            # r = 0.5: content 640 x 480
    corners = SO.zone(np.array([-0.5, 639.5]), np.array([-0.5, 479.5]), zt[[0, 0]])
    assert np.array_equal(corners, [1.0, 1.0])                                 # the content's corners are at radius 1
    lz = E.lens_zones([SC.LENS_A])
    assert lz[0, 0] == 2.0 and lz[0, 1:5].tolist() == list(SC.LENS_A.fish) and lz[0, 9] == SC.LENS_A.theta_max
    z = SO.zone(np.array([319.5, 319.5 + 200.0 * float(SC.LENS_A.thetad(0.5)), 0.0]), np.array([319.5, 319.5, 0.0]), lz[[0, 0, 0]])
    assert z[0] == 0.0 and abs(z[1] - np.degrees(0.5)) < 1e-4 and np.isinf(z[2])      # the centre is an fp32 column: 1e-5 pixel
    x, y = (200.0 - 319.5) / 200.0, (250.0 - 319.5) / 200.0                   # LensModel.newton is the same arithmetic
    assert SO.zone(np.array([200.0]), np.array([250.0]), lz[[0]])[0] == float(SC.LENS_A.newton(np.sqrt(x * x + y * y))) * (180.0 / np.pi)
