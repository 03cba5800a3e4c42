"""Test-time augmentation without a GPU: the float32 / float64 oracle (tests/tta_oracle.py) against closed forms, the conditions
the seeded scenes of tests/tta_scenes.py must meet for the GPU file to be decisive, the one place the benefit of voting is shown
(on the oracle), ``views_for`` and the argument rules."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import poly24_oracle as P  # noqa: E402
import polynms_oracle as N  # noqa: E402
import tta_oracle as T  # noqa: E402
import tta_scenes as S  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
Y24 = os.path.join(ROOT, "exploration-of-potential_amd", "yolox_24p")


# ---- 1. mirror-unmap geometry ----------------------------------------------------------------------------
def test_mirrored_unmap_is_the_mirror_of_the_vertices_and_ray_k_comes_from_ray_12_minus_k():
    rng = np.random.default_rng(5)
    rows = np.zeros((40, 28), np.float32)
    rows[:, 0:2] = rng.uniform(20.0, 76.0, (40, 2))
    rows[:, 2:26] = rng.uniform(3.0, 20.0, (40, 24))
    rows[:, 26:] = rng.uniform(0.0, 1.0, (40, 2))
    w_v = 96
    V = P.det_polygons(rows).astype(np.float64)
    Vm = V.copy()
    Vm[..., 0] = w_v - Vm[..., 0]                                                # the mirrored vertices
    got = T.unmap(rows, w_v, 1.0, True)
    G = P.det_polygons(got).astype(np.float64)
    src = (12 - np.arange(24)) % 24
    assert np.abs(G - Vm[:, src]).max() <= 1e-4                                  # ray k of the result is the mirrored ray 12 - k
    assert np.abs(G - Vm[:, (12 + np.arange(24)) % 24]).max() > 1.0              # and not the permutation turned the other way
    # as sets: every mirrored vertex is met by exactly one vertex of the result
    d = np.abs(G[:, :, None] - Vm[:, None]).max(-1)
    assert (d.min(2) <= 1e-4).all() and (d.min(1) <= 1e-4).all()
    assert np.array_equal(got[:, 26:].view(np.uint32), rows[:, 26:].view(np.uint32))
    assert np.array_equal(got[:, 1].view(np.uint32), rows[:, 1].view(np.uint32))
    # twice is the identity on the radii, and on cx to the rounding of w - (w - cx)
    back = T.unmap(got, w_v, 1.0, True)
    assert np.array_equal(back[:, 2:26], rows[:, 2:26]) and np.abs(back[:, 0] - rows[:, 0]).max() <= 1e-5


def test_unmap_scales_every_length_once_and_copies_the_rest():
    rows = np.arange(2 * 3 * 29, dtype=np.float32).reshape(2, 3, 29) / 7
    s = 640 / 544
    got = T.unmap(rows, 544, s, False)
    assert got.dtype == np.float32 and np.array_equal(got[..., :26], (rows[..., :26] * np.float32(s)).astype(np.float32))
    assert np.array_equal(got[..., 26:], rows[..., 26:])
    same = T.unmap(rows, 640, 1.0, False)
    assert np.array_equal(same.view(np.uint32), rows.view(np.uint32)) and same is not rows


# ---- 2. voting: closed forms -----------------------------------------------------------------------------
def _table(rows):
    """[n, 28] fp32 one-class table from (cx, cy, r or r[24], obj) tuples; class_conf = 1."""
    p = np.zeros((len(rows), 28), np.float32)
    for a, (cx, cy, r, obj) in enumerate(rows):
        p[a, 0:2] = (cx, cy)
        p[a, 2:26] = r
        p[a, 26], p[a, 27] = obj, 1.0
    return p


def test_identical_copies_return_the_polygon():
    r = np.random.default_rng(1).uniform(8.0, 20.0, 24)
    p = _table([(50.0, 60.0, r, 0.9), (50.0, 60.0, r, 0.8), (50.0, 60.0, r, 0.7)])
    keep, voted, nv = T.vote(p, 1, 0.3, 0.5, 0.5)
    assert list(keep) == [0] and list(nv) == [3]
    assert np.abs(voted[0] - p[0, :26]).max() <= 1e-4
    out, abst = T.consensus64([(50.0, 60.0)] * 3, [T.polygon64(50.0, 60.0, r)] * 3, [0.9, 0.8, 0.7], r)
    assert np.abs(out[2:] - r).max() <= 1e-9 and abs(out[0] - 50.0) <= 1e-12 and not abst.any()


def test_two_concentric_24_gons_give_the_weighted_radius():
    a, b = T.polygon64(100.0, 100.0, 10.0), T.polygon64(100.0, 100.0, 20.0)
    assert abs(P.poly24_iou(b[None], a[None])[0, 0] - 0.25) <= 1e-6
    out, abst = T.consensus64([(100.0, 100.0)] * 2, [a, b], [0.25, 0.75], np.full(24, 20.0))
    assert np.abs(out[2:] - 17.5).max() <= 1e-9 and np.abs(out[:2] - 100.0).max() <= 1e-12 and not abst.any()
    # the same through the whole rule on fp32 rows: the kept row is the better one, both vote at vote_thre = 0.2
    p = _table([(100.0, 100.0, 10.0, 0.25), (100.0, 100.0, 20.0, 0.75)])
    keep, voted, nv = T.vote(p, 1, 0.1, 0.5, 0.2)
    assert list(keep) == [1, 0] and list(nv) == [2, 2]                           # IoU 0.25 <= nms_thre: both kept, each hears the other
    assert np.abs(voted[:, 2:] - 17.5).max() <= 1e-5
    _, alone, nv1 = T.vote(p, 1, 0.1, 0.5, 0.3)                                   # 0.25 is not above 0.3: nobody hears anybody
    assert list(nv1) == [1, 1] and np.array_equal(alone.view(np.uint32), p[[1, 0], :26].view(np.uint32))


def test_a_voter_the_ray_does_not_cross_abstains():
    big, small = T.polygon64(100.0, 100.0, 30.0), T.polygon64(112.0, 100.0, 6.0)
    out, abst = T.consensus64([(100.0, 100.0), (112.0, 100.0)], [big, small], [0.75, 0.25], np.full(24, 30.0))
    assert abs(out[0] - 103.0) <= 1e-12 and abs(out[1] - 100.0) <= 1e-12         # the fused centre lies outside the small voter
    assert abst[0] == 0 and abs(out[2 + 0] - (0.75 * 27.0 + 0.25 * 3.0)) <= 1e-9    # ray 0 meets both: 27 and 3
    assert abst[12] == 1 and abs(out[2 + 12] - 33.0) <= 1e-9                     # ray 12 points away from the small one: it abstains
    assert abst[6] == 1 and abst[18] == 1
    # a ray nobody crosses falls back to the kept row's own radius
    far, _ = T.consensus64([(0.0, 0.0), (200.0, 0.0)], [T.polygon64(0.0, 0.0, 5.0), T.polygon64(200.0, 0.0, 5.0)], [0.5, 0.5],
                           np.arange(24.0))
    assert far[2 + 6] == 6.0 and far[2 + 18] == 18.0                              # straight up and down from (100, 0): nothing there


def test_zero_weights_and_nan_rows():
    p = _table([(50.0, 50.0, 10.0, 0.0), (50.0, 50.0, 10.5, 0.0)])
    keep, voted, nv = T.vote(p, 1, 0.0, 0.5, 0.5)                                  # scores 0 pass conf_thre 0; they sum to 0
    assert list(keep) == [0] and list(nv) == [2] and np.array_equal(voted[0].view(np.uint32), p[0, :26].view(np.uint32))
    q = _table([(50.0, 50.0, 10.0, 0.9), (50.0, 50.0, 10.0, 0.8), (50.0, 50.0, 10.0, 0.7)])
    q[1, 5] = np.nan
    keep, voted, nv = T.vote(q, 1, 0.3, 0.5, 0.5)
    assert list(keep) == [0, 1] and list(nv) == [2, 1]                            # the NaN row votes for nobody but itself
    assert np.array_equal(voted[1].view(np.uint32), q[1, :26].view(np.uint32))


# ---- 3. the scenes' conditions ---------------------------------------------------------------------------
@pytest.mark.parametrize("name,agnostic,max_candidates", S.ORACLE_SCENES)
def test_margins_and_conditions_of_the_gpu_scenes(name, agnostic, max_candidates):
    pred = S.scene(name)
    nms = min(N.decision_margin(img, S.C, S.CONF_THRE, S.NMS_THRE, agnostic, max_candidates) for img in pred)
    vote = min(T.vote_margin(img, S.C, S.CONF_THRE, S.VOTE_THRE, agnostic, max_candidates) for img in pred)
    print("%s agnostic=%s K=%s: min |iou - nms_thre| = %.3e, min |iou - vote_thre| = %.3e" % (name, agnostic, max_candidates, nms, vote))
    assert nms >= S.MARGIN and vote >= S.MARGIN                                   # else: regenerate the scene with another seed
    res = S.oracle_vote(name, agnostic, max_candidates)
    assert [len(N.score_order(img, S.C, S.CONF_THRE, max_candidates)[0]) for img in pred] == \
        [min(n, max_candidates or n) for n in S.counts(name)]
    assert any((nv >= 3).any() for _, _, nv, _, _, _ in res)                      # a kept row with at least three voters
    assert any((v < i).any() for _, _, _, kept, who, _ in res for i, v in zip(kept, who))   # a voter ranked before its kept row
    assert any((nv == 1).any() for _, _, nv, _, _, _ in res) or name in ("three", "six_views")   # and rows nobody else votes for


def test_scene_shapes_share_one_scratch():
    assert S.scene("dense200").shape == S.scene("three").shape == (1, S.A, 27 + S.C)
    assert S.scene("edges").shape[0] == len(S.counts("edges")) == 7


# ---- 4. the consensus scene ------------------------------------------------------------------------------
def test_voting_brings_the_six_views_closer_to_the_truth():
    c, r, cls = S.six_views_truth()
    th = np.arange(24) * (15.0 * np.pi / 180.0)
    truth = np.stack([c[:, 0:1] + r * np.cos(th), c[:, 1:2] + r * np.sin(th)], -1)                 # [12, 24, 2] float64
    img = S.scene("six_views")[0]
    keep, voted, nv, _, _, _ = S.oracle_vote("six_views")[0]
    star = img[keep, 1] < 400.0                                                   # the chain below the grid is not part of the claim
    keep, voted, nv = keep[star], voted[star], nv[star]
    assert len(keep) == S.SIX_OBJECTS and (nv == S.SIX_VIEWS).all()               # every object once, heard in all six views
    winners = img[keep, :26]
    obj = np.argmin(((winners[:, None, :2] - c[None]) ** 2).sum(-1), 1)
    assert sorted(obj) == list(range(S.SIX_OBJECTS))
    iou_w = np.array([P.poly24_iou(truth[o][None], P.det_polygons(winners[m][None]))[0, 0] for m, o in enumerate(obj)])
    iou_v = np.array([P.poly24_iou(truth[o][None], P.det_polygons(voted[m][None]))[0, 0] for m, o in enumerate(obj)])
    print("mean IoU to the truth: NMS winners %.4f, voted %.4f" % (iou_w.mean(), iou_v.mean()))
    assert iou_v.mean() > iou_w.mean()


# ---- 5. views_for ----------------------------------------------------------------------------------------
def test_views_for():
    from ep24 import tta
    v = tta.views_for((640, 640))
    assert v == [(640, 640, False), (640, 640, True), (544, 544, False), (544, 544, True), (448, 448, False), (448, 448, True)]
    assert tta.views_for(640, mirror=False) == [(640, 640, False), (544, 544, False), (448, 448, False)]
    with pytest.raises(ValueError, match="0.85"):
        tta.views_for((480, 640), scales=(1.0, 0.85))
    assert tta.views_for((480, 640), scales=(0.8,), mirror=False) == [(384, 512, False)]
    assert tta.views_for((480, 640), scales=(1.0, 0.8))[0] == (480, 640, False)
    assert [tta.anchors_for(s) for s in (640, 544, 448)] == [8400, 6069, 4116] and 2 * (8400 + 6069 + 4116) == 37170
    assert tta.anchors_for((480, 640)) == 60 * 80 + 30 * 40 + 15 * 20
    with pytest.raises(ValueError, match="canonical"):
        tta.check_views((640, 640), [(544, 544, False)])
    with pytest.raises(ValueError, match="aspect"):
        tta.check_views((480, 640), [(480, 640, False), (448, 512, False)])


# ---- 6. argument rules -----------------------------------------------------------------------------------
def test_vote_thre_argument_rules_come_before_the_gpu():
    import inspect
    import torch
    from ep24 import evaluate, infer
    sig = inspect.signature(infer.postprocess)
    assert sig.parameters["vote_thre"].default is None and list(sig.parameters)[-1] == "vote_thre"
    pred = torch.zeros(1, 4, 28)                                                  # a CPU tensor: the rules are checked before it is looked at
    with pytest.raises(ValueError, match="vote_thre.*poly24"):
        infer.postprocess(pred, 1, nms_iou="rect", vote_thre=0.5)
    with pytest.raises(ValueError, match="vote_thre.*poly24"):
        infer.postprocess(pred, 1, vote_thre=0.5)
    with pytest.raises(ValueError, match="at least 0"):
        infer.postprocess(pred, 1, nms_iou="poly24", vote_thre=-0.1)
    with pytest.raises(ValueError, match="at least 0"):
        infer.postprocess(pred, 1, nms_iou="poly24", vote_thre=float("nan"))
    with pytest.raises(ValueError, match="nms_iou must be one of"):              # check_nms_iou's own messages are unchanged
        infer.postprocess(pred, 1, nms_iou="bogus", vote_thre=0.5)
    with pytest.raises(ValueError, match="max_candidates belongs to nms_iou='poly24'"):
        infer.check_vote("rect", 10, None)
    infer.check_vote("rect", None, None)
    infer.check_vote("poly24", 100, 0.0)
    assert inspect.signature(evaluate.Evaluator24.__init__).parameters["vote_thre"].default is None
    assert evaluate.Evaluator24(80).vote_thre is None
    assert evaluate.Evaluator24(80, nms_iou="poly24", vote_thre=0.6).vote_thre == 0.6
    with pytest.raises(ValueError, match="vote_thre.*poly24"):
        evaluate.Evaluator24(80, vote_thre=0.6)
    with pytest.raises(ValueError, match="at least 0"):
        evaluate.Evaluator24(80, nms_iou="poly24", vote_thre=-1.0)


@pytest.fixture
def y24():
    sys.path.insert(0, Y24)
    try:
        yield
    finally:
        sys.path.remove(Y24)


def test_trainer_flags(y24):
    import importlib
    mod = importlib.import_module("train_24p")
    parse = mod.make_parser().parse_args
    d = parse([])
    assert (d.eval_tta, d.eval_tta_scales, d.eval_vote) == (False, None, None)
    a = parse(["--eval-tta"])
    assert a.eval_tta and a.eval_vote is None
    a = parse(["--eval-tta", "--eval-tta-scales", "1.0", "0.8", "--eval-vote", "0.6"])
    assert a.eval_tta_scales == [1.0, 0.8] and a.eval_vote == 0.6
    assert parse(["--nms-iou", "poly24", "--eval-vote", "0.5"]).eval_vote == 0.5  # voting without views
    assert parse(["--eval-tta", "--nms-iou", "poly24"]).nms_iou == "poly24"
    with pytest.raises(SystemExit):
        parse(["--eval-vote", "0.5"])                                             # no poly24 NMS: refused while parsing
    with pytest.raises(SystemExit):
        parse(["--nms-iou", "rect", "--eval-vote", "0.5"])
    with pytest.raises(SystemExit):
        parse(["--eval-tta", "--nms-iou", "rect"])                                # --eval-tta implies poly24
    with pytest.raises(SystemExit):
        parse(["--eval-tta", "--eval-vote", "-0.5"])
    with pytest.raises(SystemExit):
        parse(["--eval-tta-scales", "1.0", "0.8"])                                # scales without --eval-tta
    with pytest.raises(SystemExit):
        parse(["--eval-tta", "--eval-tta-scales", "0.8", "1.0"])                  # the canonical view comes first
    # the Exp receives them: --eval-tta implies the polygon NMS
    from exp import get_exp
    exp = get_exp(os.path.join(Y24, "load_train", "yolox_24p_train.py"))
    assert (exp.eval_tta, exp.eval_tta_scales, exp.eval_vote) == (False, (1.0, 0.85, 0.7), None)
    assert exp.get_evaluator(4).vote_thre is None and exp.get_evaluator(4).max_candidates is None
    mod.apply_eval_args(exp, parse(["--eval-tta", "--eval-vote", "0.6"]))
    assert exp.eval_tta and exp.nms_iou_type == "poly24" and exp.eval_vote == 0.6
    ev = exp.get_evaluator(4)
    assert (ev.nms_iou, ev.vote_thre, ev.max_candidates) == ("poly24", 0.6, 8400)  # the canonical view's anchors at 640 x 640


def test_show_flags(y24):
    import importlib
    mod = importlib.import_module("show_24p")
    parse = mod.make_parser().parse_args
    d = parse([])
    assert (d.tta, d.vote) == (False, None)
    a = parse(["--tta", "--vote", "0.6"])
    assert a.tta and a.vote == 0.6
    assert parse(["--nms-iou", "poly24", "--vote", "0.5"]).vote == 0.5
    with pytest.raises(SystemExit):
        parse(["--vote", "0.5"])
    with pytest.raises(SystemExit):
        parse(["--tta", "--nms-iou", "rect"])
