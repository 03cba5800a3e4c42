"""Test-time augmentation on the GPU (csrc/tta.hip, ep24/tta.py): ``ep24_mirror_f32`` and ``ep24_tta_unmap`` bit for bit
against numpy and the float32 oracle, ``tta.predict`` against views built separately, and ``ep24_post_vote_poly24`` through
``postprocess(..., vote_thre=)`` against the float64 oracle (tests/tta_oracle.py) on the seeded scenes of tests/tta_scenes.py,
whose decisions all stay 1e-6 away from both thresholds (asserted in tests/test_tta_oracle.py)."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import polynms_oracle as N  # noqa: E402
import polynms_scenes as PS  # noqa: E402
import tta_oracle as T  # noqa: E402
import tta_scenes as S  # noqa: E402
from ep24 import _lib, evaluate as E, infer, multiscale, nn as enn, synth, tta  # noqa: E402
from ep24._lib import ptr  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TOL = 1e-3                              # px: the project's label tolerance (tests/test_gpu_fisheye.py)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _dev(a):
    return torch.from_numpy(np.array(a)).to(DEV)


# ---- 1. ep24_mirror_f32 ----------------------------------------------------------------------------------
MIRROR_SHAPES = [(1, 1, 1), (3, 2, 3), (2, 5, 4), (1, 3, 63), (2, 2, 64), (1, 2, 65), (1, 1, 257)]


@pytest.mark.parametrize("guard", [4, 1])                                        # 4: rows stay 16-byte aligned; 1: they do not
@pytest.mark.parametrize("shape", MIRROR_SHAPES)
def test_mirror_is_bit_equal_to_numpy_and_stays_inside_its_buffer(shape, guard):
    n, h, w = shape
    rng = np.random.default_rng(n * 1000 + h * 100 + w)
    words = rng.integers(0, 2 ** 32, (n, h, w), dtype=np.uint64).astype(np.uint32)
    words.reshape(-1)[::3] = np.array([0x7FC12345, 0xFFA00001, 0x7F800001], np.uint32)[np.arange(len(words.reshape(-1)[::3])) % 3]
    src = _dev(words.view(np.float32))
    fill = 0xDEADBEEF
    out = torch.from_numpy(np.full(n * h * w + 2 * guard, fill, np.uint32).view(np.float32)).to(DEV)
    _lib.call("mirror_f32", ptr(src), n, h, w, ptr(out, guard), _lib.stream_ptr())
    got = _bits(out.cpu().numpy())
    assert np.array_equal(got[guard:-guard].reshape(n, h, w), words[..., ::-1])
    assert (got[:guard] == fill).all() and (got[-guard:] == fill).all()
    assert np.array_equal(_bits(src.cpu().numpy()), words)


def test_mirror_refuses_in_place():
    x = torch.zeros(2, 3, 8, device=DEV)
    with pytest.raises(_lib.Ep24Error, match="in == out"):
        _lib.call("mirror_f32", ptr(x), 2, 3, 8, ptr(x), _lib.stream_ptr())


# ---- 2. ep24_tta_unmap -----------------------------------------------------------------------------------
def _unmap(view, w_v, s, mirror, merged, off):
    B, A_v, ncols = view.shape
    _lib.call("tta_unmap", ptr(view), B, A_v, ncols, w_v, s, mirror, ptr(merged), merged.shape[1], off, _lib.stream_ptr())


@pytest.mark.parametrize("ncols", [27, 28, 107])
@pytest.mark.parametrize("A_v", [1, 63, 64, 65])
def test_unmap_is_bit_equal_to_the_oracle_and_touches_only_its_slice(A_v, ncols):
    B, extra = 2, 7
    rng = np.random.default_rng(A_v * 1000 + ncols)
    view = rng.uniform(0.0, 600.0, (B, A_v, ncols)).astype(np.float32)
    view[..., 26:] = rng.uniform(0.0, 1.0, (B, A_v, ncols - 26))
    view[0, 0, 26] = np.array([0x7FC12345], np.uint32).view(np.float32)[0]      # a NaN payload in a copied column
    base = rng.integers(0, 2 ** 32, (B, A_v + extra, ncols), dtype=np.uint64).astype(np.uint32)
    dview = _dev(view)
    for w_v, s in ((640, 1.0), (544, 640 / 544)):
        for mirror in (0, 1):
            want_rows = T.unmap(view, w_v, s, bool(mirror))
            for off in (0, 3, extra):
                merged = _dev(base.view(np.float32))
                _unmap(dview, w_v, s, mirror, merged, off)
                want = base.copy()
                want[:, off:off + A_v] = _bits(want_rows)
                assert np.array_equal(_bits(merged.cpu().numpy()), want), (w_v, mirror, off)
    assert np.array_equal(_bits(T.unmap(view, 640, 1.0, False)), _bits(view))     # s == 1, unmirrored: a bit copy


def test_unmap_refused_arguments_leave_every_byte_alone():
    view = torch.rand(2, 5, 28, device=DEV)
    base = np.random.default_rng(3).integers(0, 2 ** 32, (2, 9, 28), dtype=np.uint64).astype(np.uint32)
    merged = _dev(base.view(np.float32))
    s_ = _lib.stream_ptr()
    for kw in (dict(off=-1), dict(off=5), dict(s=0.0), dict(s=-1.0), dict(s=float("inf")), dict(s=float("nan"))):
        with pytest.raises(_lib.Ep24Error):
            _lib.call("tta_unmap", ptr(view), 2, 5, 28, 640, kw.get("s", 1.0), 0, ptr(merged), 9, kw.get("off", 0), s_)
    v26, m26 = torch.rand(2, 5, 26, device=DEV), torch.zeros(2, 9, 26, device=DEV)
    with pytest.raises(_lib.Ep24Error, match="ncols"):
        _lib.call("tta_unmap", ptr(v26), 2, 5, 26, 640, 1.0, 0, ptr(m26), 9, 0, s_)
    assert np.array_equal(_bits(merged.cpu().numpy()), base) and float(m26.abs().sum()) == 0.0


# ---- 3. tta.predict --------------------------------------------------------------------------------------
def test_predict_equals_the_views_built_separately_bit_for_bit():
    torch.manual_seed(0)
    model = enn.YOLOX(enn.YOLOPAFPN(0.33, 0.125), enn.YOLOXHead(80, 0.125))
    model.head.initialize_biases(1e-2)
    model.to(DEV).eval()
    B, S0 = 2, 128
    images = synth.make_images(B, S0, seed=3).to(DEV)
    views = tta.views_for(S0, scales=(1.0, 0.75, 0.5))
    assert [v[:2] for v in views[::2]] == [(128, 128), (96, 96), (64, 64)]
    before = set(model._engines)
    with torch.no_grad():
        merged = tta.predict(model, images, views)
        again = tta.predict(model, images, views).cpu().numpy()
        p = tta.predictor(model, B, S0, views)
        assert p.offsets == [0, 336, 672, 861, 1050, 1134] and p.total_anchors == 1218 == merged.shape[1] and p.canonical_anchors == 336
        got = merged.cpu().numpy()
        assert np.array_equal(_bits(got), _bits(again))                          # a second call gives the same bits
        labels = torch.zeros(B, 1, 51, device=DEV)
        for (h, w, mir), off, A_v in zip(p.views, p.offsets, p.anchors):
            x = images if (h, w) == (S0, S0) else multiscale.resize_batch(images, labels, (h, w))[0]
            if mir:
                x = torch.flip(x.cpu(), dims=[3]).contiguous().to(DEV)
            out = model(x, train=False).cpu().numpy()
            want = T.unmap(out, w, S0 / w, mir)
            assert np.array_equal(_bits(got[:, off:off + A_v]), _bits(want)), (h, w, mir)
    assert set(model._engines) - before == {(B, 128), (B, 96), (B, 64)}           # one eval plan per view size
    torch.cuda.synchronize()
    tta.release(model)
    assert set(model._engines) == before                                         # and they leave with the predictor
    with pytest.raises(_lib.Ep24Error):
        tta.predict(model, images.cpu())


# ---- 4. voting against the float64 oracle ----------------------------------------------------------------
def _vote(pred, agnostic=False, max_candidates=None, vote_thre=S.VOTE_THRE):
    """postprocess with voting -> (per-image [n, 29] or None, n_voters [B, A] of the launch)."""
    B, A, ncols = pred.shape
    kw = {} if max_candidates is None else {"max_candidates": max_candidates}
    got = infer.postprocess(_dev(pred), ncols - 27, S.CONF_THRE, S.NMS_THRE, agnostic, nms_iou="poly24", vote_thre=vote_thre, **kw)
    ws = infer._scratch[(B, A, str(torch.device(DEV)))]
    K = A if max_candidates is None else min(max_candidates, A)
    return got, ws.poly(K).n_voters.cpu().numpy()


def _check(got, n_voters, pred, oracle):
    assert len(got) == len(oracle)
    singles = multis = 0
    for b, (g, (keep, voted, nv, _, _, _)) in enumerate(zip(got, oracle)):
        if len(keep) == 0:
            assert g is None, b
            continue
        _, conf, cls = N.score_order(pred[b], S.C, S.CONF_THRE)
        assert g is not None and tuple(g.shape) == (len(keep), 29), (b, None if g is None else tuple(g.shape), len(keep))
        g = g.cpu().numpy()
        tail = np.concatenate([pred[b][keep, 26:27], conf[keep, None], cls[keep, None].astype(np.float32)], 1)
        assert np.array_equal(_bits(g[:, 26:]), _bits(tail)), b                  # kept rows, order, obj_conf, class_conf, class
        assert np.array_equal(n_voters[b, :len(keep)], nv), (b, n_voters[b, :len(keep)], nv)
        err = np.abs(g[:, :26].astype(np.float64) - voted.astype(np.float64)).max()
        print("image %d: %d kept, voters %d..%d, max |voted - oracle| = %.3e px" % (b, len(keep), nv.min(), nv.max(), err))
        assert err <= TOL, (b, err)
        one = nv == 1
        assert np.array_equal(_bits(g[one, :26]), _bits(pred[b][keep[one], :26])), b   # a single voter: the input row, bit for bit
        singles += int(one.sum())
        multis += int((~one).sum())
    return singles, multis


@pytest.mark.parametrize("name,agnostic,max_candidates", S.ORACLE_SCENES)
def test_voted_rows_equal_the_oracle(name, agnostic, max_candidates):
    """Candidate counts 0, 1, 2, 63, 64, 65, 129 ("edges": the word and wave boundaries of the voter mask), 200 and 3, class-aware
    and agnostic, the 64 best only, and the six views."""
    pred = S.scene(name)
    got, n_voters = _vote(pred, agnostic, max_candidates)
    singles, multis = _check(got, n_voters, pred, S.oracle_vote(name, agnostic, max_candidates))
    assert multis > 0 and (singles > 0 or name in ("three", "six_views"))


def _one_class(rows):
    """[1, n, 28] fp32 one-class table from (cx, cy, r, obj) tuples; class_conf = 1."""
    p = np.zeros((1, len(rows), 28), np.float32)
    for a, (cx, cy, r, obj) in enumerate(rows):
        p[0, a, 0:2] = (cx, cy)
        p[0, a, 2:26] = r
        p[0, a, 26], p[0, a, 27] = obj, 1.0
    return p


def _post_one_class(pred, conf, nms, vote):
    got = infer.postprocess(_dev(pred), 1, conf, nms, False, nms_iou="poly24", vote_thre=vote)
    ws = infer._scratch[(1, pred.shape[1], str(torch.device(DEV)))]
    return got[0].cpu().numpy(), ws.poly(pred.shape[1]).n_voters.cpu().numpy()[0]


def test_a_voter_the_ray_does_not_cross_abstains_on_the_gpu():
    """A circle of radius 6 inside one of radius 30 (IoU 0.04 > vote_thre 0.02): the fused centre (103, 100) lies outside the
    small one, which abstains on the rays that point away from it."""
    pred = _one_class([(100.0, 100.0, 30.0, 0.75), (112.0, 100.0, 6.0, 0.25)])
    keep, voted, nv, _, _, abst = T.vote(pred[0], 1, 0.1, 0.5, 0.02, detail=True)
    assert list(keep) == [0, 1] and list(nv) == [2, 2] and abst[0][12] == 1 and abst[0][0] == 0
    got, n_voters = _post_one_class(pred, 0.1, 0.5, 0.02)
    assert list(n_voters[:2]) == [2, 2] and np.abs(got[:, :26].astype(np.float64) - voted).max() <= TOL
    assert abs(got[0, 0] - 103.0) <= TOL and abs(got[0, 2 + 12] - 33.0) <= TOL and abs(got[0, 2] - 21.0) <= TOL


def test_more_voters_than_one_list_holds():
    """1100 concentric circles of radii 19.5 .. 20.5 and distinct scores: one kept row that all of them vote for, more than the
    1024 voters the kernel lists at a time.  Their IoU is (r_min / r_max)^2 >= 0.9, far from both thresholds, so the oracle takes
    it in closed form."""
    n = 1100
    rng = np.random.default_rng(9)
    r = rng.uniform(19.5, 20.5, n)
    pred = _one_class([(300.0, 200.0, r[a], 0.4 + 0.5 * (a * 7919 % n) / n) for a in range(n)])

    def iou(order):
        rr = pred[0, order, 2].astype(np.float64)
        return (np.minimum(rr[:, None], rr[None]) / np.maximum(rr[:, None], rr[None])) ** 2
    keep, voted, nv = T.vote(pred[0], 1, 0.3, 0.5, 0.5, iou=iou)
    assert len(keep) == 1 and list(nv) == [n]
    got, n_voters = _post_one_class(pred, 0.3, 0.5, 0.5)
    assert got.shape == (1, 29) and n_voters[0] == n
    err = np.abs(got[0, :26].astype(np.float64) - voted[0]).max()
    print("1100 voters: max |voted - oracle| = %.3e px" % err)
    assert err <= TOL and abs(got[0, 2] - pred[0, keep[0], 2]) > 0.05              # the consensus, not the kept row's own radius


# ---- 5. the voter sets follow the kernel's own IoU values ------------------------------------------------
def _gpu_matrix(rows26):
    """pairwise_iou's poly24 matrix of the rows against themselves: row i = GT side (its vertices formed in torch fp32 on the
    CPU, product then sum), column j = detection side - the orientation of the vote, kept row = a."""
    q = torch.from_numpy(np.ascontiguousarray(rows26[:, :26]))
    cs = torch.from_numpy(E.ray_cos_sin())
    x = q[:, 0:1] + q[:, 2:26] * cs[None, :24]
    y = q[:, 1:2] + q[:, 2:26] * cs[None, 24:]
    gt50 = torch.cat([q[:, :2], torch.stack([x, y], -1).reshape(len(q), 48)], 1)
    return E.pairwise_iou(gt50.to(DEV), q.to(DEV), "poly24").cpu().numpy()


@pytest.mark.parametrize("agnostic", [False, True])
def test_voters_follow_the_kernels_own_iou_matrix(agnostic):
    pred = S.scene("dense200")
    img = pred[0]

    def iou(order):
        M = _gpu_matrix(img[order])
        assert int((M > 0).sum()) >= 2000
        return M
    oracle = T.vote(img, S.C, S.CONF_THRE, S.NMS_THRE, S.VOTE_THRE, agnostic, iou=iou, detail=True)
    assert 0 < len(oracle[0]) < 200 and (oracle[2] >= 3).any()
    got, n_voters = _vote(pred, agnostic)
    _check(got, n_voters, pred, [oracle])


# ---- 6. stale scratch ------------------------------------------------------------------------------------
def test_scratch_of_a_larger_scene_does_not_leak_into_a_smaller_one():
    big, small = S.scene("dense200"), S.scene("three")
    assert big.shape == small.shape                                               # one (B, A): the same scratch
    got, _ = _vote(big)
    assert got[0].shape[0] > 3
    got, n_voters = _vote(small)
    _check(got, n_voters, small, S.oracle_vote("three"))


# ---- 7. max_candidates -----------------------------------------------------------------------------------
def test_only_the_k_best_are_eligible_voters():
    pred = S.scene("edges")
    got, n_voters = _vote(pred, max_candidates=64)
    oracle = S.oracle_vote("edges", False, 64)
    _check(got, n_voters, pred, oracle)
    full = S.oracle_vote("edges")
    assert any(len(a[0]) != len(b[0]) or not np.array_equal(a[2], b[2]) for a, b in zip(oracle, full))   # the cut changes something
    for K in (129, S.A, 10 ** 6):                                                 # at or above every image's candidates: nothing changes
        for a, b in zip(_vote(pred, max_candidates=K)[0], _vote(pred)[0]):
            assert (a is None) == (b is None) and (a is None or torch.equal(a, b))


# ---- 8. defaults are untouched; the evaluator ------------------------------------------------------------
def _labels(pred, C, n=6):
    """[B, n, 51] labels: the polygons of the n best rows of every image (class, centre, 24 vertices)."""
    import poly24_oracle as P
    lab = np.zeros((len(pred), n, 51), np.float32)
    for b, img in enumerate(pred):
        order, _, cls = N.score_order(img, C, 0.0)
        rows = order[:n]
        lab[b, :len(rows), 0] = cls[rows]
        lab[b, :len(rows), 1:3] = img[rows, :2]
        lab[b, :len(rows), 3:] = P.det_polygons(img[rows]).reshape(len(rows), 48)
    return torch.from_numpy(lab).to(DEV)


def _same_evaluation(a, b):
    sa, sb = a.summarize(), b.summarize()
    assert a.n_records == b.n_records > 0
    ra, rb = a.records(), b.records()
    for k in ra:
        assert np.array_equal(ra[k], rb[k]), k
    assert np.array_equal(sa["precision"], sb["precision"]) and np.array_equal(sa["recall"], sb["recall"])


@pytest.mark.parametrize("name", ["edges_a", "edges_b", "nan"])
def test_vote_thre_none_is_the_call_without_the_keyword(name):
    pred = PS.scene(name)
    p = _dev(pred)
    for kw in (dict(nms_iou="poly24"), dict(nms_iou="rect"), dict(nms_iou="poly24", max_candidates=64)):
        plain = infer.postprocess(p, PS.C, PS.CONF_THRE, PS.NMS_THRE, **kw)
        named = infer.postprocess(p, PS.C, PS.CONF_THRE, PS.NMS_THRE, vote_thre=None, **kw)
        for a, b in zip(plain, named):
            assert (a is None) == (b is None) and (a is None or np.array_equal(_bits(a.cpu().numpy()), _bits(b.cpu().numpy())))


def test_default_evaluator_is_unchanged_and_the_voting_one_is_postprocess_plus_update_detections():
    pred = PS.scene("edges_b")
    p, lab = _dev(pred), _labels(pred, PS.C)
    a = E.Evaluator24(PS.C, iou_type="poly24", conf_thre=PS.CONF_THRE, nms_thre=PS.NMS_THRE, nms_iou="poly24")
    b = E.Evaluator24(PS.C, iou_type="poly24", conf_thre=PS.CONF_THRE, nms_thre=PS.NMS_THRE, nms_iou="poly24", vote_thre=None)
    c = E.Evaluator24(PS.C, iou_type="poly24", conf_thre=PS.CONF_THRE, nms_thre=PS.NMS_THRE)
    a.update(p, lab)
    b.update(p, lab)
    c.update_detections(infer.postprocess(p, PS.C, PS.CONF_THRE, PS.NMS_THRE, nms_iou="poly24"), lab)
    _same_evaluation(a, b)
    _same_evaluation(a, c)
    six = S.scene("six_views")
    p, lab = _dev(six), _labels(six, S.C, n=12)
    v = E.Evaluator24(S.C, iou_type="poly24", conf_thre=S.CONF_THRE, nms_thre=S.NMS_THRE, nms_iou="poly24", vote_thre=S.VOTE_THRE)
    w = E.Evaluator24(S.C, iou_type="poly24", conf_thre=S.CONF_THRE, nms_thre=S.NMS_THRE)
    v.update(p, lab)
    dets = infer.postprocess(p, S.C, S.CONF_THRE, S.NMS_THRE, False, "poly24", vote_thre=S.VOTE_THRE)
    w.update_detections(dets, lab)
    _same_evaluation(v, w)
    plain = infer.postprocess(p, S.C, S.CONF_THRE, S.NMS_THRE, False, "poly24")
    assert not torch.equal(plain[0][:, :26], dets[0][:, :26]) and torch.equal(plain[0][:, 26:], dets[0][:, 26:])


def test_two_identical_calls_are_bit_equal_and_a_negative_threshold_is_refused():
    pred = S.scene("dense200")
    a, na = _vote(pred)
    b, nb = _vote(pred)
    assert torch.equal(a[0], b[0]) and np.array_equal(na[0, :a[0].shape[0]], nb[0, :a[0].shape[0]])
    B, A, ncols = pred.shape
    ws = infer._scratch[(B, A, str(torch.device(DEV)))]
    ps = ws.poly(A)
    with pytest.raises(_lib.Ep24Error, match="vote_thre"):
        _lib.call("post_vote_poly24", ptr(_dev(pred)), ncols, ptr(ws.score), B, A, A, -0.1, 0, ptr(ws.sidx), ws.P, ptr(ps.n_cand),
                  ptr(ps.verts), ptr(ps.vbox), ptr(ps.vcls), ptr(ws.keep), ptr(ws.count), ptr(ps.voted), ptr(ps.n_voters),
                  _lib.stream_ptr())
