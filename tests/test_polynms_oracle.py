"""Polygon NMS without a GPU: the new ABI entry and host surface, the motivating two-circle case, the greedy semantics of the
float64 oracle (tests/polynms_oracle.py), and the decision margins of every seeded scene tests/test_gpu_polynms.py compares
against that oracle."""
import ctypes
import inspect
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import poly24_oracle as P  # noqa: E402
import polynms_oracle as N  # noqa: E402
import polynms_scenes as S  # noqa: E402
from ep24 import _lib  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
Y24 = os.path.join(ROOT, "exploration-of-potential_amd", "yolox_24p")


# ---------------------------------------------------------------------------------------------------- API / ABI
def test_symbol_is_declared_and_exported():
    protos = _lib.parse_header()
    assert "ep24_post_nms_poly24" in protos
    ret, params = protos["ep24_post_nms_poly24"]
    assert params[-1] == ("void*", "stream")
    names = [n for _, n in params]
    for n in ("K", "P", "nms_thre", "class_agnostic", "ray_cs", "n_cand", "verts", "vbox", "vcls", "mask", "keep", "keep_count"):
        assert n in names, n
    assert hasattr(ctypes.CDLL(_lib.LIB_PATH), "ep24_post_nms_poly24")
    assert _lib.lib().fn["ep24_abi_version"]() == 3                              # additions only: the version stays


def test_entry_point_refuses_bad_arguments():
    """The argument checks run before any launch, so they answer on a host without a GPU too.  The calls run on a thread of their
    own: the library's last-error text is per thread, and other tests expect this thread's to stay empty."""
    import threading
    fn = _lib.lib().fn["ep24_post_nms_poly24"]
    x = 4096                                                                      # any non-null address: nothing is dereferenced
    names = ("pred", "score", "cls", "ray_cs", "sort_key", "sort_idx", "n_cand", "verts", "vbox", "vcls", "mask", "keep", "keep_count")

    def rc(B=1, A=100, K=100, thr=0.5, P=128, null=None):
        ptrs = {n: x for n in names}
        if null:
            ptrs[null] = None
        return fn(ptrs["pred"], 30, ptrs["score"], ptrs["cls"], B, A, K, thr, 0, ptrs["ray_cs"], ptrs["sort_key"], ptrs["sort_idx"],
                  P, ptrs["n_cand"], ptrs["verts"], ptrs["vbox"], ptrs["vcls"], ptrs["mask"], ptrs["keep"], ptrs["keep_count"], None)
    got = {}

    def calls():
        got["null"] = [rc(null=n) for n in names]
        got["K"] = [rc(K=0), rc(K=101)]                                           # K < 1, K > A
        got["P"] = [rc(P=64), rc(P=100), rc(P=192)]                               # P < A, P no power of two
        got["thr"] = [rc(thr=-0.01), rc(thr=float("nan"))]
        got["thr_text"] = _lib.lib().last_error()
        got["big"] = rc(A=70000, K=70000, P=131072)                               # more than 65536 candidates per image
    th = threading.Thread(target=calls)
    th.start()
    th.join()
    assert got["null"] == [-1] * len(names) and got["K"] == [-1, -1] and got["P"] == [-1, -1, -1] and got["thr"] == [-1, -1]   # EP24_E_ARG
    assert "nms_thre" in got["thr_text"]
    assert got["big"] == -3                                                       # EP24_E_UNSUPPORTED
    assert _lib.lib().last_error() == ""


def test_postprocess_signature_and_argument_errors():
    from ep24 import infer
    sig = inspect.signature(infer.postprocess)
    assert sig.parameters["nms_iou"].default == "rect" and sig.parameters["max_candidates"].default is None
    pred = torch.zeros(1, 4, 28)
    with pytest.raises(ValueError):                                               # before the GPU check: also on this host
        infer.postprocess(pred, 1, nms_iou="bogus")
    with pytest.raises(ValueError):
        infer.postprocess(pred, 1, nms_iou="rect", max_candidates=10)
    with pytest.raises(ValueError):
        infer.postprocess(pred, 1, nms_iou="poly24", max_candidates=0)
    sys.path.insert(0, Y24)
    try:
        import utils
        assert utils.postprocess is infer.postprocess                             # the re-export follows by itself
    finally:
        sys.path.remove(Y24)


def test_product_refuses_to_run_without_a_gpu():
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    from ep24 import infer
    with pytest.raises(_lib.Ep24Error):
        infer.postprocess(torch.zeros(1, 4, 28), 1, nms_iou="poly24")


def test_evaluator_takes_the_nms_choice():
    from ep24 import evaluate
    ev = evaluate.Evaluator24(80)
    assert (ev.nms_iou, ev.max_candidates) == ("rect", None)
    ev = evaluate.Evaluator24(80, iou_type="poly24", nms_iou="poly24", max_candidates=1000)
    assert (ev.nms_iou, ev.max_candidates) == ("poly24", 1000)
    with pytest.raises(ValueError):
        evaluate.Evaluator24(80, nms_iou="polygon")
    with pytest.raises(ValueError):
        evaluate.Evaluator24(80, max_candidates=10)


def test_exp_passes_the_nms_iou_on():
    sys.path.insert(0, Y24)
    try:
        from exp import get_exp
        exp = get_exp(os.path.join(Y24, "load_train", "yolox_24p_train.py"))
        assert exp.nms_iou_type == "rect"
        assert exp.get_evaluator(4).nms_iou == "rect"
        exp.nms_iou_type = "poly24"
        assert exp.get_evaluator(4).nms_iou == "poly24"
    finally:
        sys.path.remove(Y24)


def test_nms_iou_flag():
    sys.path.insert(0, Y24)
    try:
        import importlib
        mod = importlib.import_module("train_24p")
        assert mod.make_parser().parse_args([]).nms_iou is None
        for name in ("rect", "poly24"):
            assert mod.make_parser().parse_args(["--nms-iou", name]).nms_iou == name
        with pytest.raises(SystemExit):
            mod.make_parser().parse_args(["--nms-iou", "circle24"])
    finally:
        sys.path.remove(Y24)


# ---------------------------------------------------------------------------------------------------- the motivating case
def _rect_kept(pred, conf, thr):
    from oracle import post as opost
    out = opost.postprocess(torch.from_numpy(pred.copy()), pred.shape[2] - 27, conf_thre=conf, nms_thre=thr)[0]
    return 0 if out is None else len(out)


def _poly_kept(pred, conf, thr, agnostic=False):
    out = N.postprocess(pred, pred.shape[2] - 27, conf, thr, agnostic)[0]
    return 0 if out is None else len(out)


@pytest.mark.parametrize("d,thr,poly_iou_max", [(25.0, 0.45, 0.0), (19.0, 0.65, 0.01)])
def test_touching_circles_lose_a_member_to_the_rectangle_only(d, thr, poly_iou_max):
    pred = S.circles(d)
    iou = N.iou_matrix(pred[0])[0, 1]
    assert 0.0 <= iou <= poly_iou_max
    assert _rect_kept(pred, 0.3, thr) == 1
    assert _poly_kept(pred, 0.3, thr) == 2


def test_overlapping_circles_lose_a_member_to_both():
    pred = S.circles(2.0)
    assert abs(N.iou_matrix(pred[0])[0, 1] - 0.8) < 0.05
    for thr in (0.45, 0.65):
        assert _rect_kept(pred, 0.3, thr) == 1 and _poly_kept(pred, 0.3, thr) == 1


# ---------------------------------------------------------------------------------------------------- greedy semantics
def _row(cx, cy, r, obj, cls, C=2):
    p = np.zeros(27 + C, np.float32)
    p[0], p[1], p[2:26], p[26] = cx, cy, r, obj
    p[27 + cls] = 1.0
    return p


def _chain(classes=(0, 0, 0)):
    """A > B > C along a line: A and B overlap, B and C overlap, A and C barely."""
    return np.stack([_row(100.0, 100.0, 20.0, 0.9, classes[0]), _row(110.0, 100.0, 20.0, 0.8, classes[1]),
                     _row(120.0, 100.0, 20.0, 0.7, classes[2])])


def test_chain_keeps_what_only_a_removed_candidate_would_remove():
    pred = _chain()
    M = N.iou_matrix(pred)
    assert M[0, 1] > 0.5 and M[1, 2] > 0.5 and M[0, 2] < 0.5
    assert list(N.nms_rows(pred, 2, 0.3, 0.5)) == [0, 2]                          # B is gone before it can remove C
    assert list(N.nms_rows(pred[1:], 2, 0.3, 0.5)) == [0]                         # B alone does remove C


def test_classes_separate_unless_agnostic():
    pred = _chain((0, 1, 0))
    assert list(N.nms_rows(pred, 2, 0.3, 0.5)) == [0, 1, 2]
    assert list(N.nms_rows(pred, 2, 0.3, 0.5, agnostic=True)) == [0, 2]


def test_order_is_score_descending_with_ties_to_the_lower_row():
    pred = np.stack([_row(300.0, 300.0, 10.0, 0.5, 0), _row(100.0, 100.0, 10.0, 0.9, 0), _row(200.0, 200.0, 10.0, 0.5, 0),
                     _row(400.0, 400.0, 10.0, 0.2, 0)])
    order, _, _ = N.score_order(pred, 2, 0.3)
    assert list(order) == [1, 0, 2]
    assert list(N.score_order(pred, 2, 0.3, max_candidates=2)[0]) == [1, 0]


def test_exact_duplicate_is_removed():
    pred = np.stack([_row(100.0, 100.0, 17.5, 0.9, 0)] * 2)
    assert N.iou_matrix(pred)[0, 1] == pytest.approx(1.0, abs=1e-12)
    assert list(N.nms_rows(pred, 2, 0.3, 0.99)) == [0]


def test_nan_row_is_kept_and_removes_nobody():
    pred = np.stack([_row(100.0, 100.0, 20.0, 0.9, 0), _row(100.0, 100.0, 20.0, 0.8, 0), _row(101.0, 100.0, 20.0, 0.7, 0)])
    pred[0, 5] = np.nan                                                           # the best row: would remove both others
    assert list(N.nms_rows(pred, 2, 0.3, 0.5)) == [0, 1]
    pred = np.stack([_row(100.0, 100.0, 20.0, 0.9, 0), _row(100.0, 100.0, 20.0, 0.8, 0)])
    pred[1, 5] = np.nan                                                           # a NaN candidate is not removed either
    assert list(N.nms_rows(pred, 2, 0.3, 0.5)) == [0, 1]


def test_max_candidates_drops_the_tail():
    pred = S.scene("edges_b")[3]
    order, _, _ = N.score_order(pred, S.C, S.CONF_THRE)
    assert len(order) == 129
    best = set(order[:64].tolist())
    kept = S.oracle_keep("edges_b", False, 64)[3]
    assert set(kept) <= best and 0 < len(kept) < 64
    full = S.oracle_keep("edges_b", False, None)[3]
    assert kept == tuple(a for a in N.nms_rows(pred, S.C, S.CONF_THRE, S.NMS_THRE, False, 64))
    assert len(full) >= len(kept)


# ---------------------------------------------------------------------------------------------------- the GPU file's scenes
def test_scenes_have_the_candidate_counts_they_claim():
    seen = set()
    for name in S.SCENES:
        for img, n in zip(S.scene(name), S.counts(name)):
            assert len(N.score_order(img, S.C, S.CONF_THRE)[0]) == n
            seen.add(n)
    assert {0, 1, 2, 63, 64, 65, 128, 129, 200} <= seen
    M = N.iou_matrix(S.scene("dense200")[0][N.score_order(S.scene("dense200")[0], S.C, S.CONF_THRE)[0]])
    assert int((np.triu(M, 1) > 0).sum()) >= 1000                                 # the bit-equality test's overlapping pairs


@pytest.mark.parametrize("name,agnostic,max_candidates", S.ORACLE_SCENES)
def test_decision_margins_of_the_gpu_scenes(name, agnostic, max_candidates):
    """A GPU IoU within 1e-9 of the oracle's (tests/test_gpu_poly24.py) cannot flip a decision that is 1e-6 away."""
    worst = min(N.decision_margin(img, S.C, S.CONF_THRE, S.NMS_THRE, agnostic, max_candidates) for img in S.scene(name))
    print("%s agnostic=%s K=%s: min |iou - thr| = %.3e" % (name, agnostic, max_candidates, worst))
    assert worst >= S.MARGIN
    # the suppression does something in the scene: some candidates go, some stay
    n_in = sum(min(n, max_candidates or n) for n in S.counts(name))
    n_kept = sum(len(k) for k in S.oracle_keep(name, agnostic, max_candidates))
    assert 0 < n_kept < n_in or n_in <= 2
