"""Polygon NMS on the GPU (csrc/polynms.hip through ``postprocess(..., nms_iou="poly24")`` and the evaluator) against the
float64 oracle (tests/polynms_oracle.py) on the seeded scenes of tests/polynms_scenes.py, whose decisions all stay 1e-6 away
from the threshold (asserted in tests/test_polynms_oracle.py), and bit for bit against the kernel's own IoU matrix."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import polynms_oracle as N  # noqa: E402
import polynms_scenes as S  # noqa: E402
import test_gpu_eval24 as T  # noqa: E402
from ep24 import _lib, evaluate as E, infer, synth  # noqa: E402
from ep24._lib import ptr  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _post(pred, agnostic=False, max_candidates=None, thr=S.NMS_THRE, conf=S.CONF_THRE, nms_iou="poly24"):
    kw = {} if nms_iou is None else {"nms_iou": nms_iou}
    if max_candidates is not None:
        kw["max_candidates"] = max_candidates
    return infer.postprocess(torch.from_numpy(np.array(pred)).to(DEV), pred.shape[2] - 27, conf, thr, agnostic, **kw)


def _check(got, pred, keeps):
    """Per image: the kept rows, in order, are the oracle's - the [n, 29] tables equal bit for bit."""
    assert len(got) == len(keeps)
    for b, (g, keep) in enumerate(zip(got, keeps)):
        if not keep:
            assert g is None, b
            continue
        _, conf, cls = N.score_order(pred[b], S.C, S.CONF_THRE)
        k = np.array(keep)
        want = np.concatenate([pred[b][k, :27], conf[k, None], cls[k, None].astype(np.float32)], 1)
        assert g is not None and tuple(g.shape) == want.shape, (b, None if g is None else tuple(g.shape), want.shape)
        assert np.array_equal(g.cpu().numpy().view(np.uint32), want.view(np.uint32)), b


# ---- 1. keep lists equal the oracle's exactly -----------------------------------------------------------
@pytest.mark.parametrize("agnostic", [False, True])
@pytest.mark.parametrize("name", ["edges_a", "edges_b"])
def test_keep_lists_equal_the_oracle(name, agnostic):
    """Candidate counts 0, 1, 2, 63, 200 (edges_a: five images, one more than the other tests use, so that two calls cover the
    nine counts) and 64, 65, 128, 129 (edges_b): the word and wave boundaries of the bit matrix and of the scan."""
    pred = S.scene(name)
    _check(_post(pred, agnostic), pred, S.oracle_keep(name, agnostic))


# ---- 2. bit-equal on the kernel's own numbers ------------------------------------------------------------
def _gpu_matrix(rows26):
    """pairwise_iou's poly24 matrix of the rows against themselves: GT side = the rows' vertices formed in torch fp32 on the CPU
    (product, then sum), detection side = the rows, whose vertices the kernel forms."""
    q = torch.from_numpy(np.ascontiguousarray(rows26[:, :26]))
    cs = torch.from_numpy(E.ray_cos_sin())
    x = q[:, 0:1] + q[:, 2:26] * cs[None, :24]
    y = q[:, 1:2] + q[:, 2:26] * cs[None, 24:]
    gt50 = torch.cat([q[:, :2], torch.stack([x, y], -1).reshape(len(q), 48)], 1)
    return E.pairwise_iou(gt50.to(DEV), q.to(DEV), "poly24").cpu().numpy()


@pytest.mark.parametrize("agnostic", [False, True])
def test_keep_follows_the_kernels_own_iou_matrix_bit_for_bit(agnostic):
    pred = S.scene("dense200")
    img = pred[0]

    def iou(order):
        M = _gpu_matrix(img[order])
        assert int((np.triu(M, 1) > 0).sum()) >= 1000
        return M
    keep = N.nms_rows(img, S.C, S.CONF_THRE, S.NMS_THRE, agnostic, iou=iou)
    assert 0 < len(keep) < 200
    _check(_post(pred, agnostic), pred, [tuple(int(a) for a in keep)])


# ---- 3. stale scratch ------------------------------------------------------------------------------------
def test_scratch_of_a_larger_scene_does_not_leak_into_a_smaller_one():
    big, small = S.scene("dense200"), S.scene("three")
    assert big.shape == small.shape                                               # one (B, A): the same scratch
    assert sum(g.shape[0] for g in _post(big) if g is not None) > 3
    _check(_post(small), small, S.oracle_keep("three"))


def _abi_call(pred, fill, K=None, agnostic=0, thr=S.NMS_THRE):
    """ep24_post_prepare + ep24_post_nms_poly24 on buffers of the caller's, every scratch and output byte pre-filled with ``fill``."""
    B, A, ncols = pred.shape
    K = A if K is None else K
    P = 1
    while P < A:
        P <<= 1
    p = torch.from_numpy(np.array(pred)).to(DEV)
    ws = infer._Scratch(B, A, p.device)
    s = _lib.stream_ptr()
    _lib.call("post_prepare", ptr(p), ncols, ncols - 27, B * A, S.CONF_THRE, ptr(ws.ray), ptr(ws.score), ptr(ws.conf), ptr(ws.cls),
              ptr(ws.rect), s)

    def buf(n, dtype):
        return torch.full((n * torch.empty(0, dtype=dtype).element_size(),), fill, dtype=torch.uint8, device=DEV).view(dtype)
    skey, sidx = buf(B * P, torch.float32), buf(B * P, torch.int32)
    n_cand, verts, vbox, vcls = buf(B, torch.int32), buf(B * K * 48, torch.float32), buf(B * K * 4, torch.float32), buf(B * K, torch.int32)
    mask = buf(B * K * ((K + 63) // 64), torch.int64)
    keep, count = buf(B * A, torch.int32), buf(B, torch.int32)
    cs = torch.from_numpy(E.ray_cos_sin()).to(DEV)
    _lib.call("post_nms_poly24", ptr(p), ncols, ptr(ws.score), ptr(ws.cls), B, A, K, float(thr), agnostic, ptr(cs), ptr(skey), ptr(sidx),
              P, ptr(n_cand), ptr(verts), ptr(vbox), ptr(vcls), ptr(mask), ptr(keep), ptr(count), s)
    count, keep = count.cpu().numpy(), keep.cpu().numpy().reshape(B, A)
    return [tuple(int(a) for a in keep[b, :count[b]]) for b in range(B)], n_cand.cpu().numpy()


def test_abi_call_on_0xff_filled_buffers_equals_one_on_zeroed_buffers():
    pred = S.scene("edges_b")
    zero, nz = _abi_call(pred, 0)
    ones, no = _abi_call(pred, 0xFF)
    assert zero == ones and np.array_equal(nz, no) and list(nz) == list(S.counts("edges_b"))
    assert zero == list(S.oracle_keep("edges_b"))
    z64, n64 = _abi_call(pred, 0, K=64)
    o64, _ = _abi_call(pred, 0xFF, K=64)
    assert z64 == o64 == list(S.oracle_keep("edges_b", False, 64)) and list(n64) == [64, 64, 64, 64]


# ---- 4. max_candidates -----------------------------------------------------------------------------------
def test_max_candidates():
    pred = S.scene("edges_b")
    _check(_post(pred, max_candidates=64), pred, S.oracle_keep("edges_b", False, 64))
    full = _post(pred)
    for K in (129, S.A, 10 ** 6):                                                 # at or above every image's candidates: nothing changes
        for a, b in zip(_post(pred, max_candidates=K), full):
            assert torch.equal(a, b)


# ---- 5. the default path is untouched --------------------------------------------------------------------
def test_rect_is_the_default_and_unchanged():
    from oracle import post as opost
    raw = synth.make_raw_head(2, size=640, seed=7)
    pred = synth.decode_head(raw, size=640)
    pred[..., 26:] = torch.sigmoid(raw[..., 26:] + 3.0)
    plain = infer.postprocess(pred.to(DEV), 80, conf_thre=0.25, nms_thre=0.5)
    named = infer.postprocess(pred.to(DEV), 80, conf_thre=0.25, nms_thre=0.5, nms_iou="rect")
    want = opost.postprocess(pred.clone(), 80, conf_thre=0.25, nms_thre=0.5)
    assert any(w is not None and len(w) > 100 for w in want)
    for a, b, w in zip(plain, named, want):
        assert (a is None) == (b is None) == (w is None)
        if a is not None:
            assert torch.equal(a, b) and torch.equal(a.cpu(), w)


# ---- 6. the two-circle case ------------------------------------------------------------------------------
@pytest.mark.parametrize("d,thr", [(25.0, 0.45), (19.0, 0.65)])
def test_touching_circles(d, thr):
    pred = S.circles(d)
    rect = _post(pred, thr=thr, nms_iou=None)[0]
    poly = _post(pred, thr=thr)[0]
    assert rect.shape[0] == 1 and poly.shape[0] == 2
    assert np.array_equal(poly.cpu().numpy()[:, :27], pred[0][:, :27])            # both rows, the better one first
    assert _post(S.circles(2.0), thr=thr)[0].shape[0] == 1                        # IoU ~ 0.8: one goes on either path


# ---- 7. evaluator and trainer path -----------------------------------------------------------------------
def _same_evaluation(a, b):
    sa, sb = a.summarize(), b.summarize()
    assert a.n_records == b.n_records > 0
    ra, rb = a.records(), b.records()
    for k in ra:
        assert np.array_equal(ra[k], rb[k]), k
    assert np.array_equal(sa["precision"], sb["precision"]) and np.array_equal(sa["recall"], sb["recall"])
    return sa, sb


def test_evaluator_update_equals_update_detections_of_postprocess():
    B, S_, C = 2, 320, 80
    pred = synth.decode_head(synth.make_raw_head(B, S_, seed=21, num_classes=C), S_)
    pred[..., 26:] = torch.sigmoid(pred[..., 26:])
    pred = pred.to(DEV)
    labels = synth.make_labels(B, [6, 12], size=S_, seed=22).to(DEV)
    a = E.Evaluator24(C, iou_type="poly24", nms_iou="poly24")
    a.update(pred, labels)
    b = E.Evaluator24(C, iou_type="poly24")
    dets = infer.postprocess(pred, C, 0.01, 0.65, nms_iou="poly24")
    b.update_detections(dets, labels)
    sa, sb = _same_evaluation(a, b)
    assert sa["nms_iou"] == "poly24" and sb["nms_iou"] == "rect"
    rect = infer.postprocess(pred, C, 0.01, 0.65)
    assert sum(len(d) for d in dets) > sum(len(d) for d in rect)                  # the rectangle rule removes more


def test_exp_eval_with_poly24_nms_equals_the_decomposed_path():
    from ep24.input import TrainTransform
    exp = T._small_exp()
    exp.eval_iou_type = "poly24"
    exp.nms_iou_type = "poly24"
    torch.manual_seed(0)
    model = exp.get_model().to(DEV)
    ev = exp.get_evaluator(4)
    assert ev.iou_type == "poly24" and ev.nms_iou == "poly24"
    ap, ap50, summary = exp.eval(model, ev, False)
    assert model.training and "Average Precision" in summary and ev.stats["nms_iou"] == "poly24"
    ref = E.Evaluator24(exp.num_classes, iou_type="poly24", conf_thre=exp.test_conf, nms_thre=exp.nmsthre)
    model.eval()
    tt = TrainTransform(max_labels=50)
    with torch.no_grad():
        for images, targets, _, _ in exp.get_eval_loader(4):
            imgs, labs = tt.batch(images, targets, (320, 320))
            eng = model.engine(imgs.shape[0], 320)
            out = eng.forward_eval(imgs)
            ref.update_detections(infer.postprocess(out, exp.num_classes, exp.test_conf, exp.nmsthre, nms_iou="poly24"), labs)
    st = ref.summarize()
    model.train()
    assert ref.seq == 10 and ev.seq == 10
    assert np.all(np.isfinite(ev.stats["precision"])) and np.all(np.isfinite(ev.stats["recall"]))
    assert np.array_equal(st["precision"], ev.stats["precision"]) and np.array_equal(st["recall"], ev.stats["recall"])
    assert (ap, ap50) == (st["AP"], st["AP50"]) and np.isfinite(ap) and np.isfinite(ap50)


# ---- 8. repeatability and argument errors ----------------------------------------------------------------
def test_two_identical_calls_are_bit_equal():
    pred = S.scene("edges_a")
    for a, b in zip(_post(pred), _post(pred)):
        assert (a is None) == (b is None)
        if a is not None:
            assert torch.equal(a, b)


def test_nan_radius_row_is_kept_and_removes_nobody():
    pred = S.scene("nan")
    got = _post(pred)
    _check(got, pred, S.oracle_keep("nan"))
    for g in got:
        assert int(torch.isnan(g[:, 2:26]).any(1).sum()) == 1                     # the NaN row above the threshold is among the kept
    # a NaN row that duplicates the best candidate's centre removes nobody: both neighbours stay
    p = S.circles(2.0).copy()
    p[0, 0, 7] = np.nan
    assert _post(p)[0].shape[0] == 2


def test_negative_threshold_is_refused():
    pred = S.circles(25.0)
    with pytest.raises(_lib.Ep24Error):
        _post(pred, thr=-0.1)
    assert _post(pred, thr=-0.1, nms_iou="rect")[0].shape[0] == 1                 # the rectangle path takes it as before
