"""Numpy float64 restatement of the polygon NMS contract (include/ep24.h ``ep24_post_nms_poly24``),
written from the contract and independently of csrc/polynms.hip.

* ``score_order``: candidates (``obj * class_conf >= conf_thre`` in fp32) and their order (score descending, ties to the lower
  row), cut to the ``max_candidates`` best.
* ``iou_matrix``: ``poly24_oracle.poly24_iou`` of the candidates' own 24 points (``poly24_oracle.det_polygons``), row = suppressor.
* ``greedy``: the greedy pass over any IoU matrix - class-aware or agnostic, ``iou > float32(thr)``, a NaN never suppresses.
"""
import numpy as np

import poly24_oracle as P


def score_order(pred, num_classes, conf_thre, max_candidates=None):
    """pred [A, 27 + C] -> (order, class_conf [A], class_pred [A]): ``order`` = the candidate rows, best first."""
    p = np.asarray(pred, dtype=np.float32)
    cc = p[:, 27:27 + num_classes]
    cls = np.argmax(cc, 1)                                                       # the first maximum, as torch.max
    conf = cc[np.arange(len(p)), cls]
    score = (p[:, 26] * conf).astype(np.float32)
    with np.errstate(invalid="ignore"):
        cand = np.nonzero(score >= np.float32(conf_thre))[0]                      # a NaN score is no candidate
    order = cand[np.lexsort((cand, -score[cand].astype(np.float64)))]
    if max_candidates is not None:
        order = order[:max_candidates]
    return order, conf, cls


def iou_matrix(rows26):
    """[n, >= 26] detection rows -> [n, n] float64, entry (i, j) = poly24_iou(a = P_i, b = P_j)."""
    poly = P.det_polygons(rows26)
    return P.poly24_iou(poly, poly)


def greedy(iou, cls, thr, agnostic=False):
    """Positions kept by greedy NMS over candidates 0 .. n-1 in their order: j is removed by a kept i < j iff the classes agree
    (or ``agnostic``) and iou[i, j] > (double)(float)thr."""
    n = len(cls)
    cls = np.asarray(cls)
    t = np.float64(np.float32(thr))
    removed = np.zeros(n, bool)
    keep = []
    for i in range(n):
        if removed[i]:
            continue
        keep.append(i)
        with np.errstate(invalid="ignore"):
            hit = np.asarray(iou[i]) > t                                          # False for NaN
        hit[:i + 1] = False
        if not agnostic:
            hit &= cls == cls[i]
        removed |= hit
    return keep


def nms_rows(pred, num_classes, conf_thre, nms_thre, agnostic=False, max_candidates=None, iou=None):
    """Kept rows of one image in NMS order.  ``iou``: a function order -> [n, n] matrix in place of the oracle's own."""
    order, conf, cls = score_order(pred, num_classes, conf_thre, max_candidates)
    if len(order) == 0:
        return order
    p = np.asarray(pred, dtype=np.float32)
    M = iou_matrix(p[order]) if iou is None else iou(order)
    return order[greedy(M, cls[order], nms_thre, agnostic)]


def postprocess(prediction, num_classes, conf_thre=0.7, nms_thre=0.45, class_agnostic=False, max_candidates=None):
    """[B, A, 27 + C] -> per image None or [n, 29] fp32 = (row[:27], class_conf, class_pred), as ``ep24.infer.postprocess``."""
    out = []
    for pred in np.asarray(prediction, dtype=np.float32):
        _, conf, cls = score_order(pred, num_classes, conf_thre)
        keep = nms_rows(pred, num_classes, conf_thre, nms_thre, class_agnostic, max_candidates)
        if len(keep) == 0:
            out.append(None)
            continue
        out.append(np.concatenate([pred[keep, :27], conf[keep, None], cls[keep, None].astype(np.float32)], 1))
    return out


def decision_margin(pred, num_classes, conf_thre, nms_thre, agnostic=False, max_candidates=None):
    """min |iou - thr| over the candidate pairs the class rule lets decide anything (inf when there is none): how far the scene
    stays from a decision that a last-bit difference in the IoU could flip."""
    order, _, cls = score_order(pred, num_classes, conf_thre, max_candidates)
    if len(order) < 2:
        return np.inf
    M = iou_matrix(np.asarray(pred, dtype=np.float32)[order])
    c = cls[order]
    pair = np.triu(np.ones(M.shape, bool), 1)
    if not agnostic:
        pair &= c[:, None] == c[None, :]
    pair &= ~np.isnan(M)
    if not pair.any():
        return np.inf
    return float(np.abs(M[pair] - np.float64(np.float32(nms_thre))).min())
