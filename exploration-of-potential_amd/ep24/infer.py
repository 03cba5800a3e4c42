"""Inference-side mirror of the reference: ``postprocess`` (yolox_24p/utils/boxes.py:29-99).

The eval-mode network itself is ``model.eval(); model(images, train=False)`` (ep24.nn / ep24.engine.forward_eval):
decoded predictions ``[B, A, 27 + C]`` with sigmoid objectness / class scores, as ``YOLOXHead`` returns them with
``decode_in_inference`` (yolo_head_24p.py:190-210, 239-256).
"""
import torch

from . import _lib
from ._lib import call, ptr, stream_ptr


class _Scratch:
    def __init__(self, B, A, dev):
        self.key = (B, A, str(dev))
        P = 1
        while P < A:
            P <<= 1
        self.P = P
        f = dict(device=dev)
        self.score = torch.empty(B * A, dtype=torch.float32, **f)
        self.conf = torch.empty(B * A, dtype=torch.float32, **f)
        self.cls = torch.empty(B * A, dtype=torch.int32, **f)
        self.rect = torch.empty(B * A * 4, dtype=torch.float32, **f)
        self.skey = torch.empty(B * P, dtype=torch.float32, **f)
        self.sidx = torch.empty(B * P, dtype=torch.int32, **f)
        self.dead = torch.empty(B * P, dtype=torch.uint8, **f)
        self.keep = torch.empty(B * A, dtype=torch.int32, **f)
        self.count = torch.zeros(B, dtype=torch.int32, **f)
        theta = torch.arange(24) * torch.tensor(15 * 3.141592653589793 / 180)          # boxes.py:31-33, fp32
        self.ray = torch.cat((theta * torch.cos(theta), theta * torch.sin(theta))).float().to(dev)
        self._poly = {}

    def poly(self, K):
        """The polygon NMS's buffers for K candidates per image, allocated when that path first runs with this K: vertices,
        boxes, classes and the suppression matrix, ``K * ceil(K / 64) * 8`` bytes per image (8.9 MB at K = 8 400, 141 MB at
        33 600; ``max_candidates`` sizes it)."""
        ps = self._poly.get(K)
        if ps is None:
            from .evaluate import ray_cos_sin
            B, dev = self.key[0], self.score.device
            self._poly.clear()                             # one live K at a time: the matrix is the large part of the scratch
            ps = self._poly[K] = _PolyScratch()
            ps.n_cand = torch.zeros(B, dtype=torch.int32, device=dev)
            ps.verts = torch.empty(B * K * 48, dtype=torch.float32, device=dev)
            ps.vbox = torch.empty(B * K * 4, dtype=torch.float32, device=dev)
            ps.vcls = torch.empty(B * K, dtype=torch.int32, device=dev)
            ps.mask = torch.empty(B * K * ((K + 63) // 64), dtype=torch.int64, device=dev)
            ps.cs = torch.from_numpy(ray_cos_sin()).to(dev)
        return ps


class _PolyScratch:
    pass


_scratch = {}
NMS_IOUS = ("rect", "poly24")


def check_nms_iou(nms_iou, max_candidates):
    """The argument rules of ``postprocess`` and ``Evaluator24``, checked before anything touches the GPU."""
    if nms_iou not in NMS_IOUS:
        raise ValueError("nms_iou must be one of %s, got %r" % (list(NMS_IOUS), nms_iou))
    if max_candidates is not None:
        if nms_iou == "rect":
            raise ValueError("max_candidates belongs to nms_iou='poly24'; the rectangle path takes every candidate")
        if int(max_candidates) < 1:
            raise ValueError("max_candidates must be at least 1, got %r" % (max_candidates,))


def check_vote(nms_iou, max_candidates, vote_thre):
    """``check_nms_iou``'s rules plus those of ``vote_thre``: ``None`` (no voting) or a threshold >= 0 on the polygons' area IoU,
    which belongs to ``nms_iou="poly24"`` - the voters are found in the buffers the polygon NMS leaves behind."""
    check_nms_iou(nms_iou, max_candidates)
    if vote_thre is None:
        return
    if isinstance(vote_thre, bool) or not isinstance(vote_thre, (int, float)):
        raise ValueError("vote_thre must be None or a number, got %r" % (vote_thre,))
    if nms_iou != "poly24":
        raise ValueError("vote_thre belongs to nms_iou='poly24'; the rectangle path keeps no polygon of the candidates it removes")
    if not float(vote_thre) >= 0.0:
        raise ValueError("vote_thre must be at least 0 (the voters' box pre-test is exact from there), got %r" % (vote_thre,))


def vote_poly24(ws, pred, ncols, B, A, vote_thre, class_agnostic, max_candidates, s):
    """``ep24_post_vote_poly24`` (csrc/tta.hip) after ``nms_poly24`` on the same ``ws`` and arguments: -> (voted [B, A, 26],
    n_voters [B, A]); row m of image b belongs to ``ws.keep[b * A + m]``, rows from ``ws.count[b]`` on are not written.  One
    launch, no host synchronisation."""
    K = A if max_candidates is None else min(int(max_candidates), A)
    ps = ws.poly(K)
    if getattr(ps, "voted", None) is None:
        ps.voted = torch.empty(B, A, 26, dtype=torch.float32, device=pred.device)
        ps.n_voters = torch.empty(B, A, dtype=torch.int32, device=pred.device)
    call("post_vote_poly24", ptr(pred), ncols, ptr(ws.score), B, A, K, float(vote_thre), 1 if class_agnostic else 0,
         ptr(ws.sidx), ws.P, ptr(ps.n_cand), ptr(ps.verts), ptr(ps.vbox), ptr(ps.vcls), ptr(ws.keep), ptr(ws.count), ptr(ps.voted),
         ptr(ps.n_voters), s)
    return ps.voted, ps.n_voters


def nms_poly24(ws, pred, ncols, B, A, nms_thre, class_agnostic, max_candidates, s):
    """The four launches of csrc/polynms.hip on ``post_prepare``'s outputs in ``ws``: ``ws.keep`` / ``ws.count`` as ``post_nms``
    leaves them.  No host synchronisation."""
    K = A if max_candidates is None else min(int(max_candidates), A)
    ps = ws.poly(K)
    call("post_nms_poly24", ptr(pred), ncols, ptr(ws.score), ptr(ws.cls), B, A, K, float(nms_thre), 1 if class_agnostic else 0,
         ptr(ps.cs), ptr(ws.skey), ptr(ws.sidx), ws.P, ptr(ps.n_cand), ptr(ps.verts), ptr(ps.vbox), ptr(ps.vcls), ptr(ps.mask),
         ptr(ws.keep), ptr(ws.count), s)


def postprocess(prediction, num_classes, conf_thre=0.7, nms_thre=0.45, class_agnostic=False, nms_iou="rect", max_candidates=None,
                vote_thre=None):
    """``prediction [B, A, 27 + C]`` (decoded, sigmoid scores) -> list of B entries: ``None`` (nothing kept) or
    ``[n, 29]`` = (cx, cy, 24 radii, obj_conf, class_conf, class_pred) in NMS order.  Three launches + one small D2H copy
    of the per-image counts; rectangle / score / NMS semantics are the reference's (torchvision batched_nms).

    ``nms_iou="poly24"`` keeps candidates, order and class rule and suppresses by the exact area IoU of the detections' own
    24 points instead (``poly24_iou`` > ``nms_thre``; csrc/polynms.hip, four launches in place of the NMS one).  The reference's
    rectangle is not the polygon's box - two touching circles of radius 10 lose one member to it.  ``max_candidates=K`` lets only
    the K best candidates of an image enter NMS and drops the others (``None``: all of them, exact greedy NMS).  The path's
    scratch - above all the suppression matrix, ``K * ceil(K / 64) * 8`` bytes per image: 8.9 MB at K = A = 8 400, 141 MB at
    33 600 - is allocated per (B, A, K) when the path first runs and kept.

    ``vote_thre=T`` (with ``nms_iou="poly24"`` only; ``None``: no voting, nothing changes): polygon voting.  One more launch
    (``ep24_post_vote_poly24``) replaces the first 26 columns of every kept row by the score-weighted consensus of the candidates
    whose area IoU with it is above ``T`` - the ones NMS removed in its favour when ``T >= nms_thre``; ``obj_conf``,
    ``class_conf``, class and order stay the kept row's.  A row that only itself votes for is returned bit for bit."""
    check_vote(nms_iou, max_candidates, vote_thre)
    _lib.require_gpu()
    if not prediction.is_cuda:
        raise _lib.Ep24Error("ep24: predictions must live on the GPU (no CPU fallback on the product path)")
    if prediction.dim() != 3 or prediction.shape[2] != 27 + num_classes:
        raise IndexError("expected predictions [B, A, 27 + %d], got %s" % (num_classes, tuple(prediction.shape)))
    B, A, ncols = prediction.shape
    output = [None for _ in range(B)]
    if A == 0 or B == 0:
        return output
    pred = prediction.detach().float().contiguous()
    key = (B, A, str(pred.device))
    ws = _scratch.get(key)
    if ws is None:
        ws = _scratch[key] = _Scratch(B, A, pred.device)
    s = stream_ptr()
    call("post_prepare", ptr(pred), ncols, num_classes, B * A, float(conf_thre), ptr(ws.ray), ptr(ws.score), ptr(ws.conf),
         ptr(ws.cls), ptr(ws.rect), s)
    if nms_iou == "poly24":
        nms_poly24(ws, pred, ncols, B, A, nms_thre, class_agnostic, max_candidates, s)
        if vote_thre is not None:
            voted, _ = vote_poly24(ws, pred, ncols, B, A, vote_thre, class_agnostic, max_candidates, s)
    else:
        call("post_nms", ptr(ws.score), ptr(ws.cls), ptr(ws.rect), B, A, float(nms_thre), 1 if class_agnostic else 0, ptr(ws.skey),
             ptr(ws.sidx), ptr(ws.dead), ptr(ws.keep), ptr(ws.count), ws.P, s)
    counts = ws.count.tolist()                                   # the API returns per-image tensors: one sync
    for b, n in enumerate(counts):
        if n == 0:
            continue
        det = torch.empty(n, 29, dtype=torch.float32, device=pred.device)
        call("post_gather", ptr(pred, b * A * ncols), ncols, ptr(ws.conf, b * A), ptr(ws.cls, b * A), ptr(ws.keep, b * A), n,
             ptr(det), s)
        if vote_thre is not None:
            det[:, :26] = voted[b, :n]
        output[b] = det
    return output
