"""COCO "segm" evaluation on the GPU: the 12-line summary of pycocotools' ``COCOeval(gt, dt, "segm")`` for a ground-truth
file and a result file (``ep24.results.SegmResults``, ``show_24p.py --save-segm``), without pycocotools and without a pixel or
an IoU on the host (csrc/segmeval.hip; include/ep24.h section E6).

``SegmEvaluator(gt).add_results(results)`` then ``evaluate()``.  The host does the bookkeeping with numpy (``build_plan``):
annotations and results grouped by (image, category) in the order of the sorted ids, results of an unknown image or category
dropped, a group's results ordered by (score descending, input order) and cut at the largest ``max_dets``, the float64 scores
turned into ``score_rank`` - the dense rank among the run's distinct scores, 0 the highest - so that two results whose scores
differ only beyond fp32 keep pycocotools' order in the 64-bit sort key.  The images are walked in chunks of at most
``chunk_bytes`` of decoded masks; per chunk ``cocomask.decode_batch``, ``ep24_rle_pack_bytes``, ``ep24_segm_mask_stats``,
``ep24_segm_iou`` and ``ep24_segm_match`` run on the device, at the end ``ep24_eval_sort`` and ``ep24_segm_accumulate``, and the
precision / recall tables come back in one copy.  As in pycocotools' ``loadRes`` a result's area is the pixel count of its mask;
a GT's area is the annotation's ``area`` field and its ignore flag the annotation's ``ignore`` OR ``iscrowd``.

``SegmEvaluator(gt, iou_type="boundary")`` scores the same results by Boundary IoU (Cheng et al., CVPR 2021; include/ep24.h section
E7): every pair's IoU becomes ``min(mask IoU, IoU of the two masks' boundary bands)``, the band being the mask pixels within
``d = max(1, round(dilation_ratio * image diagonal))`` pixels of the mask's outside.  Per chunk ``ep24_mask_boundary`` writes the
bands into a second packed buffer (each mask with its own image's ``d``), ``ep24_segm_mask_stats`` and ``ep24_segm_iou`` run on them
as on the masks (a crowd GT divides by the area of the detection's band) and ``ep24_segm_iou_min`` folds the second IoU table into
the first; the matcher, the areas of the area ranges (the MASK's pixel count) and everything after are those of "segm".
"""
import json
import math

import numpy as np
import torch

from . import _lib, cocomask
from ._lib import Ep24Error, call, ptr, stream_ptr
from .evaluate import IOU_THRS, REC_THRS, sort_records

AREA_RANGES = ((0 ** 2, 1e5 ** 2), (0 ** 2, 32 ** 2), (32 ** 2, 96 ** 2), (96 ** 2, 1e5 ** 2))
AREA_LABELS = ("all", "small", "medium", "large")
MAX_DETS_LIMIT = 128                                     # the position in the group takes 7 bits of the record key
MAX_AREA_RANGES = 4
MAX_MAX_DETS = 4
MAX_IMAGES = 1 << 25
MAX_CLASSES = 65535
IOU_TYPES = ("segm", "boundary")


def dilation(h, w, ratio=0.02):
    """The radius of the boundary band of an ``h x w`` image: ``max(1, round(ratio * diagonal))``, Python's round (half to even)."""
    return max(1, int(round(ratio * math.sqrt(h * h + w * w))))


def _load(obj, what):
    if isinstance(obj, (str, bytes)) or hasattr(obj, "__fspath__"):
        with open(obj) as f:
            try:
                return json.load(f)
            except json.JSONDecodeError as e:
                raise ValueError("%s: not JSON (%s)" % (what, e))
    return obj


def _need(rec, key, what):
    if not isinstance(rec, dict) or key not in rec:
        raise ValueError("%s without %r" % (what, key))
    return rec[key]


def _check_segmentation(seg, h, w, what):
    if isinstance(seg, dict):
        size = _need(seg, "size", what + ": RLE")
        _need(seg, "counts", what + ": RLE")
        if [int(v) for v in size] != [h, w]:
            raise ValueError("%s: the segmentation's size %s is not the image's %s" % (what, list(size), [h, w]))
    elif not isinstance(seg, (list, tuple)) or not seg:
        raise ValueError("%s: a segmentation is an RLE dict or a list of polygons" % what)


def load_gt(gt):
    """A COCO instances dict (or its path) -> the tables of the evaluation: sorted ``img_ids`` / ``cat_ids``, ``sizes`` [I, 2]
    and per annotation image index, category index, area, iscrowd, ignore0 = ignore OR iscrowd, segmentation."""
    gt = _load(gt, "ground truth")
    if not isinstance(gt, dict):
        raise ValueError("ground truth: a COCO instances dict with images, annotations and categories")
    images, anns, cats = (_need(gt, k, "ground truth") for k in ("images", "annotations", "categories"))
    img_ids = sorted({_need(im, "id", "image") for im in images})
    cat_ids = sorted({_need(c, "id", "category") for c in cats})
    if len(img_ids) != len(images) or len(cat_ids) != len(cats):
        raise ValueError("ground truth: image ids and category ids must be unique")
    ii, ci = {v: n for n, v in enumerate(img_ids)}, {v: n for n, v in enumerate(cat_ids)}
    sizes = np.zeros((len(img_ids), 2), dtype=np.int64)
    for im in images:
        sizes[ii[im["id"]]] = (int(_need(im, "height", "image")), int(_need(im, "width", "image")))
    if len(sizes) and sizes.min() < 1:
        raise ValueError("ground truth: image height and width must be positive")
    n = len(anns)
    t = {"img_ids": img_ids, "cat_ids": cat_ids, "sizes": sizes, "img": np.zeros(n, dtype=np.int64), "cat": np.zeros(n, dtype=np.int64),
         "area": np.zeros(n, dtype=np.float64), "crowd": np.zeros(n, dtype=np.uint8), "ignore0": np.zeros(n, dtype=np.uint8), "seg": []}
    for k, a in enumerate(anns):
        what = "annotation %s" % (a.get("id", k) if isinstance(a, dict) else k)
        i, c = _need(a, "image_id", what), _need(a, "category_id", what)
        if i not in ii or c not in ci:
            raise ValueError("%s names image %r / category %r, which the file does not list" % (what, i, c))
        t["img"][k], t["cat"][k] = ii[i], ci[c]
        t["area"][k] = float(_need(a, "area", what))
        t["crowd"][k] = 1 if a.get("iscrowd", 0) else 0
        t["ignore0"][k] = 1 if (a.get("ignore", 0) or a.get("iscrowd", 0)) else 0
        seg = _need(a, "segmentation", what)
        _check_segmentation(seg, int(sizes[ii[i], 0]), int(sizes[ii[i], 1]), what)
        t["seg"].append(seg)
    return t


def score_ranks(scores):
    """Dense rank of every float64 score among the distinct scores, 0 = the highest."""
    s = np.asarray(scores, dtype=np.float64).reshape(-1)
    u = np.unique(s)
    return (len(u) - 1 - np.searchsorted(u, s)).astype(np.int32)


def build_plan(gt, results, cut):
    """The grouping of an evaluation, numpy only.  ``gt``: ``load_gt``'s tables; ``results``: the list of result dicts in input
    order; ``cut``: the largest maxDets.  -> dict: ``groups`` [J, 2] (image index, category index) in image-major order - every
    pair with a GT or a kept result; per group ``gt_first``, ``G``, ``dt_first``, ``D``; ``gt_ann`` (annotation indices in group
    order, each group's in file order); ``dt_res`` (result indices in record order: a group's by (score descending, input order),
    at most ``cut``); ``score`` and ``score_rank`` of the records; ``dropped`` (results of an unknown image or category)."""
    K = len(gt["cat_ids"])
    ii, ci = {v: n for n, v in enumerate(gt["img_ids"])}, {v: n for n, v in enumerate(gt["cat_ids"])}
    n = len(results)
    r_img, r_cat, score = np.zeros(n, dtype=np.int64), np.zeros(n, dtype=np.int64), np.zeros(n, dtype=np.float64)
    for k, r in enumerate(results):
        what = "result %d" % k
        i, c = _need(r, "image_id", what), _need(r, "category_id", what)
        r_img[k], r_cat[k] = ii.get(i, -1), ci.get(c, -1)
        score[k] = float(_need(r, "score", what))
        seg = _need(r, "segmentation", what)
        if r_img[k] >= 0 and r_cat[k] >= 0:
            _check_segmentation(seg, int(gt["sizes"][r_img[k], 0]), int(gt["sizes"][r_img[k], 1]), what)
    if not np.isfinite(score).all():
        raise ValueError("result scores must be finite")
    valid = np.flatnonzero((r_img >= 0) & (r_cat >= 0))
    key = r_img[valid] * K + r_cat[valid]
    o = np.lexsort((valid, -score[valid], key))                                  # group, score descending, input order
    dt_res, dkey = valid[o], key[o]
    first = np.searchsorted(dkey, dkey, side="left")
    keep = np.arange(len(dkey)) - first < cut
    dt_res, dkey = dt_res[keep], dkey[keep]
    akey = gt["img"] * K + gt["cat"]
    ao = np.argsort(akey, kind="stable")
    gkey = akey[ao]
    keys = np.unique(np.concatenate([gkey, dkey]))
    g0, g1 = np.searchsorted(gkey, keys, side="left"), np.searchsorted(gkey, keys, side="right")
    d0, d1 = np.searchsorted(dkey, keys, side="left"), np.searchsorted(dkey, keys, side="right")
    return {"groups": np.stack([keys // K, keys % K], 1).astype(np.int64) if len(keys) else np.zeros((0, 2), dtype=np.int64),
            "gt_first": g0, "G": g1 - g0, "dt_first": d0, "D": d1 - d0, "gt_ann": ao, "dt_res": dt_res,
            "score": score[dt_res], "score_rank": score_ranks(score[dt_res]), "dropped": int(n - len(valid))}


def plan_chunks(plan, sizes, chunk_bytes):
    """Consecutive group ranges [j0, j1) that end on image boundaries and hold at most ``chunk_bytes`` of decoded masks (one byte
    per pixel of every GT and result mask); an image that alone exceeds the bound is a chunk of its own."""
    img = plan["groups"][:, 0]
    nbytes = (plan["G"] + plan["D"]) * sizes[img, 0] * sizes[img, 1] if len(img) else np.zeros(0, dtype=np.int64)
    out, j0, acc, j = [], 0, 0, 0
    J = len(img)
    while j < J:
        j1 = j
        while j1 < J and img[j1] == img[j]:
            j1 += 1
        b = int(nbytes[j:j1].sum())
        if j > j0 and acc + b > chunk_bytes:
            out.append((j0, j))
            j0, acc = j, 0
        acc += b
        j = j1
    if J > j0:
        out.append((j0, J))
    return out


def summarize_tables(precision, recall, max_dets, area_labels=AREA_LABELS):
    """pycocotools ``summarize``: (stats, lines).  With three maxDets and the four standard ranges these are its 12 numbers in its
    order: AP, AP50, AP75 and AP per further area range at the last maxDets, AR per maxDets, AR per further range."""
    def one(ap, t, a, m):
        s = precision[:, :, :, a, m] if ap else recall[:, :, a, m]
        if t is not None:
            s = s[t:t + 1]
        v = s[s > -1]
        v = float(np.mean(v)) if v.size else -1.0
        iou = "%0.2f:%0.2f" % (IOU_THRS[0], IOU_THRS[-1]) if t is None else "%0.2f" % IOU_THRS[t]
        return v, " {:<18} {} @[ IoU={:<9} | area={:>6s} | maxDets={:>3d} ] = {:0.3f}".format(
            "Average Precision" if ap else "Average Recall", "(AP)" if ap else "(AR)", iou, area_labels[a], int(max_dets[m]), v)
    last, NA = len(max_dets) - 1, precision.shape[3]
    rows = [one(True, None, 0, last), one(True, 0, 0, last), one(True, 5, 0, last)]
    rows += [one(True, None, a, last) for a in range(1, NA)]
    rows += [one(False, None, 0, m) for m in range(len(max_dets))]
    rows += [one(False, None, a, last) for a in range(1, NA)]
    return [r[0] for r in rows], [r[1] for r in rows]


class SegmEvaluator:
    """``SegmEvaluator(gt, max_dets=(1, 10, 100), area_ranges=COCO's four, device="cuda:0", chunk_bytes=256 MiB)``: ``gt`` a COCO
    instances dict or its path.  ``add_results(results)``: a list of result dicts (``image_id``, ``category_id``, ``score``,
    ``segmentation`` = an RLE dict, compressed or not, or a list of polygons), a path, or a ``SegmResults``; several calls add up.
    ``evaluate()`` -> dict with ``stats`` (the 12 numbers in pycocotools' order), ``precision`` [10, 101, K, A, M], ``recall``
    [10, K, A, M] and ``per_class_AP`` (range 0, the last maxDets); ``summary`` holds the printed lines.  ``iou_type="boundary"``
    with ``dilation_ratio`` (0.02): Boundary IoU in place of the mask IoU, everything else - and the summary's text - unchanged."""

    def __init__(self, gt, max_dets=(1, 10, 100), area_ranges=AREA_RANGES, device="cuda:0", chunk_bytes=256 << 20, area_labels=None,
                 iou_type="segm", dilation_ratio=0.02):
        if iou_type not in IOU_TYPES:
            raise ValueError("iou_type %r: one of %s" % (iou_type, IOU_TYPES))
        if isinstance(dilation_ratio, bool) or not isinstance(dilation_ratio, (int, float)) or not (math.isfinite(dilation_ratio) and dilation_ratio > 0):
            raise ValueError("dilation_ratio %r: a positive finite number" % (dilation_ratio,))
        self.iou_type, self.dilation_ratio = iou_type, float(dilation_ratio)
        self.max_dets = [int(m) for m in max_dets]
        self.area_ranges = np.asarray(area_ranges, dtype=np.float64).reshape(-1, 2)
        if not 1 <= len(self.max_dets) <= MAX_MAX_DETS or min(self.max_dets) < 1 or max(self.max_dets) > MAX_DETS_LIMIT:
            raise Ep24Error("ep24: max_dets=%s: 1 to %d values in 1..%d (EP24_E_UNSUPPORTED)" % (self.max_dets, MAX_MAX_DETS, MAX_DETS_LIMIT))
        if not 1 <= len(self.area_ranges) <= MAX_AREA_RANGES:
            raise Ep24Error("ep24: %d area ranges: 1 to %d (EP24_E_UNSUPPORTED)" % (len(self.area_ranges), MAX_AREA_RANGES))
        if area_labels is None:
            area_labels = AREA_LABELS if len(self.area_ranges) == 4 else ["a%d" % a for a in range(len(self.area_ranges))]
        self.area_labels = list(area_labels)
        if len(self.area_labels) != len(self.area_ranges):
            raise ValueError("one label per area range")
        if int(chunk_bytes) < 1:
            raise ValueError("chunk_bytes must be positive")
        self.gt = load_gt(gt)
        if not 1 <= len(self.gt["cat_ids"]) <= MAX_CLASSES:
            raise Ep24Error("ep24: %d categories: 1 to %d (EP24_E_UNSUPPORTED)" % (len(self.gt["cat_ids"]), MAX_CLASSES))
        if len(self.gt["img_ids"]) > MAX_IMAGES:
            raise Ep24Error("ep24: more than 2^25 images in one evaluation (EP24_E_UNSUPPORTED)")
        self.device, self.chunk_bytes = device, int(chunk_bytes)
        self.results = []
        self.stats = self.summary = self.plan = None
        self.chunks = 0

    def add_results(self, results):
        if hasattr(results, "records") and not isinstance(results, dict):
            results = results.records                                                # a SegmResults
        results = _load(results, "results")
        if not isinstance(results, (list, tuple)):
            raise ValueError("results: a list of result dicts")
        build_plan(self.gt, results, max(self.max_dets))                             # raises on a malformed record
        self.results.extend(results)
        return len(results)

    # ---- device pipeline ----------------------------------------------------------------------------
    def _chunk(self, plan, j0, j1, dev, thr, rng, rec, npig):
        """Groups [j0, j1): decode, pack, statistics, IoU, match.  The chunk's masks are its GTs, then its results in record order."""
        gt, s = self.gt, stream_ptr()
        G, D = plan["G"][j0:j1], plan["D"][j0:j1]
        ga0, da0 = int(plan["gt_first"][j0]), int(plan["dt_first"][j0])
        nG, nD = int(G.sum()), int(D.sum())
        J, n = j1 - j0, nG + nD
        if n == 0:
            return
        ann, res = plan["gt_ann"][ga0:ga0 + nG], plan["dt_res"][da0:da0 + nD]
        img = np.repeat(plan["groups"][j0:j1, 0], G), np.repeat(plan["groups"][j0:j1, 0], D)
        hw = gt["sizes"][np.concatenate(img)]
        segs = [gt["seg"][a] for a in ann] + [self.results[r]["segmentation"] for r in res]
        buf, desc = cocomask.decode_batch(segs, hw, dev)
        words = np.concatenate([[0], np.cumsum(hw[:, 0] * ((hw[:, 1] + 31) // 32))])
        if int(words[-1]) >= 1 << 40 or n >= 1 << 31:
            raise Ep24Error("ep24: a chunk of %d masks, %d words: lower chunk_bytes (EP24_E_UNSUPPORTED)" % (n, int(words[-1])))
        boundary = self.iou_type == "boundary"
        rad = np.array([dilation(int(h), int(w), self.dilation_ratio) for h, w in hw], dtype=np.int64) if boundary else np.zeros(n, dtype=np.int64)
        tab = torch.from_numpy(np.ascontiguousarray(np.stack([words[:-1], hw[:, 0], hw[:, 1], rad], 1))).to(dev)
        bits = torch.empty(int(words[-1]), dtype=torch.int32, device=dev)
        call("rle_pack_bytes", ptr(buf), buf.numel(), ptr(desc), ptr(tab), n, int(hw[:, 0].max()), ptr(bits), s)
        bbox = torch.empty(n, 4, dtype=torch.int32, device=dev)
        area = torch.empty(n, dtype=torch.int32, device=dev)
        call("segm_mask_stats", ptr(bits), ptr(tab), n, ptr(bbox), ptr(area), s)
        gfirst = np.concatenate([[0], np.cumsum(G)])
        dfirst = np.concatenate([[0], np.cumsum(D)])
        ioff = np.concatenate([[0], np.cumsum(G * D)])
        pairs = int(ioff[-1])
        gh = gt["sizes"][plan["groups"][j0:j1, 0]]
        z = np.zeros(J, dtype=np.int64)
        grp = np.stack([gh[:, 0], gh[:, 1], gfirst[:-1], G, nG + dfirst[:-1], D, ioff[:-1], z], 1)
        mgrp = np.stack([gfirst[:-1], G, dfirst[:-1], D, ioff[:-1], plan["groups"][j0:j1, 1], plan["groups"][j0:j1, 0], z], 1)
        tabs = torch.from_numpy(np.ascontiguousarray(np.concatenate([grp, mgrp]).astype(np.int64))).to(dev)
        crowd = np.zeros(max(n, 1), dtype=np.uint8)
        crowd[:nG] = gt["crowd"][ann]
        flags = torch.from_numpy(np.concatenate([crowd, gt["ignore0"][ann], np.zeros(1, dtype=np.uint8)])).to(dev)
        gt_area = torch.from_numpy(np.concatenate([gt["area"][ann], np.zeros(1)])).to(dev)
        dt_rank = torch.from_numpy(np.concatenate([plan["score_rank"][da0:da0 + nD], np.zeros(1, dtype=np.int32)])).to(dev)
        dt_area = area[nG:].to(torch.float64)
        iou = torch.empty(max(pairs, 1), dtype=torch.float64, device=dev)
        scratch = torch.empty(max(nG, 1), dtype=torch.int64, device=dev)
        call("segm_iou", ptr(bits), ptr(tab), n, ptr(bbox), ptr(area), ptr(flags), ptr(tabs), J, pairs, ptr(iou), None, s)
        if boundary:                                                                 # the bands' IoU, then the smaller of the two
            band = torch.empty_like(bits)
            band_bbox, band_area, band_iou = torch.empty_like(bbox), torch.empty_like(area), torch.empty_like(iou)
            call("mask_boundary", ptr(bits), ptr(tab), n, int(hw[:, 0].max()), int(hw[:, 1].max()), 0, ptr(band), s)
            call("segm_mask_stats", ptr(band), ptr(tab), n, ptr(band_bbox), ptr(band_area), s)
            call("segm_iou", ptr(band), ptr(tab), n, ptr(band_bbox), ptr(band_area), ptr(flags), ptr(tabs), J, pairs, ptr(band_iou), None, s)
            call("segm_iou_min", ptr(iou), ptr(band_iou), pairs, s)
        NA = len(self.area_ranges)
        call("segm_match", ptr(tabs, J * 8), J, ptr(iou), ptr(flags), ptr(flags, len(crowd)), ptr(gt_area), ptr(dt_area), ptr(dt_rank),
             ptr(rng), NA, ptr(thr), len(gt["cat_ids"]), ptr(scratch), ptr(rec["m"], da0 * NA), ptr(rec["key"], da0), ptr(rec["cls"], da0),
             ptr(npig), s)

    def evaluate(self):
        plan = self.plan = build_plan(self.gt, self.results, max(self.max_dets))
        _lib.require_gpu()
        dev = torch.device(self.device)
        K, NA, NM = len(self.gt["cat_ids"]), len(self.area_ranges), len(self.max_dets)
        n = len(plan["dt_res"])
        if n > 0x7FFFFFFF:
            raise Ep24Error("ep24: %d records: at most 2^31 - 1 (EP24_E_UNSUPPORTED)" % n)
        thr, rthr = torch.from_numpy(IOU_THRS.copy()).to(dev), torch.from_numpy(REC_THRS.copy()).to(dev)
        rng = torch.from_numpy(np.ascontiguousarray(self.area_ranges)).to(dev)
        md = torch.tensor(self.max_dets, dtype=torch.int32, device=dev)
        npig = torch.zeros(K * NA, dtype=torch.int32, device=dev)
        rec = {"m": torch.empty(max(n, 1) * NA, dtype=torch.int32, device=dev), "key": torch.empty(max(n, 1), dtype=torch.int64, device=dev),
               "cls": torch.empty(max(n, 1), dtype=torch.int32, device=dev)}
        chunks = plan_chunks(plan, self.gt["sizes"], self.chunk_bytes)
        self.chunks = len(chunks)
        for j0, j1 in chunks:
            self._chunk(plan, j0, j1, dev, thr, rng, rec, npig)
        order = sort_records(rec["key"][:n], rec["cls"][:n], 7 + max(len(self.gt["img_ids"]) - 1, 0).bit_length(), max(K - 1, 0).bit_length())
        np_, nr_ = 10 * 101 * K * NA * NM, 10 * K * NA * NM
        out = torch.empty(np_ + nr_, dtype=torch.float64, device=dev)
        ctp = torch.empty(NA * NM * max(n, 1), dtype=torch.int32, device=dev)
        env = torch.empty(NA * NM * max(n, 1), dtype=torch.float64, device=dev)
        call("segm_accumulate", ptr(order), ptr(rec["key"]), ptr(rec["cls"]), ptr(rec["m"]), n, ptr(npig), K, NA, ptr(md), NM, ptr(rthr),
             None, ptr(ctp), ptr(env), ptr(out), ptr(out, np_), stream_ptr())
        host = out.cpu().numpy()                                                     # the one device-to-host copy
        precision, recall = host[:np_].reshape(10, 101, K, NA, NM), host[np_:].reshape(10, K, NA, NM)
        stats, lines = summarize_tables(precision, recall, self.max_dets, self.area_labels)
        per_class = []
        for k in range(K):
            v = precision[:, :, k, 0, NM - 1]
            v = v[v > -1]
            per_class.append(float(np.mean(v)) if v.size else -1.0)
        self.summary = "\n".join(lines) + "\n"
        self.stats = {"stats": stats, "precision": precision, "recall": recall, "per_class_AP": np.array(per_class),
                      "category_ids": list(self.gt["cat_ids"]), "images": len(self.gt["img_ids"]), "results": len(self.results),
                      "dropped": plan["dropped"], "records": n, "chunks": self.chunks, "iou_type": self.iou_type,
                      "dilation_ratio": self.dilation_ratio}
        return self.stats
