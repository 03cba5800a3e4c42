"""COCO-style AP of 24-point detections on the GPU (csrc/evaluate.hip).

The reference scores axis-aligned boxes through pycocotools and never wires an evaluator into its 24-point trainer
(exp/yolox_base.py ``get_evaluator`` is commented out).  ``Evaluator24`` gives the trainer a validation metric with the
semantics of pycocotools ``evaluateImg`` + ``accumulate`` for one area range ("all"), no crowd / ignore regions and one
``maxDets``, over three IoU types:

* ``"circle24"`` (default): the model's own geometry - per ray the IoU of the GT's and the detection's ray circles
  (``ray_inter`` of geom.h), averaged over the 24 rays in fp32.  A similarity in [0, 1], not the loss's GIoU.
* ``"rect"``: the bounding boxes of the 24 points (detections: c + r_k (cos, sin)(15 deg k)), IoU in float64.
* ``"poly24"``: the exact area IoU of the two 24-gons (GT vertices against the detection's 24 points) in float64
  (csrc/poly24.h): how well the predicted shape covers the object.

Matching (per image and class, all 10 thresholds), the sort of the records over the whole evaluation and the accumulation
run as HIP kernels; the host reads one count per batch and, in ``summarize``, the [10, 101, C] precision and [10, C] recall
tables once.  Torch only allocates and copies.

``Evaluator24(..., strata=[...], max_dets=(1, 10, 100))`` evaluates by object size and distortion zone as well (csrc/evalstrata.hip):
a ``Stratum`` is a range of object area (original-image pixels) and of a zone value of the object's centre - its distance from the
image centre (``radius_zones``) or its incidence angle through a calibrated lens (``lens_zones``) - and what lies outside a stratum is
ignored in it, as pycocotools ignores what lies outside an area range.  ``measure`` returns the two measures themselves.
"""
import numpy as np
import torch

from . import _lib
from ._lib import Ep24Error, call, ptr, stream_ptr

IOU_TYPES = {"circle24": 0, "rect": 1, "poly24": 2}
IOU_THRS = np.linspace(0.5, 0.95, 10)                    # float64, as pycocotools Params
REC_THRS = np.linspace(0.0, 1.0, 101)
MAX_GT_ROWS = 256
MAX_DETS = 128


def ray_cos_sin():
    """[48] fp32: cos(15 deg * k) then sin(15 deg * k), computed in float64 and rounded."""
    th = np.arange(24, dtype=np.float64) * (15.0 * np.pi / 180.0)
    return np.concatenate([np.cos(th), np.sin(th)]).astype(np.float32)


def _iou_type(iou_type):
    if iou_type not in IOU_TYPES:
        raise ValueError("iou_type must be one of %s, got %r" % (sorted(IOU_TYPES), iou_type))
    return IOU_TYPES[iou_type]


_consts = {}


def _device_consts(dev):
    key = str(dev)
    c = _consts.get(key)
    if c is None:
        c = _consts[key] = (torch.from_numpy(ray_cos_sin()).to(dev), torch.from_numpy(IOU_THRS.copy()).to(dev),
                            torch.from_numpy(REC_THRS.copy()).to(dev))
    return c


def pairwise_iou(gt50, det26, iou_type="circle24"):
    """IoU matrix [G, D] float64 of GT rows ``gt50 [G, 50]`` (centre + 24 vertices in pixels: label columns 1..50) against
    detections ``det26 [D, 26]`` (centre + 24 radii), both on the GPU."""
    _lib.require_gpu()
    t = _iou_type(iou_type)
    if not (gt50.is_cuda and det26.is_cuda):
        raise Ep24Error("ep24: pairwise_iou takes GPU tensors (no CPU fallback on the product path)")
    if gt50.dim() != 2 or gt50.shape[1] != 50 or det26.dim() != 2 or det26.shape[1] != 26:
        raise IndexError("expected gt50 [G, 50] and det26 [D, 26], got %s and %s" % (tuple(gt50.shape), tuple(det26.shape)))
    g = gt50.detach().float().contiguous()
    d = det26.detach().float().contiguous()
    out = torch.empty(g.shape[0], d.shape[0], dtype=torch.float64, device=g.device)
    cs, _, _ = _device_consts(g.device)
    call("eval_iou", ptr(g), ptr(d), g.shape[0], d.shape[0], t, ptr(cs), ptr(out), stream_ptr())
    return out


class _MatchScratch:
    """Per-batch buffers of the match kernel for B images of at most P detections and ``cap`` records."""

    def __init__(self, B, P, cap, dev, NA=0):
        f = dict(device=dev)
        self.sort = torch.empty(B * P, dtype=torch.int64, **f)
        self.key = torch.empty(cap, dtype=torch.int64, **f)
        self.cls = torch.empty(cap, dtype=torch.int32, **f)
        self.p = torch.empty(cap, dtype=torch.int32, **f)
        self.tp = torch.empty(cap * max(NA, 1), dtype=torch.int32, **f)      # with strata: rec_m [cap, NA]
        self.val = torch.empty(cap * 2, dtype=torch.float64, **f) if NA else None
        self.count = torch.zeros(1, dtype=torch.int32, **f)


_match_scratch = {}


def _h2d(a, dev):
    """A small host array on the device without a host synchronisation (page-locked staging, asynchronous copy)."""
    return torch.from_numpy(np.ascontiguousarray(a)).pin_memory().to(dev, non_blocking=True)


_row_offs = {}


def _pow2(n):
    P = 1
    while P < n:
        P <<= 1
    return P


def sort_records(key, cls, low_bits, cls_bits):
    """``ep24_eval_sort`` with its scratch: the int32 order of the records by (class, key), the passes covering the key's low
    ``low_bits`` bits, its high half and the class's low ``cls_bits`` bits."""
    n = key.numel()
    if n > 0x7FFFFFFF:
        raise Ep24Error("ep24: %d records: at most 2^31 - 1 (EP24_E_UNSUPPORTED)" % n)
    dev = key.device
    order = torch.empty(n, dtype=torch.int32, device=dev)
    if n:
        key_tmp = torch.empty(2 * n, dtype=torch.int64, device=dev)
        cls_tmp = torch.empty(2 * n, dtype=torch.int32, device=dev)
        idx_tmp = torch.empty(2 * n, dtype=torch.int32, device=dev)
        hist = torch.empty(256 * ((n + 4095) // 4096), dtype=torch.int32, device=dev)
        call("eval_sort", ptr(key), ptr(cls), n, low_bits, cls_bits, ptr(key_tmp), ptr(cls_tmp), ptr(idx_tmp), ptr(hist), ptr(order),
             stream_ptr())
    return order


# ---- strata: object size and distortion zone ----------------------------------------------------------------------------
MAX_STRATA = 8
MAX_MAXDETS = 4
ZT_D = 16            # doubles per image of the zone table: kind, fx, fy, cx, cy, k1..k4, theta_max, thetad(theta_max), 0...
ROW_KINDS = {"label": 0, "det": 1}


class Stratum:
    """``Stratum(name, area=(0, 1e10), zone=(0, inf))``: an object belongs to it iff ``area[0] <= A <= area[1]`` (original-image
    pixels, closed as pycocotools' area ranges) and ``zone[0] <= z < zone[1]`` (half open: zones partition).  What lies outside
    is ignored in the stratum's evaluation, as pycocotools ignores what lies outside an area range."""

    def __init__(self, name, area=(0.0, 1e10), zone=(0.0, float("inf"))):
        self.name = str(name)
        self.area = (float(area[0]), float(area[1]))
        self.zone = (float(zone[0]), float(zone[1]))
        if not self.area[0] <= self.area[1]:
            raise ValueError("Stratum %r: area range %r needs lo <= hi" % (self.name, self.area))
        if not self.zone[0] <= self.zone[1]:
            raise ValueError("Stratum %r: zone range %r needs lo <= hi" % (self.name, self.zone))

    def row(self):
        return self.area + self.zone

    def __repr__(self):
        return "Stratum(%r, area=%r, zone=%r)" % (self.name, self.area, self.zone)


def coco_area_strata():
    """pycocotools' four area ranges: all, small [0, 32^2], medium [32^2, 96^2], large [96^2, 1e10]."""
    return [Stratum("all"), Stratum("small", (0.0, 32.0 ** 2)), Stratum("medium", (32.0 ** 2, 96.0 ** 2)),
            Stratum("large", (96.0 ** 2, 1e10))]


def zone_strata(edges, unit=""):
    """One stratum per pair of consecutive ``edges`` (ascending; the last may be ``inf``), named ``"lo-hi" + unit``."""
    e = [float(x) for x in edges]
    if len(e) < 2 or any(not a < b for a, b in zip(e, e[1:])):
        raise ValueError("zone_strata: edges must ascend and hold at least two values, got %r" % (list(edges),))
    return [Stratum("%.4g-%.4g%s" % (a, b, unit), zone=(a, b)) for a, b in zip(e, e[1:])]


def letterbox_scales(sizes, input_dim):
    """The letterbox ratio r = min(S_h / h, S_w / w) of every raw (h, w): input pixels per original pixel."""
    return np.array([min(input_dim[0] / h, input_dim[1] / w) for h, w in sizes], dtype=np.float64)


def no_zones(n):
    """``n`` zone-table rows of kind 0: every zone value is 0."""
    return np.zeros((n, ZT_D), dtype=np.float64)


def radius_zones(sizes, input_dim):
    """Zone-table rows of kind 1 for raw images of ``sizes`` (h, w) letterboxed into ``input_dim``: the zone value is the centre's
    distance from the centre of the image content (pixel-index coordinates) in units of half the content's diagonal: 0 .. 1."""
    zt = no_zones(len(sizes))
    for i, (h, w) in enumerate(sizes):
        r = min(input_dim[0] / h, input_dim[1] / w)
        rh, rw = int(h * r), int(w * r)
        f = 0.5 * float(np.sqrt(float(rw) * rw + float(rh) * rh))
        zt[i, :5] = (1.0, f, f, (rw - 1) / 2.0, (rh - 1) / 2.0)
    return zt


def lens_zones(models):
    """Zone-table rows of kind 2 from ``ep24.lens.LensModel``s already in the input frame (``lens.image_model`` / ``scaled`` make
    those): the zone value is the incidence angle of the centre in degrees, ``inf`` beyond the field of view."""
    zt = no_zones(len(models))
    for i, m in enumerate(models):
        zt[i, :11] = (2.0,) + tuple(m.fish) + tuple(m.k) + (m.theta_max, float(m.thetad(m.theta_max)))
    return zt


def _check_tables(B, scales, zones):
    """-> (scales [B], zones [B, 16]) float64 host arrays; raises ValueError naming the argument."""
    sc = np.ones(B, dtype=np.float64) if scales is None else np.asarray(scales, dtype=np.float64).reshape(-1)
    zt = no_zones(B) if zones is None else np.asarray(zones, dtype=np.float64)
    if sc.shape != (B,) or not (np.isfinite(sc).all() and (sc > 0).all()):
        raise ValueError("scales: one finite positive factor per image (%d), got %r" % (B, sc))
    if zt.shape != (B, ZT_D):
        raise ValueError("zones: a [%d, %d] table (radius_zones / lens_zones), got shape %r" % (B, ZT_D, zt.shape))
    if not np.isfinite(zt).all():
        raise ValueError("zones: non-finite entries")
    for b in range(B):
        if zt[b, 0] not in (0.0, 1.0, 2.0):
            raise ValueError("zones: row %d has the unknown kind %r (0 none, 1 radius, 2 lens)" % (b, float(zt[b, 0])))
        if zt[b, 0] and not (zt[b, 1] > 0 and zt[b, 2] > 0):
            raise ValueError("zones: row %d needs positive fx, fy, got %r" % (b, zt[b, 1:3]))
    return sc, zt


def measure(rows, kind, image, scales, zones):
    """(area, zone) [n, 2] float64 on the GPU of ``rows``: label rows [n, 51] (``kind="label"``) or detection rows [n, >= 26]
    (``kind="det"``); ``image [n]`` names every row's entry of ``scales [B]`` and ``zones [B, 16]``."""
    _lib.require_gpu()
    if kind not in ROW_KINDS:
        raise ValueError("kind must be 'label' or 'det', got %r" % (kind,))
    if not rows.is_cuda:
        raise Ep24Error("ep24: measure takes GPU tensors (no CPU fallback on the product path)")
    if rows.dim() != 2 or rows.shape[1] < (51 if kind == "label" else 26):
        raise IndexError("expected rows [n, %s], got %s" % ("51" if kind == "label" else ">= 26", tuple(rows.shape)))
    sc = np.asarray(scales, dtype=np.float64).reshape(-1)
    sc, zt = _check_tables(len(sc), sc, zones)
    img = np.asarray(image.cpu() if isinstance(image, torch.Tensor) else image, dtype=np.int64).reshape(-1)
    n = rows.shape[0]
    if img.shape != (n,) or (n and (img.min() < 0 or img.max() >= len(sc))):
        raise ValueError("image: one index in [0, %d) per row (%d rows)" % (len(sc), n))
    dev = rows.device
    r = rows.detach().float().contiguous()
    out = torch.empty(n, 2, dtype=torch.float64, device=dev)
    cs, _, _ = _device_consts(dev)
    img_d, sc_d, zt_d = _h2d(img.astype(np.int32), dev), _h2d(sc, dev), _h2d(zt, dev)     # named: they live until the launch is queued
    call("eval_measure", ptr(r), r.shape[1], ROW_KINDS[kind], ptr(img_d), n, ptr(sc_d), ptr(zt_d), len(sc), ptr(cs), ptr(out), stream_ptr())
    return out


class Evaluator24:
    """``Evaluator24(num_classes, iou_type="circle24", max_dets=100, conf_thre=0.01, nms_thre=0.65, nms_iou="rect",
    max_candidates=None, vote_thre=None)``.  ``nms_iou`` / ``max_candidates`` / ``vote_thre`` are ``ep24.infer.postprocess``'s:
    ``"poly24"`` lets ``update`` suppress by the polygons' area IoU (class-aware, as its rectangle NMS is); with a ``vote_thre``
    (polygon voting, ``nms_iou="poly24"`` only) ``update`` is ``update_detections(postprocess(..., vote_thre=...))``.

    ``update(predictions, labels)``: decoded eval-mode predictions [B, A, 27 + C] (the evaluator runs post_prepare +
    post_nms itself) and the label table [B, L, 51]; ``update_detections(dets, labels)``: ``ep24.infer.postprocess`` output.
    Both give bit-identical results for the same detections.  ``summarize()`` returns a dict with ``AP`` (0.5:0.95),
    ``AP50``, ``AP75``, ``AR100``, ``per_class_AP`` and the tables; ``summary`` holds the printed form.

    ``strata``: a list of up to 8 ``Stratum`` (``coco_area_strata()``, ``zone_strata(...)``), and ``max_dets`` may then be an
    ascending tuple of up to 4 values.  ``update`` / ``update_detections`` take ``scales`` (input pixels per original pixel, default
    1) and ``zones`` (``radius_zones`` / ``lens_zones`` rows, default none) per image; the tables gain the axes [NA, NM]; the
    headline numbers are those of the first stratum at the largest maxDets and ``stats["strata"][name]`` holds every stratum's.
    With ``strata=None`` and an int ``max_dets`` every call, buffer and result is what it was without them."""

    def __init__(self, num_classes, iou_type="circle24", max_dets=100, conf_thre=0.01, nms_thre=0.65, device=None, nms_iou="rect",
                 max_candidates=None, vote_thre=None, strata=None):
        from .infer import check_vote
        check_vote(nms_iou, max_candidates, vote_thre)
        self.nms_iou, self.max_candidates, self.vote_thre = nms_iou, max_candidates, vote_thre
        if not 0 < int(num_classes) < 0xFFFF:
            raise Ep24Error("ep24: Evaluator24 takes 1 .. 65534 classes, got %d (EP24_E_UNSUPPORTED)" % num_classes)
        mds = tuple(int(m) for m in max_dets) if isinstance(max_dets, (tuple, list)) else (int(max_dets),)
        if not 1 <= len(mds) <= MAX_MAXDETS or any(not a < b for a, b in zip(mds, mds[1:])):
            raise Ep24Error("ep24: max_dets=%r: one value or an ascending tuple of up to %d (EP24_E_UNSUPPORTED)" % (max_dets, MAX_MAXDETS))
        if not 0 < mds[0] or mds[-1] > MAX_DETS:
            raise Ep24Error("ep24: max_dets=%r: at most %d detections per image and class (EP24_E_UNSUPPORTED)" % (max_dets, MAX_DETS))
        self.strata = None
        if strata is not None or isinstance(max_dets, (tuple, list)):
            self.strata = [Stratum("all")] if strata is None else list(strata)
            if not 1 <= len(self.strata) <= MAX_STRATA or not all(isinstance(s, Stratum) for s in self.strata):
                raise Ep24Error("ep24: strata: 1 .. %d Stratum objects, got %d (EP24_E_UNSUPPORTED)" % (MAX_STRATA, len(self.strata)))
            if len({s.name for s in self.strata}) != len(self.strata):
                raise ValueError("strata: names must differ, got %r" % [s.name for s in self.strata])
            self._strata_rows = np.array([s.row() for s in self.strata], dtype=np.float64)
        self.num_classes = int(num_classes)
        self.iou_type = iou_type
        self._t = _iou_type(iou_type)
        self._mds = mds
        self.max_dets = mds[-1] if self.strata is None else mds       # an int without strata, as ever
        self.conf_thre, self.nms_thre = float(conf_thre), float(nms_thre)
        self.device = device
        self.reset()

    def reset(self):
        self._recs = []                                   # per batch: (key, cls, p, m [n, NA], val [n, 2] or None) device tensors
        self._npig = None
        self._err = None
        self.seq = 0                                      # images seen: the next image's sequence number
        self.n_records = 0
        self.stats = None

    # ---- inputs ------------------------------------------------------------------------------------
    def _prepare(self, labels, dev):
        _lib.require_gpu()
        if labels.dim() != 3 or labels.shape[2] != 51:
            raise IndexError("expected labels [B, L, 51], got %s" % (tuple(labels.shape),))
        if labels.shape[1] > MAX_GT_ROWS:
            raise Ep24Error("ep24: %d GT rows per image: at most %d (EP24_E_UNSUPPORTED)" % (labels.shape[1], MAX_GT_ROWS))
        if self._npig is None:
            self.device = dev
            self._npig = torch.zeros(self.num_classes * (len(self.strata) if self.strata else 1), dtype=torch.int32, device=dev)
            self._err = torch.zeros(1, dtype=torch.int32, device=dev)
        return labels.detach().to(dev).float().contiguous()

    def _tables(self, B, scales, zones):
        """The per-image tables of a batch, checked on the host before any launch: None without strata."""
        if self.strata is None:
            if scales is not None or zones is not None:
                raise ValueError("scales / zones: this Evaluator24 has no strata to apply them to")
            return None
        return _check_tables(B, scales, zones)

    def update(self, predictions, labels, scales=None, zones=None):
        """predictions [B, A, 27 + C] decoded (sigmoid scores) on the GPU, labels [B, L, 51]; with strata, ``scales [B]`` and
        ``zones [B, 16]`` of the images."""
        _lib.require_gpu()
        tables = self._tables(len(predictions), scales, zones)
        if not predictions.is_cuda:
            raise Ep24Error("ep24: predictions must live on the GPU (no CPU fallback on the product path)")
        C = self.num_classes
        if predictions.dim() != 3 or predictions.shape[2] != 27 + C:
            raise IndexError("expected predictions [B, A, 27 + %d], got %s" % (C, tuple(predictions.shape)))
        B, A, ncols = predictions.shape
        if labels.shape[0] != B:
            raise IndexError("predictions hold %d images, labels %d" % (B, labels.shape[0]))
        if A > 65536:
            raise Ep24Error("ep24: %d anchors per image: at most 65536 (EP24_E_UNSUPPORTED)" % A)
        pred = predictions.detach().float().contiguous()
        lab = self._prepare(labels, pred.device)
        if B == 0 or A == 0:
            self.seq += B
            return
        from . import infer
        if self.vote_thre is not None:                    # the voted rows are no rows of `pred`: the evaluator takes them as a table
            self.update_detections(infer.postprocess(pred, C, self.conf_thre, self.nms_thre, False, self.nms_iou, self.max_candidates,
                                                     self.vote_thre), lab, scales, zones)
            return
        key = (B, A, str(pred.device))
        ws = infer._scratch.get(key)
        if ws is None:
            ws = infer._scratch[key] = infer._Scratch(B, A, pred.device)
        s = stream_ptr()
        call("post_prepare", ptr(pred), ncols, C, B * A, self.conf_thre, ptr(ws.ray), ptr(ws.score), ptr(ws.conf), ptr(ws.cls),
             ptr(ws.rect), s)
        if self.nms_iou == "poly24":
            infer.nms_poly24(ws, pred, ncols, B, A, self.nms_thre, False, self.max_candidates, s)
        else:
            call("post_nms", ptr(ws.score), ptr(ws.cls), ptr(ws.rect), B, A, self.nms_thre, 0, ptr(ws.skey), ptr(ws.sidx), ptr(ws.dead),
                 ptr(ws.keep), ptr(ws.count), ws.P, s)
        rk = (B, A, str(pred.device))
        row_off = _row_offs.get(rk)
        if row_off is None:
            row_off = _row_offs[rk] = _h2d(np.arange(B, dtype=np.int64) * A, pred.device)
        self._match(lab, pred, ncols, row_off, ws.keep, A, ws.count, ws.conf, ws.cls, B, _pow2(A), B * A, tables)

    def update_detections(self, dets, labels, scales=None, zones=None):
        """dets: list of B entries, None or [n, 29] (cx, cy, 24 radii, obj_conf, class_conf, class) as postprocess returns."""
        B = len(dets)
        if labels.shape[0] != B:
            raise IndexError("%d detection entries, labels hold %d images" % (B, labels.shape[0]))
        _lib.require_gpu()
        tables = self._tables(B, scales, zones)
        dev = next((d.device for d in dets if d is not None), labels.device)
        if dev.type != "cuda":
            dev = torch.device("cuda", torch.cuda.current_device())
        lab = self._prepare(labels, dev)
        counts, parts = [], []
        for d in dets:
            if d is None or d.shape[0] == 0:
                counts.append(0)
                continue
            if d.dim() != 2 or d.shape[1] != 29:
                raise IndexError("expected detections [n, 29], got %s" % (tuple(d.shape),))
            counts.append(int(d.shape[0]))
            parts.append(d.detach().to(dev).float())
        if B == 0:
            return
        if max(counts) > 65536:
            raise Ep24Error("ep24: %d detections in one image: at most 65536 (EP24_E_UNSUPPORTED)" % max(counts))
        N = sum(counts)
        if N == 0:
            rows = torch.zeros(1, 29, dtype=torch.float32, device=dev)
        else:
            rows = torch.cat(parts).contiguous()
        off = np.zeros(B, dtype=np.int64)
        off[1:] = np.cumsum(counts)[:-1]
        row_off = _h2d(off, dev)
        count = _h2d(np.array(counts, dtype=np.int32), dev)
        self._match(lab, rows, 29, row_off, None, 0, count, None, None, B, _pow2(max(max(counts), 1)), max(N, 1), tables)

    def _match(self, lab, rows, ncols, row_off, keep, keep_stride, count, conf, cls, B, P, cap, tables=None):
        if self.seq + B > (1 << 25):
            raise Ep24Error("ep24: more than 2^25 images in one evaluation (EP24_E_UNSUPPORTED)")
        dev = rows.device
        NA = len(self.strata) if self.strata else 0
        key = (B, P, cap, str(dev), NA)
        ms = _match_scratch.get(key)
        if ms is None:
            _match_scratch.clear()                        # one live shape at a time: an evaluation feeds batches of one size
            ms = _match_scratch[key] = _MatchScratch(B, P, cap, dev, NA)
        ms.count.zero_()
        cs, thr, _ = _device_consts(dev)
        head = [ptr(lab), lab.shape[1], B, ptr(rows), ncols, ptr(row_off), ptr(keep), keep_stride, ptr(count), ptr(conf), ptr(cls),
                self.num_classes, self._t, ptr(cs), ptr(thr), self._mds[-1], self.seq, ptr(ms.sort), P]
        recs = [ptr(ms.key), ptr(ms.cls), ptr(ms.p), ptr(ms.tp)]
        tail = [ptr(ms.count), ptr(self._npig), ptr(self._err), stream_ptr()]
        if NA:
            sc, zt = _h2d(tables[0], dev), _h2d(tables[1], dev)
            call("eval_match_strata", *head, ptr(sc), ptr(zt), self._strata_rows.ctypes.data, NA, *recs, ptr(ms.val), *tail)
        else:
            call("eval_match", *head, *recs, *tail)
        n = int(ms.count.item())                          # the batch's one host synchronisation
        if n:
            w = max(NA, 1)
            self._recs.append((ms.key[:n].clone(), ms.cls[:n].clone(), ms.p[:n].clone(), ms.tp[:n * w].view(n, w).clone(),
                               ms.val[:2 * n].view(n, 2).clone() if NA else None))
        self.n_records += n
        self.seq += B

    # ---- accumulation ------------------------------------------------------------------------------
    def _sorted(self):
        """The records of the evaluation sorted by (class, score desc, image seq, rank): (key, cls, p, m, order) on the device,
        m [n, NA] (one column without strata: the TP bits)."""
        dev = self.device
        if self._recs:
            key, cls, p, m = (torch.cat([r[i] for r in self._recs]) for i in range(4))
        else:
            key = torch.zeros(0, dtype=torch.int64, device=dev)
            cls = p = torch.zeros(0, dtype=torch.int32, device=dev)
            m = torch.zeros(0, len(self.strata) if self.strata else 1, dtype=torch.int32, device=dev)
        order = sort_records(key, cls, 7 + max(self.seq - 1, 0).bit_length(), max(self.num_classes - 1, 0).bit_length())
        return key, cls, p, m, order

    def records(self):
        """Host copy of the sorted records: dict of numpy arrays cls, score (fp32), seq, rank, p, tp (10-bit masks); with strata
        also m [n, NA] (10 TP bits | 10 ignore bits << 16; tp is the first stratum's TP bits), area and zone of the detections."""
        if self._npig is None:
            raise Ep24Error("ep24: no update() yet")
        key, cls, p, m, order = self._sorted()
        o = order.long()
        k = key[o].cpu().numpy().view(np.uint64)
        sbits = (~(k >> np.uint64(32))).astype(np.uint32)
        sbits = np.where(sbits & np.uint32(0x80000000), sbits & np.uint32(0x7FFFFFFF), ~sbits).astype(np.uint32)
        m = m[o].cpu().numpy()
        rec = {"cls": cls[o].cpu().numpy(), "score": sbits.view(np.float32), "seq": ((k >> np.uint64(7)) & np.uint64((1 << 25) - 1)).astype(np.int64),
               "rank": (k & np.uint64(127)).astype(np.int64), "p": p[o].cpu().numpy(), "tp": m[:, 0] & 0x3FF}
        if self.strata:
            val = torch.cat([r[4] for r in self._recs]) if self._recs else torch.zeros(0, 2, dtype=torch.float64, device=self.device)
            val = val[o].cpu().numpy()
            rec.update(m=m, area=val[:, 0], zone=val[:, 1])
        return rec

    def npig(self):
        """Host copy of the GT counts: [C], with strata the non-ignored GTs [C, NA]."""
        if self._npig is None:
            raise Ep24Error("ep24: no update() yet")
        n = self._npig.cpu().numpy().astype(np.int64)
        return n.reshape(self.num_classes, len(self.strata)) if self.strata else n

    def accumulate(self):
        """-> (precision [10, 101, C], recall [10, C]) float64 numpy arrays: one device-to-host copy.  With strata:
        (precision [10, 101, C, NA, NM], recall [10, C, NA, NM])."""
        if self._npig is None:
            raise Ep24Error("ep24: no update() yet")
        _lib.require_gpu()
        dev, C = self.device, self.num_classes
        shape = (C, len(self.strata), len(self._mds)) if self.strata else (C,)
        key, cls, p, m, order = self._sorted()
        n = key.numel()
        _, _, rthr = _device_consts(dev)
        cols = int(np.prod(shape[1:]))                    # NA * NM tables per class
        npr, nrc = 10 * 101 * C * cols, 10 * C * cols
        out = torch.empty(npr + nrc, dtype=torch.float64, device=dev)
        ctp = torch.empty(cols * max(n, 1), dtype=torch.int32, device=dev)
        env = torch.empty(ctp.numel(), dtype=torch.float64, device=dev)
        if self.strata:
            md = _h2d(np.array(self._mds, dtype=np.int32), dev)
            call("eval_accumulate_strata", ptr(order), ptr(key), ptr(cls), ptr(m), n, ptr(self._npig), C, shape[1], ptr(md), shape[2],
                 ptr(rthr), ptr(ctp), ptr(env), ptr(out), ptr(out, npr), stream_ptr())
        else:
            call("eval_accumulate", ptr(order), ptr(cls), ptr(m), n, ptr(self._npig), C, ptr(rthr), None, ptr(ctp), ptr(env), ptr(out),
                 ptr(out, npr), stream_ptr())
        if int(self._err.item()):
            raise Ep24Error("ep24: eval_match%s met an image with more detections than its scratch holds" % ("_strata" if self.strata else ""))
        host = out.cpu().numpy()
        return host[:npr].reshape(10, 101, *shape), host[npr:].reshape(10, *shape)

    def summarize(self):
        precision, recall = self.accumulate()
        if self.strata:
            # the headline numbers: the first stratum at the largest maxDets
            self.stats = summarize_tables(precision[:, :, :, 0, -1], recall[:, :, 0, -1])
            self.stats.update(precision=precision, recall=recall, max_dets=self.max_dets,
                              strata=summarize_strata(precision, recall, self.strata, self.max_dets, self.npig()))
            self.summary = format_strata_summary(self.stats, self.strata, self.max_dets)
        else:
            self.stats = summarize_tables(precision, recall)
            self.summary = format_summary(self.stats, self.max_dets)
        self.stats["iou_type"] = self.iou_type
        self.stats["nms_iou"] = self.nms_iou
        self.stats["images"] = self.seq
        return self.stats


def _mean_valid(x):
    v = x[x > -1]
    return float(np.mean(v)) if v.size else -1.0


def summarize_tables(precision, recall):
    """pycocotools ``summarize`` for one area range and one maxDets: means over the entries > -1."""
    return {"AP": _mean_valid(precision), "AP50": _mean_valid(precision[0]), "AP75": _mean_valid(precision[5]),
            "AR100": _mean_valid(recall), "per_class_AP": np.array([_mean_valid(precision[:, :, k]) for k in range(precision.shape[2])]),
            "precision": precision, "recall": recall}


def format_summary(stats, max_dets=100):
    lines = [" Average Precision  (AP) @[ IoU=0.50:0.95 | area=   all | maxDets=%3d ] = %.3f" % (max_dets, stats["AP"]),
             " Average Precision  (AP) @[ IoU=0.50      | area=   all | maxDets=%3d ] = %.3f" % (max_dets, stats["AP50"]),
             " Average Precision  (AP) @[ IoU=0.75      | area=   all | maxDets=%3d ] = %.3f" % (max_dets, stats["AP75"]),
             " Average Recall     (AR) @[ IoU=0.50:0.95 | area=   all | maxDets=%3d ] = %.3f" % (max_dets, stats["AR100"])]
    return "\n".join(lines) + "\n"


def summarize_strata(precision, recall, strata, max_dets, npig):
    """{name: {AP, AP50, AP75, AR<maxDets> for every maxDets, npig}} from the [.., NA, NM] tables: pycocotools' means over the
    entries > -1, the APs at the largest maxDets; ``npig [C, NA]``: the stratum's non-ignored GTs."""
    out = {}
    for a, s in enumerate(strata):
        d = {"AP": _mean_valid(precision[:, :, :, a, -1]), "AP50": _mean_valid(precision[0, :, :, a, -1]),
             "AP75": _mean_valid(precision[5, :, :, a, -1]), "npig": int(npig[:, a].sum())}
        for mi, md in enumerate(max_dets):
            d["AR%d" % md] = _mean_valid(recall[:, :, a, mi])
        out[s.name] = d
    return out


def _is_coco_rows(strata):
    ref = coco_area_strata()
    return len(strata) >= 4 and all(s.name == r.name and s.row() == r.row() for s, r in zip(strata, ref))


def format_strata_summary(stats, strata, max_dets):
    """pycocotools' twelve lines when the strata begin with the four COCO area rows and max_dets == (1, 10, 100), else the four
    lines of the first stratum; then one table row per stratum that restricts the zone: name, GT count, AP, AP50, AR."""
    st, last = stats["strata"], max_dets[-1]

    def line(ap, iou, name, md, v):
        return " {:<18} {} @[ IoU={:<9} | area={:>6s} | maxDets={:>3d} ] = {:0.3f}".format(
            "Average Precision" if ap else "Average Recall", "(AP)" if ap else "(AR)", iou, name, md, v)
    if _is_coco_rows(strata) and tuple(max_dets) == (1, 10, 100):
        names = [s.name for s in strata[:4]]
        lines = [line(True, "0.50:0.95", "all", last, st["all"]["AP"]), line(True, "0.50", "all", last, st["all"]["AP50"]),
                 line(True, "0.75", "all", last, st["all"]["AP75"])]
        lines += [line(True, "0.50:0.95", n, last, st[n]["AP"]) for n in names[1:]]
        lines += [line(False, "0.50:0.95", "all", md, st["all"]["AR%d" % md]) for md in max_dets]
        lines += [line(False, "0.50:0.95", n, last, st[n]["AR%d" % last]) for n in names[1:]]
        text = "\n".join(lines) + "\n"
    else:
        text = format_summary(stats, last)
    zoned = [s for s in strata if s.zone != (0.0, float("inf"))]
    if zoned:
        text += " %-18s %8s %7s %7s %7s\n" % ("zone", "GTs", "AP", "AP50", "AR%d" % last)
        for s in zoned:
            d = st[s.name]
            text += " %-18s %8d %7.3f %7.3f %7.3f\n" % (s.name, d["npig"], d["AP"], d["AP50"], d["AR%d" % last])
    return text
