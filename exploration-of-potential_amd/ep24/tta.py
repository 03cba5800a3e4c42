"""Test-time augmentation for the 24-ray detector (csrc/tta.hip; DESIGN.md section 7, "Test-time augmentation").

The batch is run at a few smaller sizes, each plain and mirrored left to right, and the decoded predictions of every view are
brought back into the canonical frame (``ep24_tta_unmap``: centre and radii times ``W0 / w``; a mirrored view has
``cx' = w - cx`` and ray ``k`` taken from ray ``(12 - k) mod 24``) and laid side by side in one table
``merged [B, sum of A_v, 27 + C]``:

* view-major: the rows of view 0 first, then view 1, ... in the order of ``views`` (``Predictor.offsets`` has the first row of
  each), the canonical unmirrored view first;
* inside a view, the anchors in the head's own order (stride 8, 16, 32; row-major in each level).

``merged`` goes through ``ep24.infer.postprocess`` like any prediction table.  With ``nms_iou="poly24"`` and a ``vote_thre`` the
candidates of the other views that NMS removes are not thrown away: each kept detection becomes their score-weighted consensus
(``ep24_post_vote_poly24``).  ``postprocess`` below fills in ``max_candidates`` = the canonical view's anchor count, so that the
suppression matrix stays the size plain polygon NMS uses (8.9 MB per image at 640 x 640, against about 170 MB for all 37 170
merged anchors).

Cost: one eval-mode forward per view, by construction.
"""
import weakref

import torch

from . import _lib, infer
from ._lib import call, ptr, stream_ptr

DEFAULT_SCALES = (1.0, 0.85, 0.7)


def _hw(size):
    return (int(size), int(size)) if isinstance(size, int) else (int(size[0]), int(size[1]))


def anchors_for(hw):
    """Rows of the decoded prediction table for an input of ``hw``: the cells of strides 8, 16 and 32."""
    h, w = _hw(hw)
    return (h // 8) * (w // 8) + (h // 16) * (w // 16) + (h // 32) * (w // 32)


def views_for(base_hw, scales=DEFAULT_SCALES, mirror=True):
    """``[(h, w, mirrored), ...]`` for a network input of ``base_hw = (H0, W0)``: per scale ``w = round(W0 * s / 32) * 32`` and
    ``h = H0 * w / W0``, plain and (``mirror``) mirrored.  The resize must be uniform - rays do not survive an anisotropic one -
    so a scale whose ``h`` is no whole multiple of 32 raises ``ValueError``.  640 x 640 with the default scales: 640, 544, 448, the
    canonical unmirrored view first (a predictor insists on that)."""
    H0, W0 = _hw(base_hw)
    if H0 <= 0 or W0 <= 0 or H0 % 32 or W0 % 32:
        raise ValueError("views_for: the base size %s must be positive multiples of 32" % ((H0, W0),))
    views = []
    for s in scales:
        s = float(s)
        w = int(round(W0 * s / 32.0)) * 32
        if not (s > 0.0 and w > 0):
            raise ValueError("views_for: scale %r gives no view of %s" % (s, (H0, W0)))
        if (H0 * w) % W0 or (H0 * w // W0) % 32:
            raise ValueError("views_for: scale %r turns %s into %g x %d: the height is no multiple of 32, and rays do not survive an "
                             "anisotropic resize" % (s, (H0, W0), H0 * w / W0, w))
        h = H0 * w // W0
        views.append((h, w, False))
        if mirror:
            views.append((h, w, True))
    return views


def check_views(base_hw, views):
    """The rules ``views_for`` guarantees, for a list of the caller's."""
    H0, W0 = _hw(base_hw)
    out = []
    for v in views:
        h, w, m = int(v[0]), int(v[1]), bool(v[2])
        if h <= 0 or w <= 0 or h % 32 or w % 32 or h * W0 != w * H0:
            raise ValueError("tta: view %r of base %s: positive multiples of 32 with the base's aspect ratio" % (v, (H0, W0)))
        out.append((h, w, m))
    if not out or out[0] != (H0, W0, False):
        raise ValueError("tta: the canonical unmirrored view %s comes first" % ((H0, W0),))
    return out


class Predictor:
    """``Predictor(model, batch, base_hw, views=None)(images) -> merged [B, sum A_v, 27 + C]``.

    Per view, in order: ``ep24_resize_bilinear_f32`` if the size differs, ``ep24_mirror_f32`` if mirrored,
    ``model(x, train=False)``, ``ep24_tta_unmap`` into the view's slice.  Everything runs on the current stream; there is no host
    synchronisation.  The model keeps one eval plan per (batch, size); the plans this predictor made the model build are
    forgotten again by ``release()``."""

    def __init__(self, model, batch, base_hw, views=None):
        _lib.require_gpu()
        self.model, self.batch = model, int(batch)
        self.base_hw = _hw(base_hw)
        self.views = views_for(self.base_hw) if views is None else check_views(self.base_hw, views)
        self.anchors = [anchors_for(v[:2]) for v in self.views]
        self.offsets = [sum(self.anchors[:i]) for i in range(len(self.views))]
        self.total_anchors = sum(self.anchors)
        self.canonical_anchors = self.anchors[0]
        # s = the fp32 value of W0 / w, computed in double and rounded once (ctypes rounds the double to the float argument)
        self.scales = [self.base_hw[1] / v[1] for v in self.views]
        self._owned = set()
        self._bufs = {}

    def _buffers(self, hw, dev):
        b = self._bufs.get(hw)
        if b is None or b[0].device != dev:
            b = self._bufs[hw] = (torch.empty(self.batch, 3, hw[0], hw[1], dtype=torch.float32, device=dev),
                                  torch.empty(self.batch, 3, hw[0], hw[1], dtype=torch.float32, device=dev))
        return b

    def _plan_key(self, hw):
        size = hw[0] if hw[0] == hw[1] else hw
        dt = getattr(self.model, "compute_dtype", torch.bfloat16)
        return (self.batch, size) if dt == torch.bfloat16 else (self.batch, size, dt)

    def __call__(self, images):
        _lib.require_gpu()
        if not images.is_cuda:
            raise _lib.Ep24Error("ep24: input images must live on the GPU (no CPU fallback on the product path)")
        H0, W0 = self.base_hw
        if images.dim() != 4 or tuple(images.shape) != (self.batch, 3, H0, W0):
            raise IndexError("tta: expected images %s, got %s" % ((self.batch, 3, H0, W0), tuple(images.shape)))
        x0 = images.detach().float().contiguous()
        B, s = self.batch, stream_ptr()
        merged = None
        for (h, w, mir), off, A_v, sc in zip(self.views, self.offsets, self.anchors, self.scales):
            x = x0
            if (h, w) != (H0, W0) or mir:
                resized, mirrored = self._buffers((h, w), x0.device)
                if (h, w) != (H0, W0):
                    call("resize_bilinear_f32", ptr(x0), B * 3, H0, W0, ptr(resized), h, w, s)
                    x = resized
                if mir:
                    call("mirror_f32", ptr(x), B * 3, h, w, ptr(mirrored), s)
                    x = mirrored
            key = self._plan_key((h, w))
            engines = getattr(self.model, "_engines", None)
            if engines is not None and key not in engines:
                self._owned.add(key)
            out = self.model(x, train=False)
            if out.dim() != 3 or out.shape[0] != B or out.shape[1] != A_v or out.shape[2] < 27:
                raise IndexError("tta: view %s gave predictions %s, expected [%d, %d, 27 + C]" % ((h, w, mir), tuple(out.shape), B, A_v))
            out = out.float().contiguous()
            if merged is None:
                merged = torch.empty(B, self.total_anchors, out.shape[2], dtype=torch.float32, device=out.device)
            call("tta_unmap", ptr(out), B, A_v, out.shape[2], w, sc, 1 if mir else 0, ptr(merged), self.total_anchors, off, s)
        return merged

    def release(self):
        """Forgets the eval plans this predictor made the model build, and its own view buffers.  The caller has synchronised."""
        engines = getattr(self.model, "_engines", None)
        if engines is not None:
            for key in self._owned:
                engines.pop(key, None)
        self._owned.clear()
        self._bufs.clear()


_predictors = weakref.WeakKeyDictionary()                 # model -> {(batch, base_hw, views): Predictor}


def predictor(model, batch, base_hw, views=None):
    """The cached ``Predictor`` of ``predict`` for this model, batch, size and views."""
    base_hw = _hw(base_hw)
    key = (int(batch), base_hw, None if views is None else tuple(tuple(v) for v in views))
    per_model = _predictors.setdefault(model, {})
    p = per_model.get(key)
    if p is None:
        p = per_model[key] = Predictor(model, batch, base_hw, views)
    return p


def predict(model, images, views=None):
    """``merged [B, sum A_v, 27 + C]`` of ``images [B, 3, H0, W0]`` (GPU; the model in eval mode) over ``views`` (default:
    ``views_for((H0, W0))``); rows as the module's docstring lays them out.  The predictor (its buffers, the eval plans it made
    the model build) is kept per model, batch, size and views until ``release(model)``."""
    _lib.require_gpu()
    if not images.is_cuda:
        raise _lib.Ep24Error("ep24: input images must live on the GPU (no CPU fallback on the product path)")
    if images.dim() != 4 or images.shape[1] != 3:
        raise IndexError("tta: expected images [B, 3, H, W], got %s" % (tuple(images.shape),))
    return predictor(model, images.shape[0], (images.shape[2], images.shape[3]), views)(images)


def release(model):
    """Releases every predictor ``predict`` keeps for ``model`` (after a synchronisation of the caller's)."""
    for p in _predictors.pop(model, {}).values():
        p.release()


def postprocess(merged, num_classes, canonical_anchors, conf_thre=0.7, nms_thre=0.45, class_agnostic=False, vote_thre=None,
                max_candidates=None):
    """``ep24.infer.postprocess`` of a merged table with polygon NMS: ``max_candidates`` defaults to ``canonical_anchors``
    (``Predictor.canonical_anchors`` / ``anchors_for(base_hw)``), an explicit value wins."""
    K = canonical_anchors if max_candidates is None else max_candidates
    return infer.postprocess(merged, num_classes, conf_thre, nms_thre, class_agnostic, nms_iou="poly24", max_candidates=K,
                             vote_thre=vote_thre)
