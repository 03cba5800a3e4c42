"""Instance masks of 24-point detections on the GPU (csrc/mask.hip): polygons -> bit-packed masks -> mask IoU.

The model's product is a star polygon per object: a centre and 24 radii on the 15-degree rays.  ``detection_polygons``
turns detection rows into vertices, ``rasterize`` fills them into bit-packed instance masks (what a COCO "segm" evaluation
or any downstream user of an instance detector consumes), ``mask_iou`` compares two sets of masks by AND + popcount,
``boundary`` keeps the band of a mask that Boundary IoU compares (csrc/boundary.hip).

Packed format: ``bits`` int32 ``[N, H, ceil(W / 32)]`` holding uint32 words (pixel x is bit ``x & 31`` of word ``x >> 5``,
bits at x >= W are zero), ``bbox`` int32 ``[N, 4]`` = (x0, y0, x1, y1), the smallest and largest set pixel, or
(W, H, -1, -1) for an empty mask, ``area`` int32 ``[N]`` = set pixels.

Pixel rule: the centre of pixel (x, y) is the point (x, y); in float64, for the row yc = y an edge
(x0, y0) -> (x1, y1) counts iff ``(y0 <= yc) != (y1 <= yc)``, crosses at ``x0 + ((yc - y0) * (x1 - x0)) / (y1 - y0)`` and
pixel x is set iff an odd number of counting edges have ``x < xc``.  Left and top boundary pixels are in, right and bottom
ones out (cv2.fillPoly sets all four).  All compute runs as HIP kernels; torch only allocates and copies.
"""
import math

import torch

from . import _lib
from ._lib import Ep24Error, call, ptr, stream_ptr
from .evaluate import _device_consts


class PackedMasks:
    """``bits [N, H, ceil(W / 32)]`` int32 (uint32 words), ``bbox [N, 4]`` int32, ``area [N]`` int32, ``size = (H, W)``."""

    def __init__(self, bits, bbox, area, size):
        self.bits, self.bbox, self.area = bits, bbox, area
        self.size = (int(size[0]), int(size[1]))

    def __len__(self):
        return int(self.bits.shape[0])


def _size(size):
    H, W = int(size[0]), int(size[1])
    if H <= 0 or W <= 0 or H * W >= 1 << 31:
        raise Ep24Error("ep24: mask size %s: H, W > 0 and H * W < 2^31 (EP24_E_UNSUPPORTED)" % (tuple(size),))
    return H, W


def _alloc(N, H, W, dev):
    return PackedMasks(torch.empty(N, H, (W + 31) // 32, dtype=torch.int32, device=dev),
                       torch.empty(N, 4, dtype=torch.int32, device=dev), torch.empty(N, dtype=torch.int32, device=dev), (H, W))


def _gpu(t, what):
    _lib.require_gpu()
    if not t.is_cuda:
        raise Ep24Error("ep24: %s takes GPU tensors (no CPU fallback on the product path)" % what)


def _vertices(det, ratio):
    if det.dim() != 2 or det.shape[1] not in (26, 29):
        raise IndexError("expected detections [n, 26] or [n, 29], got %s" % (tuple(det.shape),))
    d = det.detach().float().contiguous()
    out = torch.empty(d.shape[0], 24, 2, dtype=torch.float32, device=d.device)
    cs, _, _ = _device_consts(d.device)
    call("poly24_vertices", ptr(d), d.shape[1], d.shape[0], ptr(cs), float(ratio), ptr(out), stream_ptr())
    return out


def detection_polygons(det):
    """``det [n, 26]`` (cx, cy, 24 radii) or the ``[n, 29]`` rows of ``postprocess`` -> vertices ``[n, 24, 2]`` fp32:
    ``cx + r_k * cos(15 deg k)``, ``cy + r_k * sin(15 deg k)``, product and sum as separate fp32 operations (the evaluator's
    "rect" and "poly24" geometry)."""
    _gpu(det, "detection_polygons")
    return _vertices(det, 1.0)


def rasterize(polys, size, out=None):
    """``polys [N, 24, 2]`` fp32 vertices in the pixel coordinates of a ``size = (H, W)`` canvas -> ``PackedMasks``.
    ``out``: a ``PackedMasks`` of N masks of that size to fill (every word of it is written) instead of a new one."""
    _gpu(polys, "rasterize")
    H, W = _size(size)
    if polys.dim() != 3 or tuple(polys.shape[1:]) != (24, 2):
        raise IndexError("expected polygons [N, 24, 2], got %s" % (tuple(polys.shape),))
    v = polys.detach().float().contiguous()
    if out is None:
        pm = _alloc(v.shape[0], H, W, v.device)
    else:
        pm = out
        if not (isinstance(pm, PackedMasks) and pm.size == (H, W) and len(pm) == v.shape[0]):
            raise IndexError("rasterize: out must hold %d masks of size %s" % (v.shape[0], (H, W)))
        if pm.bits.device != v.device or pm.bbox.device != v.device or pm.area.device != v.device:
            raise IndexError("rasterize: out lives on another device")
        _check_packed(pm, "rasterize")
    call("poly24_raster", ptr(v), v.shape[0], H, W, ptr(pm.bits), ptr(pm.bbox), ptr(pm.area), stream_ptr())
    return pm


def pack(masks_u8):
    """``masks_u8 [N, H, W]`` uint8 or bool (non-zero = set) -> ``PackedMasks`` with boxes and areas."""
    _gpu(masks_u8, "pack")
    if masks_u8.dim() != 3 or masks_u8.dtype not in (torch.uint8, torch.bool):
        raise IndexError("expected masks [N, H, W] uint8 or bool, got %s %s" % (tuple(masks_u8.shape), masks_u8.dtype))
    N = masks_u8.shape[0]
    H, W = _size(masks_u8.shape[1:])
    m = masks_u8.detach().contiguous()
    m = m.view(torch.uint8) if m.dtype == torch.bool else m
    pm = _alloc(N, H, W, m.device)
    call("mask_pack_u8", ptr(m), N, H, W, ptr(pm.bits), ptr(pm.bbox), ptr(pm.area), stream_ptr())
    return pm


def _check_packed(p, what):
    if not isinstance(p, PackedMasks):
        raise IndexError("%s takes PackedMasks, got %s" % (what, type(p).__name__))
    _gpu(p.bits, what)
    H, W = p.size
    N = p.bits.shape[0]
    if tuple(p.bits.shape) != (N, H, (W + 31) // 32) or tuple(p.bbox.shape) != (N, 4) or tuple(p.area.shape) != (N,):
        raise IndexError("PackedMasks of size %s with bits %s, bbox %s, area %s" % (p.size, tuple(p.bits.shape), tuple(p.bbox.shape),
                                                                                   tuple(p.area.shape)))
    if not (p.bits.dtype == p.bbox.dtype == p.area.dtype == torch.int32 and p.bbox.is_cuda and p.area.is_cuda
            and p.bits.is_contiguous() and p.bbox.is_contiguous() and p.area.is_contiguous()):
        raise IndexError("PackedMasks holds contiguous int32 GPU tensors")


def unpack(packed):
    """``PackedMasks`` -> bool ``[N, H, W]``."""
    _check_packed(packed, "unpack")
    H, W = packed.size
    N = len(packed)
    out = torch.empty(N, H, W, dtype=torch.uint8, device=packed.bits.device)
    call("mask_unpack_u8", ptr(packed.bits), N, H, W, ptr(out), stream_ptr())
    return out.view(torch.bool)


def mask_iou(a, b):
    """-> ``(inter [G, D] int64, iou [G, D] float64)`` of two ``PackedMasks`` of one size: the common pixels and
    ``inter / (area_a + area_b - inter)`` (0 for two empty masks).  Only the overlap of a pair's boxes is read."""
    _check_packed(a, "mask_iou")
    _check_packed(b, "mask_iou")
    if a.size != b.size:
        raise IndexError("mask_iou: sizes %s and %s differ" % (a.size, b.size))
    H, W = a.size
    G, D = len(a), len(b)
    dev = a.bits.device
    inter = torch.empty(G, D, dtype=torch.int64, device=dev)
    iou = torch.empty(G, D, dtype=torch.float64, device=dev)
    call("mask_iou", ptr(a.bits), ptr(a.bbox), ptr(a.area), G, ptr(b.bits), ptr(b.bbox), ptr(b.area), D, H, W, ptr(inter), ptr(iou), stream_ptr())
    return inter, iou


def boundary(packed, d=None, dilation_ratio=0.02):
    """``PackedMasks`` -> ``PackedMasks`` of the boundary bands of Boundary IoU (include/ep24.h section E7): the mask pixels within
    ``d`` pixels of the mask's outside, the outside of the image included (``mask & ~erode(mask, d)``, a (2d + 1)-square erosion).
    ``d`` defaults to ``max(1, round(dilation_ratio * diagonal of packed.size))``; ``bbox`` and ``area`` are the bands'."""
    _check_packed(packed, "boundary")
    H, W = _size(packed.size)
    if d is None:
        if not (math.isfinite(dilation_ratio) and dilation_ratio > 0):
            raise ValueError("dilation_ratio %r: a positive finite number" % (dilation_ratio,))
        d = max(1, int(round(dilation_ratio * math.sqrt(H * H + W * W))))
    d = int(d)
    if d < 1:
        raise Ep24Error("ep24: boundary radius d=%d: at least 1 (EP24_E_UNSUPPORTED)" % d)
    N, dev = len(packed), packed.bits.device
    out = _alloc(N, H, W, dev)
    if N == 0:
        return out
    WW = (W + 31) // 32
    tab = torch.zeros(N, 4, dtype=torch.int64)                                       # the statistics kernel names its masks by a table
    tab[:, 0], tab[:, 1], tab[:, 2] = torch.arange(N, dtype=torch.int64) * (H * WW), H, W
    tab = tab.to(dev)
    s = stream_ptr()
    call("mask_boundary", ptr(packed.bits), None, N, H, W, min(d, max(H, W)), ptr(out.bits), s)
    call("segm_mask_stats", ptr(out.bits), ptr(tab), N, ptr(out.bbox), ptr(out.area), s)
    return out


def detections_to_masks(dets, ratio, image_hw):
    """One image's ``postprocess`` rows (``[n, 29]``, ``[n, 26]`` or None) -> ``PackedMasks`` on the original image
    ``image_hw = (h, w)``: centre and radii are divided by the letterbox ``ratio`` in fp32 (the reference's demo maps its boxes
    back with ``bboxes /= ratio``), then the polygons are rasterised."""
    _lib.require_gpu()
    H, W = _size(image_hw)
    if dets is None or dets.shape[0] == 0:
        dev = dets.device if dets is not None and dets.is_cuda else torch.device("cuda", torch.cuda.current_device())
        return _alloc(0, H, W, dev)
    _gpu(dets, "detections_to_masks")
    return rasterize(_vertices(dets, ratio), (H, W))
