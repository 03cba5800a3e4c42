"""Drawing 24-point detections onto an image on the GPU (csrc/draw.hip): what the reference's ``Evaluator.vis`` does with OpenCV
on the host (show_24p.py:325-367) - centre dot, a dot on each of the 24 points, the closed 24-gon, the class label - plus an
optional translucent fill of the polygon.

The pixel rules are this package's own and exact (include/ep24.h E3): integer geometry as the reference forms
it (``bboxes /= ratio``, truncation to int, vertices clipped to ``[0, W] x [0, H]``), squared-distance tests in integers instead of
cv2's Bresenham lines, a 5 x 7 bitmap font (``ep24.font5x7``) instead of Hershey text.  Two launches per call - one thread per
detection row builds a primitive record, one workgroup per 64 x 16 pixel tile gathers the records that touch it and paints its own
pixels in row order - and no host synchronisation.  The result is a bit-exact function of the inputs.
"""
import numpy as np
import torch

from . import _lib
from ._lib import Ep24Error, call, ptr, stream_ptr
from .evaluate import _device_consts
from .font5x7 import FONT

REC_WORDS = 64                      # EP24_DRAW_REC_WORDS
MAX_SIDE = 16384                    # EP24_DRAW_MAX_SIDE
MAX_FONT_SCALE = 1024               # EP24_DRAW_MAX_FONT_SCALE
LABEL_BYTES = 24
NAME_BYTES = 21                     # a class name is cut here so that " dd" (show_scores) still fits in 24 bytes

__all__ = ["FONT", "draw_detections", "palette", "label_table"]


def palette(C):
    """uint8 ``[C, 3]``: a golden-ratio walk round the hue circle at full value, with the saturation stepping through three
    levels, in integer arithmetic only (the same bytes everywhere).  Pairwise distinct for C <= 80 (tests/test_draw24_oracle.py)."""
    C = int(C)
    if C < 0:
        raise ValueError("palette: C must not be negative, got %d" % C)
    out = np.zeros((C, 3), dtype=np.uint8)
    for i in range(C):
        h = (i * 40503 + 9973) & 0xFFFF                      # 40503 / 65536 = 0.61803: the golden ratio's fraction
        sat = (255, 200, 150)[i % 3]
        sector, f = divmod(h * 6, 65536)                     # hue sector 0..5 and the position inside it, 16 bits
        v = 255
        p = v * (255 - sat) // 255
        q = v * (255 * 65536 - sat * f) // (255 * 65536)
        t = v * (255 * 65536 - sat * (65536 - f)) // (255 * 65536)
        out[i] = ((v, t, p), (q, v, p), (p, v, t), (p, q, v), (t, p, v), (v, p, q))[sector]
    return torch.from_numpy(out)


def label_table(num_classes, class_names=None):
    """-> (uint8 ``[C, 24]`` numpy, int32 ``[C]`` numpy): the label bytes of every class and their lengths.  The decimal class index
    by default; the entries of ``class_names`` when given (at least ``num_classes`` of them), encoded as UTF-8 and cut to 21 bytes."""
    C = int(num_classes)
    if class_names is not None and len(class_names) < C:
        raise ValueError("class_names has %d entries for %d classes" % (len(class_names), C))
    tab = np.zeros((C, LABEL_BYTES), dtype=np.uint8)
    lens = np.zeros(C, dtype=np.int32)
    for c in range(C):
        raw = (str(c) if class_names is None else str(class_names[c])).encode("utf-8")[:NAME_BYTES]
        tab[c, :len(raw)] = np.frombuffer(raw, dtype=np.uint8)
        lens[c] = len(raw)
    return tab, lens


_fonts, _palettes, _labels, _scratch = {}, {}, {}, {}


def _font(dev):
    f = _fonts.get(str(dev))
    if f is None:                                            # uploaded once per device
        f = _fonts[str(dev)] = torch.tensor(FONT, dtype=torch.uint8).to(dev)
    return f


def _records(dev, n):
    """The per-device primitive scratch, int32 ``[capacity, 64]`` with capacity >= n: kept between calls, grown when n outgrows it."""
    r = _scratch.get(str(dev))
    if r is None or r.shape[0] < n:
        cap = max(256, 1 << (max(int(n), 1) - 1).bit_length())
        r = _scratch[str(dev)] = torch.empty(cap, REC_WORDS, dtype=torch.int32, device=dev)
    return r


def _check(image, dets, ratio, conf, num_classes, class_names, colors, fill_alpha, font_scale, out):
    """Every shape and argument rule, before anything touches the GPU."""
    if not isinstance(image, torch.Tensor) or image.dim() != 3 or image.shape[2] != 3:
        raise IndexError("draw_detections: image must be a uint8 tensor [H, W, 3], got %s"
                         % (tuple(image.shape) if isinstance(image, torch.Tensor) else type(image).__name__,))
    if image.dtype != torch.uint8:
        raise ValueError("draw_detections: image must be uint8, got %s" % image.dtype)
    H, W = int(image.shape[0]), int(image.shape[1])
    if not (1 <= H <= MAX_SIDE and 1 <= W <= MAX_SIDE):
        raise IndexError("draw_detections: image sides must lie in 1..%d, got %d x %d" % (MAX_SIDE, H, W))
    if dets is not None:
        if not isinstance(dets, torch.Tensor) or dets.dim() != 2 or dets.shape[1] != 29:
            raise IndexError("draw_detections: dets must be the [n, 29] rows of postprocess (or None), got %s"
                             % (tuple(dets.shape) if isinstance(dets, torch.Tensor) else type(dets).__name__,))
        if not dets.dtype.is_floating_point:
            raise ValueError("draw_detections: dets must be a floating-point tensor, got %s" % dets.dtype)
    if int(num_classes) < 1:
        raise ValueError("draw_detections: num_classes must be at least 1, got %r" % (num_classes,))
    if isinstance(fill_alpha, bool) or int(fill_alpha) != fill_alpha or not 0 <= int(fill_alpha) <= 255:
        raise ValueError("draw_detections: fill_alpha must be an integer in 0..255, got %r" % (fill_alpha,))
    if isinstance(font_scale, bool) or int(font_scale) != font_scale or not 1 <= int(font_scale) <= MAX_FONT_SCALE:
        raise ValueError("draw_detections: font_scale must be an integer in 1..%d, got %r" % (MAX_FONT_SCALE, font_scale))
    ratio, conf = float(ratio), float(conf)
    if not (0.0 < ratio < float("inf")):
        raise ValueError("draw_detections: ratio must be a positive finite number, got %r" % (ratio,))
    if conf != conf:
        raise ValueError("draw_detections: conf is NaN")
    if class_names is not None and len(class_names) < int(num_classes):
        raise ValueError("draw_detections: class_names has %d entries for %d classes" % (len(class_names), int(num_classes)))
    if colors is not None:
        shape = tuple(colors.shape) if hasattr(colors, "shape") else None
        if shape != (int(num_classes), 3):
            raise IndexError("draw_detections: colors must be uint8 [%d, 3], got %s" % (int(num_classes), shape))
        if str(colors.dtype).replace("torch.", "") != "uint8":
            raise ValueError("draw_detections: colors must be uint8, got %s" % (colors.dtype,))
    if out is not None:
        if not isinstance(out, torch.Tensor) or tuple(out.shape) != tuple(image.shape):
            raise IndexError("draw_detections: out must have the image's shape %s" % (tuple(image.shape),))
        if out.dtype != torch.uint8:
            raise ValueError("draw_detections: out must be uint8, got %s" % out.dtype)
        if not out.is_contiguous():
            raise ValueError("draw_detections: out must be contiguous")
    return H, W, ratio, conf


def draw_detections(image, dets, ratio=1.0, conf=0.0, num_classes=80, class_names=None, colors=None, fill_alpha=0, font_scale=2,
                    show_scores=False, out=None):
    """Draws the detections ``dets [n, 29]`` (the rows of ``postprocess``; ``None`` or empty: nothing) onto ``image``, uint8
    ``[H, W, 3]`` on the GPU, and returns the result: a new tensor, or ``out`` (``out is image`` draws in place).

    ``ratio`` maps the rows back to the image (``preproc_batch``'s letterbox ratio), rows with ``obj * class_conf < conf`` are left
    out, ``colors`` is uint8 ``[num_classes, 3]`` (default ``palette(num_classes)``; the channel order is the image's), the label of
    a class is its decimal index or ``class_names[c]`` cut to 21 bytes, followed by the score's two decimals with ``show_scores``;
    ``fill_alpha`` in 1..255 also blends the class colour over the polygon's inside; ``font_scale`` is the integer zoom of the
    5 x 7 font.  Shape and argument errors are raised before anything touches the GPU; there is no host synchronisation."""
    H, W, ratio, conf = _check(image, dets, ratio, conf, num_classes, class_names, colors, fill_alpha, font_scale, out)
    C = int(num_classes)
    _lib.require_gpu()
    if not image.is_cuda or (dets is not None and not dets.is_cuda) or (out is not None and not out.is_cuda):
        raise Ep24Error("ep24: draw_detections takes GPU tensors (no CPU fallback on the product path)")
    dev = image.device
    if (dets is not None and dets.device != dev) or (out is not None and out.device != dev):
        raise IndexError("draw_detections: image, dets and out must live on one device")
    if out is None:
        out = image.detach().clone(memory_format=torch.contiguous_format)
    elif out is not image:
        out.copy_(image)
    elif not image.is_contiguous():
        raise ValueError("draw_detections: drawing in place needs a contiguous image")
    n = 0 if dets is None else int(dets.shape[0])
    if n == 0:
        return out
    d = dets.detach().float().contiguous()
    if colors is None:
        col = _palettes.get((str(dev), C))
        if col is None:
            col = _palettes[(str(dev), C)] = palette(C).to(dev)
    else:
        col = (colors if isinstance(colors, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(colors))).to(dev).contiguous()
    key = (str(dev), C, None if class_names is None else tuple(str(s) for s in class_names[:C]))
    lab = _labels.get(key)
    if lab is None:
        if len(_labels) >= 16:
            _labels.clear()
        tab, lens = label_table(C, class_names)
        lab = _labels[key] = (torch.from_numpy(tab).to(dev), torch.from_numpy(lens).to(dev))
    cs, _, _ = _device_consts(dev)
    rec = _records(dev, n)
    s = stream_ptr()
    call("draw24_prepare", ptr(d), n, ratio, conf, ptr(cs), H, W, ptr(col), C, ptr(lab[0]), ptr(lab[1]), int(font_scale),
         1 if show_scores else 0, ptr(rec), s)
    call("draw24_paint", ptr(out), H, W, ptr(rec), n, ptr(_font(dev)), int(fill_alpha), int(font_scale), s)
    return out
