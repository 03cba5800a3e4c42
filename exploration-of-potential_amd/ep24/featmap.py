"""Feature-map response study on the GPU (csrc/featmap.hip; include/ep24.h E4): what the reference's title
experiment, ``yolox/demo_featuremap.py``, measures for the three FPN levels - the channel mean of each neck output as a heat map
(``create_2D_feature_map``, :330-347), the mean of that map inside the ground-truth region (:377-385), and the AP of the detections,
for one object shifted to several vertical offsets, undistorted and sector-warped at a list of angles (:443-542).

The maps are read straight from the launch plan's neck outputs (``engine.pans``, bf16 NHWC): no NCHW copy and no torch arithmetic.
Every function checks its arguments before anything touches the GPU, works on the current stream and does not synchronise the host
(``study`` does, where it reads results back).  There is no CPU fallback.
"""
import json
import os

import numpy as np
import torch

from . import _lib
from ._lib import Ep24Error, call, ptr, stream_ptr

MAX_SCALE = 64                      # EP24_FEATMAP_MAX_SCALE
MAX_SIDE = 16384                    # EP24_DRAW_MAX_SIDE
REGIONS = {"rect": 0, "poly24": 1}
STRIDES = (8, 16, 32)

__all__ = ["channel_mean", "fpn_maps", "value_range", "render", "colormap", "response", "Response", "shifted_inputs", "study"]


# ------------------------------------------------------------------------------------------------ channel mean
def _is_act(x):
    return all(hasattr(x, a) for a in ("buf", "c0", "C", "B", "H", "W"))


def _mean_source(x):
    """-> (address, ld, (B, H, W), C, is_cuda, device) of an engine Act or of a bf16 tensor [B,H,W,C] that is a channel slice of a
    dense NHWC tensor; every rule of ep24_featmap_mean_bf16 is checked here."""
    if _is_act(x):
        t = x.buf.t
        if t.dtype != torch.bfloat16:
            raise ValueError("channel_mean: the Act holds %s; the kernel reads bfloat16 activations" % t.dtype)
        B, H, W, C, ld, addr = x.B, x.H, x.W, x.C, x.ld, x.ptr()
    elif isinstance(x, torch.Tensor):
        if x.dim() != 4:
            raise IndexError("channel_mean: expected an NHWC tensor [B, H, W, C], got %s" % (tuple(x.shape),))
        if x.dtype != torch.bfloat16:
            raise ValueError("channel_mean: expected bfloat16, got %s" % x.dtype)
        t = x
        B, H, W, C = (int(v) for v in x.shape)
        if B * H * W == 0:
            ld = max(C, 8) if C % 8 == 0 else C
        else:
            ld = int(x.stride(2)) if W > 1 else (int(x.stride(1)) if H > 1 else (int(x.stride(0)) if B > 1 else C))
            want = (H * W * ld, W * ld, ld, 1)
            for d, n in enumerate((B, H, W, C)):
                if n > 1 and int(x.stride(d)) != want[d]:
                    raise ValueError("channel_mean: strides %s are not a channel slice of a dense NHWC tensor" % (tuple(x.stride()),))
        addr = x.data_ptr()
    else:
        raise IndexError("channel_mean: expected an engine Act or a bfloat16 tensor [B, H, W, C], got %s" % type(x).__name__)
    if C < 8 or C % 8:
        raise ValueError("channel_mean: C = %d must be a positive multiple of 8" % C)
    if ld < C or ld % 8:
        raise ValueError("channel_mean: row stride %d must be a multiple of 8 and at least C = %d" % (ld, C))
    if B * H * W and addr % 16:
        raise ValueError("channel_mean: the slice must start on a 16-byte boundary (a channel offset that is a multiple of 8)")
    return addr, ld, (B, H, W), C, t.is_cuda, t.device


def channel_mean(x, out=None):
    """fp32 ``[B, H, W]``: the mean over the channels of ``x`` - an engine ``Act``, or a bf16 CUDA tensor ``[B, H, W, C]`` that is
    a channel slice of a dense NHWC tensor (C and the row stride multiples of 8).  fp32 sum in a fixed order, one true division."""
    addr, ld, shape, C, is_cuda, dev = _mean_source(x)
    if out is not None:
        if not isinstance(out, torch.Tensor) or tuple(out.shape) != shape:
            raise IndexError("channel_mean: out must have the shape %s" % (shape,))
        if out.dtype != torch.float32 or not out.is_contiguous():
            raise ValueError("channel_mean: out must be a contiguous float32 tensor")
    _lib.require_gpu()
    if not is_cuda or (out is not None and not out.is_cuda):
        raise Ep24Error("ep24: channel_mean takes GPU tensors (no CPU fallback on the product path)")
    if out is None:
        out = torch.empty(shape, dtype=torch.float32, device=dev)
    call("featmap_mean_bf16", addr, ld, shape[0] * shape[1] * shape[2], C, ptr(out), stream_ptr())
    return out


def fpn_maps(model, images):
    """One eval-mode forward, then ``channel_mean`` on the plan's three neck outputs -> ``(pred [B, A, 27 + C], [m8, m16, m32])``.
    The model must be in eval mode: otherwise this raises what ``model(images, train=False)`` raises."""
    pred = model(images, train=False)
    eng = model.engine(images.shape[0], (images.shape[2], images.shape[3]), model.compute_dtype)
    return pred, [channel_mean(a) for a in eng.pans]


# ------------------------------------------------------------------------------------------------ heat maps
def colormap():
    """uint8 ``[256, 3]``: the package's own heat ramp (black - red - yellow - white), in integer arithmetic only; 256 distinct rows."""
    out = np.zeros((256, 3), dtype=np.uint8)
    for i in range(256):
        v = 3 * i
        out[i] = (min(v, 255), min(max(v - 255, 0), 255), min(max(v - 510, 0), 255))
    return torch.from_numpy(out)


_luts = {}


def _check_maps(maps, what):
    if not isinstance(maps, torch.Tensor) or maps.dim() != 3:
        raise IndexError("%s: maps must be a float32 tensor [N, H, W], got %s"
                         % (what, tuple(maps.shape) if isinstance(maps, torch.Tensor) else type(maps).__name__))
    if maps.dtype != torch.float32:
        raise ValueError("%s: maps must be float32, got %s" % (what, maps.dtype))
    if not maps.is_contiguous():
        raise ValueError("%s: maps must be contiguous" % what)
    return (int(v) for v in maps.shape)


def value_range(maps):
    """fp32 ``[N, 2]``: (min, max) of every map of ``maps [N, H, W]``; NaNs are ignored."""
    N, H, W = _check_maps(maps, "value_range")
    _lib.require_gpu()
    if not maps.is_cuda:
        raise Ep24Error("ep24: value_range takes GPU tensors (no CPU fallback on the product path)")
    out = torch.empty(N, 2, dtype=torch.float32, device=maps.device)
    call("featmap_range", ptr(maps), N, H * W, ptr(out), stream_ptr())
    return out


def _finite(v, name):
    if v is None:
        return None
    v = float(v)
    if v != v or v in (float("inf"), float("-inf")):
        raise ValueError("render: %s must be a finite number, got %r" % (name, v))
    return v


def render(maps, scale, base=None, alpha=128, vmin=None, vmax=None, lut=None, out=None):
    """uint8 ``[N, H * scale, W * scale, 3]``: every cell of ``maps [N, H, W]`` as a ``scale`` x ``scale`` block of the colour
    ``lut[idx]`` (default ``colormap()``), idx from the map's own (min, max) - or ``vmin`` / ``vmax`` where given.  With ``base``
    (fp32 ``[N, 3, H * scale, W * scale]``, the network input) the colour is blended over it with weight ``alpha`` / 256."""
    N, H, W = _check_maps(maps, "render")
    if isinstance(scale, bool) or int(scale) != scale or not 1 <= int(scale) <= MAX_SCALE:
        raise ValueError("render: scale must be an integer in 1..%d, got %r" % (MAX_SCALE, scale))
    scale = int(scale)
    if isinstance(alpha, bool) or int(alpha) != alpha or not 0 <= int(alpha) <= 255:
        raise ValueError("render: alpha must be an integer in 0..255, got %r" % (alpha,))
    if H < 1 or W < 1 or H * scale > MAX_SIDE or W * scale > MAX_SIDE:
        raise IndexError("render: output sides must lie in 1..%d, got %d x %d" % (MAX_SIDE, H * scale, W * scale))
    vmin, vmax = _finite(vmin, "vmin"), _finite(vmax, "vmax")
    shape = (N, H * scale, W * scale, 3)
    if base is not None:
        if not isinstance(base, torch.Tensor) or tuple(base.shape) != (N, 3, H * scale, W * scale):
            raise IndexError("render: base must be float32 [%d, 3, %d, %d]" % (N, H * scale, W * scale))
        if base.dtype != torch.float32 or not base.is_contiguous():
            raise ValueError("render: base must be a contiguous float32 tensor")
    if lut is not None:
        if not hasattr(lut, "shape") or tuple(lut.shape) != (256, 3):
            raise IndexError("render: lut must be uint8 [256, 3]")
        if str(lut.dtype).replace("torch.", "") != "uint8":
            raise ValueError("render: lut must be uint8, got %s" % (lut.dtype,))
    if out is not None:
        if not isinstance(out, torch.Tensor) or tuple(out.shape) != shape:
            raise IndexError("render: out must have the shape %s" % (shape,))
        if out.dtype != torch.uint8 or not out.is_contiguous():
            raise ValueError("render: out must be a contiguous uint8 tensor")
    _lib.require_gpu()
    if not maps.is_cuda or (base is not None and not base.is_cuda) or (out is not None and not out.is_cuda):
        raise Ep24Error("ep24: render takes GPU tensors (no CPU fallback on the product path)")
    dev = maps.device
    if lut is None:
        table = _luts.get(str(dev))
        if table is None:
            table = _luts[str(dev)] = colormap().to(dev)
    else:
        table = (lut if isinstance(lut, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(lut))).to(dev).contiguous()
    if vmin is not None and vmax is not None:
        rng = torch.empty(max(N, 1), 2, dtype=torch.float32, device=dev)
    else:
        rng = value_range(maps)
    if vmin is not None:
        rng[:, 0] = vmin                                      # device-side fills: no host synchronisation
    if vmax is not None:
        rng[:, 1] = vmax
    if out is None:
        out = torch.empty(shape, dtype=torch.uint8, device=dev)
    call("featmap_render", ptr(maps), N, H, W, scale, ptr(rng), ptr(table), ptr(base), int(alpha), ptr(out), stream_ptr())
    return out


# ------------------------------------------------------------------------------------------------ response
class Response:
    """``mean`` and ``sum`` float64 ``[levels, B, L]``, ``count`` int32 ``[levels, B, L]`` on the device; ``region``, ``strides``."""

    def __init__(self, mean, sum, count, region, strides):
        self.mean, self.sum, self.count, self.region, self.strides = mean, sum, count, region, strides


def response(maps, labels, strides=STRIDES, region="rect"):
    """The mean of every map inside every label's region.  ``maps``: one fp32 ``[B, H, W]`` tensor per level (``fpn_maps``' list),
    ``labels`` fp32 ``[B, L, 51]`` in pixels of the network input, ``strides`` the levels' strides.  ``region="rect"`` is the
    reference's rule (the bounding rectangle of the 24 vertices, ``int()`` edges, :378-385), ``"poly24"`` the cells whose anchor
    centre lies inside the 24-gon.  Padding rows and empty regions give count 0 and mean 0."""
    if isinstance(maps, torch.Tensor):
        maps = [maps]
    maps, strides = list(maps), [s for s in strides]
    if region not in REGIONS:
        raise ValueError("response: region must be 'rect' or 'poly24', got %r" % (region,))
    if len(maps) == 0 or len(maps) != len(strides):
        raise IndexError("response: %d maps for %d strides" % (len(maps), len(strides)))
    for s in strides:
        if isinstance(s, bool) or int(s) != s or int(s) < 1:
            raise ValueError("response: strides must be positive integers, got %r" % (s,))
    if not isinstance(labels, torch.Tensor) or labels.dim() != 3 or labels.shape[2] != 51:
        raise IndexError("response: labels must be float32 [B, L, 51], got %s"
                         % (tuple(labels.shape) if isinstance(labels, torch.Tensor) else type(labels).__name__,))
    if labels.dtype != torch.float32:
        raise ValueError("response: labels must be float32, got %s" % labels.dtype)
    B, L = int(labels.shape[0]), int(labels.shape[1])
    for m in maps:
        _, H, W = _check_maps(m, "response")
        if int(m.shape[0]) != B:
            raise IndexError("response: a map holds %d images, labels %d" % (m.shape[0], B))
        if not (1 <= H <= MAX_SIDE and 1 <= W <= MAX_SIDE):
            raise IndexError("response: map sides must lie in 1..%d, got %d x %d" % (MAX_SIDE, H, W))
    _lib.require_gpu()
    if not labels.is_cuda or not all(m.is_cuda for m in maps):
        raise Ep24Error("ep24: response takes GPU tensors (no CPU fallback on the product path)")
    dev = labels.device
    if any(m.device != dev for m in maps):
        raise IndexError("response: maps and labels must live on one device")
    lab = labels.detach().contiguous()
    n = len(maps)
    mean = torch.empty(n, B, L, dtype=torch.float64, device=dev)
    tot = torch.empty(n, B, L, dtype=torch.float64, device=dev)
    count = torch.empty(n, B, L, dtype=torch.int32, device=dev)
    s = stream_ptr()
    for k, (m, st) in enumerate(zip(maps, strides)):
        call("featmap_response", ptr(m), B, int(m.shape[1]), int(m.shape[2]), int(st), ptr(lab), L, REGIONS[region],
             ptr(tot, k * B * L), ptr(count, k * B * L), ptr(mean, k * B * L), s)
    return Response(mean, tot, count, region, tuple(int(v) for v in strides))


# ------------------------------------------------------------------------------------------------ the study
def _polygon_mask(h, w, verts):
    """bool [h, w]: the pixels whose centre (x, y) lies inside the polygon ``verts [24, 2]``, by the rasteriser's crossing rule."""
    ys = np.arange(h, dtype=np.float64)[:, None]
    xs = np.arange(w, dtype=np.float64)[None, :]
    inside = np.zeros((h, w), dtype=bool)
    for k in range(len(verts)):
        (x0, y0), (x1, y1) = verts[k], verts[(k + 1) % len(verts)]
        counts = (y0 <= ys) != (y1 <= ys)
        if y1 == y0 or not counts.any():
            continue
        xc = x0 + ((ys - y0) * (x1 - x0)) / (y1 - y0)
        inside ^= counts & (xs < xc)
    return inside


def shifted_inputs(image_u8, rows, offsets, isolate=True):
    """The host half of the study, in numpy as in the reference (``get_img_mask``, :199-236): for every offset the image shifted
    down by ``offset`` rows onto a 114 canvas, and its label rows ``[k, 51]`` (class + 50 coordinates normalised by width / height)
    with the y coordinates moved along; a row whose centre leaves the image is dropped.  ``isolate``: pixels outside all of the
    image's polygons become 114.  -> (list of uint8 [h, w, 3], list of float64 [k_i, 51])."""
    img = np.ascontiguousarray(image_u8)
    if img.ndim != 3 or img.shape[2] != 3 or img.dtype != np.uint8:
        raise IndexError("study: the image must be uint8 [h, w, 3], got %s %s" % (img.shape, img.dtype))
    rows = np.asarray(rows, dtype=np.float64)
    rows = rows.reshape(-1, 51) if rows.size else np.zeros((0, 51))
    if not np.isfinite(rows).all():
        raise ValueError("study: non-finite label rows")
    h, w = img.shape[:2]
    src = img
    if isolate:
        keep = np.zeros((h, w), dtype=bool)
        for r in rows:
            keep |= _polygon_mask(h, w, np.stack([r[3::2] * w, r[4::2] * h], 1))
        src = np.where(keep[:, :, None], img, np.uint8(114))
    images, targets = [], []
    for off in offsets:
        off = int(off)
        canvas = np.full((h, w, 3), 114, dtype=np.uint8)
        if off >= 0:
            if off < h:
                canvas[off:] = src[:h - off]
        elif -off < h:
            canvas[:h + off] = src[-off:]
        t = rows.copy()
        t[:, 2::2] += off / float(h)
        cy = t[:, 2] * h
        images.append(canvas)
        targets.append(t[(cy >= 0) & (cy < h)])
    return images, targets


def _key(offset, tag):
    return "offset_%s_%s" % (str(int(offset)).zfill(3), tag)                  # the reference's table_dic keys (:457, :499)


def _write_ppm(path, img):
    with open(path, "wb") as fh:
        fh.write(b"P6\n%d %d\n255\n" % (img.shape[1], img.shape[0]))
        fh.write(np.ascontiguousarray(img, dtype=np.uint8).tobytes())


def _label_rows_as_dets(lab):
    """Host: the valid rows of one image's label table [L, 51] as detection rows [n, 29] (radii = vertex distances, scores 1)."""
    lab = lab[lab.sum(1) > 0]
    vx, vy = lab[:, 3::2] - lab[:, 1:2], lab[:, 4::2] - lab[:, 2:3]
    return np.concatenate([lab[:, 1:3], np.sqrt(vx * vx + vy * vy), np.ones((len(lab), 2), np.float32), lab[:, 0:1]], 1).astype(np.float32)


def study(model, image_u8, rows, test_size, thetas=range(30, 95, 5), offsets=(-100, -50, 0, 50, 100), conf=0.01, nms=0.65,
          isolate=True, save_dir=None):
    """The reference's ``Undistorted`` + ``Distorted`` loops (:443-542) for the 24-point model: one object (``image_u8`` uint8
    ``[h, w, 3]`` with its label rows ``[k, 51]``) at every offset, undistorted ("none") and sector-warped at every angle of
    ``thetas``; each distortion is one batch of ``len(offsets)`` images through ``TrainTransform.batch`` / ``FisheyeTransform.batch``,
    ``fpn_maps``, ``response`` for both regions, ``postprocess`` and ``Evaluator24.update_detections`` (one summary per distortion).

    Returns (and, with ``save_dir``, writes as ``response.json``) a dict: ``table`` maps the reference's ``table_dic`` keys
    (``"offset_%03d_none"``, ``"offset_%03d_theta_%d"``) to the per-level, per-region means and counts of the image's labels;
    ``AP`` holds the per-distortion summary; ``map_sizes`` the three map sizes.  With ``save_dir`` every image also leaves its
    network input (``<key>_input.npy``), and per level the map (``<key>_s<stride>_map.npy``), ``render`` over the input
    (``<key>_s<stride>_heat.npy``) and the same with the ground truth and the detections drawn (``<key>_s<stride>_vis.ppm``)."""
    from .draw import draw_detections
    from .evaluate import Evaluator24
    from .fisheye import FisheyeTransform
    from .infer import postprocess
    from .input import TrainTransform
    S_h, S_w = (int(test_size), int(test_size)) if isinstance(test_size, int) else (int(test_size[0]), int(test_size[1]))
    if S_h % 32 or S_w % 32 or S_h <= 0 or S_w <= 0:
        raise IndexError("study: test_size must be positive multiples of 32, got %s" % (test_size,))
    offsets, thetas = [int(o) for o in offsets], [int(t) for t in thetas]
    if not offsets:
        raise ValueError("study: no offsets")
    for t in thetas:
        if not 15 <= t <= 180:
            raise ValueError("study: angles must lie in 15..180, got %d" % t)
    images, targets = shifted_inputs(image_u8, rows, offsets, isolate)
    _lib.require_gpu()
    if model.training:
        raise NotImplementedError("ep24: study on a model in training mode - call model.eval() first, as demo_featuremap.py does")
    C = model.head.num_classes
    dev = next(model.parameters()).device
    if save_dir is not None:
        os.makedirs(save_dir, exist_ok=True)
    result = {"test_size": [S_h, S_w], "strides": list(STRIDES), "map_sizes": None, "offsets": offsets, "thetas": thetas,
              "conf": float(conf), "nms": float(nms), "isolate": bool(isolate), "AP": {}, "table": {}}
    gt_color = torch.tensor([[0, 255, 0]] * C, dtype=torch.uint8)
    with torch.no_grad(), torch.cuda.device(dev):
        for tag in ["none"] + ["theta_%d" % t for t in thetas]:
            if tag == "none":
                tf = TrainTransform(max_labels=50)
            else:
                tf = FisheyeTransform(theta=(int(tag[6:]),) * 2, max_labels=50, device=str(dev))
            imgs, labs = tf.batch(images, targets, (S_h, S_w))
            pred, maps = fpn_maps(model, imgs)
            resp = {region: response(maps, labs, STRIDES, region) for region in ("rect", "poly24")}
            dets = postprocess(pred, C, conf_thre=conf, nms_thre=nms)
            ev = Evaluator24(C, conf_thre=conf, nms_thre=nms)
            ev.update_detections(dets, labs)
            stats = ev.summarize()
            result["AP"][tag] = {k: float(stats[k]) for k in ("AP", "AP50", "AP75", "AR100")}
            result["map_sizes"] = [[int(m.shape[1]), int(m.shape[2])] for m in maps]
            lab_h = labs.cpu().numpy()
            valid = lab_h.sum(2) > 0
            host = {region: (r.mean.cpu().numpy(), r.count.cpu().numpy()) for region, r in resp.items()}
            for b, off in enumerate(offsets):
                entry = {"labels": int(valid[b].sum()), "detections": 0 if dets[b] is None else int(dets[b].shape[0]), "levels": []}
                for k, st in enumerate(STRIDES):
                    lev = {"stride": st}
                    for region, (mean, count) in host.items():
                        lev[region] = {"mean": [float(v) for v in mean[k, b][valid[b]]], "count": [int(v) for v in count[k, b][valid[b]]]}
                    entry["levels"].append(lev)
                result["table"][_key(off, tag)] = entry
            if save_dir is not None:
                for k, st in enumerate(STRIDES):
                    heat = render(maps[k], st, base=imgs, alpha=128)
                    heat_h, maps_h = heat.cpu().numpy(), maps[k].cpu().numpy()
                    for b, off in enumerate(offsets):
                        stem = os.path.join(save_dir, "%s_s%d" % (_key(off, tag), st))
                        vis = draw_detections(heat[b], torch.from_numpy(_label_rows_as_dets(lab_h[b])).to(dev), num_classes=C,
                                              colors=gt_color)
                        vis = draw_detections(vis, dets[b], num_classes=C, out=vis)
                        np.save(stem + "_map.npy", maps_h[b])
                        np.save(stem + "_heat.npy", heat_h[b])
                        _write_ppm(stem + "_vis.ppm", vis.cpu().numpy())
                imgs_h = imgs.cpu().numpy()
                for b, off in enumerate(offsets):
                    np.save(os.path.join(save_dir, _key(off, tag) + "_input.npy"), imgs_h[b])
    if save_dir is not None:
        with open(os.path.join(save_dir, "response.json"), "w") as fh:
            json.dump(result, fh, indent=1)
    return result
