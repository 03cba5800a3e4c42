"""Fisheye lens model by calibration (csrc/lens.hip): images, points and 24-point labels between a pinhole frame and the
fisheye frame of a real lens, described as OpenCV's ``cv2.fisheye`` does (``K``, ``D``: the Kannala-Brandt model).

``LensModel`` is the calibration: intrinsics of both frames, ``k1..k4`` and the field of view; it validates itself on the host.
``map_points`` moves points, ``warp_images`` images (uint8 HWC, for demos and rectification), ``preproc_images`` writes the network
input directly, ``warp_labels`` carries the 24-point labels - each in either direction: ``"distort"`` (pinhole -> fisheye) or
``"undistort"`` (fisheye -> pinhole).  ``LensTransform`` is the ``TrainTransform`` that a ``DataPrefetcher`` takes: pinhole-labelled
data as one of the given lenses would see it.  include/ep24.h states the arithmetic.  There is no CPU fallback.
"""
import json
import math

import numpy as np
import torch

from . import _lib
from ._lib import call, ptr, stream_ptr
from .augment import _rot, position_rng
from .input import TrainTransform

MODEL_D = 14        # doubles per model
IMG_D = 18          # doubles per image in the table of ep24_lens_warp_u8 / ep24_lens_preproc_u8
GEO_D = 22          # doubles per image in the table of ep24_lens_labels
DIRECTIONS = {"distort": 0, "undistort": 1}


def _direction(direction):
    if direction not in DIRECTIONS:
        raise ValueError("direction must be 'distort' (pinhole -> fisheye) or 'undistort' (fisheye -> pinhole), got %r" % (direction,))
    return DIRECTIONS[direction]


def _four(name, v):
    v = tuple(float(x) for x in np.asarray(v, dtype=np.float64).reshape(-1))
    if len(v) != 4 or not all(math.isfinite(x) for x in v):
        raise ValueError("LensModel: %s takes four finite numbers, got %r" % (name, v))
    return v


class LensModel:
    """``pin`` / ``fish``: (fx, fy, cx, cy) of the pinhole and of the fisheye frame in pixel-index coordinates (pixel i is centred at
    i); ``k``: k1..k4; ``fov_deg``: the full field of view, below 180.  ``size``: (h, w) of the frames the intrinsics were given for,
    if known - ``LensTransform`` and the trainer scale a model from it.  Raises ``ValueError`` naming what failed."""

    def __init__(self, pin, fish, k=(0.0, 0.0, 0.0, 0.0), fov_deg=170.0, size=None):
        self.pin, self.fish, self.k = _four("pin", pin), _four("fish", fish), _four("k", k)
        self.fov_deg = float(fov_deg)
        self.size = None if size is None else (int(size[0]), int(size[1]))
        if min(self.pin[0], self.pin[1], self.fish[0], self.fish[1]) <= 0.0:
            raise ValueError("LensModel: focal lengths must be positive (pin %r, fish %r)" % (self.pin, self.fish))
        if not 0.0 < self.fov_deg < 180.0:
            raise ValueError("LensModel: fov_deg %r is outside (0, 180): a pinhole frame holds less than a half space" % fov_deg)
        self.theta_max = math.radians(self.fov_deg / 2.0)
        th = np.linspace(0.0, self.theta_max, 4096)
        slope = self.dthetad(th)
        if not (np.isfinite(slope).all() and (slope > 0.0).all()):
            bad = float(th[np.argmax(~(slope > 0.0))])
            raise ValueError("LensModel: thetad is not increasing on [0, theta_max]: d thetad / d theta = %.3g at theta = %.4f rad "
                             "(k = %r, fov_deg = %r)" % (float(self.dthetad(bad)), bad, self.k, self.fov_deg))
        th = np.linspace(0.0, self.theta_max, 1024)
        err = float(np.abs(self.newton(self.thetad(th)) - th).max())
        if not err <= 1e-14:
            raise ValueError("LensModel: the 12-step Newton iteration misses theta by %.3g (> 1e-14) on [0, theta_max] "
                             "(k = %r, fov_deg = %r)" % (err, self.k, self.fov_deg))

    # ---- the model's arithmetic on the host (float64, the operations of include/ep24.h in their order)
    def thetad(self, th):
        k1, k2, k3, k4 = self.k
        t2 = th * th
        return th * (1.0 + t2 * (k1 + t2 * (k2 + t2 * (k3 + t2 * k4))))

    def dthetad(self, th):
        k1, k2, k3, k4 = self.k
        t2 = th * th
        return 1.0 + t2 * (3.0 * k1 + t2 * (5.0 * k2 + t2 * (7.0 * k3 + t2 * (9.0 * k4))))

    def newton(self, td):
        td = np.asarray(td, dtype=np.float64)
        th = td.copy()
        with np.errstate(all="ignore"):
            for _ in range(12):
                th = th - (self.thetad(th) - td) / self.dthetad(th)
                th = np.fmin(np.fmax(th, 0.0), self.theta_max)
        return th

    def table(self):
        """The 14 doubles the kernels read."""
        return np.array(self.pin + self.fish + self.k + (self.theta_max, float(self.thetad(self.theta_max))), dtype=np.float64)

    # ---- constructors
    @classmethod
    def from_opencv(cls, K, D, pin=None, fov_deg=170.0, size=None):
        """``K`` 3x3 and ``D`` (4) of ``cv2.fisheye.calibrate``; ``pin``: the pinhole frame's (fx, fy, cx, cy), by default those of
        ``K`` (what ``cv2.fisheye.undistortImage(..., Knew=K)`` uses)."""
        K = np.asarray(K, dtype=np.float64)
        D = np.asarray(D, dtype=np.float64).reshape(-1)
        if K.shape != (3, 3) or D.shape != (4,):
            raise ValueError("LensModel.from_opencv: K is 3x3 and D has 4 coefficients, got %r and %r" % (K.shape, D.shape))
        if K[0, 1] != 0.0:
            raise ValueError("LensModel.from_opencv: a skew K[0][1] = %r is not part of the model" % float(K[0, 1]))
        fish = (K[0, 0], K[1, 1], K[0, 2], K[1, 2])
        return cls(fish if pin is None else pin, fish, D, fov_deg, size)

    @classmethod
    def from_json(cls, path):
        """A file of numbers only: ``K`` (3x3) and ``D`` (4) in OpenCV's layout, and optionally ``pinhole`` (fx, fy, cx, cy),
        ``fov_deg`` and ``size`` (h, w)."""
        with open(path) as f:
            d = json.load(f)
        unknown = set(d) - {"K", "D", "pinhole", "fov_deg", "size"}
        if unknown or "K" not in d or "D" not in d:
            raise ValueError("LensModel.from_json: %s must hold K and D (and may hold pinhole, fov_deg, size); unknown: %s"
                             % (path, sorted(unknown)))
        return cls.from_opencv(d["K"], d["D"], d.get("pinhole"), d.get("fov_deg", 170.0), d.get("size"))

    def to_json(self, path):
        fx, fy, cx, cy = self.fish
        d = {"K": [[fx, 0.0, cx], [0.0, fy, cy], [0.0, 0.0, 1.0]], "D": list(self.k), "pinhole": list(self.pin), "fov_deg": self.fov_deg}
        if self.size is not None:
            d["size"] = list(self.size)
        with open(path, "w") as f:
            json.dump(d, f)

    @classmethod
    def equidistant(cls, src_size, dst_size, fov_deg=120.0):
        """The ideal lens (k = 0) that shows a pinhole image of ``src_size`` (h, w) in a fisheye frame of ``dst_size``: principal
        points at the centres, the shorter half side of either frame at the rim of the field."""
        (h, w), (dh, dw) = src_size, dst_size
        tm = math.radians(float(fov_deg) / 2.0)
        if not 0.0 < tm < math.pi / 2:
            raise ValueError("LensModel: fov_deg %r is outside (0, 180)" % fov_deg)
        fp, ff = (min(h, w) / 2.0) / math.tan(tm), (min(dh, dw) / 2.0) / tm
        return cls((fp, fp, (w - 1) / 2.0, (h - 1) / 2.0), (ff, ff, (dw - 1) / 2.0, (dh - 1) / 2.0), (0.0, 0.0, 0.0, 0.0), fov_deg, (dh, dw))

    @staticmethod
    def _scale4(v, sx, sy):
        return (v[0] * sx, v[1] * sy, (v[2] + 0.5) * sx - 0.5, (v[3] + 0.5) * sy - 0.5)

    def scaled(self, sx, sy=None, pin=True, fish=True):
        """The model of the frames resized by (sx, sy): focal * s, principal point (c + 0.5) * s - 0.5.  ``pin`` / ``fish``: which
        frames are resized."""
        sy = sx if sy is None else sy
        size = self.size
        if size is not None and fish:
            size = (int(round(size[0] * sy)), int(round(size[1] * sx)))
        return LensModel(self._scale4(self.pin, sx, sy) if pin else self.pin, self._scale4(self.fish, sx, sy) if fish else self.fish,
                         self.k, self.fov_deg, size)

    def __repr__(self):
        return "LensModel(pin=%r, fish=%r, k=%r, fov_deg=%r, size=%r)" % (self.pin, self.fish, self.k, self.fov_deg, self.size)


def _models(model_or_list, n, what):
    if isinstance(model_or_list, LensModel):
        return [model_or_list] * n
    models = list(model_or_list)
    if len(models) != n or not all(isinstance(m, LensModel) for m in models):
        raise ValueError("%s: %d items and %d lens models" % (what, n, len(models)))
    return models


def _sizes(out_size, n, what):
    """One (h, w) for all or one per item -> list of n (h, w)."""
    if len(out_size) == 2 and not hasattr(out_size[0], "__len__"):
        sizes = [(int(out_size[0]), int(out_size[1]))] * n
    else:
        sizes = [(int(s[0]), int(s[1])) for s in out_size]
    if len(sizes) != n:
        raise ValueError("%s: %d items and %d sizes" % (what, n, len(sizes)))
    if any(h <= 0 or w <= 0 for h, w in sizes):
        raise ValueError("%s: sizes must be positive, got %r" % (what, sizes))
    return sizes


def map_points(points, model, direction, device="cuda:0"):
    """points [m,2] (x, y) in pixel-index coordinates of the pinhole frame (``"distort"``) or of the fisheye frame (``"undistort"``)
    -> their positions [m,2] float64 in the other frame, on the device (``ep24_lens_points``)."""
    _lib.require_gpu()
    d = _direction(direction)
    pts = torch.as_tensor(points, dtype=torch.float64).to(device).contiguous()
    if pts.dim() != 2 or pts.shape[1] != 2:
        raise IndexError("map_points takes points [m,2]")
    out = torch.empty_like(pts)
    tab = model.table()
    call("lens_points", ptr(pts), pts.shape[0], tab.ctypes.data, d, ptr(out), stream_ptr())
    return out


def _sources(images, dev, what):
    """-> (one packed uint8 device buffer, desc rows [offset, h, w], sizes)."""
    flat, desc, off = [], [], 0
    for im in images:
        if not isinstance(im, torch.Tensor):
            im = np.ascontiguousarray(im)
            im = torch.from_numpy(im if im.flags.writeable else im.copy())
        if im.dim() != 3 or im.shape[2] != 3 or im.dtype != torch.uint8 or im.shape[0] == 0 or im.shape[1] == 0:
            raise ValueError("%s takes uint8 [h,w,3] images" % what)
        h, w = int(im.shape[0]), int(im.shape[1])
        if max(h, w) >= 1 << 26:
            raise ValueError("%s: an image of %d x %d is beyond the kernel's index range" % (what, h, w))
        desc.append([off, h, w])
        flat.append(im.contiguous().reshape(-1))
        off += h * w * 3
    buf = torch.cat([f.to(dev, non_blocking=True) for f in flat])
    return buf, desc


def _fill(fill):
    if not 0 <= int(fill) <= 255:
        raise ValueError("fill must be in 0..255, got %r" % (fill,))
    return int(fill)


def warp_images(images, model_or_list, direction, out_size, fill=114, device="cuda:0"):
    """images: list of uint8 [h,w,3] arrays / tensors of any sizes; one model or one per image; ``out_size``: (h, w) of the
    destination frame, one for all or one per image.  Returns a list of uint8 [h',w',3] device tensors (views of one buffer): the
    images as the lens sees them (``"distort"``: the sources are pinhole images) or rectified (``"undistort"``).  One launch."""
    _lib.require_gpu()
    d, fill, n, dev = _direction(direction), _fill(fill), len(images), torch.device(device)
    models, sizes = _models(model_or_list, n, "warp_images"), _sizes(out_size, n, "warp_images")
    if n == 0:
        return []
    buf, desc = _sources(images, dev, "warp_images")
    tab, off = np.zeros((n, IMG_D), dtype=np.float64), 0
    for i, (m, (oh, ow)) in enumerate(zip(models, sizes)):
        tab[i, :MODEL_D] = m.table()
        tab[i, MODEL_D:] = (d, oh, ow, off)
        off += oh * ow * 3
    out = torch.empty(off, dtype=torch.uint8, device=dev)
    desc_t = torch.tensor(desc, dtype=torch.int64, device=dev)
    tab_t = torch.from_numpy(tab).to(dev)
    for lo in range(0, n, 65535):
        hi = min(n, lo + 65535)
        call("lens_warp_u8", ptr(buf), ptr(desc_t, lo * 3), ptr(tab_t, lo * IMG_D), hi - lo, max(oh * ow for oh, ow in sizes[lo:hi]),
             ptr(out), fill, stream_ptr())
    return [out[int(t[17]):int(t[17]) + oh * ow * 3].view(oh, ow, 3) for t, (oh, ow) in zip(tab, sizes)]


def preproc_images(images, model_or_list, direction, input_size, fill=114, out=None, device="cuda:0"):
    """The same pixels as ``warp_images`` at ``out_size = input_size``, written as the network input: [n,3,S_h,S_w] fp32 on the
    device, channel order kept.  The destination frame IS the input canvas: no letterbox pass follows.  One launch."""
    _lib.require_gpu()
    d, fill, n = _direction(direction), _fill(fill), len(images)
    S_h, S_w = int(input_size[0]), int(input_size[1])
    dev = out.device if out is not None else torch.device(device)
    models = _models(model_or_list, n, "preproc_images")
    if out is None:
        out = torch.empty(n, 3, S_h, S_w, dtype=torch.float32, device=dev)
    elif tuple(out.shape) != (n, 3, S_h, S_w) or out.dtype != torch.float32 or not out.is_contiguous():
        raise ValueError("preproc_images: out must be a contiguous fp32 [n, 3, S_h, S_w] tensor")
    if n == 0:
        return out
    buf, desc = _sources(images, dev, "preproc_images")
    tab = np.zeros((n, IMG_D), dtype=np.float64)
    for i, m in enumerate(models):
        tab[i, :MODEL_D] = m.table()
        tab[i, MODEL_D:] = (d, S_h, S_w, 0)
    desc_t = torch.tensor(desc, dtype=torch.int64, device=dev)
    tab_t = torch.from_numpy(tab).to(dev)
    for lo in range(0, n, 65535):
        hi = min(n, lo + 65535)
        call("lens_preproc_u8", ptr(buf), ptr(desc_t, lo * 3), ptr(tab_t, lo * IMG_D), hi - lo, ptr(out, lo * 3 * S_h * S_w), S_h, S_w, fill,
             stream_ptr())
    return out


def warp_labels(targets, sizes, models, direction, out_size, max_labels=50, out=None, scales=None, device="cuda:0"):
    """targets: list of [k_i,51] label rows normalised by the size of their SOURCE image; sizes: that (h, w); models: one model or
    one per image; ``out_size``: (h, w) of the destination frame (one for all or one per image), to which the new vertices are
    clamped; ``scales``: a factor per image on the results (default 1).  Returns (labels [n,max_labels,51] fp32 in destination
    pixels, counts [n] int32, flags [n,max_labels] int32 - bit 0: the box centre of the mapped outline fell outside it and the mapped
    old centre was used), all on the device and without a host synchronisation.  At most ``max_labels`` rows per image are read;
    survivors keep their order."""
    _lib.require_gpu()
    d, n = _direction(direction), len(targets)
    if len(sizes) != n:
        raise ValueError("warp_labels: %d label tables, %d sizes" % (n, len(sizes)))
    models, osz = _models(models, n, "warp_labels"), _sizes(out_size, n, "warp_labels")
    scales = [1.0] * n if scales is None else [float(s) for s in scales]
    if len(scales) != n:
        raise ValueError("warp_labels: %d label tables, %d scales" % (n, len(scales)))
    if max_labels <= 0:
        raise ValueError("warp_labels: max_labels must be positive")
    dev = out.device if out is not None else torch.device(device)
    if out is None:
        out = torch.empty(n, max_labels, 51, dtype=torch.float32, device=dev)
    elif tuple(out.shape) != (n, max_labels, 51) or out.dtype != torch.float32 or not out.is_contiguous():
        raise ValueError("warp_labels: out must be a contiguous fp32 [n, max_labels, 51] tensor")
    rows, first = [], 0
    geo = np.zeros((n, GEO_D), dtype=np.float64)
    for i, (t, (h, w), m, (oh, ow), s) in enumerate(zip(targets, sizes, models, osz, scales)):
        t = np.asarray(t, dtype=np.float64)
        t = t.reshape(-1, 51) if t.size else np.zeros((0, 51))
        if h <= 0 or w <= 0:
            raise ValueError("warp_labels: image %d has size %r x %r" % (i, h, w))
        geo[i, :MODEL_D] = m.table()
        geo[i, MODEL_D:] = (d, h, w, oh, ow, s, first, t.shape[0])
        rows.append(t)
        first += t.shape[0]
    # one upload: the parameter table [n,22], then the label rows [R,51]
    dbl = np.concatenate([geo.reshape(-1)] + [t.reshape(-1) for t in rows] + [np.zeros(51)])
    if not np.isfinite(dbl).all():
        raise ValueError("warp_labels: non-finite label rows")
    counts = torch.empty(n, dtype=torch.int32, device=dev)
    flags = torch.empty(n, max_labels, dtype=torch.int32, device=dev)
    if n == 0:
        return out, counts, flags
    dbl_t = torch.from_numpy(dbl).to(dev)
    cand = torch.empty(n, max_labels, 51, dtype=torch.float32, device=dev)
    keep = torch.empty(n, max_labels, dtype=torch.int32, device=dev)
    rot = _rot(dev)
    for lo in range(0, n, 65535):
        hi = min(n, lo + 65535)
        call("lens_labels", ptr(dbl_t, n * GEO_D), ptr(dbl_t, lo * GEO_D), ptr(rot), hi - lo, max_labels, ptr(cand, lo * max_labels * 51),
             ptr(keep, lo * max_labels), ptr(out, lo * max_labels * 51), ptr(counts, lo), ptr(flags, lo * max_labels), stream_ptr())
    return out, counts, flags


def image_model(model, h, w, input_dim):
    """``model`` (given for frames of ``input_dim``) for a raw h x w pinhole image that the letterbox would place top-left in the
    pinhole frame at r = min(S_h / h, S_w / w): the pinhole intrinsics in the raw image's own pixels."""
    r = min(input_dim[0] / h, input_dim[1] / w)
    return model.scaled(1.0 / r, 1.0 / r, fish=False)


class LensTransform(TrainTransform):
    """``TrainTransform`` that shows every pinhole image, WITH its labels, as one of ``models`` sees it: same ``batch(...)`` signature,
    so ``DataPrefetcher`` takes it unchanged.  One model per image, drawn from the generator of the batch's data position -
    ``set_position(epoch, it)`` reseeds it from (seed, epoch, it), so a resumed run reproduces its batches.  The models are given for
    frames of their ``size`` (the Exp's ``input_size``) and are ``scaled`` to the ``input_dim`` of the call; the raw image stands in
    the pinhole frame as the letterbox would place it.  The fisheye frame is the network's input canvas: one image launch."""

    def __init__(self, models, max_labels=50, seed=0, device="cuda:0"):
        super().__init__(max_labels=max_labels, seed=seed)
        self.models = [models] if isinstance(models, LensModel) else list(models)
        if not self.models or not all(isinstance(m, LensModel) for m in self.models):
            raise ValueError("LensTransform takes one or more LensModel")
        self.seed, self.device = int(seed), device
        self.last_choices = self.last_counts = self.last_flags = None
        self.set_position(0, 0)

    def set_position(self, epoch, it):
        self.position = (int(epoch), int(it))
        self._lens_rng = position_rng(self.seed, epoch, it)

    def sample(self, n):
        return [int(self._lens_rng.randint(0, len(self.models))) for _ in range(n)]

    def models_for(self, choices, sizes, input_dim):
        """The per-image models of a batch: model ``choices[i]`` at ``input_dim`` for a raw image of ``sizes[i]``."""
        S_h, S_w = int(input_dim[0]), int(input_dim[1])
        out = []
        for c, (h, w) in zip(choices, sizes):
            m = self.models[c]
            if m.size is not None and m.size != (S_h, S_w):
                m = m.scaled(S_w / m.size[1], S_h / m.size[0])
            out.append(image_model(m, h, w, (S_h, S_w)))
        return out

    def batch(self, images, targets, input_dim, out_images=None, out_labels=None):
        _lib.require_gpu()
        choices = self.sample(len(images))
        from .jpeg import finish_checked
        images = finish_checked(images, device=self.device)
        dev_imgs = [torch.as_tensor(np.ascontiguousarray(im) if isinstance(im, np.ndarray) else im).to(self.device) for im in images]
        sizes = [tuple(im.shape[:2]) for im in dev_imgs]
        models = self.models_for(choices, sizes, input_dim)
        imgs = preproc_images(dev_imgs, models, "distort", input_dim, out=out_images, device=self.device)
        labs, counts, flags = warp_labels(targets, sizes, models, "distort", input_dim, self.max_labels, out=out_labels, device=self.device)
        self.last_choices, self.last_counts, self.last_flags = choices, counts, flags
        return imgs, labs
