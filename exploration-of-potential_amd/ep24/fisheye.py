"""Fisheye sector warp that carries the 24-point labels (csrc/sector.hip).

``TrainTransform(fisheye=...)`` warps the images and passes the label rows through unchanged; the reference itself only returns
the warped mask's bounding box (``sector_distort``) and would cast the 24 rays through the warped mask per object
(2+24_labels_create.py).  Here the polygons themselves go through the warp's continuous map (``Image_Distortion.map_points``
is that map for arbitrary points) and the 24 rays are re-cast from the centre of the mapped outline's box
(``ep24_sector_labels``): two small launches per batch and no mask.

``warp_labels`` is the label half on explicit angles; ``FisheyeTransform`` is the ``TrainTransform`` that a ``DataPrefetcher``
takes: one angle per image, the image through ``distort_batch``, letterbox, the labels through ``warp_labels`` with the same
angle.  There is no CPU fallback.
"""
import numpy as np
import torch

from . import _lib
from ._lib import call, ptr, stream_ptr
from .augment import _rot, position_rng
from .input import TrainTransform, preproc_batch
from .sector import Image_Distortion

GEO_D = 12          # doubles per image in the parameter table of ep24_sector_labels


def warp_labels(targets, sizes, thetas, input_size, max_labels=50, custom_rows=None, out=None, device="cuda:0"):
    """targets: list of [k_i,51] normalised label rows; sizes: (h, w) of every SOURCE image; thetas: its angle.  Returns
    (labels [n,max_labels,51] fp32 in pixels of the letterboxed warped image, counts [n] int32, flags [n,max_labels] int32 -
    bit 0: the box centre of the warped outline fell outside it and the warped old centre was used), all on the device and
    without a host synchronisation.  At most ``max_labels`` rows per image are read; survivors keep their order."""
    _lib.require_gpu()
    n = len(targets)
    if len(sizes) != n or len(thetas) != n:
        raise ValueError("warp_labels: %d label tables, %d sizes, %d angles" % (n, len(sizes), len(thetas)))
    if max_labels <= 0:
        raise ValueError("warp_labels: max_labels must be positive")
    S_h, S_w = int(input_size[0]), int(input_size[1])
    dev = out.device if out is not None else torch.device(device)
    if out is None:
        out = torch.empty(n, max_labels, 51, dtype=torch.float32, device=dev)
    elif tuple(out.shape) != (n, max_labels, 51) or out.dtype != torch.float32 or not out.is_contiguous():
        raise ValueError("warp_labels: out must be a contiguous fp32 [n, max_labels, 51] tensor")
    counts = torch.empty(n, dtype=torch.int32, device=dev)
    flags = torch.empty(n, max_labels, dtype=torch.int32, device=dev)
    if n == 0:
        return out, counts, flags
    rows, first = [], 0
    geo = np.zeros((n, GEO_D), dtype=np.float64)
    for i, (t, (h, w), th) in enumerate(zip(targets, sizes, thetas)):
        t = np.asarray(t, dtype=np.float64)
        t = t.reshape(-1, 51) if t.size else np.zeros((0, 51))
        T, cw, (y0, _, x0, _), (oh, ow) = Image_Distortion.geometry(th, h, w, custom_rows)
        if T < 2 or oh <= 0 or ow <= 0:
            raise ValueError("warp_labels: image %d (%d x %d at %s degrees) has no sector" % (i, h, w, th))
        geo[i] = (float(th), T, h, w, cw, x0, y0, oh, ow, min(S_h / oh, S_w / ow), first, t.shape[0])
        rows.append(t)
        first += t.shape[0]
    # one upload: the parameter table [n,12], then the label rows [R,51]
    dbl = np.concatenate([geo.reshape(-1)] + [t.reshape(-1) for t in rows] + [np.zeros(51)])
    if not np.isfinite(dbl).all():
        raise ValueError("warp_labels: non-finite label rows")
    dbl_t = torch.from_numpy(dbl).to(dev)
    cand = torch.empty(n, max_labels, 51, dtype=torch.float32, device=dev)
    keep = torch.empty(n, max_labels, dtype=torch.int32, device=dev)
    rot = _rot(dev)
    for lo in range(0, n, 65535):
        hi = min(n, lo + 65535)
        call("sector_labels", ptr(dbl_t, n * GEO_D), ptr(dbl_t, lo * GEO_D), ptr(rot), hi - lo, max_labels, ptr(cand, lo * max_labels * 51),
             ptr(keep, lo * max_labels), ptr(out, lo * max_labels * 51), ptr(counts, lo), ptr(flags, lo * max_labels), stream_ptr())
    return out, counts, flags


class FisheyeTransform(TrainTransform):
    """``TrainTransform`` whose every image goes through the sector warp WITH its labels: same ``batch(...)`` signature, so
    ``DataPrefetcher`` takes it unchanged.  ``theta=(lo, hi)``: one integer angle per image, drawn from the generator of the
    batch's data position - ``set_position(epoch, it)`` reseeds it from (seed, epoch, it), so a resumed run reproduces its batches."""

    def __init__(self, theta=(30, 90), max_labels=50, custom_rows=None, seed=0, device="cuda:0"):
        super().__init__(max_labels=max_labels, seed=seed)
        lo, hi = int(theta[0]), int(theta[1])
        if not 15 <= lo <= hi <= 180:
            raise ValueError("FisheyeTransform: angles must satisfy 15 <= lo <= hi <= 180")
        self.theta, self.custom_rows, self.seed, self.device = (lo, hi), custom_rows, int(seed), device
        self.last_thetas = self.last_counts = self.last_flags = None
        self.set_position(0, 0)

    def set_position(self, epoch, it):
        self.position = (int(epoch), int(it))
        self._theta_rng = position_rng(self.seed, epoch, it)

    def sample(self, n):
        lo, hi = self.theta
        return [int(self._theta_rng.randint(lo, hi + 1)) for _ in range(n)]

    def batch(self, images, targets, input_dim, out_images=None, out_labels=None):
        _lib.require_gpu()
        if self._dist is None:
            self._dist = Image_Distortion(self.device)
        thetas = self.sample(len(images))
        from .jpeg import finish_checked
        images = finish_checked(images, device=self.device)
        dev_imgs = [torch.as_tensor(np.ascontiguousarray(im) if isinstance(im, np.ndarray) else im).to(self.device) for im in images]
        warped = self._dist.distort_batch(dev_imgs, None, thetas, self.custom_rows)[0]
        imgs, _ = preproc_batch(warped, input_dim, device=self.device, out=out_images)
        labs, counts, flags = warp_labels(targets, [tuple(im.shape[:2]) for im in dev_imgs], thetas, input_dim, self.max_labels,
                                          self.custom_rows, out=out_labels, device=self.device)
        self.last_thetas, self.last_counts, self.last_flags = thetas, counts, flags
        return imgs, labs
