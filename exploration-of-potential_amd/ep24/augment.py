"""Training augmentation on the GPU for 24-point labels: mosaic, random affine, mixup, mirror, HSV (csrc/augment.hip).

The reference's 24p ``TrainTransform`` accepts ``flip_prob`` / ``hsv_prob`` and ignores them, and its mosaic /
``random_affine`` code (yolox_24p/data/) transforms boxes only.  Here the raw uint8 images that the prefetcher uploads
anyway are sampled straight into the network input through the inverse affine map, and every 24-point polygon is mapped
forward and its 24 rays are re-cast from the new centre (``ep24_augment_labels``).

``sample_params`` draws what stock YOLOX draws (``MosaicDetection.__getitem__``, ``get_affine_matrix``, ``_mirror``,
``augment_hsv``); ``sample_mixup`` adds ``MosaicDetection.mixup``'s draws from a generator of its own; ``mosaic_batch`` runs
the two launches on explicit parameters; ``MosaicTransform`` is the ``TrainTransform`` that a ``DataPrefetcher`` takes.

Mixup blends one more source of the batch into a mosaic image, in the same two launches (``ep24_augment_mix_u8`` /
``ep24_augment_mix_labels``): the partner is letterboxed, its canvas scaled by ``jit``, mirrored, cropped at (x_off, y_off) and
averaged with the mosaic as ``(a + b) >> 1`` BEFORE HSV; its polygons go through their own map and the same keep and re-cast
rules, behind the four tiles' rows.

Copy-paste (``sample_paste``, ``paste_batch``; csrc/paste.hip) is a post-pass of two more launches over the finished batch: an image
pastes objects of another image of the batch through a rigid integer transform (shift, optional mirror), each object's 24-gon being
its mask, wherever the object lies inside the image and hides less than ``paste_ioa`` of every object already there.  It is
YOLOv5's ``copy_paste``, which stock YOLOX and the reference lack; off unless ``AugParams.paste`` is set.

Deviations from the reference, on purpose: the three mosaic partners and the mixup partner of an image come from the SAME BATCH
(the reference draws them from the whole dataset; here nothing extra is uploaded); the reference mixes only when the mosaic has
labels left (``len(mosaic_labels) != 0``), which only the GPU knows - here the host-known stand-in is "the four tiles' sources
have at least one label row between them"; and the partner's pixel is ONE bilinear sample of the raw source, where cv2 resizes
twice (letterbox, then jitter).  There is no CPU fallback.
"""
import math

import numpy as np
import torch

from . import _lib
from ._lib import call, ptr, stream_ptr
from .input import TrainTransform, letterbox_geometry

HSV_GAINS = (5.0, 30.0, 30.0)         # augment_hsv's hgain, sgain, vgain


def affine_inverse(M):
    """Inverse of o = A c + t as the kernels take it: [[i00, i01, i02], [i10, i11, i12]] in double."""
    a00, a01, t0, a10, a11, t1 = (float(v) for v in np.asarray(M, dtype=np.float64).reshape(6))
    det = a00 * a11 - a01 * a10
    if det == 0.0:
        raise ValueError("singular affine matrix")
    i00, i01, i10, i11 = a11 / det, -a01 / det, -a10 / det, a00 / det
    return np.array([[i00, i01, -(i00 * t0 + i01 * t1)], [i10, i11, -(i10 * t0 + i11 * t1)]], dtype=np.float64)


def affine_matrix(angle, scale, shear_x, shear_y, tx, ty):
    """``get_affine_matrix``'s matrix: rotation by ``angle`` degrees about the origin times ``scale``
    (cv2.getRotationMatrix2D's convention: [[a, b], [-b, a]], a = scale*cos, b = scale*sin), then the two shears (degrees),
    then the translation in output pixels."""
    a, b = scale * math.cos(math.radians(angle)), scale * math.sin(math.radians(angle))
    r0, r1 = (a, b), (-b, a)
    kx, ky = math.tan(math.radians(shear_x)), math.tan(math.radians(shear_y))
    return np.array([[r0[0] + ky * r1[0], r0[1] + ky * r1[1], tx],
                     [r1[0] + kx * r0[0], r1[1] + kx * r0[1], ty]], dtype=np.float64)


class AugParams:
    """Explicit parameters of one batch of n output images: ``mosaic`` bool [n]; ``centre`` int [n,2] = (xc, yc) on the
    2S canvas; ``partners`` int [n,4] = source index of the top-left, top-right, bottom-left, bottom-right tile (column 0
    is the image itself); ``M`` float64 [n,2,3] canvas -> output and ``Minv`` its inverse; ``mirror`` bool [n];
    ``hsv_on`` bool [n]; ``hsv`` float64 [n,3] = gains (dh, ds, dv).  Without mosaic an image is its own single tile,
    letterboxed at the top left of an S canvas, and ``M`` is whatever the caller sets (``sample_params``: identity).
    Mixup, off by default (``sample_mixup`` fills it): ``mixup`` bool [n]; ``mix_partner`` int [n] = source index of the blended
    image; ``mix_jit`` float64 [n] = scale of its letterbox canvas; ``mix_flip`` bool [n]; ``mix_off`` int [n,2] = (x_off, y_off),
    the corner of the S_h x S_w window cut out of the jittered canvas.
    Copy-paste, off by default (``sample_paste`` fills it): ``paste`` bool [n]; ``paste_partner`` int [n] = the image of the batch
    whose objects are pasted (the image itself is allowed); ``paste_flip`` bool [n]; ``paste_off`` int [n,2] = (dx, dy) in output
    pixels; ``paste_select`` uint64 [n], bit k = the partner's k-th surviving row may be pasted."""

    def __init__(self, n):
        self.n = n
        self.mosaic = np.zeros(n, dtype=bool)
        self.centre = np.zeros((n, 2), dtype=np.int64)
        self.partners = np.tile(np.arange(n, dtype=np.int64)[:, None], (1, 4))
        self.M = np.tile(np.array([[1.0, 0.0, 0.0], [0.0, 1.0, 0.0]]), (n, 1, 1))
        self.Minv = self.M.copy()
        self.mirror = np.zeros(n, dtype=bool)
        self.hsv_on = np.zeros(n, dtype=bool)
        self.hsv = np.zeros((n, 3), dtype=np.float64)
        self.mixup = np.zeros(n, dtype=bool)
        self.mix_partner = np.arange(n, dtype=np.int64)
        self.mix_jit = np.ones(n, dtype=np.float64)
        self.mix_flip = np.zeros(n, dtype=bool)
        self.mix_off = np.zeros((n, 2), dtype=np.int64)
        self.paste = np.zeros(n, dtype=bool)
        self.paste_partner = np.arange(n, dtype=np.int64)
        self.paste_flip = np.zeros(n, dtype=bool)
        self.paste_off = np.zeros((n, 2), dtype=np.int64)
        self.paste_select = np.zeros(n, dtype=np.uint64)

    def set_matrix(self, i, M):
        self.M[i] = np.asarray(M, dtype=np.float64).reshape(2, 3)
        self.Minv[i] = affine_inverse(self.M[i])


def identity_params(n):
    """Parameters that make ``mosaic_batch`` the plain ``TrainTransform``."""
    return AugParams(n)


def position_rng(seed, epoch, it):
    """The generator of batch (epoch, it) of a run seeded with ``seed``."""
    return np.random.RandomState(np.array([seed, epoch, it], dtype=np.uint32))


def sample_params(rng, sizes, input_size, mosaic_prob=1.0, degrees=10.0, translate=0.1, mosaic_scale=(0.5, 1.5), shear=2.0,
                  flip_prob=0.5, hsv_prob=1.0):
    """Draws the parameters of ``len(sizes)`` output images from ``rng`` (a ``np.random.RandomState``).

    Per output image, in this order and ALWAYS all 20 numbers (what a coin switches off is drawn and dropped, so the
    parameters of image i depend on the generator's state and i only):
      1  u_mosaic  = random_sample()              mosaic if u_mosaic < mosaic_prob
      2  yc        = int(uniform(0.5 S_h, 1.5 S_h))
      3  xc        = int(uniform(0.5 S_w, 1.5 S_w))
      4-6 partners = randint(0, n) three times    (top-right, bottom-left, bottom-right; same batch)
      7  angle     = uniform(-degrees, degrees)
      8  scale     = uniform(*mosaic_scale)
      9  shear_x, 10 shear_y = uniform(-shear, shear)
      11 tx = uniform(-translate, translate) * S_w, 12 ty = ... * S_h
      13 u_mirror  = random_sample()              mirror if u_mirror < flip_prob
      14 u_hsv     = random_sample()              HSV if u_hsv < hsv_prob
      15-17 gains  = uniform(-1, 1) * (5, 30, 30), 18-20 switches = randint(0, 2); gain * switch truncated to an integer
    Without mosaic the matrix is the identity (stock YOLOX applies mirror and HSV only to such an image)."""
    n = len(sizes)
    S_h, S_w = int(input_size[0]), int(input_size[1])
    p = AugParams(n)
    for i in range(n):
        u_mosaic = rng.random_sample()
        yc = int(rng.uniform(0.5 * S_h, 1.5 * S_h))
        xc = int(rng.uniform(0.5 * S_w, 1.5 * S_w))
        partners = [int(rng.randint(0, n)) for _ in range(3)]
        angle = rng.uniform(-degrees, degrees)
        scale = rng.uniform(mosaic_scale[0], mosaic_scale[1])
        shear_x, shear_y = rng.uniform(-shear, shear), rng.uniform(-shear, shear)
        tx, ty = rng.uniform(-translate, translate) * S_w, rng.uniform(-translate, translate) * S_h
        u_mirror, u_hsv = rng.random_sample(), rng.random_sample()
        gains = [rng.uniform(-1.0, 1.0) * g for g in HSV_GAINS]
        switches = [int(rng.randint(0, 2)) for _ in range(3)]
        if u_mosaic < mosaic_prob:
            p.mosaic[i] = True
            p.centre[i] = (xc, yc)
            p.partners[i, 1:] = partners
            p.set_matrix(i, affine_matrix(angle, scale, shear_x, shear_y, tx, ty))
        p.mirror[i] = u_mirror < flip_prob
        p.hsv_on[i] = u_hsv < hsv_prob
        p.hsv[i] = [float(int(g * s)) for g, s in zip(gains, switches)]
    return p


def mixup_rng(seed, epoch, it):
    """The generator of the mixup draws of batch (epoch, it): its own stream, so ``sample_params``' draws do not move."""
    return np.random.RandomState(np.array([seed, epoch, it, 1], dtype=np.uint32))


def mixup_canvas(jit, input_size):
    """(Wj, Hj) = the partner's letterbox canvas after the jitter: int(S_w*jit), int(S_h*jit), as the reference's cv2.resize."""
    Wj, Hj = int(int(input_size[1]) * jit), int(int(input_size[0]) * jit)
    if Wj < 1 or Hj < 1:
        raise ValueError("mixup: a jitter of %r leaves an empty %d x %d canvas" % (jit, Wj, Hj))
    return Wj, Hj


def sample_mixup(rng, params, sizes, label_counts, input_size, mixup_prob=1.0, mixup_scale=(0.5, 1.5)):
    """Fills the mixup fields of ``params`` (an ``AugParams`` for ``len(sizes)`` images) from ``rng`` (``mixup_rng``) and returns
    ``params``.  ``label_counts``: label rows per source image.

    Per output image, in this order and ALWAYS all 6 numbers:
      1  u_mix   = random_sample()              wanted if u_mix < mixup_prob
      2  jit     = uniform(*mixup_scale)
      3  u_flip  = random_sample()              flip if u_flip > 0.5
      4  partner = randint(0, n)
      5  u_y, 6 u_x = random_sample()           y_off = int(u_y*(Hj - S_h)) if Hj > S_h else 0, x likewise: randint(0, Hj-S_h-1)'s range
    Mixup is ON for image i iff it is wanted, the image is a mosaic, a partner with labels exists (the drawn index, else the next
    one cyclically that has label rows; none in the batch: no mixup) and the four tiles' sources have a label row between them
    (the host-known stand-in for the reference's ``len(mosaic_labels) != 0``)."""
    n = len(sizes)
    if params.n != n or len(label_counts) != n:
        raise ValueError("sample_mixup: %d sizes, %d label counts, parameters for %d" % (n, len(label_counts), params.n))
    S_h, S_w = int(input_size[0]), int(input_size[1])
    has = [int(c) > 0 for c in label_counts]
    for i in range(n):
        u_mix = rng.random_sample()
        jit = rng.uniform(mixup_scale[0], mixup_scale[1])
        u_flip = rng.random_sample()
        partner = int(rng.randint(0, n))
        u_y, u_x = rng.random_sample(), rng.random_sample()
        params.mixup[i] = False
        if not (u_mix < mixup_prob and params.mosaic[i] and any(has) and any(has[int(j)] for j in params.partners[i])):
            continue
        while not has[partner]:
            partner = (partner + 1) % n
        Wj, Hj = mixup_canvas(jit, (S_h, S_w))
        params.mixup[i] = True
        params.mix_partner[i], params.mix_jit[i], params.mix_flip[i] = partner, jit, u_flip > 0.5
        params.mix_off[i] = (int(u_x * (Wj - S_w)) if Wj > S_w else 0, int(u_y * (Hj - S_h)) if Hj > S_h else 0)
    return params


def mixup_layout(params, i, sizes, input_size):
    """The mixup descriptor of output image i as the kernels take it (include/ep24.h): (int64 [16] without the byte offset and
    the label rows, float64 [12]), or None when mixup is off for the image."""
    if not params.mixup[i]:
        return None
    S_h, S_w = int(input_size[0]), int(input_size[1])
    j = int(params.mix_partner[i])
    h, w = sizes[j]
    s, rh, rw = letterbox_geometry(h, w, (S_h, S_w))
    Wj, Hj = mixup_canvas(float(params.mix_jit[i]), (S_h, S_w))
    x_off, y_off = int(params.mix_off[i][0]), int(params.mix_off[i][1])
    flip = bool(params.mix_flip[i])
    if x_off < 0 or y_off < 0:
        raise ValueError("mixup: negative crop offset (%d, %d)" % (x_off, y_off))
    if rw <= 0 or rh <= 0:
        raise ValueError("mixup: the partner's letterbox is empty")
    ints = np.zeros(16, dtype=np.int64)
    ints[:12] = (1, 0, h, w, 3 * w, rw, rh, Wj, Hj, x_off, y_off, int(flip))
    a00, a11 = (-(Wj / S_w) if flip else Wj / S_w), Hj / S_h
    dbl = np.zeros(12, dtype=np.float64)
    dbl[:11] = (S_w / Wj, S_h / Hj, 1.0 / (rw / w), 1.0 / (rh / h), s, a00, a11, float(Wj - x_off if flip else -x_off),
                float(-y_off), 1.0 / a00, 1.0 / a11)
    return ints, dbl


def paste_rng(seed, epoch, it):
    """The generator of the copy-paste draws of batch (epoch, it): its own stream, so ``sample_params``' and ``sample_mixup``'s
    draws do not move."""
    return np.random.RandomState(np.array([seed, epoch, it, 2], dtype=np.uint32))


def sample_paste(rng, params, n, input_size, paste_prob, obj_prob=0.5):
    """Fills the copy-paste fields of ``params`` (an ``AugParams`` for ``n`` images) from ``rng`` (``paste_rng``) and returns
    ``params``.

    Per output image, in this order and ALWAYS all 69 numbers, whatever the outcome:
      1  u_on    = random_sample()              paste if u_on < paste_prob
      2  partner = randint(0, n)                the image of the batch whose objects are pasted (the image itself is allowed)
      3  u_flip  = random_sample()              flip if u_flip < 0.5
      4  dx      = randint(-(S_w // 2), S_w // 2 + 1)      i.e. [-S_w//2, S_w//2], in output pixels
      5  dy      = randint(-(S_h // 2), S_h // 2 + 1)
      6-69 u_k   = random_sample(), k = 0 .. 63            bit k of the select mask is set if u_k < obj_prob
    Which of the selected objects are pasted is decided on the GPU (``ep24_paste_labels``: inside the image, and hiding less than
    the IoA threshold of every object already there)."""
    if params.n != n:
        raise ValueError("sample_paste: %d images, parameters for %d" % (n, params.n))
    S_h, S_w = int(input_size[0]), int(input_size[1])
    for i in range(n):
        u_on = rng.random_sample()
        partner = int(rng.randint(0, n))
        u_flip = rng.random_sample()
        dx = int(rng.randint(-(S_w // 2), S_w // 2 + 1))
        dy = int(rng.randint(-(S_h // 2), S_h // 2 + 1))
        bits = rng.random_sample(64) < obj_prob
        params.paste[i] = u_on < paste_prob
        params.paste_partner[i], params.paste_flip[i], params.paste_off[i] = partner, u_flip < 0.5, (dx, dy)
        params.paste_select[i] = np.uint64(sum(1 << k for k in range(64) if bits[k]))
    return params


def paste_descriptors(params):
    """The copy-paste descriptors of a batch as the kernels take them (include/ep24.h): int64 [n, 8] = (on, partner, flip, dx, dy,
    select, 0, 0).  The library cannot read a descriptor in device memory, so this is the check that refuses a partner outside the
    batch (``EP24_E_ARG``); the kernels treat such a descriptor as off."""
    n = params.n
    desc = np.zeros((n, 8), dtype=np.int64)
    desc[:, 0] = np.asarray(params.paste, dtype=bool)
    desc[:, 1] = params.paste_partner
    desc[:, 2] = np.asarray(params.paste_flip, dtype=bool)
    desc[:, 3:5] = params.paste_off
    desc[:, 5] = np.asarray(params.paste_select, dtype=np.uint64).view(np.int64)
    check_paste_descriptors(desc)
    return desc


def check_paste_descriptors(desc):
    desc = np.asarray(desc)
    n = len(desc)
    bad = (desc[:, 0] != 0) & ((desc[:, 1] < 0) | (desc[:, 1] >= n))
    if bad.any():
        i = int(np.nonzero(bad)[0][0])
        raise _lib.Ep24Error("ep24_paste_labels failed (-1, EP24_E_ARG): copy-paste partner %d of image %d is not in the batch of %d"
                             % (int(desc[i, 1]), i, n))


def paste_batch(pre_images, pre_labels, pre_counts, desc, min_margin=2.0, ioa_thr=0.30, out_images=None, out_labels=None,
                counts=None, check=True):
    """The copy-paste post-pass (``ep24_paste_labels``, then ``ep24_paste_u8`` on its rows) over a batch that the augmentation's two
    launches produced: pre_images [n,3,S_h,S_w] fp32, pre_labels [n,max_labels,51] fp32, pre_counts [n] int32, ``desc`` int64
    [n,8] (``paste_descriptors``).  The inputs are a snapshot: the outputs are other buffers.
    Returns (images, labels, counts [n] int32, paste_range [n,2] int32)."""
    _lib.require_gpu()
    n, _, S_h, S_w = (int(v) for v in pre_images.shape)
    max_labels = int(pre_labels.shape[1])
    dev = pre_images.device
    if not (pre_images.dtype == pre_labels.dtype == torch.float32 and pre_counts.dtype == torch.int32 and pre_images.is_contiguous()
            and pre_labels.is_contiguous() and pre_counts.is_contiguous() and tuple(pre_labels.shape) == (n, max_labels, 51)
            and tuple(pre_counts.shape) == (n,)):
        raise ValueError("paste_batch takes contiguous fp32 [n,3,S_h,S_w] images, fp32 [n,max_labels,51] labels and int32 [n] counts")
    desc = np.array(desc, dtype=np.int64).reshape(n, 8)                            # a copy: the upload wants a writable array
    if check:
        check_paste_descriptors(desc)
    if out_images is None:
        out_images = torch.empty_like(pre_images)
    if out_labels is None:
        out_labels = torch.empty_like(pre_labels)
    if counts is None:
        counts = torch.empty(n, dtype=torch.int32, device=dev)
    ranges = torch.empty(n, 2, dtype=torch.int32, device=dev)
    desc_t = torch.from_numpy(desc).to(dev)
    call("paste_labels", ptr(pre_labels), ptr(pre_counts), ptr(desc_t), n, S_h, S_w, float(min_margin), float(ioa_thr),
         ptr(out_labels), ptr(counts), ptr(ranges), max_labels, stream_ptr())
    call("paste_u8", ptr(pre_images), ptr(out_labels), ptr(ranges), ptr(desc_t), n, ptr(out_images), S_h, S_w, max_labels,
         stream_ptr())
    return out_images, out_labels, counts, ranges


def _paste_staging(cache, n, S_h, S_w, max_labels, dev):
    """The buffers the augmentation's two launches write when copy-paste follows, kept in ``cache`` (a dict of the caller's or the
    transform's) per (n, S_h, S_w, max_labels, device)."""
    key = (n, S_h, S_w, max_labels, str(dev))
    if cache is None or key not in cache:
        bufs = (torch.empty(n, 3, S_h, S_w, dtype=torch.float32, device=dev),
                torch.empty(n, max_labels, 51, dtype=torch.float32, device=dev), torch.empty(n, dtype=torch.int32, device=dev))
        if cache is None:
            return bufs
        cache[key] = bufs
    return cache[key]


def tile_layout(params, i, sizes, input_size):
    """The tiles of output image i: list of (source index, rw, rh, (lx1, ly1, lx2, ly2), padw, padh).  Mosaic: quadrant q
    (bit 0 = right, bit 1 = bottom) holds its source, resized to (rw, rh), with the corner that touches the mosaic centre
    (xc, yc) pinned there and the far side cropped at the 2S canvas - the placement of the reference's mosaic."""
    S_h, S_w = int(input_size[0]), int(input_size[1])
    out = []
    if not params.mosaic[i]:
        h, w = sizes[i]
        _, rh, rw = letterbox_geometry(h, w, (S_h, S_w))
        return [(i, rw, rh, (0, 0, rw, rh), 0, 0)]
    xc, yc = int(params.centre[i][0]), int(params.centre[i][1])
    for q in range(4):
        j = int(params.partners[i][q])
        h, w = sizes[j]
        _, rh, rw = letterbox_geometry(h, w, (S_h, S_w))
        if q & 1:
            lx1, lx2, padw = xc, min(xc + rw, 2 * S_w), xc
        else:
            lx1, lx2, padw = max(xc - rw, 0), xc, xc - rw
        if q & 2:
            ly1, ly2, padh = yc, min(yc + rh, 2 * S_h), yc
        else:
            ly1, ly2, padh = max(yc - rh, 0), yc, yc - rh
        out.append((j, rw, rh, (lx1, ly1, lx2, ly2), padw, padh))
    return out


_ROT = {}


def _rot(dev):
    from .labels24 import _rot_table
    if dev not in _ROT:
        _ROT[dev] = _rot_table(dev).clone()
    return _ROT[dev]


def mosaic_batch(images, targets, params, input_size, max_labels=50, out_images=None, out_labels=None, min_margin=2.0,
                 device="cuda:0", paste_ioa=0.30, paste_staging=None):
    """images: list of uint8 [h,w,3] arrays / tensors; targets: list of [k,51] normalised label rows; params: ``AugParams``.
    Returns (images [n,3,S_h,S_w] fp32, labels [n,max_labels,51] fp32, survivors per image [n] int32) on the device.
    With ``params.paste`` set on any image the two launches write staging buffers (kept in the dict ``paste_staging`` per shape, if
    one is given) and the copy-paste post-pass (``paste_batch``, IoA threshold ``paste_ioa``) writes the outputs; the count then
    includes the pasted rows.  With it set on none the calls are those of a batch without the fields."""
    _lib.require_gpu()
    n = len(images)
    if params.n != n or len(targets) != n:
        raise ValueError("mosaic_batch: %d images, %d label tables, parameters for %d" % (n, len(targets), params.n))
    S_h, S_w = int(input_size[0]), int(input_size[1])
    dev = out_images.device if out_images is not None else torch.device(device)
    if out_images is None:
        out_images = torch.empty(n, 3, S_h, S_w, dtype=torch.float32, device=dev)
    if out_labels is None:
        out_labels = torch.empty(n, max_labels, 51, dtype=torch.float32, device=dev)
    counts = torch.empty(n, dtype=torch.int32, device=dev)
    if n == 0:
        return out_images, out_labels, counts
    final = None
    if bool(np.asarray(params.paste).any()):
        desc = paste_descriptors(params)                                           # refuses a partner outside the batch before any launch
        final = (out_images, out_labels, counts)
        out_images, out_labels, counts = _paste_staging(paste_staging, n, S_h, S_w, max_labels, dev)
    flat, offs, sizes, off = [], [], [], 0
    for im in images:
        im = im if isinstance(im, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(im))
        if im.dim() != 3 or im.shape[2] != 3 or im.dtype != torch.uint8 or im.shape[0] == 0 or im.shape[1] == 0:
            raise ValueError("mosaic_batch takes uint8 [h,w,3] images")
        h, w = int(im.shape[0]), int(im.shape[1])
        flat.append(im.reshape(-1))
        offs.append(off)
        sizes.append((h, w))
        off += h * w * 3
    rows, row_off = [], [0]
    for t in targets:
        t = np.asarray(t, dtype=np.float64)
        t = t.reshape(-1, 51) if t.size else np.zeros((0, 51))
        rows.append(t)
        row_off.append(row_off[-1] + t.shape[0])
    tiles = np.zeros((n, 4, 16), dtype=np.int64)
    # doubles in one upload: tile scales [n,4,3], parameters [n,16], label rows [R,51]
    dbl = np.zeros(n * 12 + n * 16 + max(row_off[-1], 1) * 51, dtype=np.float64)
    tsc, par = dbl[:n * 12].reshape(n, 4, 3), dbl[n * 12:n * 28].reshape(n, 16)
    if row_off[-1]:
        dbl[n * 28:] = np.concatenate(rows, 0).reshape(-1)
    flags = np.zeros((n, 2), dtype=np.int32)
    mixing = bool(np.asarray(params.mixup).any())
    mix_i, mix_d = np.zeros((n, 16), dtype=np.int64), np.zeros((n, 12), dtype=np.float64)
    for i in range(n):
        for q, (j, rw, rh, (lx1, ly1, lx2, ly2), padw, padh) in enumerate(tile_layout(params, i, sizes, (S_h, S_w))):
            h, w = sizes[j]
            if rw <= 0 or rh <= 0 or lx2 <= lx1 or ly2 <= ly1:
                continue                                                       # nothing of this tile is on the canvas
            tiles[i, q, :14] = (offs[j], h, w, 3 * w, rw, rh, lx1, ly1, lx2, ly2, padw, padh, row_off[j], row_off[j + 1])
            tsc[i, q] = (1.0 / (rw / w), 1.0 / (rh / h), min(S_h / h, S_w / w))
        par[i, 0:6] = params.M[i].reshape(6)
        par[i, 6:12] = params.Minv[i].reshape(6)
        par[i, 12:15] = params.hsv[i]
        flags[i] = (int(params.mirror[i]), int(params.hsv_on[i]))
        if params.mixup[i]:
            j = int(params.mix_partner[i])
            if not 0 <= j < n:
                raise ValueError("mosaic_batch: mixup partner %d of image %d is not in the batch" % (j, i))
            mix_i[i], mix_d[i] = mixup_layout(params, i, sizes, (S_h, S_w))
            mix_i[i, 1], mix_i[i, 12], mix_i[i, 13] = offs[j], row_off[j], row_off[j + 1]
    if not (np.isfinite(par).all() and np.isfinite(tsc).all() and np.isfinite(mix_d).all()):
        raise ValueError("mosaic_batch: non-finite parameters")
    buf = torch.cat([f.to(dev, non_blocking=True) for f in flat])
    tiles_t = torch.from_numpy(tiles).to(dev)
    dbl_t = torch.from_numpy(dbl).to(dev)
    flags_t = torch.from_numpy(flags).to(dev)
    rot = _rot(dev)
    if mixing:
        mi_t, md_t = torch.from_numpy(mix_i).to(dev), torch.from_numpy(mix_d).to(dev)
        for lo in range(0, n, 65535):
            hi = min(n, lo + 65535)
            call("augment_mix_u8", ptr(buf), ptr(tiles_t, lo * 64), ptr(dbl_t, lo * 12), ptr(dbl_t, n * 12 + lo * 16), ptr(flags_t, lo * 2),
                 ptr(mi_t, lo * 16), ptr(md_t, lo * 12), hi - lo, ptr(out_images, lo * 3 * S_h * S_w), S_h, S_w, stream_ptr())
        call("augment_mix_labels", ptr(dbl_t, n * 28), ptr(tiles_t), ptr(dbl_t), ptr(dbl_t, n * 12), ptr(flags_t), ptr(mi_t), ptr(md_t),
             ptr(rot), n, S_h, S_w, float(min_margin), ptr(out_labels), ptr(counts), max_labels, stream_ptr())
    else:
        for lo in range(0, n, 65535):
            hi = min(n, lo + 65535)
            call("augment_u8", ptr(buf), ptr(tiles_t, lo * 64), ptr(dbl_t, lo * 12), ptr(dbl_t, n * 12 + lo * 16), ptr(flags_t, lo * 2),
                 hi - lo, ptr(out_images, lo * 3 * S_h * S_w), S_h, S_w, stream_ptr())
        call("augment_labels", ptr(dbl_t, n * 28), ptr(tiles_t), ptr(dbl_t), ptr(dbl_t, n * 12), ptr(flags_t), ptr(rot), n, S_h, S_w,
             float(min_margin), ptr(out_labels), ptr(counts), max_labels, stream_ptr())
    if final is not None:
        return paste_batch(out_images, out_labels, counts, desc, min_margin=min_margin, ioa_thr=paste_ioa, out_images=final[0],
                           out_labels=final[1], counts=final[2], check=False)[:3]
    return out_images, out_labels, counts


class MosaicTransform(TrainTransform):
    """``TrainTransform`` with the augmentation switched on: same ``batch(...)`` signature, so ``DataPrefetcher`` takes it
    unchanged.  ``enabled = False`` makes it the plain transform (the last ``no_aug_epochs`` of a YOLOX run).
    ``set_position(epoch, it)`` reseeds the generator from (seed, epoch, it): the batch at a data position gets the same
    parameters whenever it is produced, so a resumed run reproduces the batches it would have seen.  ``mixup_prob > 0`` adds
    mixup (``sample_mixup``, from a generator of its own at the same position); with 0 the transform is what it is without.
    ``copy_paste_prob > 0`` adds copy-paste (``sample_paste``, a third generator at the same position): an image pastes objects of
    another image of the batch, each selected with ``copy_paste_obj_prob``, where they hide less than ``copy_paste_ioa`` of every
    object already there; with 0 the transform is what it is without."""

    def __init__(self, max_labels=50, flip_prob=0.5, hsv_prob=1.0, mosaic_prob=1.0, degrees=10.0, translate=0.1,
                 mosaic_scale=(0.5, 1.5), shear=2.0, min_margin=2.0, seed=0, enabled=True, mixup_prob=0.0,
                 mixup_scale=(0.5, 1.5), copy_paste_prob=0.0, copy_paste_obj_prob=0.5, copy_paste_ioa=0.30):
        super().__init__(max_labels=max_labels, flip_prob=flip_prob, hsv_prob=hsv_prob, seed=seed)
        self.hsv_prob, self.mosaic_prob, self.degrees, self.translate = hsv_prob, mosaic_prob, degrees, translate
        self.mosaic_scale, self.shear, self.min_margin = tuple(mosaic_scale), shear, min_margin
        self.seed, self.enabled = int(seed), enabled
        self.mixup_prob, self.mixup_scale = mixup_prob, tuple(mixup_scale)
        self.copy_paste_prob, self.copy_paste_obj_prob, self.copy_paste_ioa = copy_paste_prob, copy_paste_obj_prob, copy_paste_ioa
        self._paste_staging = {}
        self.last_params = self.last_counts = None
        self.set_position(0, 0)

    @classmethod
    def from_exp(cls, exp, max_labels=50, seed=0, mixup=False, copy_paste=False):
        """``mixup=True`` reads the Exp's ``mixup_prob`` / ``mixup_scale`` (``train_24p.py --mixup``); otherwise mixup stays off.
        ``copy_paste=True`` reads the Exp's ``copy_paste_prob`` (``train_24p.py --copy-paste``); otherwise copy-paste stays off."""
        extra = dict(mixup_prob=exp.mixup_prob, mixup_scale=exp.mixup_scale) if mixup else {}
        if copy_paste:
            extra["copy_paste_prob"] = exp.copy_paste_prob
        return cls(max_labels=max_labels, flip_prob=exp.flip_prob, hsv_prob=exp.hsv_prob, mosaic_prob=exp.mosaic_prob,
                   degrees=exp.degrees, translate=exp.translate, mosaic_scale=exp.mosaic_scale, shear=exp.shear, seed=seed, **extra)

    def set_position(self, epoch, it):
        self.position = (int(epoch), int(it))
        self._aug_rng = position_rng(self.seed, epoch, it)
        self._mix_rng = mixup_rng(self.seed, epoch, it)
        self._paste_rng = paste_rng(self.seed, epoch, it)

    def sample(self, sizes, input_dim, label_counts=None):
        """The parameters of the next batch; mixup needs ``label_counts`` (label rows per source) and is left off without."""
        p = sample_params(self._aug_rng, sizes, input_dim, mosaic_prob=self.mosaic_prob, degrees=self.degrees,
                          translate=self.translate, mosaic_scale=self.mosaic_scale, shear=self.shear,
                          flip_prob=self.flip_prob, hsv_prob=self.hsv_prob)
        if self.mixup_prob > 0 and label_counts is not None:
            sample_mixup(self._mix_rng, p, sizes, label_counts, input_dim, mixup_prob=self.mixup_prob, mixup_scale=self.mixup_scale)
        if self.copy_paste_prob > 0:
            sample_paste(self._paste_rng, p, len(sizes), input_dim, self.copy_paste_prob, obj_prob=self.copy_paste_obj_prob)
        return p

    def batch(self, images, targets, input_dim, out_images=None, out_labels=None):
        if not self.enabled:
            return super().batch(images, targets, input_dim, out_images=out_images, out_labels=out_labels)
        _lib.require_gpu()
        from .jpeg import finish_checked
        images = finish_checked(images)                   # entropy-decoded JPEG files (ep24.jpeg.JpegCoefficients) -> uint8 BGR on the device
        params = self.sample([tuple(im.shape[:2]) for im in images], input_dim,
                             [np.asarray(t).size // 51 for t in targets])
        imgs, labs, counts = mosaic_batch(images, targets, params, input_dim, self.max_labels, out_images, out_labels,
                                          min_margin=self.min_margin, paste_ioa=self.copy_paste_ioa,
                                          paste_staging=self._paste_staging)
        self.last_params, self.last_counts = params, counts
        return imgs, labs
