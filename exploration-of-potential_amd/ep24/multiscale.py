"""Multiscale training (the reference's ``Exp.random_resize`` / ``Exp.preprocess``, exp/yolox_base.py:93-118, driven by
core/trainer.py:250-254): the finished fp32 batch and its label table are resized to the step's input size on the GPU
(csrc/preproc.hip: ``ep24_resize_bilinear_f32``, ``ep24_scale_labels`` - two launches), and ``MultiScaleStep`` keeps one
captured ``ep24.train.TrainStep`` per visited size on the one model, loss, EMA copy and parameter home.

Every plan owns its activations, so the number of resident plans is bounded: ``max_plans`` of them, or - automatic - as many as
the free device memory holds (least recently used first out).  DESIGN.md section 7 has the rule and the measured footprints.
"""
import collections
import gc
import random
import time

import torch

from . import _lib
from ._lib import call, ptr, stream_ptr


def _hw(size):
    return (int(size), int(size)) if isinstance(size, int) else (int(size[0]), int(size[1]))


def resize_batch(images, labels, tsize, out_images=None, out_labels=None):
    """images [B,3,H,W], labels [B,L,51]: CUDA fp32 contiguous.  Returns (images [B,3,tsize], labels with the x columns times
    tsize[1] / W and the y columns times tsize[0] / H), written into ``out_images`` / ``out_labels`` when given (``out_labels`` may
    be ``labels`` itself).  Two launches on the current stream."""
    if images.dim() != 4 or images.shape[1] != 3 or labels.dim() != 3 or labels.shape[2] != 51 or labels.shape[0] != images.shape[0]:
        raise IndexError("resize_batch takes images [B,3,H,W] and labels [B,L,51], got %s and %s" % (tuple(images.shape), tuple(labels.shape)))
    th, tw = _hw(tsize)
    B, _, H, W = images.shape
    if th <= 0 or tw <= 0 or H <= 0 or W <= 0:
        raise IndexError("resize_batch: empty size %s -> %s" % ((H, W), (th, tw)))
    for name, x in (("images", images), ("labels", labels), ("out_images", out_images), ("out_labels", out_labels)):
        if x is None:
            continue
        if not x.is_cuda:
            raise _lib.Ep24Error("ep24: resize_batch %s must live on the GPU (no CPU fallback on the product path)" % name)
        if x.dtype != torch.float32 or not x.is_contiguous():
            raise IndexError("resize_batch: %s must be contiguous float32" % name)
    _lib.require_gpu()
    if out_images is None:
        out_images = torch.empty(B, 3, th, tw, dtype=torch.float32, device=images.device)
    elif tuple(out_images.shape) != (B, 3, th, tw):
        raise IndexError("resize_batch: out_images is %s, expected %s" % (tuple(out_images.shape), (B, 3, th, tw)))
    if out_labels is None:
        out_labels = torch.empty_like(labels)
    elif out_labels.shape != labels.shape:
        raise IndexError("resize_batch: out_labels is %s, expected %s" % (tuple(out_labels.shape), tuple(labels.shape)))
    if B:
        call("resize_bilinear_f32", ptr(images), B * 3, H, W, ptr(out_images), th, tw, stream_ptr())
        if labels.shape[1]:
            call("scale_labels", ptr(labels), ptr(out_labels), B * labels.shape[1], tw / W, th / H, stream_ptr())
    return out_images, out_labels


def size_for(exp, seed, k):
    """The input size of the ``k``-th draw of a run: ``exp.random_resize`` on a generator that follows from ``(seed, k)`` alone, so
    a resumed run continues the sequence of the run it resumes."""
    return exp.random_resize(rng=random.Random(int(seed) + 1000003 * int(k)))


def free_device_bytes():
    """What a new plan can still allocate: the driver's free bytes plus what torch's allocator has reserved and not handed out."""
    return torch.cuda.mem_get_info()[0] + torch.cuda.memory_reserved() - torch.cuda.memory_allocated()


class MultiScaleStep:
    """One captured training step per input size.  ``step(images, labels, tsize)`` takes the batch at ``base_size`` (or the
    buffers of ``inputs(tsize)``, already filled) and returns what ``TrainStep.step`` returns.

    ``max_plans > 0``: at most that many plans stay resident; ``0``: a plan is created only while the free device memory is at
    least 1.25 x the largest footprint seen so far, scaled by the ratio of pixel counts - least recently used plans go first, the
    plan about to run never.  An evicted size is built and captured again when it comes back (``captures`` counts)."""

    HEADROOM = 1.25

    def __init__(self, model, loss_fn, lr, momentum, batch, base_size, ema=None, weight_decay=0.0, use_l1=False, max_plans=0,
                 **trainstep_kw):
        _lib.require_gpu()
        if max_plans < 0:
            raise ValueError("MultiScaleStep: negative max_plans %r" % (max_plans,))
        self.model, self.loss_fn, self.ema = model, loss_fn, ema
        self.lr, self.momentum, self.batch = lr, momentum, batch
        self.weight_decay, self.use_l1 = float(weight_decay), bool(use_l1)
        self.base_size = _hw(base_size)
        self.max_plans = int(max_plans)
        self.kw = trainstep_kw
        self.plans = collections.OrderedDict()           # size -> TrainStep, least recently used first
        self.sizes_seen = []                             # every size a step ran at, in order of first use
        self.captures = 0
        self.footprints = {}                             # size -> bytes: memory_allocated() delta of construction + first capture
        self.capture_seconds = {}                        # size -> host seconds of the latest capture (synchronised)
        self.evictions = 0

    @property
    def resident(self):
        return list(self.plans)

    # ---- the setters of TrainStep: every resident plan, and (through the stored values) every later one
    def set_lr(self, lr):
        self.lr = lr
        for ts in self.plans.values():
            ts.set_lr(lr)

    def set_weight_decay(self, w):
        w = float(w)
        if w < 0:
            raise ValueError("MultiScaleStep: negative weight_decay %r" % w)
        self.weight_decay = w
        for ts in self.plans.values():
            ts.set_weight_decay(w)

    def set_use_l1(self, on):
        self.use_l1 = bool(on)
        for ts in self.plans.values():
            ts.set_use_l1(on)

    # ---- residency
    def _need(self, size):
        px = size[0] * size[1]
        return max((self.HEADROOM * b * px / (s[0] * s[1]) for s, b in self.footprints.items()), default=0.0)

    def _evict(self, size):
        """Synchronises, drops the plan's step object with its graphs and workspace, and the engine behind it."""
        torch.cuda.synchronize()
        ts = self.plans.pop(size)
        ts.graphs = ts.g_fwd = ts.g_bwd = ts.g_upd = ts.g_upd_early = ts.g_pre = ts.g_pre_bwd = None
        if self.loss_fn._ws is ts.ws:
            self.loss_fn._ws = None
        del ts
        self.model.release_engine(self.batch, size)
        gc.collect()                                     # the engine's launch lists refer back to it
        self.evictions += 1

    def _make_room(self, size):
        if self.max_plans > 0:
            while len(self.plans) >= self.max_plans:
                self._evict(next(iter(self.plans)))
            return
        need = self._need(size)
        while self.plans and free_device_bytes() < need:
            self._evict(next(iter(self.plans)))

    def _plan(self, size):
        size = _hw(size)
        ts = self.plans.get(size)
        if ts is not None:
            self.plans.move_to_end(size)
            return ts
        from .train import TrainStep
        self._make_room(size)
        gc.collect()                                     # garbage that dies while the plan is built would be taken off its footprint
        m0 = torch.cuda.memory_allocated()
        ts = TrainStep(self.model, self.loss_fn, lr=self.lr, momentum=self.momentum, batch=self.batch, size=size, ema=self.ema,
                       use_l1=self.use_l1, weight_decay=self.weight_decay, **self.kw)
        ts._ms_bytes = torch.cuda.memory_allocated() - m0
        self.plans[size] = ts
        return ts

    def inputs(self, tsize):
        """The (images, labels) input buffers of the plan for ``tsize`` (created on first use): what ``resize_batch`` /
        ``Exp.preprocess(..., out=)`` writes into."""
        ts = self._plan(tsize)
        return ts.eng.images, ts.labels

    def step(self, images, labels, tsize):
        size = _hw(tsize)
        ts = self._plan(size)
        if size not in self.sizes_seen:
            self.sizes_seen.append(size)
        if size == self.base_size:
            args = (images, labels)
        else:
            own = images.data_ptr() == ts.eng.images.data_ptr() and labels.data_ptr() == ts.labels.data_ptr()
            if not own:                                  # the batch at another size: resized straight into the plan's inputs
                resize_batch(images, labels, size, out_images=ts.eng.images, out_labels=ts.labels)
            args = ()
        if ts.graphs is None and ts.use_graph:
            # TrainStep.step captures now (its warm-up restores the BatchNorm statistics and the loss state: not a step)
            torch.cuda.synchronize()
            m0, t0 = torch.cuda.memory_allocated(), time.perf_counter()
            res = ts.step(*args)
            torch.cuda.synchronize()
            self.capture_seconds[size] = time.perf_counter() - t0
            self.captures += 1
            if hasattr(ts, "_ms_bytes"):                 # the plan's first capture: its footprint is known now
                self.footprints[size] = ts._ms_bytes + torch.cuda.memory_allocated() - m0
                del ts._ms_bytes
            return res
        return ts.step(*args)
