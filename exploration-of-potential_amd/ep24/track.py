"""Tracking of 24-point detections across frames (csrc/track.hip; include/ep24.h section T1; DESIGN.md section 7, "Tracking").

``Tracker24`` keeps S independent streams of at most ``max_tracks`` objects in three device tables and associates every frame's
``postprocess`` rows to them by the exact area IoU of the 24-gons: first the rows with score >= ``high_thre`` against every live
track, then the rows between ``low_thre`` and ``high_thre`` against the confirmed tracks that were seen in the last frame
(ByteTrack's two stages with its published thresholds).  A matched track follows its detection through a constant-gain filter on
the centre, its velocity and the 24 radii; an unmatched one coasts for ``max_age`` frames; unmatched high rows with score >=
``new_thre`` start tentative tracks that are confirmed after ``min_hits`` matches.  A frame is two launches and - through
``update_padded`` - no host synchronisation.  No tracking quality (MOTA / IDF1) has been measured for these defaults.
"""
import collections
import json
import math
import os

import numpy as np
import torch

from . import _lib
from ._lib import call, ptr, stream_ptr

__all__ = ["Tracker24", "Tracks", "check_args", "draw_tracks", "write_tracks", "track_rows", "MAX_TRACKS", "MAX_DETS"]

MAX_TRACKS = 1024                   # ep24_track_step: one slot per thread of its workgroup
MAX_DETS = 4096                     # and its row tables in LDS
ID_COLORS = 1000                    # draw_tracks: colour and label of a track are those of "class" id % 1000

Tracks = collections.namedtuple("Tracks", ["dets", "ids", "hits"])


def _number(name, v):
    if isinstance(v, bool) or not isinstance(v, (int, float)):
        raise ValueError("%s must be a number, got %r" % (name, v))
    return float(v)


def _integer(name, v, lo):
    if isinstance(v, bool) or not isinstance(v, int):
        raise ValueError("%s must be an integer, got %r" % (name, v))
    if v < lo:
        raise ValueError("%s must be at least %d, got %r" % (name, lo, v))
    return int(v)


def check_args(streams=1, max_tracks=256, max_dets=256, high_thre=0.5, low_thre=0.1, new_thre=0.6, match_thre=0.2, match_low_thre=0.5,
               max_age=30, min_hits=3, alpha=0.5, beta=0.25, gamma=0.5):
    """The argument rules of ``Tracker24`` (those of ``ep24_track_cost`` / ``ep24_track_step``), checked before anything touches
    the GPU."""
    _integer("streams", streams, 1)
    if _integer("max_tracks", max_tracks, 1) % 64 or max_tracks > MAX_TRACKS:
        raise ValueError("max_tracks must be a multiple of 64 in 64..%d, got %r" % (MAX_TRACKS, max_tracks))
    if _integer("max_dets", max_dets, 1) > MAX_DETS:
        raise ValueError("max_dets must lie in 1..%d, got %r" % (MAX_DETS, max_dets))
    for name, v in (("high_thre", high_thre), ("low_thre", low_thre), ("new_thre", new_thre), ("match_thre", match_thre),
                    ("match_low_thre", match_low_thre)):
        if not math.isfinite(_number(name, v)):
            raise ValueError("%s must be finite, got %r" % (name, v))
    for name, v in (("match_thre", match_thre), ("match_low_thre", match_low_thre)):
        if v < 0:
            raise ValueError("%s must be at least 0 (the box pre-test of the IoU matrix is exact from there), got %r" % (name, v))
    for name, v in (("alpha", alpha), ("beta", beta), ("gamma", gamma)):
        if not 0.0 <= _number(name, v) <= 1.0:
            raise ValueError("%s must lie in [0, 1], got %r" % (name, v))
    _integer("max_age", max_age, 0)
    _integer("min_hits", min_hits, 1)


class Tracker24:
    """``Tracker24(streams=S)``: S sequences tracked side by side, ``max_tracks`` slots (a multiple of 64 up to 1024) and at most
    ``max_dets`` (up to 4096) detection rows per frame each.  The thresholds are ByteTrack's published defaults (track 0.5, new =
    track + 0.1, first association IoU > 1 - 0.8, second > 0.5, buffer 30 frames); the gains are dyadic by choice."""

    def __init__(self, streams=1, max_tracks=256, max_dets=256, high_thre=0.5, low_thre=0.1, new_thre=0.6, match_thre=0.2,
                 match_low_thre=0.5, max_age=30, min_hits=3, alpha=0.5, beta=0.25, gamma=0.5, class_agnostic=False, device="cuda"):
        check_args(streams, max_tracks, max_dets, high_thre, low_thre, new_thre, match_thre, match_low_thre, max_age, min_hits, alpha,
                   beta, gamma)
        self.S, self.T, self.N = int(streams), int(max_tracks), int(max_dets)
        self.high_thre, self.low_thre, self.new_thre = float(high_thre), float(low_thre), float(new_thre)
        self.match_thre, self.match_low_thre = float(match_thre), float(match_low_thre)
        self.max_age, self.min_hits = int(max_age), int(min_hits)
        self.alpha, self.beta, self.gamma = float(alpha), float(beta), float(gamma)
        self.class_agnostic = bool(class_agnostic)
        _lib.require_gpu()
        dev = torch.device(device)
        if dev.type != "cuda":
            raise _lib.Ep24Error("ep24: Tracker24 lives on the GPU (no CPU fallback on the product path), got device %r" % (device,))
        self.device = torch.device("cuda", dev.index if dev.index is not None else torch.cuda.current_device())
        from .evaluate import ray_cos_sin
        S, T, N, f = self.S, self.T, self.N, dict(device=self.device)
        self.trk_f = torch.zeros(S, T, 32, dtype=torch.float32, **f)
        self.trk_i = torch.zeros(S, T, 8, dtype=torch.int32, **f)
        self.hdr = torch.zeros(S, 4, dtype=torch.int32, **f)
        self.hdr[:, 0] = 1
        self.cs = torch.from_numpy(ray_cos_sin()).to(self.device)
        self.iou = torch.empty(S, T, N, dtype=torch.float64, **f)               # scratch and outputs: written whole by every frame
        self.dscore = torch.empty(S, N, dtype=torch.float32, **f)
        self.det_track = torch.empty(S, N, dtype=torch.int32, **f)
        self.out_f = torch.empty(S, T, 29, dtype=torch.float32, **f)
        self.out_i = torch.empty(S, T, 4, dtype=torch.int32, **f)
        self.out_count = torch.empty(S, dtype=torch.int32, **f)
        self._pad = {}

    # ---- the device path ---------------------------------------------------------------------------------
    def _check_padded(self, det, count):
        if not isinstance(det, torch.Tensor) or det.dim() != 3 or det.shape[0] != self.S or det.shape[1] != self.N or det.shape[2] < 29:
            raise IndexError("update_padded: det must be [%d, %d, >= 29], got %s"
                             % (self.S, self.N, tuple(det.shape) if isinstance(det, torch.Tensor) else type(det).__name__))
        if det.dtype != torch.float32 or not det.is_contiguous():
            raise ValueError("update_padded: det must be a contiguous float32 tensor, got %s" % det.dtype)
        if not isinstance(count, torch.Tensor) or tuple(count.shape) != (self.S,) or count.dtype != torch.int32:
            raise IndexError("update_padded: count must be int32 [%d], got %s"
                             % (self.S, (tuple(count.shape), count.dtype) if isinstance(count, torch.Tensor) else type(count).__name__))
        if det.device != self.device or count.device != self.device:
            raise _lib.Ep24Error("ep24: update_padded takes tensors on the tracker's device %s (no CPU fallback)" % self.device)

    def update_padded(self, det, count):
        """``det [S, N, ncols]`` float32 (``N = max_dets``, ``ncols >= 29``), ``count [S]`` int32, both on the tracker's device:
        one frame.  -> the tracker's own device tensors ``(out_f [S, T, 29], out_i [S, T, 4], out_count [S], det_track [S, N])``,
        overwritten by the next frame.  Two launches, no host synchronisation: it can be captured."""
        self._check_padded(det, count)
        S, T, N, ncols, s = self.S, self.T, self.N, int(det.shape[2]), stream_ptr()
        call("track_cost", ptr(det), ncols, ptr(count), ptr(self.trk_f), ptr(self.trk_i), S, T, N, self.low_thre,
             1 if self.class_agnostic else 0, ptr(self.cs), ptr(self.iou), ptr(self.dscore), s)
        call("track_step", ptr(det), ncols, ptr(self.iou), ptr(self.dscore), ptr(self.trk_f), ptr(self.trk_i), ptr(self.hdr), S, T, N,
             self.high_thre, self.new_thre, self.match_thre, self.match_low_thre, self.alpha, self.beta, self.gamma, self.max_age,
             self.min_hits, ptr(self.det_track), ptr(self.out_f), ptr(self.out_i), ptr(self.out_count), s)
        return self.out_f, self.out_i, self.out_count, self.det_track

    def update(self, dets):
        """``dets``: ``postprocess``'s list of S entries, each ``None`` or ``[n, >= 29]`` with n <= ``max_dets``.  -> a list of S
        ``Tracks(dets [m, 29], ids [m] int32, hits [m] int32)``: the confirmed tracks seen in this frame, in slot order - the
        filtered shape in columns 0..25, the matched row's obj_conf, class_conf and class after it.  The read of the S counts is
        the only host synchronisation."""
        if not isinstance(dets, (list, tuple)) or len(dets) != self.S:
            raise IndexError("update: dets must be a list of %d entries (None or [n, >= 29]), got %s"
                             % (self.S, len(dets) if isinstance(dets, (list, tuple)) else type(dets).__name__))
        ncols = 29
        for d in dets:
            if d is None:
                continue
            if not isinstance(d, torch.Tensor) or d.dim() != 2 or d.shape[1] < 29:
                raise IndexError("update: an entry must be None or [n, >= 29], got %s"
                                 % (tuple(d.shape) if isinstance(d, torch.Tensor) else type(d).__name__,))
            if d.shape[0] > self.N:
                raise ValueError("update: %d rows in one stream, max_dets is %d" % (d.shape[0], self.N))
            if not d.is_cuda:
                raise _lib.Ep24Error("ep24: update takes GPU tensors (no CPU fallback on the product path)")
            ncols = max(ncols, int(d.shape[1]))
        pad = self._pad.get(ncols)
        if pad is None:
            pad = self._pad[ncols] = (torch.zeros(self.S, self.N, ncols, dtype=torch.float32, device=self.device),
                                      torch.zeros(self.S, dtype=torch.int32, device=self.device))
        det, count = pad
        ns = [0 if d is None else int(d.shape[0]) for d in dets]
        for b, d in enumerate(dets):
            if ns[b]:
                det[b, :ns[b], :d.shape[1]] = d.detach().float()
        count.copy_(torch.tensor(ns, dtype=torch.int32), non_blocking=False)
        out_f, out_i, out_count, _ = self.update_padded(det, count)
        res = []
        for b, m in enumerate(out_count.tolist()):
            res.append(Tracks(out_f[b, :m].clone(), out_i[b, :m, 0].clone(), out_i[b, :m, 2].clone()))
        return res

    # ---- state -------------------------------------------------------------------------------------------
    def reset(self, streams=None):
        """Forget every track of the given streams (an index or a list of them; ``None``: all); their ids start at 1 again."""
        idx = list(range(self.S)) if streams is None else ([streams] if isinstance(streams, int) else list(streams))
        for b in idx:
            if isinstance(b, bool) or not isinstance(b, int) or not 0 <= b < self.S:
                raise IndexError("reset: stream %r of %d" % (b, self.S))
        for b in idx:
            self.trk_f[b].zero_()
            self.trk_i[b].zero_()
            self.hdr[b].zero_()
            self.hdr[b, 0] = 1

    def state_dict(self):
        """The three tables on the host: everything a sequence needs to go on."""
        return {"trk_f": self.trk_f.cpu().clone(), "trk_i": self.trk_i.cpu().clone(), "hdr": self.hdr.cpu().clone()}

    def load_state_dict(self, state):
        for name, ref in (("trk_f", self.trk_f), ("trk_i", self.trk_i), ("hdr", self.hdr)):
            t = state.get(name) if isinstance(state, dict) else None
            if not isinstance(t, torch.Tensor) or tuple(t.shape) != tuple(ref.shape) or t.dtype != ref.dtype:
                raise IndexError("load_state_dict: %s must be %s %s, got %s" % (
                    name, ref.dtype, tuple(ref.shape), (t.dtype, tuple(t.shape)) if isinstance(t, torch.Tensor) else type(t).__name__))
        for name, ref in (("trk_f", self.trk_f), ("trk_i", self.trk_i), ("hdr", self.hdr)):
            ref.copy_(state[name])

    def table(self, stream=0):
        """The live slots of a stream, lost ones included: a dict of host arrays ``slot``, ``id``, ``cls``, ``status``, ``hits``,
        ``age``, ``birth``, ``row`` (int32 ``[m]``), ``shape`` ``[m, 26]``, ``velocity`` ``[m, 2]``, ``score`` ``[m]``, and the
        stream's ``next_id``, ``frame``, ``dropped``, ``live``.  For tests and tools: it synchronises."""
        if isinstance(stream, bool) or not isinstance(stream, int) or not 0 <= stream < self.S:
            raise IndexError("table: stream %r of %d" % (stream, self.S))
        ti, tf, h = self.trk_i[stream].cpu().numpy(), self.trk_f[stream].cpu().numpy(), self.hdr[stream].cpu().numpy()
        slot = np.nonzero(ti[:, 0])[0].astype(np.int32)
        out = {"slot": slot, "shape": tf[slot, :26], "velocity": tf[slot, 26:28], "score": tf[slot, 28]}
        for k, name in enumerate(("id", "cls", "status", "hits", "age", "birth", "row")):
            out[name] = ti[slot, k]
        out.update(next_id=int(h[0]), frame=int(h[1]), dropped=int(h[2]), live=int(h[3]))
        return out


# ---- drawing and files ---------------------------------------------------------------------------------------
def id_rows(tracks):
    """``Tracks`` -> its ``[m, 29]`` rows with the class column replaced by ``id % 1000``: what ``draw_tracks`` draws."""
    rows = tracks.dets.detach().clone()
    rows[:, 28] = (tracks.ids.to(rows.device) % ID_COLORS).to(rows.dtype)
    return rows


def draw_tracks(image, tracks, ratio=1.0, **kw):
    """``ep24.draw.draw_detections`` of a stream's ``Tracks`` with the id in the place of the class: the class column is replaced
    by ``id % 1000``, ``num_classes=1000`` and ``colors=palette(1000)``, so a track keeps its colour and its label is its id.
    ``kw`` goes on to ``draw_detections`` (``conf``, ``fill_alpha``, ``font_scale``, ``show_scores``, ``out``)."""
    from . import draw
    if not isinstance(tracks, Tracks):
        raise IndexError("draw_tracks: tracks must be a Tracks tuple of Tracker24.update, got %s" % type(tracks).__name__)
    for name in ("num_classes", "colors", "class_names"):
        if name in kw:
            raise ValueError("draw_tracks: %s is fixed (the label of a track is its id)" % name)
    rows = id_rows(tracks) if tracks.dets.shape[0] else None
    return draw.draw_detections(image, rows, ratio=ratio, num_classes=ID_COLORS, colors=draw.palette(ID_COLORS), **kw)


def track_rows(tracks, ratio=1.0):
    """One frame's ``Tracks`` -> a list of (id, x, y, w, h, score, class, shape26) in original-image pixels: the bounding
    rectangle of the 24 vertices c + r_k * (cos, sin)(15 deg * k) of the shape divided by ``ratio``, in float64 on the host."""
    d = np.asarray(tracks.dets.detach().cpu().numpy() if isinstance(tracks.dets, torch.Tensor) else tracks.dets, dtype=np.float64)
    ids = np.asarray(tracks.ids.cpu().numpy() if isinstance(tracks.ids, torch.Tensor) else tracks.ids)
    if d.ndim != 2 or d.shape[1] != 29 or ids.shape != (d.shape[0],):
        raise IndexError("track_rows: Tracks with dets [m, 29] and ids [m], got %s and %s" % (d.shape, ids.shape))
    th = np.arange(24, dtype=np.float64) * (15.0 * np.pi / 180.0)
    shape = d[:, :26] / float(ratio)
    xs = shape[:, 0:1] + shape[:, 2:26] * np.cos(th)[None]
    ys = shape[:, 1:2] + shape[:, 2:26] * np.sin(th)[None]
    out = []
    for m in range(d.shape[0]):
        x0, y0 = float(xs[m].min()), float(ys[m].min())
        out.append((int(ids[m]), x0, y0, float(xs[m].max()) - x0, float(ys[m].max()) - y0, float(d[m, 26] * d[m, 27]), int(d[m, 28]),
                    [float(v) for v in shape[m]]))
    return out


def write_tracks(path, frames):
    """``frames``: a list of ``(frame_number, Tracks)`` or ``(frame_number, Tracks, ratio)``.  ``.txt``: MOTChallenge rows
    ``frame,id,x,y,w,h,score,class,-1,-1`` (the bounding rectangle of the 24 vertices in original-image pixels); ``.json``: a list
    of objects with the same fields plus ``shape``, the 26 shape numbers in original-image pixels.  Host only."""
    ext = os.path.splitext(str(path))[1].lower()
    if ext not in (".txt", ".json"):
        raise ValueError("write_tracks: %s: the name must end in .txt (MOTChallenge) or .json" % (path,))
    rows = []
    for entry in frames:
        if not isinstance(entry, (list, tuple)) or len(entry) not in (2, 3):
            raise IndexError("write_tracks: an entry is (frame, Tracks) or (frame, Tracks, ratio)")
        ratio = float(entry[2]) if len(entry) == 3 else 1.0
        if not (0.0 < ratio < float("inf")):
            raise ValueError("write_tracks: ratio must be a positive finite number, got %r" % (entry[2],))
        for r in track_rows(entry[1], ratio):
            rows.append((int(entry[0]),) + r)
    with open(path, "w") as fh:
        if ext == ".txt":
            for fr, tid, x, y, w, h, sc, c, _ in rows:
                fh.write("%d,%d,%.2f,%.2f,%.2f,%.2f,%.6f,%d,-1,-1\n" % (fr, tid, x, y, w, h, sc, c))
        else:
            json.dump([{"frame": fr, "id": tid, "x": x, "y": y, "w": w, "h": h, "score": sc, "class": c, "shape": shape}
                       for fr, tid, x, y, w, h, sc, c, shape in rows], fh, indent=1)
    return len(rows)
