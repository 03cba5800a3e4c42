"""Tracking on the GPU (csrc/track.hip through the C ABI and through ``ep24.track.Tracker24``) against the numpy oracle
(tests/track_oracle.py) on the seeded scenes of tests/track_scenes.py, whose decisions all stay 1e-6 away from their thresholds
and from each other (asserted in tests/test_track_oracle.py): the integer tables equal the oracle's, the float tables bit for bit.
The oracle's replay of a scene is computed once (``track_scenes.replay``) and shared."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import track_scenes as S  # noqa: E402
from ep24 import _lib, draw, evaluate as E, track  # noqa: E402
from ep24._lib import ptr  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD = 64                                                     # words on either side of every buffer
DEAD = -559038737                                              # 0xDEADBEEF as int32
FILLS = {torch.int32: DEAD, torch.float32: float("nan"), torch.float64: float("nan")}


class _Guarded:
    """A buffer of n elements between two guard zones holding the fill pattern."""

    def __init__(self, n, dtype, zero=False):
        self.fill = FILLS[dtype]
        self.whole = torch.full((n + 2 * GUARD,), self.fill, dtype=dtype, device=DEV)
        self.t = self.whole[GUARD:GUARD + n]
        if zero:
            self.t.zero_()

    def refill(self):
        self.t.fill_(self.fill)

    def guards_intact(self):
        g = torch.cat([self.whole[:GUARD], self.whole[-GUARD:]]).cpu().numpy()
        return bool(np.isnan(g).all()) if g.dtype.kind == "f" else bool((g == DEAD).all())


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32 if a.dtype.itemsize == 4 else np.uint64)


@functools.lru_cache(maxsize=None)
def _abi_replay(name, prefill):
    """The scene through ep24_track_cost / ep24_track_step on buffers of the test's own, every one between guard words; with
    ``prefill`` every scratch and output buffer is filled with NaN / 0xDEADBEEF before every frame, without it with zeros.
    -> per frame a dict of host copies, and whether every guard word survived."""
    sc = S.scene(name)
    kw = dict(high_thre=0.5, low_thre=0.1, new_thre=0.6, match_thre=0.2, match_low_thre=0.5, max_age=30, min_hits=3, alpha=0.5,
              beta=0.25, gamma=0.5, class_agnostic=False)
    kw.update(sc.kw)
    St, T, N = kw["streams"], kw["max_tracks"], kw["max_dets"]
    B = dict(trk_f=_Guarded(St * T * 32, torch.float32, True), trk_i=_Guarded(St * T * 8, torch.int32, True),
             hdr=_Guarded(St * 4, torch.int32, True), iou=_Guarded(St * T * N, torch.float64), dscore=_Guarded(St * N, torch.float32),
             det_track=_Guarded(St * N, torch.int32), out_f=_Guarded(St * T * 29, torch.float32),
             out_i=_Guarded(St * T * 4, torch.int32), out_count=_Guarded(St, torch.int32))
    B["hdr"].t.view(St, 4)[:, 0] = 1
    cs = torch.from_numpy(E.ray_cos_sin()).to(DEV)
    shapes = dict(trk_f=(St, T, 32), trk_i=(St, T, 8), hdr=(St, 4), iou=(St, T, N), dscore=(St, N), det_track=(St, N),
                  out_f=(St, T, 29), out_i=(St, T, 4), out_count=(St,))
    s = _lib.stream_ptr()
    frames = []
    for det, count in sc.frames:
        d, c = torch.from_numpy(det).to(DEV), torch.from_numpy(count).to(DEV)
        for k in ("iou", "dscore", "det_track", "out_f", "out_i", "out_count"):
            if prefill:
                B[k].refill()
            else:
                B[k].t.zero_()
        _lib.call("track_cost", ptr(d), det.shape[2], ptr(c), ptr(B["trk_f"].t), ptr(B["trk_i"].t), St, T, N, kw["low_thre"],
                  1 if kw["class_agnostic"] else 0, ptr(cs), ptr(B["iou"].t), ptr(B["dscore"].t), s)
        _lib.call("track_step", ptr(d), det.shape[2], ptr(B["iou"].t), ptr(B["dscore"].t), ptr(B["trk_f"].t), ptr(B["trk_i"].t),
                  ptr(B["hdr"].t), St, T, N, kw["high_thre"], kw["new_thre"], kw["match_thre"], kw["match_low_thre"], kw["alpha"],
                  kw["beta"], kw["gamma"], kw["max_age"], kw["min_hits"], ptr(B["det_track"].t), ptr(B["out_f"].t), ptr(B["out_i"].t),
                  ptr(B["out_count"].t), s)
        frames.append({k: B[k].t.cpu().numpy().reshape(shapes[k]).copy() for k in shapes})
    return frames, all(b.guards_intact() for b in B.values())


INT_KEYS = ("trk_i", "hdr", "out_i", "out_count", "det_track")
BIT_KEYS = ("trk_f", "out_f", "dscore")


def _same(got, want, where):
    for k in INT_KEYS:
        assert np.array_equal(got[k], want[k]), (where, k)
    for k in BIT_KEYS:
        assert np.array_equal(_bits(got[k]), _bits(want[k])), (where, k)


# ---- 1. ep24_track_cost ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["edges", "chain", "nan", "classes", "classes_agnostic"])
def test_cost_matrix_equals_the_oracle(name):
    """Every frame's matrix: within 1e-9 of the oracle's (tests/test_gpu_poly24.py's bound for poly24_iou), the entries the
    contract puts at 0 exactly 0, NaN where the oracle has NaN."""
    frames, _ = _abi_replay(name, True)
    _, want = S.replay(name)
    seen = 0
    for f, (g, w) in enumerate(zip(frames, want)):
        gi, wi = g["iou"], w["iou"]
        assert np.array_equal(np.isnan(gi), np.isnan(wi)), f
        assert np.array_equal(gi == 0.0, wi == 0.0), f
        ok = ~np.isnan(wi)
        err = float(np.abs(gi[ok] - wi[ok]).max())
        seen += int((wi[ok] > 0).sum())
        assert err <= 1e-9, (f, err)
    assert seen > 0


# ---- 2. scene replay --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", S.NAMES)
def test_scene_replay_equals_the_oracle(name):
    frames, guards = _abi_replay(name, True)
    _, want = S.replay(name)
    assert len(frames) == len(want)
    for f, (g, w) in enumerate(zip(frames, want)):
        _same(g, w, (name, f))
    assert guards


# ---- 3. buffer hygiene ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["edges", "nan"])
def test_prefilled_buffers_change_nothing_and_guards_survive(name):
    a, ga = _abi_replay(name, True)
    b, gb = _abi_replay(name, False)
    assert ga and gb
    for f, (x, y) in enumerate(zip(a, b)):
        for k in x:
            assert np.array_equal(_bits(x[k]), _bits(y[k])), (f, k)


# ---- 4. the Python surface ----------------------------------------------------------------------------------------
def _tracker(name, **over):
    kw = dict(S.scene(name).kw)
    kw.update(over)
    return track.Tracker24(device=DEV, **kw)


def _snap(trk, outs=None):
    d = {k: getattr(trk, k).cpu().numpy().copy() for k in ("trk_f", "trk_i", "hdr")}
    if outs is not None:
        for k, t in zip(("out_f", "out_i", "out_count", "det_track"), outs):
            d[k] = t.cpu().numpy().copy()
    return d


def _run_padded(trk, frames, streams=None):
    out = []
    for det, count in frames:
        if streams is not None:
            det, count = det[streams], count[streams]
        outs = trk.update_padded(torch.from_numpy(np.ascontiguousarray(det)).to(DEV), torch.from_numpy(np.ascontiguousarray(count)).to(DEV))
        out.append(_snap(trk, outs))
    return out


def test_streams_are_independent():
    sc = S.scene("edges")
    both = _run_padded(_tracker("edges"), sc.frames)
    for s in range(3):
        one = _run_padded(_tracker("edges", streams=1), sc.frames, slice(s, s + 1))
        for f, (a, b) in enumerate(zip(both, one)):
            for k in a:
                assert np.array_equal(_bits(a[k][s:s + 1]), _bits(b[k])), (s, f, k)


def test_second_run_from_reset_is_bit_identical():
    sc = S.scene("crossing")
    trk = _tracker("crossing")
    first = _run_padded(trk, sc.frames)
    trk.reset()
    assert int(trk.trk_i.abs().sum()) == 0 and trk.hdr.cpu().tolist() == [[1, 0, 0, 0]]
    second = _run_padded(trk, sc.frames)
    for f, (a, b) in enumerate(zip(first, second)):
        for k in a:
            assert np.array_equal(_bits(a[k]), _bits(b[k])), (f, k)
    _, want = S.replay("crossing")
    for k in INT_KEYS:
        assert np.array_equal(first[-1][k], want[-1][k]), k


def test_update_agrees_with_update_padded_and_state_round_trip():
    sc = S.scene("occlusion")
    _, want = S.replay("occlusion")
    a, b = _tracker("occlusion"), _tracker("occlusion")
    half = len(sc.frames) // 2
    for f, (det, count) in enumerate(sc.frames):
        if f == half:                                             # b goes on in a fresh tracker from a's saved tables
            state = a.state_dict()
            assert set(state) == {"trk_f", "trk_i", "hdr"} and not state["trk_f"].is_cuda
            b = _tracker("occlusion")
            b.load_state_dict(state)
        outs = a.update_padded(torch.from_numpy(det).to(DEV), torch.from_numpy(count).to(DEV))
        pa = _snap(a, outs)
        n = int(count[0])
        got = b.update([torch.from_numpy(det[0, :n]).to(DEV) if n else None])
        pb = _snap(b)
        for k in ("trk_f", "trk_i", "hdr"):
            assert np.array_equal(_bits(pa[k]), _bits(pb[k])), (f, k)
        m = int(pa["out_count"][0])
        assert len(got) == 1 and isinstance(got[0], track.Tracks)
        assert np.array_equal(_bits(got[0].dets.cpu().numpy()), _bits(pa["out_f"][0, :m])), f
        assert np.array_equal(got[0].ids.cpu().numpy(), pa["out_i"][0, :m, 0]) and got[0].ids.dtype == torch.int32
        assert np.array_equal(got[0].hits.cpu().numpy(), pa["out_i"][0, :m, 2])
        assert np.array_equal(pa["trk_i"], want[f]["trk_i"]), f
    tab = a.table(0)
    live = np.nonzero(want[-1]["trk_i"][0, :, 0])[0]
    assert np.array_equal(tab["slot"], live) and np.array_equal(tab["id"], want[-1]["trk_i"][0, live, 0])
    assert tab["next_id"] == int(want[-1]["hdr"][0, 0]) and tab["frame"] == len(sc.frames)
    with pytest.raises(ValueError):
        a.update([torch.zeros(17, 29, device=DEV)])


def test_captured_frame_replays_like_the_eager_one():
    """One frame's two launches under torch.cuda.graph - a linear graph - replayed over 6 frames through static inputs."""
    N = T = 64
    srcs = [S.scene("crossing").frames, S.scene("occlusion").frames]
    frames = []
    for f in range(6):
        det = np.zeros((2, N, 29), dtype=np.float32)
        count = np.zeros(2, dtype=np.int32)
        for s in range(2):
            d, c = srcs[s][f + 4]
            det[s, :d.shape[1]] = d[0]
            count[s] = c[0]
        frames.append((det, count))
    eager = _run_padded(track.Tracker24(streams=2, max_tracks=T, max_dets=N, min_hits=2, device=DEV), frames)
    trk = track.Tracker24(streams=2, max_tracks=T, max_dets=N, min_hits=2, device=DEV)
    sdet, scount = torch.zeros(2, N, 29, device=DEV), torch.zeros(2, dtype=torch.int32, device=DEV)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        trk.update_padded(sdet, scount)                               # warm-up on empty input, then back to the start
    torch.cuda.current_stream().wait_stream(side)
    trk.reset()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        outs = trk.update_padded(sdet, scount)
    trk.reset()
    for f, (det, count) in enumerate(frames):
        sdet.copy_(torch.from_numpy(det))
        scount.copy_(torch.from_numpy(count))
        g.replay()
        got = _snap(trk, outs)
        for k in got:
            assert np.array_equal(_bits(got[k]), _bits(eager[f][k])), (f, k)
    assert int(eager[-1]["out_count"].sum()) > 0


def test_draw_tracks_equals_draw_detections_on_the_rewritten_rows():
    sc = S.scene("crossing")
    trk = _tracker("crossing")
    for det, count in sc.frames[:6]:
        res = trk.update([torch.from_numpy(det[0, :int(count[0])]).to(DEV)])
    tr = res[0]
    assert tr.dets.shape[0] == 2
    big = track.Tracks(tr.dets, tr.ids + 2000, tr.hits)               # ids beyond the palette wrap round
    image = torch.full((260, 320, 3), 30, dtype=torch.uint8, device=DEV)
    rows = big.dets.clone()
    rows[:, 28] = (big.ids % 1000).float()
    want = draw.draw_detections(image, rows, ratio=1.0, num_classes=1000, colors=draw.palette(1000), fill_alpha=40)
    got = track.draw_tracks(image, big, fill_alpha=40)
    assert torch.equal(got, want) and not torch.equal(got, image)
    empty = track.Tracks(tr.dets[:0], tr.ids[:0], tr.hits[:0])
    assert torch.equal(track.draw_tracks(image, empty), image)


def test_show_24p_tracks_a_folder_of_frames(tmp_path):
    """``show_24p.py --track --save-tracks`` in a fresh process, the small Exp with its initial parameters on four copies of one
    image (-b 3: the frames still reach the tracker one at a time): whatever the untrained model detects is the same in every
    frame, so the tracks born in frame 1 are confirmed in frame 2 and keep their ids."""
    import glob
    import json
    from test_gpu_show24p import _run
    in_dir, out_dir, txt = tmp_path / "frames", str(tmp_path / "shown"), str(tmp_path / "t.txt")
    in_dir.mkdir()
    img = np.random.default_rng(0).integers(0, 256, (96, 128, 3), dtype=np.uint8)
    for f in range(4):
        np.save(str(in_dir / ("f%02d.npy" % f)), img)
    log = _run("show_24p.py", "-p", str(in_dir), "-b", "3", "--conf", "1e-5", "--draw-conf", "0", "--output-dir", out_dir, "--track",
               "--track-low", "1e-5", "--track-high", "2e-5", "--track-new", "2e-5", "--track-min-hits", "2", "--save-tracks", txt)
    runs = glob.glob(os.path.join(out_dir, "*"))
    assert len(runs) == 1, (runs, log[-2000:])
    assert json.load(open(os.path.join(runs[0], "detections.json")))["track"] is True
    rows = [ln.split(",") for ln in open(txt).read().splitlines()]
    assert rows and all(len(r) == 10 and r[8:] == ["-1", "-1"] for r in rows), log[-2000:]
    per = {f: sorted(int(r[1]) for r in rows if int(r[0]) == f) for f in (1, 2, 3, 4)}
    assert per[1] == [] and per[2] and per[2] == per[3] == per[4]
    for f in range(4):
        ids = np.load(os.path.join(runs[0], "f%02d.npy.ids.npy" % f))
        dets = np.load(os.path.join(runs[0], "f%02d.npy.dets.npy" % f))
        assert sorted(ids.tolist()) == per[f + 1] and dets.shape == (len(ids), 29)
        assert np.load(os.path.join(runs[0], "f%02d.npy" % f)).shape == img.shape
