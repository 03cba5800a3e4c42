"""The host surface of ep24.track without a GPU: the ABI entries, every argument rule raised before anything touches the GPU, the
refusal without one, the new show_24p flags, and write_tracks in both formats on hand-made tracks."""
import json
import math
import os
import sys

import numpy as np
import pytest
import torch

from ep24 import _lib, track

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
Y24 = os.path.join(ROOT, "exploration-of-potential_amd", "yolox_24p")


def test_abi_entries():
    protos = _lib.parse_header()
    assert [n for _, n in protos["ep24_track_cost"][1]] == ["det", "ncols", "count", "trk_f", "trk_i", "S", "T", "N", "low_thre",
                                                           "class_agnostic", "ray_cs", "iou", "dscore", "stream"]
    assert len(protos["ep24_track_step"][1]) == 24 and protos["ep24_track_step"][1][2][0] == "const double*"
    fn = _lib.lib().fn
    assert "ep24_track_cost" in fn and "ep24_track_step" in fn


def test_library_refuses_bad_arguments():
    """The C entry points' own checks, with dummy non-null pointers: every one returns before a launch.  On a thread of its own:
    the library's last-error text is per thread."""
    import threading
    L = _lib.lib()
    cost, step = L.fn["ep24_track_cost"], L.fn["ep24_track_step"]
    p = 4096                                                      # never dereferenced: the argument checks come first
    got = {}

    def calls():
        def c(**o):
            a = dict(det=p, ncols=29, count=p, f=p, i=p, S=1, T=64, N=16, low=0.1, agn=0, cs=p, iou=p, ds=p)
            a.update(o)
            return cost(a["det"], a["ncols"], a["count"], a["f"], a["i"], a["S"], a["T"], a["N"], a["low"], a["agn"], a["cs"], a["iou"],
                        a["ds"], None)

        def s(**o):
            a = dict(det=p, ncols=29, iou=p, ds=p, f=p, i=p, h=p, S=1, T=64, N=16, high=0.5, new=0.6, m=0.2, ml=0.5, al=0.5, be=0.25,
                     ga=0.5, age=30, hits=3, dt=p, of=p, oi=p, oc=p)
            a.update(o)
            return step(a["det"], a["ncols"], a["iou"], a["ds"], a["f"], a["i"], a["h"], a["S"], a["T"], a["N"], a["high"], a["new"],
                        a["m"], a["ml"], a["al"], a["be"], a["ga"], a["age"], a["hits"], a["dt"], a["of"], a["oi"], a["oc"], None)
        E_ARG, E_UNS = c(det=None), c(T=2048)
        got["codes"] = (E_ARG, E_UNS)
        got["arg"] = [c(iou=None), c(ncols=28), c(S=0), c(N=0), c(low=math.nan), c(low=math.inf), s(oc=None), s(h=None), s(ncols=28),
                      s(high=math.nan), s(new=math.inf), s(m=-0.1), s(ml=math.nan), s(al=1.5), s(be=-0.1), s(ga=math.nan), s(hits=0),
                      s(age=-1)]
        got["uns"] = [c(T=96), c(T=1088), c(N=4097), c(S=65536), s(T=32), s(T=2048), s(N=4097)]
        got["text"] = L.last_error()
    th = threading.Thread(target=calls)
    th.start()
    th.join()
    e_arg, e_uns = got["codes"]
    assert e_arg < 0 and e_uns < 0 and e_arg != e_uns
    assert got["arg"] == [e_arg] * len(got["arg"]), got["arg"]
    assert got["uns"] == [e_uns] * len(got["uns"]), got["uns"]
    assert "track_step" in got["text"]


GOOD = dict(streams=1, max_tracks=256, max_dets=256, high_thre=0.5, low_thre=0.1, new_thre=0.6, match_thre=0.2, match_low_thre=0.5,
            max_age=30, min_hits=3, alpha=0.5, beta=0.25, gamma=0.5)
BAD = [("streams", 0), ("streams", 1.5), ("max_tracks", 0), ("max_tracks", 100), ("max_tracks", 1088), ("max_tracks", True),
       ("max_dets", 0), ("max_dets", 4097), ("high_thre", math.nan), ("low_thre", math.inf), ("new_thre", "0.6"), ("match_thre", -0.1),
       ("match_thre", math.nan), ("match_low_thre", -1), ("max_age", -1), ("max_age", 1.0), ("min_hits", 0), ("alpha", 1.5),
       ("beta", -0.01), ("gamma", math.nan), ("gamma", None)]


@pytest.mark.parametrize("name,value", BAD)
def test_argument_rules_come_before_the_gpu(name, value):
    track.check_args(**GOOD)
    kw = dict(GOOD)
    kw[name] = value
    with pytest.raises(ValueError):
        track.Tracker24(**kw)                                    # a ValueError, not the Ep24Error of a machine without a GPU


def test_defaults_are_the_published_ones():
    import inspect
    d = {k: v.default for k, v in inspect.signature(track.Tracker24.__init__).parameters.items() if k != "self"}
    assert d == dict(GOOD, class_agnostic=False, device="cuda")


def test_refusal_without_a_gpu():
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    with pytest.raises(_lib.Ep24Error):
        track.Tracker24()
    tr = track.Tracks(torch.zeros(1, 29), torch.ones(1, dtype=torch.int32), torch.ones(1, dtype=torch.int32))
    with pytest.raises(_lib.Ep24Error):
        track.draw_tracks(torch.zeros(8, 8, 3, dtype=torch.uint8), tr)
    with pytest.raises(IndexError):                              # shape rules first
        track.draw_tracks(torch.zeros(8, 8, dtype=torch.uint8), tr)
    with pytest.raises(ValueError):
        track.draw_tracks(torch.zeros(8, 8, 3, dtype=torch.uint8), tr, num_classes=3)
    with pytest.raises(IndexError):
        track.draw_tracks(torch.zeros(8, 8, 3, dtype=torch.uint8), tr.dets)


def _hand_made():
    sq = 10.0 / np.maximum(np.abs(np.cos(np.arange(24) * np.pi / 12)), np.abs(np.sin(np.arange(24) * np.pi / 12)))
    a = np.concatenate([[100.0, 60.0], np.full(24, 20.0), [0.8, 0.5, 3.0]]).astype(np.float32)      # a circle of radius 20
    b = np.concatenate([[40.0, 30.0], sq, [1.0, 0.25, 7.0]]).astype(np.float32)                      # the square of half side 10
    t1 = track.Tracks(torch.from_numpy(np.stack([a, b])), torch.tensor([5, 1002], dtype=torch.int32), torch.tensor([3, 9], dtype=torch.int32))
    t2 = track.Tracks(torch.from_numpy(a[None]), torch.tensor([5], dtype=torch.int32), torch.tensor([4], dtype=torch.int32))
    empty = track.Tracks(torch.zeros(0, 29), torch.zeros(0, dtype=torch.int32), torch.zeros(0, dtype=torch.int32))
    return [(1, t1), (2, empty), (3, t2, 0.5)]


def test_write_tracks_txt(tmp_path):
    path = str(tmp_path / "t.txt")
    assert track.write_tracks(path, _hand_made()) == 3
    lines = open(path).read().splitlines()
    assert lines[0] == "1,5,80.00,40.00,40.00,40.00,0.400000,3,-1,-1"
    assert lines[1] == "1,1002,30.00,20.00,20.00,20.00,0.250000,7,-1,-1"
    assert lines[2] == "3,5,160.00,80.00,80.00,80.00,0.400000,3,-1,-1"          # ratio 0.5: original-image pixels
    assert len(lines) == 3


def test_write_tracks_json(tmp_path):
    path = str(tmp_path / "t.json")
    assert track.write_tracks(path, _hand_made()) == 3
    rows = json.load(open(path))
    assert [r["frame"] for r in rows] == [1, 1, 3] and [r["id"] for r in rows] == [5, 1002, 5]
    assert set(rows[0]) == {"frame", "id", "x", "y", "w", "h", "score", "class", "shape"}
    assert len(rows[2]["shape"]) == 26 and rows[2]["shape"][:3] == [200.0, 120.0, 40.0]
    assert abs(rows[1]["x"] - 30.0) < 1e-5 and abs(rows[1]["w"] - 20.0) < 1e-5 and rows[1]["class"] == 7
    with pytest.raises(ValueError):
        track.write_tracks(str(tmp_path / "t.csv"), _hand_made())
    with pytest.raises(IndexError):
        track.write_tracks(path, [(1,)])
    with pytest.raises(ValueError):
        track.write_tracks(path, [(1, _hand_made()[0][1], 0.0)])


@pytest.fixture
def y24():
    sys.path.insert(0, Y24)
    try:
        yield
    finally:
        sys.path.remove(Y24)


def test_show_flags(y24, capsys):
    import importlib
    mod = importlib.import_module("show_24p")
    parse = mod.make_parser().parse_args
    d = parse([])
    assert (d.track, d.track_high, d.track_low, d.track_new, d.track_match, d.track_max_age, d.track_min_hits, d.save_tracks) == \
        (False, 0.5, 0.1, None, 0.2, 30, 3, None)
    a = parse(["--track"])
    assert a.track and abs(a.track_new - 0.6) < 1e-12 and a.nms_iou == "rect"
    a = parse(["--track", "--track-high", "0.4", "--track-low", "0.05", "--track-new", "0.7", "--track-match", "0.3", "--track-max-age",
               "10", "--track-min-hits", "1", "--save-tracks", "out/t.json", "--tta", "--vote", "0.6", "-b", "8"])
    assert (a.track_high, a.track_low, a.track_new, a.track_match, a.track_max_age, a.track_min_hits) == (0.4, 0.05, 0.7, 0.3, 10, 1)
    assert a.save_tracks == "out/t.json" and a.tta and a.nms_iou == "poly24" and a.vote == 0.6 and a.batch_size == 8
    assert parse(["--track", "--nms-iou", "poly24"]).nms_iou == "poly24"
    for bad in (["--save-tracks", "t.txt"], ["--track", "--save-tracks", "t.csv"], ["--track", "--track-match", "-0.5"],
                ["--track", "--track-min-hits", "0"], ["--track", "--track-max-age", "-1"], ["--track", "--track-high", "nan"]):
        with pytest.raises(SystemExit):
            parse(bad)
    capsys.readouterr()
