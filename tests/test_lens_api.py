"""``ep24.lens`` on the host: the model's validation and constructors, the trainer's flag, and that nothing runs without a GPU."""
import json
import math
import os
import sys

import numpy as np
import pytest

import lens_oracle as L
from ep24 import _lib, lens
from ep24.lens import LensModel

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
Y24 = os.path.join(ROOT, "exploration-of-potential_amd", "yolox_24p")
K = (-0.02, 0.004, -0.001, 0.0002)
PIN, FISH = (60.0, 60.0, 63.5, 47.5), (52.0, 52.0, 47.5, 39.5)


def test_model_table_and_host_arithmetic_match_the_oracle():
    m = LensModel(PIN, FISH, K, 170.0)
    o = L.model(PIN, FISH, K, 170.0)
    t = m.table()
    assert t.dtype == np.float64 and t.shape == (lens.MODEL_D,)
    assert tuple(t[:4]) == PIN and tuple(t[4:8]) == FISH and tuple(t[8:12]) == K
    assert t[12] == o["theta_max"] == math.radians(85.0) and t[13] == L.thetad(o["theta_max"], K)
    th = np.linspace(0, m.theta_max, 333)
    assert np.array_equal(m.thetad(th), L.thetad(th, K))
    assert np.abs(m.newton(m.thetad(th)) - L.invert(L.thetad(th, K), o)).max() <= 1e-14
    # the derivative the Newton step divides by is the derivative of thetad
    num = (m.thetad(th + 1e-6) - m.thetad(th - 1e-6)) / 2e-6
    assert np.abs(num - m.dthetad(th)).max() <= 1e-8


def test_bad_models_are_refused():
    with pytest.raises(ValueError, match="not increasing"):
        LensModel(PIN, FISH, (-0.5, 0.0, 0.0, 0.0), 170.0)                    # 1 - 1.5 th^2 turns negative at 0.82 rad
    LensModel(PIN, FISH, (-0.5, 0.0, 0.0, 0.0), 60.0)                         # the same lens is fine within 30 degrees
    for fov in (180.0, 200.0, 0.0, -5.0, float("nan")):
        with pytest.raises(ValueError, match="fov_deg"):
            LensModel(PIN, FISH, K, fov)
    with pytest.raises(ValueError, match="focal"):
        LensModel((0.0, 60.0, 1.0, 1.0), FISH)
    with pytest.raises(ValueError, match="four finite"):
        LensModel(PIN, (1.0, 2.0, 3.0))
    with pytest.raises(ValueError, match="four finite"):
        LensModel(PIN, FISH, (0.0, float("inf"), 0.0, 0.0))
    with pytest.raises(ValueError, match="Newton"):
        # increasing, but nearly flat at the rim: twelve steps from theta = thetad do not arrive
        LensModel(PIN, FISH, (-0.33333, 0.0, 0.0, 0.0), 2 * math.degrees(0.99999))


def test_constructors_round_trip(tmp_path):
    Kmat = [[52.0, 0.0, 47.5], [0.0, 51.0, 39.5], [0.0, 0.0, 1.0]]
    m = LensModel.from_opencv(Kmat, K, pin=PIN, fov_deg=160.0, size=(80, 96))
    assert m.fish == (52.0, 51.0, 47.5, 39.5) and m.pin == PIN and m.k == K and m.fov_deg == 160.0 and m.size == (80, 96)
    assert LensModel.from_opencv(Kmat, K).pin == m.fish
    with pytest.raises(ValueError, match="skew"):
        LensModel.from_opencv([[52.0, 0.1, 47.5], [0.0, 51.0, 39.5], [0.0, 0.0, 1.0]], K)
    with pytest.raises(ValueError, match="3x3"):
        LensModel.from_opencv(Kmat, K + (0.0,))
    path = str(tmp_path / "lens.json")
    m.to_json(path)
    assert set(json.load(open(path))) == {"K", "D", "pinhole", "fov_deg", "size"}
    back = LensModel.from_json(path)
    assert np.array_equal(back.table(), m.table()) and back.size == m.size
    json.dump({"K": Kmat, "D": list(K), "kernel": "x"}, open(path, "w"))
    with pytest.raises(ValueError, match="kernel"):
        LensModel.from_json(path)
    # scaled: focal * s, principal point (c + 0.5) * s - 0.5; there and back is the identity up to rounding
    s = m.scaled(2.0, 0.5)
    assert s.fish == (104.0, 25.5, 95.5, 19.5) and s.pin == (120.0, 30.0, 127.5, 23.5) and s.size == (40, 192) and s.k == m.k
    assert np.abs(s.scaled(0.5, 2.0).table() - m.table()).max() <= 1e-12
    only_pin = m.scaled(2.0, pin=True, fish=False)
    assert only_pin.fish == m.fish and only_pin.pin == (120.0, 120.0, 127.5, 95.5) and only_pin.size == m.size
    # the same point of the scene: a pixel of the frame resized by s maps to the resized position
    o, os_ = L.model(m.pin, m.fish, m.k, 160.0), L.model(s.pin, s.fish, s.k, 160.0)
    X, Y, _ = L.to_fisheye(np.array([20.0]), np.array([30.0]), o)
    Xs, Ys, _ = L.to_fisheye(np.array([(20.0 + 0.5) * 2.0 - 0.5]), np.array([(30.0 + 0.5) * 0.5 - 0.5]), os_)
    assert abs(Xs[0] - ((X[0] + 0.5) * 2.0 - 0.5)) <= 1e-9 and abs(Ys[0] - ((Y[0] + 0.5) * 0.5 - 0.5)) <= 1e-9
    e = LensModel.equidistant((96, 128), (80, 80), 120.0)
    assert e.k == (0.0,) * 4 and e.size == (80, 80) and e.fish[2:] == (39.5, 39.5) and e.pin[2:] == (63.5, 47.5)
    assert abs(e.fish[0] * e.theta_max - 40.0) <= 1e-12 and abs(e.pin[0] * math.tan(e.theta_max) - 48.0) <= 1e-12


def test_image_model_is_the_letterbox():
    """A raw 48 x 64 image in a 96 x 96 pinhole frame: r = 1.5; its pixel u stands at (u + 0.5) * 1.5 - 0.5 of the frame."""
    m = LensModel(PIN, FISH, K, 170.0, size=(96, 96))
    im = lens.image_model(m, 48, 64, (96, 96))
    assert im.fish == m.fish and im.size == m.size
    a, b = L.model(m.pin, m.fish, K), L.model(im.pin, im.fish, K)
    X, Y, _ = L.to_fisheye(np.array([(10.0 + 0.5) * 1.5 - 0.5]), np.array([(7.0 + 0.5) * 1.5 - 0.5]), a)
    X2, Y2, _ = L.to_fisheye(np.array([10.0]), np.array([7.0]), b)
    assert abs(X[0] - X2[0]) <= 1e-9 and abs(Y[0] - Y2[0]) <= 1e-9


def test_fisheye_lens_flag(tmp_path):
    path = str(tmp_path / "lens.json")
    LensModel(PIN, FISH, K, 170.0).to_json(path)
    sys.path.insert(0, Y24)
    try:
        import importlib
        mod = importlib.import_module("train_24p")
        assert mod.make_parser().parse_args([]).fisheye_lens is None
        a = mod.make_parser().parse_args(["--fisheye-lens", path, path])
        assert a.fisheye_lens == [path, path]
        a.raw_u8 = True
        mod.check_fisheye_lens_args(a)
        mod.check_fisheye_lens_args(mod.make_parser().parse_args([]))
        with pytest.raises(SystemExit):
            mod.make_parser().parse_args(["--fisheye-lens"])
        for extra, word in ((["--fisheye-theta", "30", "90"], "--fisheye-theta"), (["--augment"], "--augment"),
                            (["--no-prefetch"], "--no-prefetch"), (["--fp32-batches"], "--fp32-batches")):
            a = mod.make_parser().parse_args(["--fisheye-lens", path] + extra)
            a.raw_u8 = not (a.fp32_batches or a.no_prefetch)
            with pytest.raises(SystemExit, match=word):
                mod.check_fisheye_lens_args(a)
        a = mod.make_parser().parse_args(["--fisheye-lens", path + ".missing"])
        a.raw_u8 = True
        with pytest.raises(SystemExit, match="no such calibration file"):
            mod.check_fisheye_lens_args(a)
    finally:
        sys.path.remove(Y24)


def test_lens_has_no_cpu_path(monkeypatch):
    """Without a visible GPU every entry point raises: there is no CPU fallback."""
    import torch
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    m = LensModel(PIN, FISH, K, 170.0)
    img = np.zeros((8, 8, 3), dtype=np.uint8)
    with pytest.raises(_lib.Ep24Error):
        lens.map_points(np.zeros((3, 2)), m, "distort")
    with pytest.raises(_lib.Ep24Error):
        lens.warp_images([img], m, "distort", (8, 8))
    with pytest.raises(_lib.Ep24Error):
        lens.preproc_images([img], m, "undistort", (8, 8))
    with pytest.raises(_lib.Ep24Error):
        lens.warp_labels([np.zeros((0, 51))], [(8, 8)], m, "distort", (8, 8))
    with pytest.raises(_lib.Ep24Error):
        lens.LensTransform([m]).batch([img], [np.zeros((0, 51))], (8, 8))


def test_library_exports_the_lens_entry_points():
    protos = _lib.parse_header()
    for name in ("ep24_lens_points", "ep24_lens_warp_u8", "ep24_lens_preproc_u8", "ep24_lens_labels"):
        assert name in protos and name in _lib.lib().fn
