"""The label warp's surface that needs no GPU: the C ABI entries, the restated continuous map against the reference's integer scatter,
the restated labels against the reference's mask pipeline, the outline's convergence, and the transform's reproducible angle draws."""
import ctypes
import functools
import os
import sys

import numpy as np
import pytest

import fisheye_oracle as F
from ep24 import _lib
from oracle import labels24 as L24, sector as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
Y24 = os.path.join(ROOT, "exploration-of-potential_amd", "yolox_24p")

# (theta, h, w, custom_rows): the five geometries the contract was checked on, one with custom rows, one more with an odd canvas width
MAP_GEOMETRIES = [(15, 640, 427, None), (60, 64, 96, None), (90, 480, 640, None), (120, 1280, 1280, None), (180, 640, 640, None),
                  (45, 96, 128, 300), (75, 300, 400, None)]


@functools.lru_cache(maxsize=None)
def winner(theta, h, w, custom_rows):
    return S.winner_map(theta, h, w, custom_rows)


def test_symbols_are_declared_and_exported():
    protos = _lib.parse_header()
    cdll = ctypes.CDLL(_lib.LIB_PATH)
    for name in ("ep24_sector_points", "ep24_sector_labels"):
        assert name in protos, name
        assert hasattr(cdll, name), name
        assert protos[name][1][-1] == ("void*", "stream"), name
    assert _lib.lib().fn["ep24_abi_version"]() == 3                              # additions only: the version stays


@pytest.mark.parametrize("theta,h,w,custom_rows", MAP_GEOMETRIES)
def test_map_against_the_integer_scatter(theta, h, w, custom_rows):
    """Every written pixel of the reference's scatter: the centre of its winning texel, mapped forward, lands within a pixel of it.
    Bounds: the measured [-1.000, 0.999] x [-0.5, 0.5] plus the rounding of the three printed decimals."""
    src, box, T = winner(theta, h, w, custom_rows)
    g = F.geometry(theta, h, w, custom_rows)
    assert (g["T"], g["y0"], g["x0"], g["oh"], g["ow"]) == (T, box[0], box[2], box[1] - box[0], box[3] - box[2])
    if (theta, h, w) == (75, 300, 400):
        assert g["cw"] % 2 == 1
    oy, ox = np.nonzero(src >= 0)
    X, Y = F.sector_map(*F.texel_centre(src[oy, ox].astype(np.int64), g), g)
    ex, ey = X - ox, Y - oy
    print("theta %s %dx%d rows %s: X - ox in [%.4f, %.4f], Y - oy in [%.4f, %.4f]" % (theta, h, w, custom_rows, ex.min(), ex.max(),
                                                                                     ey.min(), ey.max()))
    assert np.abs(ex).max() <= 1.01 and np.abs(ey).max() <= 0.51


def test_geometry_of_the_package_is_the_restated_one():
    from ep24.sector import Image_Distortion
    for theta, h, w, custom_rows in MAP_GEOMETRIES + [(30, 48, 64, 40), (180, 64, 96, 120)]:
        g = F.geometry(theta, h, w, custom_rows)
        T, cw, (y0, y1, x0, x1), (oh, ow) = Image_Distortion.geometry(theta, h, w, custom_rows)
        assert (T, cw, y0, x0, oh, ow, y1 - y0, x1 - x0) == (g["T"], g["cw"], g["y0"], g["x0"], g["oh"], g["ow"], g["oh"], g["ow"])
    assert Image_Distortion.geometry(60, 64, 96) is Image_Distortion.geometry(60, 64, 96)          # cached, no device work


# ------------------------------------------------------------------------------------------------ the reference's mask pipeline
# (theta, h, w): natural row counts only; four smooth objects each, radii 25 .. 60 px, box centre inside the outline
PIPELINE_GEOMETRIES = [(90, 480, 640), (60, 240, 320), (120, 300, 300)]
# measured with this file's objects: mean distance of the 24 points, largest distance of the box centres, in warped pixels
PIPELINE_MEASURED = {(90, 480, 640): (1.920, 0.977), (60, 240, 320): (2.330, 1.080), (120, 300, 300): (2.873, 1.810)}
# largest change of a re-cast radius between 8 and 32 pieces per edge
CONVERGENCE_MEASURED = {(90, 480, 640): 0.0028, (60, 240, 320): 0.0084, (120, 300, 300): 0.164}


def objects(theta, h, w):
    return F.blob_rows(np.random.RandomState(theta * 7 + h), 4, h, w, 25.0, 60.0)


def raster(row, h, w):
    """Even-odd fill of the 24-gon at pixel centres -> uint8 [h, w, 1], 255 inside."""
    P = np.stack([row[3::2] * w, row[4::2] * h], 1)
    Q = np.roll(P, -1, axis=0)
    ys, xs = np.mgrid[0:h, 0:w].astype(np.float64)
    odd = np.zeros((h, w), dtype=bool)
    for p, q in zip(P, Q):
        if p[1] == q[1]:
            continue
        cross = (p[1] > ys) != (q[1] > ys)
        xc = p[0] + (ys - p[1]) * (q[0] - p[0]) / (q[1] - p[1])
        odd ^= cross & (xc > xs)
    return (odd[..., None] * 255).astype(np.uint8)


def pipeline(theta, h, w):
    """-> (mean point distance, largest centre distance) of the restatement against: rasterise, warp the mask through the reference's
    scatter, box of the warped mask, 24 rays through the warped mask from the restated centre."""
    src, _, T = winner(theta, h, w, None)
    g = F.geometry(theta, h, w)
    point_d, centre_d = [], []
    for row in objects(theta, h, w):
        resized = S.resize_linear_u8(raster(row, h, w), S.N_ANG, T).reshape(-1)
        warped = np.where(src >= 0, resized[np.maximum(src, 0)], 0).astype(np.uint8)
        x, y, bw, bh = S.mask_bbox(warped[..., None])
        out, flag, _, _ = F.warp_row(row, g, 1.0)
        assert out is not None and flag == 0
        centre_d.append(float(np.hypot(out[1] - (x + bw / 2), out[2] - (y + bh / 2))))
        pts, _ = L24.rotation_for_24p(out[1], out[2], warped)
        point_d.append(np.hypot(out[3::2] - pts[:, 0], out[4::2] - pts[:, 1]))
    return float(np.mean(point_d)), float(np.max(centre_d))


def convergence(theta, h, w):
    g = F.geometry(theta, h, w)
    return max(float(np.abs(F.warp_row(row, g, 1.0, sub=8)[3] - F.warp_row(row, g, 1.0, sub=32)[3]).max()) for row in objects(theta, h, w))


@pytest.mark.parametrize("theta,h,w", PIPELINE_GEOMETRIES)
def test_labels_against_the_reference_pipeline(theta, h, w):
    mean_point, max_centre = pipeline(theta, h, w)
    print("theta %d %dx%d: mean point distance %.3f px, largest centre distance %.3f px" % (theta, h, w, mean_point, max_centre))
    want_point, want_centre = PIPELINE_MEASURED[(theta, h, w)]
    assert mean_point <= 1.5 * want_point and max_centre <= 1.5 * want_centre


@pytest.mark.parametrize("theta,h,w", PIPELINE_GEOMETRIES)
def test_eight_pieces_per_edge_have_converged(theta, h, w):
    d = convergence(theta, h, w)
    print("theta %d %dx%d: radii at 8 against 32 pieces per edge differ by at most %.4f px" % (theta, h, w, d))
    assert d <= 1.5 * CONVERGENCE_MEASURED[(theta, h, w)]


def test_vertex_mapping_alone_is_not_enough():
    """Why the outline is subdivided: mapping the 24 vertices only moves the radii by pixels, not by fractions of one."""
    theta, h, w = PIPELINE_GEOMETRIES[0]
    g = F.geometry(theta, h, w)
    d = max(float(np.abs(F.warp_row(row, g, 1.0, sub=1)[3] - F.warp_row(row, g, 1.0, sub=32)[3]).max()) for row in objects(theta, h, w))
    assert d > 4 * CONVERGENCE_MEASURED[(theta, h, w)]


# ------------------------------------------------------------------------------------------------------------ the transform
def test_set_position_reproduces_the_angles():
    from ep24.fisheye import FisheyeTransform
    from ep24.input import TrainTransform
    a, b = FisheyeTransform(theta=(30, 90), seed=5), FisheyeTransform(theta=(30, 90), seed=5)
    assert isinstance(a, TrainTransform) and a.max_labels == 50
    a.set_position(3, 17)
    first = a.sample(8)
    a.sample(8)                                                     # the generator moves on ...
    a.set_position(3, 17)                                           # ... and comes back with the position
    b.set_position(3, 17)
    assert a.sample(8) == first == b.sample(8) and all(30 <= t <= 90 for t in first)
    b.set_position(3, 18)
    other_it = b.sample(8)
    b.set_position(4, 17)
    other_epoch = b.sample(8)
    c = FisheyeTransform(theta=(30, 90), seed=6)
    c.set_position(3, 17)
    assert first != other_it and first != other_epoch and first != c.sample(8)
    assert FisheyeTransform(theta=(45, 45)).sample(3) == [45, 45, 45]
    for bad in ((10, 90), (90, 30), (30, 181)):
        with pytest.raises(ValueError):
            FisheyeTransform(theta=bad)


def test_fisheye_theta_flag():
    sys.path.insert(0, Y24)
    try:
        import importlib
        mod = importlib.import_module("train_24p")
        assert mod.make_parser().parse_args([]).fisheye_theta is None
        a = mod.make_parser().parse_args(["--fisheye-theta", "30", "90"])
        assert a.fisheye_theta == [30, 90]
        a.raw_u8 = True
        mod.check_fisheye_args(a)
        with pytest.raises(SystemExit):
            mod.make_parser().parse_args(["--fisheye-theta", "30"])
        a = mod.make_parser().parse_args(["--fisheye-theta", "30", "90", "--augment"])
        a.raw_u8 = True
        with pytest.raises(SystemExit, match="--augment"):
            mod.check_fisheye_args(a)
        a = mod.make_parser().parse_args(["--fisheye-theta", "10", "90"])
        a.raw_u8 = True
        with pytest.raises(SystemExit):
            mod.check_fisheye_args(a)
    finally:
        sys.path.remove(Y24)


def test_warp_labels_has_no_cpu_path(monkeypatch):
    """Without a visible GPU the label warp raises: there is no CPU fallback."""
    import torch
    from ep24 import fisheye
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    with pytest.raises(_lib.Ep24Error):
        fisheye.warp_labels([np.zeros((0, 51))], [(48, 64)], [60], (64, 64))
    with pytest.raises(_lib.Ep24Error):
        fisheye.FisheyeTransform().batch([np.zeros((48, 64, 3), np.uint8)], [np.zeros((0, 51))], (64, 64))
