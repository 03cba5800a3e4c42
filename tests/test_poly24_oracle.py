"""The numpy oracle of the polygon geometry (tests/poly24_oracle.py) against closed forms and against itself: the area IoU on
analytic cases and on supersampled rasters, the packed raster form against the pixel rule.  No GPU."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import poly24_oracle as P  # noqa: E402


def _iou(a, b):
    return float(P.poly24_iou(a[None], b[None])[0, 0])


def _star(seed, cx=31.5, cy=29.25):
    rng = np.random.default_rng(seed)
    return P.regular(cx, cy, rng.uniform(5.0, 15.0, 24))


def test_identical_polygons():
    for seed in range(4):
        a = _star(seed)
        assert abs(_iou(a, a) - 1.0) <= 1e-12
    a = P.regular64(30.0, 30.0, 10.0)
    assert abs(_iou(a, a) - 1.0) <= 1e-12


@pytest.mark.parametrize("r1,r2", [(4.0, 9.0), (7.5, 8.0), (1.0, 20.0)])
def test_concentric_regular_polygons(r1, r2):
    a, b = P.regular64(32.0, 31.0, r1), P.regular64(32.0, 31.0, r2)
    assert abs(_iou(a, b) - (r1 / r2) ** 2) <= 1e-12
    assert abs(_iou(b, a) - (r1 / r2) ** 2) <= 1e-12


def _box(cx, cy, h):
    return (cx - h, cy - h, cx + h, cy + h)


@pytest.mark.parametrize("dx,dy,h2", [(3.0, 2.0, 8.0), (0.0, 0.0, 4.0), (10.0, -7.0, 8.0), (0.5, 12.0, 6.0), (-15.0, 15.0, 8.0)])
def test_axis_aligned_squares_equal_the_rectangle_formula(dx, dy, h2):
    a, b = P.square64(32.0, 32.0, 8.0), P.square64(32.0 + dx, 32.0 + dy, h2)
    assert abs(abs(P._shoelace(a)) - 256.0) <= 1e-10
    assert abs(_iou(a, b) - P.rect_iou(_box(32.0, 32.0, 8.0), _box(32.0 + dx, 32.0 + dy, h2))) <= 1e-12


def test_disjoint_and_edge_sharing_squares_are_exactly_zero():
    a = P.square64(16.0, 16.0, 8.0)
    assert _iou(a, P.square64(40.5, 16.0, 8.0)) == 0.0                           # disjoint
    b = P.square64(32.0, 16.0, 8.0)                                              # shares the edge x = 24
    assert a[:, 0].max() == b[:, 0].min() == 24.0
    assert _iou(a, b) == 0.0 and _iou(b, a) == 0.0
    assert _iou(a, P.square64(32.0, 32.0, 8.0)) == 0.0                           # shares one corner
    assert _iou(a, P.square64(16.0, 32.0, 8.0)) == 0.0                           # shares the edge y = 24


def test_invariance_under_reversal_and_swap():
    for seed in range(6):
        a, b = _star(seed), _star(100 + seed, 36.0, 33.0)
        v = _iou(a, b)
        assert 0.0 < v < 1.0
        assert abs(_iou(a[::-1].copy(), b) - v) <= 1e-12
        assert abs(_iou(a, b[::-1].copy()) - v) <= 1e-12
        assert abs(_iou(b, a) - v) <= 1e-12


def test_nan_and_empty_inputs():
    a, b = _star(1), _star(2)
    bad = b.copy()
    bad[5] = np.nan
    m = P.poly24_iou(np.stack([a, b]), np.stack([b, bad, a]))
    assert m.shape == (2, 3) and np.isnan(m[:, 1]).all() and np.isfinite(m[:, [0, 2]]).all()
    assert P.poly24_iou(np.zeros((0, 24, 2)), np.stack([a])).shape == (0, 1)
    z = P.regular(30.0, 30.0, 0.0)                                               # a point: no area, no overlap
    assert _iou(z, a) == 0.0 and _iou(z, z) == 0.0


def test_against_supersampled_rasters():
    """40 generator pairs on a 64 x 64 canvas against the IoU of their rasters at 16 x (vertices scaled by 16, 1024 x 1024).
    The bound is the raster's discretisation: boundary pixels over area at 16 x on these sizes; measured worst 2e-4."""
    rows = P.generator_pairs()
    worst = 0.0
    for pair in rows:
        a, b = P.det_polygons(pair)
        exact = _iou(a, b)
        ma = P.unpack_bits(P.raster_words(a * np.float32(16), 1024, 1024), 1024)
        mb = P.unpack_bits(P.raster_words(b * np.float32(16), 1024, 1024), 1024)
        inter, union = int((ma & mb).sum()), int((ma | mb).sum())
        worst = max(worst, abs(exact - inter / union))
    print("poly24 oracle vs 16x rasters: worst |diff| = %.3e" % worst)
    assert worst <= 1e-3


def _raster_cases():
    """Polygons that exercise the pixel rule: integer vertices (rows through a vertex), a horizontal edge, partly and wholly
    outside the canvas, zero radius, a random star."""
    rng = np.random.default_rng(3)
    th = np.arange(24) * (np.pi / 12)
    cases = [
        P.regular(16.0, 20.0, rng.uniform(3.0, 15.0, 24)),
        np.stack([np.round(16 + 11 * np.cos(th)), np.round(19 + 13 * np.sin(th))], -1).astype(np.float32),   # integer vertices
        P.square64(12.0, 18.0, 7.0).astype(np.float32),                          # horizontal edges on the rows 11 and 25
        P.regular(-3.0, 5.0, 9.0),                                               # partly left / above
        P.regular(30.0, 38.0, 12.5),                                             # partly right / below
        P.regular(-40.0, -40.0, 6.0),                                            # wholly outside
        P.regular(200.0, 20.0, 10.0),
        P.regular(10.0, 10.0, 0.0),                                              # zero radius
        P.regular(10.5, 10.5, 0.25),                                             # between pixel centres: empty
        P.regular(20.0, 20.0, 500.0),                                            # covers the canvas
    ]
    return np.stack(cases).astype(np.float32)


@pytest.mark.parametrize("W", [1, 31, 32, 33, 65])
def test_prefix_xor_words_equal_the_pixel_rule(W):
    H = 40
    for poly in _raster_cases():
        want = P.raster_pixels(poly, H, W)
        words = P.raster_words(poly, H, W)
        assert words.shape == (H, (W + 31) // 32) and words.dtype == np.uint32
        assert np.array_equal(P.unpack_bits(words, W), want)
        assert np.array_equal(P.pack_bits(want[None])[0], words)                 # also: the bits at x >= W are zero


def test_pixel_rule_boundaries_are_half_open():
    # the square [4, 12] x [4, 12]: left and top boundary pixels in, right and bottom out
    sq = P.square64(8.0, 8.0, 4.0).astype(np.float32)
    assert (sq[:, 0].min(), sq[:, 1].min(), sq[:, 0].max(), sq[:, 1].max()) == (4.0, 4.0, 12.0, 12.0)
    m = P.raster_pixels(sq, 16, 16)
    want = np.zeros((16, 16), bool)
    want[4:12, 4:12] = True
    assert np.array_equal(m, want)
    bbox, area = P.boxes_areas(m[None])
    assert bbox.tolist() == [[4, 4, 11, 11]] and area.tolist() == [64]
    e_bbox, e_area = P.boxes_areas(np.zeros((1, 5, 7), bool))
    assert e_bbox.tolist() == [[7, 5, -1, -1]] and e_area.tolist() == [0]


def test_pack_round_trip_and_mask_iou():
    rng = np.random.default_rng(5)
    m = rng.random((3, 9, 70)) < 0.4
    assert np.array_equal(P.unpack_bits(P.pack_bits(m), 70), m)
    inter, iou = P.mask_iou(m, m[:2])
    assert inter[0, 0] == m[0].sum() and iou[0, 0] == 1.0 and inter[2, 1] == (m[2] & m[1]).sum()
    _, z = P.mask_iou(np.zeros((1, 4, 4), bool), np.zeros((1, 4, 4), bool))
    assert z[0, 0] == 0.0
