"""Closed forms of the feature-map oracle (tests/featmap_oracle.py), and the reference's own expressions restated from
yolox/demo_featuremap.py against its rect mode.  No GPU."""
import numpy as np
import pytest

import featmap_oracle as O

F = np.float32


def _row(verts, cls=1.0):
    """A label row [51]: class, the centre of the vertices' box, 24 x (x, y)."""
    v = np.asarray(verts, dtype=np.float32)
    row = np.zeros(51, dtype=np.float32)
    row[0] = cls
    row[1], row[2] = (v[:, 0].min() + v[:, 0].max()) / 2, (v[:, 1].min() + v[:, 1].max()) / 2
    row[3::2], row[4::2] = v[:, 0], v[:, 1]
    return row


def square(x0, y0, x1, y1):
    """24 vertices on the boundary of an axis-aligned rectangle: six per side, counter-clockwise."""
    t = np.arange(6) / 6.0
    pts = [(x0 + (x1 - x0) * a, y0) for a in t] + [(x1, y0 + (y1 - y0) * a) for a in t]
    pts += [(x1 - (x1 - x0) * a, y1) for a in t] + [(x0, y1 - (y1 - y0) * a) for a in t]
    return np.array(pts, dtype=np.float32)


def circle(cx, cy, r):
    a = np.arange(24) * (15.0 * np.pi / 180.0)
    return np.stack([cx + r * np.cos(a), cy + r * np.sin(a)], 1).astype(np.float32)


def test_constant_map_gives_the_constant_for_both_regions():
    maps = np.full((1, 20, 20), 0.375, dtype=np.float32)
    labels = _row(circle(80.0, 72.0, 40.0))[None, None]
    for mode in ("rect", "poly24"):
        tot, cnt, mean, _ = O.response(maps, 8, labels, mode)
        assert cnt[0, 0] > 1 and mean[0, 0] == 0.375 and tot[0, 0] == 0.375 * cnt[0, 0], mode


def test_square_between_cell_centres_has_equal_counts():
    # edges on multiples of the stride: between the cell centres at (k + 0.5) * 8
    labels = _row(square(16.0, 24.0, 64.0, 56.0))[None, None]
    maps = np.arange(400, dtype=np.float32).reshape(1, 20, 20)
    r = O.response(maps, 8, labels, "rect")
    p = O.response(maps, 8, labels, "poly24")
    assert r[1][0, 0] == p[1][0, 0] == 6 * 4
    assert r[0][0, 0] == p[0][0, 0] == maps[0, 3:7, 2:8].astype(np.float64).sum()


def test_rect_narrower_than_a_cell_is_empty():
    labels = _row(square(17.0, 8.0, 22.0, 60.0))[None, None]               # x in one cell: int(17 / 8) == int(22 / 8)
    tot, cnt, mean, _ = O.response(np.ones((1, 20, 20), np.float32), 8, labels, "rect")
    assert cnt[0, 0] == 0 and tot[0, 0] == 0.0 and mean[0, 0] == 0.0


def test_padding_and_unusable_rows_are_empty():
    good = _row(circle(80.0, 80.0, 30.0))
    nan = good.copy()
    nan[7] = np.nan
    big = good.copy()
    big[8] = 2.0 ** 20
    labels = np.stack([np.zeros(51, np.float32), nan, big, good])[None]
    for mode in ("rect", "poly24"):
        _, cnt, _, _ = O.response(np.ones((1, 20, 20), np.float32), 8, labels, mode)
        assert list(cnt[0, :3]) == [0, 0, 0] and cnt[0, 3] > 0


def test_rect_edges_are_clamped_not_wrapped():
    labels = _row(square(-40.0, -16.0, 24.0, 500.0))[None, None]
    _, cnt, _, _ = O.response(np.ones((1, 20, 20), np.float32), 8, labels, "rect")
    assert cnt[0, 0] == 3 * 20                                              # x in [0, 3), y in [0, 20)


def test_color_index_closed_forms():
    assert O.color_index(1.5, 1.5, 4.0) == 0                                # v = lo
    assert O.color_index(4.0, 1.5, 4.0) == 255                              # v = hi
    assert O.color_index(2.0, 3.0, 3.0) == 0 and O.color_index(2.0, 3.0, 1.0) == 0      # hi <= lo
    assert O.color_index(np.nan, 0.0, 1.0) == 0
    assert O.color_index(-5.0, 0.0, 1.0) == 0 and O.color_index(7.0, 0.0, 1.0) == 255
    assert [O.color_index(k / 256.0, 0.0, 1.0) for k in range(256)] == list(range(256))


def test_alpha_zero_returns_the_base_byte():
    rng = np.random.default_rng(0)
    base = rng.uniform(-20.0, 290.0, (1, 3, 6, 10)).astype(np.float32)
    base[0, :, 0, :7] = np.array([-1.0, 0.0, 0.5, 254.999, 255.0, 300.0, np.nan], dtype=np.float32)
    lut = rng.integers(0, 256, (256, 3), dtype=np.uint8)
    maps = rng.normal(size=(1, 3, 5)).astype(np.float32)
    out = O.render(maps, 2, O.value_range(maps), lut, base=base, alpha=0)
    want = np.array([[[O.base_byte(base[0, ch, y, x]) for ch in range(3)] for x in range(10)] for y in range(6)], dtype=np.uint8)
    assert np.array_equal(out[0], want)
    assert list(want[0, :7, 0]) == [0, 0, 0, 254, 255, 255, 0]
    # and without a base the pixel is the colour of its cell
    plain = O.render(maps, 2, O.value_range(maps), lut)
    assert np.array_equal(plain[0, 1, 3], lut[O.color_index(maps[0, 0, 1], *O.value_range(maps)[0])])


def test_value_range_ignores_nan():
    m = np.array([[3.0, np.nan, -2.0, 7.5], [np.nan, np.nan, np.nan, np.nan]], dtype=np.float32)
    r = O.value_range(m)
    assert tuple(r[0]) == (-2.0, 7.5) and r[1, 0] == np.inf and r[1, 1] == -np.inf


def test_reference_expressions_agree_with_rect_mode():
    """demo_featuremap.py:345 and :378-385 restated: fpn_np.sum(axis=0) / fpn_channel, then for a GT box normalised by the 640 input
    gt_pixel = fpn_np_sum[int(ymin * n):int(ymax * n), int(xmin * n):int(xmax * n)] and gt_pixel.sum() / (h * w)."""
    rng = np.random.default_rng(1)
    for n, stride in ((80, 8), (40, 16), (20, 32)):
        fpn_np = rng.normal(size=(16, n, n)).astype(np.float32)
        fpn_np_sum = fpn_np.sum(axis=0) / fpn_np.shape[0]
        assert np.allclose(fpn_np_sum, O.mean_f64(fpn_np.reshape(16, -1).T).reshape(n, n), rtol=0, atol=1e-6)
        for (x0, y0, x1, y1) in ((100.0, 60.0, 420.0, 333.0), (10.0, 12.0, 630.0, 629.0), (250.5, 310.25, 330.0, 401.75)):
            gt = np.array([x0, y0, x1, y1]) / 640.0                          # gt_box_fm of get_img_mask
            xmin, ymin, xmax, ymax = gt * n
            gt_pixel = fpn_np_sum[int(ymin):int(ymax), int(xmin):int(xmax)].astype(np.float64)
            ref = gt_pixel.sum() / (gt_pixel.shape[0] * gt_pixel.shape[1])
            labels = _row(square(x0, y0, x1, y1))[None, None]
            tot, cnt, mean, _ = O.response(fpn_np_sum[None], stride, labels, "rect")
            assert cnt[0, 0] == gt_pixel.size > 0
            assert mean[0, 0] == pytest.approx(ref, rel=1e-12, abs=1e-15)


def test_mean_oracle_forms():
    rows = np.arange(-12, 12, dtype=np.float32).reshape(1, 24)
    assert O.mean_exact(rows)[0] == F(-12.0) / F(24.0)
    x = np.array([1.0, 1.00390625, 3.140625, -2.5e-3], dtype=np.float32)
    r = O.bf16_round(x)
    assert r[0] == 1.0 and r[1] == 1.0 and np.all(np.abs(r - x) <= np.abs(x) * 2.0 ** -8)    # 1 + 2^-8 ties to even
    assert np.array_equal(O.bf16_bits(r).view(np.uint16).astype(np.uint32) << 16, r.view(np.uint32))
