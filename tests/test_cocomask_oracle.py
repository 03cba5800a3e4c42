"""Pins tests/cocomask_oracle.py, the sequential restatement of the COCO mask API that ep24.cocomask is tested against:
hand-checked polygons, the per-column parity form, the real annotation of the fixture and the RLE string format."""
import json
import os
import random

import cocomask_oracle as ora
from conftest import GOLDEN

FIXTURE = os.path.join(GOLDEN, "coco_ann_130566.json")


def rect(r0, r1, c0, c1, h, w):
    return [[1 if r0 <= y < r1 and c0 <= x < c1 else 0 for x in range(w)] for y in range(h)]


SQUARE = [2, 2, 6, 2, 6, 6, 2, 6]
DOUBLED = [2, 2, 2, 2, 6, 2, 6, 2, 6, 6, 6, 6, 2, 6, 2, 6]

# (name, segmentation, h, w, expected mask or None, expected number of pixels)
TABLE = [
    ("rect", [[2, 1, 6, 1, 6, 4, 2, 4]], 8, 10, rect(1, 4, 2, 6, 8, 10), 12),
    ("rect_half", [[2.5, 1.5, 6.5, 1.5, 6.5, 4.5, 2.5, 4.5]], 8, 10, rect(2, 5, 3, 7, 8, 10), 12),
    ("unit", [[0, 0, 1, 0, 1, 1, 0, 1]], 1, 1, [[1]], 1),
    ("cover", [[-3, -3, 20, -3, 20, 20, -3, 20]], 6, 7, rect(0, 6, 0, 7, 6, 7), 42),
    ("one_vertex", [[3, 4]], 8, 10, rect(0, 0, 0, 0, 8, 10), 0),
    ("two_vertices", [[1, 1, 7, 5]], 8, 10, rect(0, 0, 0, 0, 8, 10), 0),
    ("tiny_triangle", [[.4, .4, .6, .4, .6, .6]], 8, 10, rect(0, 0, 0, 0, 8, 10), 0),
    ("square", [SQUARE], 10, 10, rect(2, 6, 2, 6, 10, 10), 16),
    ("square_doubled", [DOUBLED], 10, 10, rect(2, 6, 2, 6, 10, 10), 16),
    ("two_squares", [[1, 1, 6, 1, 6, 6, 1, 6], [4, 4, 9, 4, 9, 9, 4, 9]], 10, 10, None, 46),
    ("bow_tie", [[1, 1, 9, 9, 9, 1, 1, 9]], 12, 12, None, 32),
]


def random_polygon(g, i):
    """Case i of the seeded random set: 1 - 8 vertices up to 6 px outside an image of 1..39 on a side, coordinates rounded
    to 2 decimals, every fifth case integer-valued."""
    h, w, k = g.randint(1, 39), g.randint(1, 39), g.randint(1, 8)
    xy = []
    for _ in range(k):
        x, y = g.uniform(-6, w + 6), g.uniform(-6, h + 6)
        xy += [float(round(x)), float(round(y))] if i % 5 == 0 else [round(x, 2), round(y, 2)]
    return xy, h, w


def random_polygons(n=200, seed=2024):
    g = random.Random(seed)
    return [random_polygon(g, i) for i in range(n)]


def fixture_annotation():
    with open(FIXTURE) as f:
        d = json.load(f)
    im, an = d["images"][0], d["annotations"][0]
    return an, im["height"], im["width"]


def count(mask):
    return sum(sum(r) for r in mask)


def test_table():
    for name, seg, h, w, want, npix in TABLE:
        got = ora.ann_to_mask(seg, h, w)
        assert len(got) == h and all(len(r) == w for r in got), name
        assert count(got) == npix, (name, count(got))
        if want is not None:
            assert got == want, name


def test_union_is_or_not_xor():
    a, b = TABLE[9][1]
    ma, mb = ora.ann_to_mask([a], 10, 10), ora.ann_to_mask([b], 10, 10)
    assert count(ma) == 25 and count(mb) == 25
    assert sum(ma[y][x] ^ mb[y][x] for y in range(10) for x in range(10)) == 42
    assert ora.ann_to_mask([a, b], 10, 10) == [[ma[y][x] | mb[y][x] for x in range(10)] for y in range(10)]


def test_sequential_form_equals_column_parity():
    for xy, h, w in random_polygons(400, seed=7):
        counts = ora.rle_from_poly(xy, h, w)
        assert sum(counts) == h * w and all(c > 0 for c in counts[1:])
        assert ora.rle_decode(counts, h, w) == ora.mask_from_parity(xy, h, w), (xy, h, w)
        per_column = [0] * w
        for x, y in ora.boundary_points(xy, h, w):
            assert 0 <= x < w and 0 <= y <= h
            per_column[x] += 1
        assert all(c % 2 == 0 for c in per_column), (xy, h, w)


def test_fixture_annotation():
    an, h, w = fixture_annotation()
    assert (h, w) == (427, 640) and len(an["segmentation"]) == 1 and len(an["segmentation"][0]) == 60
    assert count(ora.ann_to_mask(an["segmentation"], h, w)) == 32513            # the annotation's own area: 32509.09
    assert abs(an["area"] - 32509.09) < 0.01


def test_rle_string_round_trip():
    for cnts in ([0, 5, 3, 2000, 7, 1, 40000, 2, 1], [12], [3, 1025, 2, 1, 1500, 1500, 31, 32, 15, 16], [0, 1]):
        s = ora.rle_to_string(cnts)
        assert all(48 <= ord(c) < 112 for c in s)
        assert ora.rle_from_string(s) == cnts and ora.rle_from_string(s.encode()) == cnts
    assert ora.rle_to_string([5, 3, 2]) == "532"                               # one char per count below 16
    assert ora.rle_from_string("0") == [0] and ora.rle_from_string("O") == [-1]                 # 0x1f: sign bit set, extended
    h, w = 6, 7
    cnts = [0, 5, 3, 2, 20, 1, 11]
    m = ora.ann_to_mask({"size": [h, w], "counts": ora.rle_to_string(cnts)}, h, w)
    assert m == ora.ann_to_mask({"size": [h, w], "counts": cnts}, h, w) and count(m) == 8
    assert [m[y][0] for y in range(h)] == [1, 1, 1, 1, 1, 0]                    # a first run of 0: the mask starts with ones
