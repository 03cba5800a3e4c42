"""ep24.draw on the GPU against the numpy oracle (tests/draw24_oracle.py), byte for byte: pixels a row covers and pixels nobody
touches alike.  Shapes are the smallest that cross the kernel's boundaries: the 64 x 16 tile (canvases one short of, equal to and
one past it), the 4-pixel quad and its aligned / unaligned store paths (row lengths 1, 63, 64, 65, 130), the 256-record chunk
(n = 255, 256, 257).  Where floats decide - the float32 vertex values before truncation - the oracle's margin (>= 1e-3 from an
integer) is asserted before any comparison."""
import numpy as np
import pytest
import torch

import draw24_oracle as O
import draw24_scenes as S
from ep24 import draw

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CANVASES = [(1, 1), (15, 63), (16, 64), (17, 65), (33, 130)]


def noise(H, W, seed):
    return np.random.default_rng(seed).integers(0, 256, (H, W, 3), dtype=np.uint8)


def gpu_draw(img, dets, **kw):
    d = None if dets is None else torch.from_numpy(np.ascontiguousarray(dets, dtype=np.float32)).to(DEV)
    return draw.draw_detections(torch.from_numpy(img).to(DEV), d, **kw)


def compare(img, dets, **kw):
    """Oracle margins first, then torch.equal on the whole image.  Returns the oracle's image."""
    margins = []
    want = O.draw(img, dets, margins=margins, **kw)
    print("rows drawn %d, smallest vertex margin %.4g" % (len(margins), min(margins) if margins else float("nan")))
    assert all(m >= S.MARGIN for m in margins), min(margins)
    got = gpu_draw(img, dets, **kw).cpu()
    bad = int((got.numpy() != want).any(axis=2).sum())
    print("pixels changed %d, pixels differing %d" % (int((want != img).any(axis=2).sum()), bad))
    assert torch.equal(got, torch.from_numpy(want)), "%d pixels differ" % bad
    return want


def seeded(n, H, W, seed, **kw):
    rows, dropped = S.random_rows(n, H, W, seed, **kw)
    print("seeded rows %d, dropped for the margin %d" % (n, dropped))
    assert dropped <= 0.05 * (n + dropped)
    return rows


@pytest.mark.parametrize("H,W", CANVASES)
def test_canvases(H, W):
    rows = seeded(6, H, W, seed=H * W)
    want = compare(noise(H, W, 1), rows, fill_alpha=100, show_scores=True)
    assert (want != noise(H, W, 1)).any()


@pytest.mark.parametrize("n", [0, 1, 255, 256, 257])
def test_chunk_boundary(n):
    """Small objects, mixed classes, many overlaps: painter's order across the 256-record chunks decides many pixels."""
    H, W = 33, 130
    rows = seeded(n, H, W, seed=n + 7, rmin=1.5, rmax=6.0)
    want = compare(noise(H, W, 2), rows, fill_alpha=77)
    if n >= 255:                                            # the order matters: the same rows backwards give another image
        assert (O.draw(noise(H, W, 2), rows[::-1], fill_alpha=77) != want).any()


@pytest.mark.parametrize("ratio", [1.0, 0.4375, 1.7])
def test_edge_case_rows(ratio):
    H, W = 33, 130
    cases = S.edge_rows(H, W, ratio)
    drawn = {name: O.row_geometry(row, ratio, 0.25, H, W, 3) is not None for name, row in cases}
    assert [name for name, ok in drawn.items() if not ok] == ["score below conf", "NaN radius", "infinite centre", "radius at least 2^20",
                                                              "centre at least 2^20", "class -1", "class 3"]
    rows = np.stack([row for _, row in cases])
    kw = dict(ratio=ratio, conf=0.25, num_classes=3, class_names=S.NAMES3, fill_alpha=90, show_scores=True)
    compare(noise(H, W, 3), rows, **kw)
    for name, row in cases:                                 # and each row by itself: a skipped row leaves every byte alone
        want = compare(noise(H, W, 3), row[None], **kw)
        assert (want != noise(H, W, 3)).any() == drawn[name], name
    geo = O.row_geometry(dict(cases)["clamped to x = W and y = H"], ratio, 0.25, H, W, 3)
    assert geo["vx"].max() == W and geo["vy"].max() == H
    geo = O.row_geometry(dict(cases)["all radii zero"], ratio, 0.25, H, W, 3)
    assert len(set(zip(geo["vx"].tolist(), geo["vy"].tolist()))) == 1          # every edge degenerate


@pytest.mark.parametrize("alpha", [0, 128, 255])
def test_fill_alpha_on_overlapping_polygons(alpha):
    H, W = 33, 130
    rows = np.stack([S.make_row(50, 16, S.wobble(11.0), cls=0), S.make_row(60, 18, S.wobble(10.0), cls=1)])
    img = noise(H, W, 4)
    want = compare(img, rows, num_classes=3, fill_alpha=alpha)
    both = (55, 17)                                         # (x, y) inside both polygons, on neither outline
    if alpha == 0:
        assert np.array_equal(want[both[1], both[0]], img[both[1], both[0]])
    else:
        c0, c1 = O.default_colors(3)[:2]
        assert np.array_equal(want[both[1], both[0]], O.blend(O.blend(img[both[1], both[0]], c0, alpha), c1, alpha))


@pytest.mark.parametrize("scale", [1, 2, 3])
@pytest.mark.parametrize("names", [None, S.NAMES3])
def test_text_scales_and_clipping(scale, names):
    """Labels cut by the left, right, top and bottom side of the canvas, with class names (one cut to 21 bytes) and index labels."""
    H, W = 33, 130
    compare(noise(H, W, 5), S.text_rows(H, W), num_classes=3, class_names=names, font_scale=scale)


def test_show_scores():
    H, W = 33, 130
    scores = [0.0, 0.057, 0.999, 1.0]
    rows = np.stack([S.make_row(8 + 30 * i, 24, S.wobble(2.0), obj=sc, cc=1.0, cls=i % 3) for i, sc in enumerate(scores)])
    assert [O.score_digits(r[26] * r[27]) for r in rows] == [b" 00", b" 05", b" 99", b" 99"]
    compare(noise(H, W, 6), rows, num_classes=3, show_scores=True, font_scale=1)
    compare(noise(H, W, 6), rows, num_classes=3, show_scores=True, class_names=S.NAMES3)


@pytest.fixture(scope="module")
def scene():
    H, W = 33, 130
    rows, dropped = S.random_rows(40, H, W, seed=11, num_classes=5)
    assert dropped <= 2
    img = noise(H, W, 7)
    kw = dict(num_classes=5, fill_alpha=60, show_scores=True)
    margins = []
    want = O.draw(img, rows, margins=margins, **kw)
    assert min(margins) >= S.MARGIN
    return img, rows, kw, torch.from_numpy(want)


def test_scratch_prefilled_with_ff(scene):
    img, rows, kw, want = scene
    rec = draw._records(torch.device(DEV), len(rows))
    rec.view(torch.uint8).fill_(0xFF)
    assert torch.equal(gpu_draw(img, rows, **kw).cpu(), want)
    skipped = rows.copy()
    skipped[::2, 28] = -1.0                                 # every other row skipped: their records must be written as well
    rec.view(torch.uint8).fill_(0xFF)
    assert torch.equal(gpu_draw(img, skipped, **kw).cpu(), torch.from_numpy(O.draw(img, skipped, **kw)))


def test_out_forms_and_repeat(scene):
    img, rows, kw, want = scene
    d = torch.from_numpy(rows).to(DEV)
    src = torch.from_numpy(img).to(DEV)
    new = draw.draw_detections(src, d, **kw)
    assert new.data_ptr() != src.data_ptr() and torch.equal(src.cpu(), torch.from_numpy(img))      # the input is left alone
    out = torch.full_like(src, 0x5A)
    assert draw.draw_detections(src, d, out=out, **kw) is out
    inplace = src.clone()
    assert draw.draw_detections(inplace, d, out=inplace, **kw) is inplace
    again = draw.draw_detections(src, d, **kw)
    for t in (new, out, inplace, again):
        assert torch.equal(t.cpu(), want)
    # nothing to draw: a copy
    for none in (None, d[:0]):
        got = draw.draw_detections(src, none, **kw)
        assert got.data_ptr() != src.data_ptr() and torch.equal(got, src)
    # an image that starts one byte into its buffer takes the byte path where the first took dwords: the same bytes
    buf = torch.zeros(img.size + 1, dtype=torch.uint8, device=DEV)
    odd = buf[1:].view(img.shape)
    odd.copy_(src)
    assert torch.equal(draw.draw_detections(odd, d, out=odd, **kw).cpu(), want)
    # user colours and a float64 detection tensor
    colors = torch.tensor([[1, 2, 3], [250, 0, 9], [0, 0, 0], [255, 255, 255], [7, 77, 177]], dtype=torch.uint8)
    got = draw.draw_detections(src, d.double(), colors=colors.to(DEV), **kw)
    assert torch.equal(got.cpu(), torch.from_numpy(O.draw(img, rows, colors=colors.numpy(), **kw)))


def test_realistic_image():
    """480 x 640, 100 detections of 15 .. 70 pixels mapped back by a letterbox ratio, fill and scores on."""
    H, W = 480, 640
    rows = seeded(100, H, W, seed=5, rmin=15.0, rmax=70.0, spill=20.0, ratio=0.75)
    compare(noise(H, W, 8), rows, ratio=0.75, fill_alpha=96, show_scores=True)
