"""The continuous sector map and the label warp on the GPU (csrc/sector.hip: ep24_sector_points, ep24_sector_labels) against their numpy
restatement (tests/fisheye_oracle.py), the GPU's own winner maps, and the image-only fisheye transform."""
import functools

import numpy as np
import pytest
import torch

import fisheye_oracle as F

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SIZES = [(48, 64), (64, 96)]
ROWS = [None, 40, 120]
THETAS = [15, 60, 90, 180]


@functools.lru_cache(maxsize=None)
def dist():
    from ep24.sector import Image_Distortion
    return Image_Distortion(DEV)


@pytest.mark.parametrize("theta", THETAS)
def test_map_points_against_the_restatement(theta):
    """Outputs are double; only the device's and numpy's sin / cos differ: 1e-6 px."""
    rng = np.random.RandomState(theta)
    for h, w in SIZES:
        for custom_rows in ROWS:
            g = F.geometry(theta, h, w, custom_rows)
            pts = np.stack([rng.uniform(-0.5, w - 0.5, 10000), rng.uniform(-0.5, h - 0.5, 10000)], 1)
            got = dist().map_points(pts, theta, h, w, custom_rows)
            assert got.dtype == torch.float64 and tuple(got.shape) == (10000, 2) and got.is_cuda
            X, Y = F.sector_map(pts[:, 0], pts[:, 1], g)
            err = np.abs(got.cpu().numpy() - np.stack([X, Y], 1)).max()
            print("theta %d %dx%d rows %s: max |difference| %.3g px" % (theta, h, w, custom_rows, err))
            assert err <= 1e-6
    assert tuple(dist().map_points(np.zeros((0, 2)), theta, 48, 64).shape) == (0, 2)


@pytest.mark.parametrize("theta", THETAS)
def test_map_points_against_the_gpu_winner_map(theta):
    """The centre of every winning texel of ``source_index`` maps forward to within a pixel of the pixel that took it (the bounds of the
    CPU test against the reference's scatter)."""
    for h, w in SIZES:
        for custom_rows in ROWS:
            g = F.geometry(theta, h, w, custom_rows)
            src = dist().source_index(theta, h, w, custom_rows).cpu().numpy()
            assert src.shape == (g["oh"], g["ow"])
            oy, ox = np.nonzero(src >= 0)
            u, v = F.texel_centre(src[oy, ox].astype(np.int64), g)
            got = dist().map_points(np.stack([u, v], 1), theta, h, w, custom_rows).cpu().numpy()
            ex, ey = got[:, 0] - ox, got[:, 1] - oy
            print("theta %d %dx%d rows %s: X - ox in [%.4f, %.4f], Y - oy in [%.4f, %.4f]" % (theta, h, w, custom_rows, ex.min(), ex.max(),
                                                                                             ey.min(), ey.max()))
            assert len(ox) > 0 and np.abs(ex).max() <= 1.01 and np.abs(ey).max() <= 0.51


# --------------------------------------------------------------------------------------------------------------- the label warp
INPUT = (256, 320)
#         rows  (h, w)      theta
SCENE = [(3, (240, 320), 30),            # a tiny object between two others: the filter drops it
         (0, (300, 200), 60),            # an image without labels between two that have some
         (5, (480, 640), 90),            # one object reaches over the image's top edge: its vertices are clamped
         (1, (200, 300), 120),           # one crafted object whose box centre lies outside its outline: the flag bit
         (4, (256, 256), 45),
         (50, (640, 640), 180),
         (53, (640, 512), 75)]           # more than max_labels: the first 50 are read


def arc_band(h, w, cx, cy, r_out, r_in):
    """A half ring, open towards -y: 12 vertices on the outer arc, 12 back on the inner one.  The middle of its box lies in the hollow;
    the row's own centre is a point of the band."""
    a = np.linspace(0.0, np.pi, 12)
    x = np.concatenate([cx + r_out * np.cos(a), cx + r_in * np.cos(a[::-1])])
    y = np.concatenate([cy + r_out * np.sin(a), cy + r_in * np.sin(a[::-1])])
    row = np.zeros(51)
    row[0], row[1], row[2] = 7, (cx + 3.0) / w, (cy + (r_out + r_in) / 2) / h
    row[3::2], row[4::2] = x / w, y / h
    return row


@functools.lru_cache(maxsize=None)
def scene():
    """-> (targets, sizes, thetas, oracle table, counts, flags, margins): computed once, shared, never written to."""
    rng = np.random.RandomState(11)
    targets, sizes, thetas = [], [], []
    for k, (h, w), theta in SCENE:
        big = min(h, w) / 6.0
        rows = F.blob_rows(rng, k, h, w, big / 3.0, big) if k < 50 else F.blob_rows(rng, k, h, w, 8.0, 20.0)
        if k == 3:
            rows[1] = F.blob_rows(rng, 1, h, w, 0.04, 0.05)[0]
        if k == 5:
            rows[2, 1::2] += 0.5 - rows[2, 1]                 # centre at the middle of the top edge: the upper part hangs over it
            rows[2, 2::2] += 0.03 - rows[2, 2]
        if k == 1:
            rows[0] = arc_band(h, w, 150.0, 70.0, 60.0, 45.0)
        targets.append(rows)
        sizes.append((h, w))
        thetas.append(theta)
    geoms = [F.geometry(t, h, w) for (h, w), t in zip(sizes, thetas)]
    for a in targets:
        a.setflags(write=False)
    return (targets, sizes, thetas) + F.warp_labels(targets, geoms, INPUT, 50)


def test_the_scene_covers_what_it_should():
    """The oracle's own view of the scene, asserted before anything is demanded from the GPU: no decision on a knife edge, the tiny
    object dropped, the crafted one flagged, something clamped, 50 of 53 read."""
    _, _, _, table, counts, flags, margins = scene()
    print("oracle margins:", margins)
    assert min(margins.values()) > 1e-6
    assert counts.tolist() == [2, 0, 5, 1, 4, 50, 50]
    assert flags[3, 0] == 1 and flags.sum() == 1
    assert (table[2, 2, 4::2] == 0).any() and (table[2, 2, 4::2] > 0).any()      # clamped to the top edge
    assert table[..., 1:].max() < 2048                                            # the fp32 rounding the tolerance assumes


def test_warp_labels_against_the_restatement():
    """Counts and flags equal; coordinates within 1e-3 px: the fp32 rounding of a value below 2048 is <= 1.3e-4, the rest is double."""
    from ep24 import fisheye
    targets, sizes, thetas, table, counts, flags, margins = scene()
    assert min(margins.values()) > 1e-6
    got, got_counts, got_flags = fisheye.warp_labels(targets, sizes, thetas, INPUT, 50)
    assert got.dtype == torch.float32 and tuple(got.shape) == (7, 50, 51) and got.is_cuda
    assert got_counts.dtype == torch.int32 and got_flags.dtype == torch.int32 and tuple(got_flags.shape) == (7, 50)
    assert got_counts.cpu().numpy().tolist() == counts.tolist()
    assert np.array_equal(got_flags.cpu().numpy(), flags)
    got = got.cpu().numpy()
    assert np.array_equal(got[..., 0], table[..., 0])
    err = np.abs(got.astype(np.float64) - table.astype(np.float64)).max()
    print("max |difference| %.3g px" % err)
    assert err <= 1e-3
    for i, c in enumerate(counts):
        assert not got[i, c:].any()


def test_warp_labels_other_max_labels_and_custom_rows():
    """max_labels that is no multiple of the four rows of a workgroup and smaller than an image's rows; a custom row count."""
    from ep24 import fisheye
    targets, sizes, thetas = scene()[:3]
    for max_labels, custom_rows in ((7, None), (50, 300)):
        geoms = [F.geometry(t, h, w, custom_rows) for (h, w), t in zip(sizes, thetas)]
        table, counts, flags, margins = F.warp_labels(targets, geoms, INPUT, max_labels)
        assert min(margins.values()) > 1e-6
        got, got_counts, got_flags = fisheye.warp_labels(targets, sizes, thetas, INPUT, max_labels, custom_rows)
        assert got_counts.cpu().numpy().tolist() == counts.tolist() and np.array_equal(got_flags.cpu().numpy(), flags)
        assert np.abs(got.cpu().numpy().astype(np.float64) - table.astype(np.float64)).max() <= 1e-3
    empty = fisheye.warp_labels([], [], [], INPUT, 50)
    assert tuple(empty[0].shape) == (0, 50, 51) and tuple(empty[1].shape) == (0,)


def test_warp_labels_is_deterministic():
    from ep24 import fisheye
    targets, sizes, thetas = scene()[:3]
    a = fisheye.warp_labels(targets, sizes, thetas, INPUT, 50)
    b = fisheye.warp_labels(targets, sizes, thetas, INPUT, 50)
    out = torch.full((7, 50, 51), float("nan"), dtype=torch.float32, device=DEV)
    c = fisheye.warp_labels(targets, sizes, thetas, INPUT, 50, out=out)
    assert c[0] is out
    for x, y, z in zip(a, b, c):
        assert torch.equal(x, y) and torch.equal(x, z)


class Replay:
    """Stands in for a RandomState: hands out the given angles."""

    def __init__(self, values):
        self.values = list(values)

    def randint(self, lo, hi):
        v = self.values.pop(0)
        assert lo <= v < hi
        return v


def test_fisheye_transform_through_a_prefetcher():
    """The images are those of ``TrainTransform(fisheye=...)`` at the same angles; the labels are ``warp_labels`` at those angles."""
    from ep24 import fisheye
    from ep24.input import DataPrefetcher, TrainTransform
    rng = np.random.RandomState(3)
    sizes, S = [(48, 64), (64, 96), (64, 64)], (64, 96)
    batches = []
    for _ in range(2):
        images = [rng.randint(0, 256, (h, w, 3)).astype(np.uint8) for h, w in sizes]
        targets = [F.blob_rows(rng, k, h, w, 4.0, 9.0) for k, (h, w) in zip((2, 0, 3), sizes)]
        batches.append((images, targets, None, None))
    tf = fisheye.FisheyeTransform(theta=(40, 70), seed=9)
    tf.set_position(2, 5)
    twin = fisheye.FisheyeTransform(theta=(40, 70), seed=9)
    twin.set_position(2, 5)
    pf = DataPrefetcher(batches, S, tf)
    for images, targets, _, _ in batches:
        thetas = twin.sample(len(images))
        got_images, got_labels = pf.next()
        torch.cuda.synchronize()
        plain = TrainTransform(max_labels=50, fisheye=(40, 70))
        plain._rng = Replay(thetas)
        want_images, _ = plain.batch(images, targets, S)
        want_labels, want_counts, _ = fisheye.warp_labels(targets, sizes, thetas, S, 50)
        assert len(set(thetas)) > 1
        assert torch.equal(got_images, want_images) and torch.equal(got_labels, want_labels)
        assert want_counts.cpu().numpy().tolist() == [2, 0, 3]
    assert pf.next() == (None, None)


def test_bad_arguments_launch_nothing():
    from ep24 import _lib
    from ep24._lib import call, ptr, stream_ptr
    from ep24.augment import _rot
    pts = torch.zeros(4, 2, dtype=torch.float64, device=DEV)
    out = torch.full((4, 2), -7.0, dtype=torch.float64, device=DEV)
    good = (ptr(pts), 4, 60.0, 100, 48, 64, 999, 0, 0, ptr(out))
    for i, bad in ((0, None), (9, None), (1, -1), (2, 10.0), (2, 200.0), (3, 1), (4, 0), (5, -3), (6, 0)):
        args = list(good)
        args[i] = bad
        with pytest.raises(_lib.Ep24Error, match="sector_points"):
            call("sector_points", *args, stream_ptr())
    call("sector_points", None, 0, 60.0, 100, 48, 64, 999, 0, 0, None, stream_ptr())       # nothing to do is not an error
    torch.cuda.synchronize()
    assert bool((out == -7.0).all())

    n, ml = 2, 4
    dbl = torch.zeros(n * 12 + 51, dtype=torch.float64, device=DEV)
    cand = torch.empty(n, ml, 51, dtype=torch.float32, device=DEV)
    keep = torch.empty(n, ml, dtype=torch.int32, device=DEV)
    lab = torch.full((n, ml, 51), -7.0, dtype=torch.float32, device=DEV)
    cnt = torch.full((n,), -7, dtype=torch.int32, device=DEV)
    flg = torch.full((n, ml), -7, dtype=torch.int32, device=DEV)
    good = (ptr(dbl, n * 12), ptr(dbl), ptr(_rot(torch.device(DEV))), n, ml, ptr(cand), ptr(keep), ptr(lab), ptr(cnt), ptr(flg))
    for i, bad in ((0, None), (1, None), (2, None), (5, None), (6, None), (7, None), (8, None), (9, None), (3, -1), (3, 65536), (4, 0),
                   (4, -2)):
        args = list(good)
        args[i] = bad
        with pytest.raises(_lib.Ep24Error, match="sector_labels"):
            call("sector_labels", *args, stream_ptr())
    call("sector_labels", None, None, None, 0, ml, None, None, None, None, None, stream_ptr())
    torch.cuda.synchronize()
    assert bool((lab == -7.0).all()) and bool((cnt == -7).all()) and bool((flg == -7).all())
    # the same table with no rows at all: every image comes out empty
    call("sector_labels", *good, stream_ptr())
    torch.cuda.synchronize()
    assert not lab.any() and not cnt.any() and not flg.any()
