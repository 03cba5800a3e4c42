"""The fisheye lens model on the GPU (csrc/lens.hip: ep24_lens_points, ep24_lens_warp_u8, ep24_lens_preproc_u8, ep24_lens_labels; ep24.lens)
against its numpy restatement (tests/lens_oracle.py).  Every oracle result is computed once, shared and never written to."""
import functools
import math

import numpy as np
import pytest
import torch

import fisheye_oracle as F
import lens_oracle as L

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
K = (-0.02, 0.004, -0.001, 0.0002)
DIRECTIONS = ("distort", "undistort")
MARGIN = 1e-9             # pixels closer than this to a decision are left out of the bit comparison
SHARE = 1e-3              # and may be this share of an image at the most


def both(pin, fish, k=K, fov=170.0):
    """-> (ep24.lens.LensModel, the oracle's dict) of one lens."""
    from ep24.lens import LensModel
    return LensModel(pin, fish, k, fov), L.model(pin, fish, k, fov)


# ------------------------------------------------------------------------------------------------------------------------ points
@pytest.mark.parametrize("direction", DIRECTIONS)
def test_map_points_against_the_restatement(direction):
    """Outputs are double; the device's and numpy's atan / tan / hypot differ, and Newton from bisection: 1e-6 px, the bound of the
    sector map's double path.  A fifth of the points lie beyond the field."""
    from ep24 import lens
    worst = 0.0
    for fov, pin, fish in ((170.0, (60.0, 60.0, 63.5, 47.5), (52.0, 52.0, 47.5, 39.5)), (120.0, (20.0, 22.0, 26.0, 18.0), (15.0, 17.0, 22.0, 20.0))):
        m, o = both(pin, fish, K, fov)
        rng = np.random.RandomState(int(fov) + len(direction))
        rim = math.tan(o["theta_max"]) if direction == "distort" else L.thetad(o["theta_max"], K)
        f = pin if direction == "distort" else fish
        r = np.concatenate([rng.uniform(0, rim, 8000), rng.uniform(rim, 3 * rim, 2000)])
        phi = rng.uniform(0, 2 * np.pi, 10000)
        pts = np.stack([f[2] + f[0] * r * np.cos(phi), f[3] + f[1] * r * np.sin(phi)], 1)
        pts[0] = (f[2], f[3])                                              # the principal point itself: r = 0
        got = lens.map_points(pts, m, direction)
        assert got.dtype == torch.float64 and tuple(got.shape) == (10000, 2) and got.is_cuda
        want = L.map_points(pts, o, direction)
        assert np.isfinite(want).all() and (np.hypot(*(pts - (f[2], f[3])).T / np.array(f[:2])[:, None]) > rim).sum() > 1000
        err = np.abs(got.cpu().numpy() - want).max()
        print("%s fov %g: max |difference| %.3g px over |coordinates| <= %.0f" % (direction, fov, err, np.abs(want).max()))
        worst = max(worst, err)
        assert tuple(lens.map_points(np.zeros((0, 2)), m, direction).shape) == (0, 2)
    assert worst <= 1e-6


# ------------------------------------------------------------------------------------------------------------------------ images
#        name    pinhole frame  fisheye frame  pin (fx, fy, cx, cy)          fish (fx, fy, cx, cy)
GEOMS = {"odd": ((37, 53), (41, 45), (20.0, 22.0, 26.0, 18.0), (15.0, 17.0, 22.0, 20.0)),        # fx != fy, tails on every side
         "ref": ((96, 128), (80, 96), (60.0, 60.0, 63.5, 47.5), (52.0, 52.0, 47.5, 39.5)),       # undistort samples everything
         "rim": ((96, 128), (80, 96), (5.0, 5.5, 63.5, 47.5), (30.0, 30.0, 47.5, 39.5)),         # the rim inside both frames
         "cap": ((96, 128), (1000, 1056), (60.0, 60.0, 63.5, 47.5), (560.0, 560.0, 527.5, 499.5))}   # 1 056 000 pixels > 4096 x 256


def frames(name, direction):
    """-> (source size, destination size) of a geometry in a direction."""
    pin_size, fish_size = GEOMS[name][:2]
    return (pin_size, fish_size) if direction == "distort" else (fish_size, pin_size)


@functools.lru_cache(maxsize=None)
def image_case(name, direction):
    """-> (source image, oracle image, sampled, margin), read-only."""
    (sh, sw), (dh, dw) = frames(name, direction)
    _, o = both(*GEOMS[name][2:])
    src = np.random.RandomState(sum(map(ord, name + direction))).randint(0, 256, (sh, sw, 3)).astype(np.uint8)
    out = (src,) + L.warp_image(src, o, direction, dh, dw)
    for a in out:
        a.setflags(write=False)
    return out


def test_the_images_cover_what_they_should():
    """The oracle's own view, asserted before anything is demanded from the GPU: each direction has sampled and filled pixels, a
    field rim crosses an image in each direction, one geometry samples everything, and next to nothing sits on a knife edge."""
    for direction in DIRECTIONS:
        shares = {}
        for name in ("odd", "ref", "rim"):
            _, out, sampled, margin = image_case(name, direction)
            shares[name] = float(sampled.mean())
            assert (margin <= MARGIN).mean() <= SHARE
            assert (out[~sampled] == 114).all()
        print(direction, shares)
        assert 0.0 < shares["rim"] < 1.0 and 0.0 < shares["odd"] <= 1.0
        assert any(0.0 < s < 1.0 for s in shares.values())
        # the rim crosses the "rim" images: pixels on both sides of it inside the frame
        (sh, sw), (dh, dw) = frames("rim", direction)
        _, o = both(*GEOMS["rim"][2:])
        oy, ox = np.mgrid[0:dh, 0:dw].astype(np.float64)
        rim = (L.to_pinhole if direction == "distort" else L.to_fisheye)(ox, oy, o)[2]
        assert (rim > 0).any() and (rim < 0).any()
    assert abs(image_case("ref", "distort")[2].mean() - 0.68) < 0.01 and image_case("ref", "undistort")[2].all()


def compare_image(got_u8, got_f32, out, margin, what):
    """Bit equality of every pixel off the knife edges, in both output forms."""
    firm = margin > MARGIN
    assert 1.0 - firm.mean() <= SHARE, what
    diff = (got_u8 != out).any(-1)
    print("%s: %d of %d pixels compared, %d differ (%d of them firm)" % (what, firm.sum(), firm.size, diff.sum(), (diff & firm).sum()))
    assert not (diff & firm).any(), what
    if got_f32 is not None:
        assert np.array_equal(got_f32, got_u8.transpose(2, 0, 1).astype(np.float32)), what + ": the fp32 form is not float(uint8)"


# the grid cap is one code path of both directions: its large destination is the fisheye frame, so it runs as "distort"
@pytest.mark.parametrize("name,direction", [(n, d) for n in ("odd", "ref", "rim") for d in DIRECTIONS] + [("cap", "distort")])
def test_images_against_the_restatement(name, direction):
    from ep24 import lens
    m, _ = both(*GEOMS[name][2:])
    src, out, sampled, margin = image_case(name, direction)
    dst = frames(name, direction)[1]
    got = lens.warp_images([src], m, direction, dst)
    assert len(got) == 1 and got[0].dtype == torch.uint8 and tuple(got[0].shape) == dst + (3,) and got[0].is_cuda
    f32 = lens.preproc_images([torch.from_numpy(src.copy())], m, direction, dst)
    assert f32.dtype == torch.float32 and tuple(f32.shape) == (1, 3) + dst
    compare_image(got[0].cpu().numpy(), f32[0].cpu().numpy(), out, margin, "%s %s" % (name, direction))


@pytest.mark.parametrize("direction", DIRECTIONS)
def test_a_batch_of_three_sizes_one_of_them_all_fill(direction):
    """One launch for three images of different source and destination sizes and three models; the middle one looks past its source
    (principal point far outside): all fill, here 7.  Then the fp32 form with one destination size, and empty batches."""
    from ep24 import lens
    names = ("odd", "rim", "ref")
    models = [both(*GEOMS[n][2:])[0] for n in names]
    away = both((20.0, 20.0, -900.0, 18.0), (15.0, 15.0, 22.0, -700.0))
    models[1] = away[0]
    cases = [image_case(n, direction) for n in names]
    srcs = [c[0] for c in cases]
    dsts = [frames(n, direction)[1] for n in names]
    got = lens.warp_images(srcs, models, direction, dsts, fill=7)
    assert [tuple(g.shape[:2]) for g in got] == dsts
    want1, sampled1, _ = L.warp_image(srcs[1], away[1], direction, *dsts[1], fill=7)
    assert not sampled1.any() and (want1 == 7).all()
    assert bool((got[1] == 7).all())
    for i in (0, 2):
        src, out, sampled, margin = cases[i]
        g = got[i].cpu().numpy()
        assert (g[~sampled & (margin > MARGIN)] == 7).all()
        firm = sampled & (margin > MARGIN)
        assert np.array_equal(g[firm], out[firm]), names[i]
    S = (48, 64)
    f32 = lens.preproc_images(srcs, models, direction, S, fill=7)
    u8 = lens.warp_images(srcs, models, direction, S, fill=7)
    for i in range(3):
        assert torch.equal(f32[i], u8[i].permute(2, 0, 1).float())
    assert bool((f32[1] == 7).all())
    assert lens.warp_images([], [], direction, S) == [] and lens.warp_images([], models[0], direction, []) == []
    assert tuple(lens.preproc_images([], models[0], direction, S).shape) == (0, 3) + S


# ------------------------------------------------------------------------------------------------------------------------ labels
def arc_band(h, w, cx, cy, r_out, r_in, cls=7):
    """A half ring, open towards -y: 12 vertices on the outer arc, 12 back on the inner one.  The middle of its box lies in the hollow;
    the row's own centre is a point of the band."""
    a = np.linspace(0.0, np.pi, 12)
    x = np.concatenate([cx + r_out * np.cos(a), cx + r_in * np.cos(a[::-1])])
    y = np.concatenate([cy + r_out * np.sin(a), cy + r_in * np.sin(a[::-1])])
    row = np.zeros(51)
    row[0], row[1], row[2] = cls, (cx + 3.0) / w, (cy + (r_out + r_in) / 2) / h
    row[3::2], row[4::2] = x / w, y / h
    return row


def blob_at(rng, h, w, cx, cy, rmin, rmax):
    """One blob row moved so that its centre stands at (cx, cy) of the h x w image (it may hang over the image's edge)."""
    row = F.blob_rows(rng, 1, h, w, rmin, rmax)[0]
    row[1::2] += cx / w - row[1]
    row[2::2] += cy / h - row[2]
    return row


# Seven images per direction.  The rows live in the SOURCE frame of the direction (distort: the pinhole frame).  The pinhole frame
# stretches without bound towards the rim, so the fisheye frames of "undistort" cover a moderate angle only (corner below 0.9 rad) and
# their pinhole frames are twice as large.
#             rows  source     destination  pin (fx, fy, cx, cy)            fish (fx, fy, cx, cy)           fov
LABEL_SCENE = {
    "distort": [(3, (96, 128), (80, 96), (60.0, 60.0, 63.5, 47.5), (52.0, 52.0, 47.5, 39.5), 170.0),          # a tiny object between two others: dropped
                (0, (120, 90), (100, 80), (50.0, 50.0, 44.5, 59.5), (40.0, 40.0, 39.5, 49.5), 170.0),         # no labels, between two images with some
                (5, (240, 320), (200, 260), (150.0, 150.0, 159.5, 119.5), (120.0, 120.0, 129.5, 99.5), 170.0),   # one lands on the top edge: clamped
                (1, (200, 300), (180, 260), (140.0, 140.0, 149.5, 99.5), (125.0, 125.0, 129.5, 89.5), 170.0),    # the crafted half ring: the flag bit
                (4, (128, 128), (128, 128), (30.0, 30.0, 63.5, 63.5), (52.0, 52.0, 63.5, 63.5), 120.0),          # one object straddles the rim
                (50, (320, 320), (320, 320), (200.0, 200.0, 159.5, 159.5), (170.0, 170.0, 159.5, 159.5), 170.0),
                (53, (320, 256), (300, 240), (180.0, 180.0, 127.5, 159.5), (150.0, 150.0, 119.5, 149.5), 170.0)],  # more than max_labels: 50 are read
    "undistort": [(3, (80, 96), (160, 192), (70.0, 70.0, 95.5, 79.5), (70.0, 70.0, 47.5, 39.5), 170.0),
                  (0, (100, 80), (200, 160), (75.0, 75.0, 79.5, 99.5), (75.0, 75.0, 39.5, 49.5), 170.0),
                  (5, (200, 260), (400, 520), (190.0, 190.0, 259.5, 199.5), (190.0, 190.0, 129.5, 99.5), 170.0),
                  (1, (180, 260), (360, 520), (180.0, 180.0, 259.5, 179.5), (180.0, 180.0, 129.5, 89.5), 170.0),
                  (4, (128, 128), (128, 128), (30.0, 30.0, 63.5, 63.5), (52.0, 52.0, 63.5, 63.5), 120.0),
                  (50, (320, 320), (640, 640), (260.0, 260.0, 319.5, 319.5), (260.0, 260.0, 159.5, 159.5), 170.0),
                  (53, (320, 256), (640, 512), (240.0, 240.0, 255.5, 319.5), (240.0, 240.0, 127.5, 159.5), 170.0)]}


@functools.lru_cache(maxsize=None)
def label_scene(direction, max_labels=50):
    """-> (targets, source sizes, LensModels, destination sizes, oracle table, counts, flags, margins, infos), read-only."""
    rng = np.random.RandomState(11 if direction == "distort" else 12)
    back = L.to_pinhole if direction == "distort" else L.to_fisheye          # from the destination frame to the source frame
    targets, sizes, models, omodels, dsts = [], [], [], [], []
    for k, (h, w), dst, pin, fish, fov in LABEL_SCENE[direction]:
        f, fd = (pin, fish) if direction == "distort" else (fish, pin)
        m, o = both(pin, fish, K, fov)
        big = min(h, w) / 6.0
        rows = F.blob_rows(rng, k, h, w, big / 3.0, big) if k < 50 else F.blob_rows(rng, k, h, w, 5.0, 12.0)
        if k == 3:
            rows[1] = F.blob_rows(rng, 1, h, w, 0.04, 0.05)[0]
        if k == 5:                                                         # the source point that lands on the destination's top edge
            sx, sy, _ = back(np.array([fd[2] + 20.0]), np.array([1.5]), o)
            rows[2] = blob_at(rng, h, w, float(sx[0]), float(sy[0]), 9.0, 12.0)
        if k == 1:
            rows[0] = arc_band(h, w, f[2] + 10.0, f[3] - 20.0, 60.0, 45.0)
        if k == 4:                                                         # three objects near the middle, the fourth centred on the rim
            rows = F.blob_rows(rng, k, h // 2, w // 2, 5.0, 9.0)
            rows[:, 1::2], rows[:, 2::2] = rows[:, 1::2] / 2 + 0.25, rows[:, 2::2] / 2 + 0.25
            rim = (math.tan(o["theta_max"]) if direction == "distort" else L.thetad(o["theta_max"], K)) * f[0]
            rows[3] = blob_at(rng, h, w, f[2] + rim * math.cos(0.6), f[3] + rim * math.sin(0.6), 7.0, 8.0)
        targets.append(rows)
        sizes.append((h, w))
        models.append(m)
        omodels.append(o)
        dsts.append(dst)
    for a in targets:
        a.setflags(write=False)
    return (targets, sizes, models, dsts) + L.warp_labels(targets, sizes, omodels, direction, dsts, max_labels)


@pytest.mark.parametrize("direction", DIRECTIONS)
def test_the_label_scene_covers_what_it_should(direction):
    """The oracle's own view of the scene: no decision on a knife edge, the tiny object dropped, the crafted one flagged, one clamped
    at a border, one with outline points on both sides of the field's rim, 50 of 53 read."""
    _, _, _, dsts, table, counts, flags, margins, infos = label_scene(direction)
    print(direction, "oracle margins:", margins, "counts:", counts.tolist())
    assert min(margins.values()) > 1e-6
    assert counts.tolist() == [2, 0, 5, 1, 4, 50, 50]
    assert infos[0][1]["dropped"] and sum(i["dropped"] for img in infos for i in img) == 1
    assert flags[3, 0] == 1 and flags.sum() == 1
    assert infos[2][2]["clamped"] and not infos[2][2]["dropped"]
    assert (table[2, 2, 4::2] == 0).any() and (table[2, 2, 4::2] > 0).any()       # clamped to the top edge
    assert infos[4][3]["rim_min"] < 0 < infos[4][3]["rim_max"] and not infos[4][3]["dropped"]
    assert sum(i["rim_min"] < 0 for img in infos for i in img) == 1
    assert len(infos[6]) == 50
    assert np.abs(table[..., 1:]).max() < 2048                                   # the fp32 rounding the tolerance assumes
    for i, (oh, ow) in enumerate(dsts):
        assert table[i, :, 3::2].max() <= ow and table[i, :, 4::2].max() <= oh


def check_labels(got, table, counts, flags):
    labels, got_counts, got_flags = got
    n, ml = table.shape[:2]
    assert labels.dtype == torch.float32 and tuple(labels.shape) == (n, ml, 51) and labels.is_cuda
    assert got_counts.dtype == torch.int32 and got_flags.dtype == torch.int32 and tuple(got_flags.shape) == (n, ml)
    assert got_counts.cpu().numpy().tolist() == counts.tolist()
    assert np.array_equal(got_flags.cpu().numpy(), flags)
    labels = labels.cpu().numpy()
    assert np.array_equal(labels[..., 0], table[..., 0])
    err = np.abs(labels.astype(np.float64) - table.astype(np.float64)).max()
    print("max |difference| %.3g px" % err)
    assert err <= 1e-3
    for i, c in enumerate(counts):
        assert not labels[i, c:].any()


@pytest.mark.parametrize("direction", DIRECTIONS)
def test_warp_labels_against_the_restatement(direction):
    """Counts, flags and classes equal; coordinates within 1e-3 px: the fp32 rounding of a value below 2048 is <= 1.3e-4, the rest is
    double; the tail of every table zero."""
    from ep24 import lens
    targets, sizes, models, dsts, table, counts, flags, margins, _ = label_scene(direction)
    assert min(margins.values()) > 1e-6
    check_labels(lens.warp_labels(targets, sizes, models, direction, dsts, 50), table, counts, flags)


@pytest.mark.parametrize("direction", DIRECTIONS)
def test_warp_labels_other_max_labels_and_scales(direction):
    """max_labels that is no multiple of the four rows of a workgroup and smaller than an image's rows; a scale per image."""
    from ep24 import lens
    targets, sizes, models, dsts = label_scene(direction)[:4]
    omodels = [L.model(m.pin, m.fish, m.k, m.fov_deg) for m in models]
    scales = [1.0, 2.0, 0.5, 1.25, 1.5, 0.75, 3.0]
    table, counts, flags, margins, _ = L.warp_labels(targets, sizes, omodels, direction, dsts, 7, scales)
    assert min(margins.values()) > 1e-6 and table[..., 1:].max() < 2048 and counts.max() == 7
    check_labels(lens.warp_labels(targets, sizes, models, direction, dsts, 7, scales=scales), table, counts, flags)
    empty = lens.warp_labels([], [], [], direction, (64, 64), 50)
    assert tuple(empty[0].shape) == (0, 50, 51) and tuple(empty[1].shape) == (0,)


def test_warp_labels_is_deterministic():
    from ep24 import lens
    targets, sizes, models, dsts = label_scene("distort")[:4]
    a = lens.warp_labels(targets, sizes, models, "distort", dsts, 50)
    b = lens.warp_labels(targets, sizes, models, "distort", dsts, 50)
    out = torch.full((7, 50, 51), float("nan"), dtype=torch.float32, device=DEV)
    c = lens.warp_labels(targets, sizes, models, "distort", dsts, 50, out=out)
    assert c[0] is out
    for x, y, z in zip(a, b, c):
        assert torch.equal(x, y) and torch.equal(x, z)


# ----------------------------------------------------------------------------------------------------------------- the transform
def test_lens_transform_through_a_prefetcher():
    """Images and labels are those of direct ``preproc_images`` / ``warp_labels`` calls with the same draws; a second transform at the
    same position reproduces them; more than one model is drawn in a batch."""
    from ep24 import lens
    from ep24.input import DataPrefetcher
    from ep24.lens import LensModel
    rng = np.random.RandomState(3)
    sizes, S = [(48, 64), (64, 96), (64, 64), (40, 40)], (64, 96)
    models = [LensModel((60.0, 60.0, 63.5, 47.5), (52.0, 52.0, 47.5, 39.5), K, 170.0, size=(80, 96)),
              LensModel.equidistant((64, 96), (64, 96), 140.0),
              LensModel((40.0, 42.0, 47.5, 31.5), (33.0, 35.0, 47.5, 31.5), K, 150.0)]                  # no size: taken as given
    batches = []
    for _ in range(2):
        images = [rng.randint(0, 256, (h, w, 3)).astype(np.uint8) for h, w in sizes]
        targets = [F.blob_rows(rng, k, h, w, 4.0, 9.0) for k, (h, w) in zip((2, 0, 3, 1), sizes)]
        batches.append((images, targets, None, None))
    tf = lens.LensTransform(models, seed=9)
    tf.set_position(2, 5)
    twin = lens.LensTransform(models, seed=9)
    twin.set_position(2, 5)
    pf = DataPrefetcher(batches, S, tf)
    drawn = set()
    for images, targets, _, _ in batches:
        choices = twin.sample(len(images))
        drawn.update(choices)
        per_image = twin.models_for(choices, sizes, S)
        assert per_image[0].fish != models[choices[0]].fish or models[choices[0]].size in (None, S)    # scaled to the call's size
        got_images, got_labels = pf.next()
        torch.cuda.synchronize()
        want_images = lens.preproc_images(images, per_image, "distort", S)
        want_labels, want_counts, _ = lens.warp_labels(targets, sizes, per_image, "distort", S, 50)
        assert len(set(choices)) > 1
        assert tuple(got_images.shape) == (4, 3) + S and torch.equal(got_images, want_images) and torch.equal(got_labels, want_labels)
        assert bool((got_images != 114).any()) and int(want_counts.sum()) > 0
    assert pf.next() == (None, None)
    assert len(drawn) > 1
    again = lens.LensTransform(models, seed=9)
    again.set_position(2, 5)
    first = again.batch(*batches[0][:2], S)
    twin.set_position(2, 5)
    assert again.last_choices == twin.sample(4)
    assert torch.equal(first[0], lens.preproc_images(batches[0][0], again.models_for(again.last_choices, sizes, S), "distort", S))
    again.set_position(2, 5)
    second = again.batch(*batches[0][:2], S)
    assert torch.equal(first[0], second[0]) and torch.equal(first[1], second[1])
    again.set_position(2, 6)
    twin.set_position(2, 5)
    assert again.sample(64) != twin.sample(64)


def test_trainer_takes_fisheye_lens_files(tmp_path):
    """``train_24p.py --synthetic --fisheye-lens A.json B.json --steps 2`` on a tiny Exp: the batches the step receives are those of a
    ``LensTransform`` of the two files at the same data positions, and they differ from the plain source."""
    import os
    import sys
    from ep24 import lens
    from ep24.lens import LensModel
    Y24 = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "exploration-of-potential_amd", "yolox_24p")
    files = [str(tmp_path / "a.json"), str(tmp_path / "b.json")]
    LensModel((300.0, 300.0, 159.5, 159.5), (110.0, 110.0, 159.5, 159.5), K, 170.0).to_json(files[0])              # no size: the Exp's
    LensModel((600.0, 600.0, 319.5, 319.5), (260.0, 250.0, 319.5, 319.5), K, 160.0, size=(640, 640)).to_json(files[1])
    sys.path.insert(0, Y24)
    try:
        import importlib
        mod = importlib.import_module("train_24p")
        from exp import get_exp
        exp = get_exp(os.path.join(Y24, "load_train", "yolox_24p_train.py"))
        exp.width, exp.input_size, exp.synthetic_len, exp.synthetic_gts = 0.25, (320, 320), 8, 4
        exp.max_epoch, exp.no_aug_epochs = 1, 0
        seen = []
        plain_preprocess = exp.preprocess

        def recording(inputs, targets, tsize):
            seen.append((inputs.clone(), targets.clone()))
            return plain_preprocess(inputs, targets, tsize)

        exp.preprocess = recording
        args = mod.make_parser().parse_args(["-b", "4", "-l", "0.01", "--synthetic", "--fisheye-lens"] + files + [
            "--augment-seed", "5", "--steps", "2", "--log-interval", "1", "--loader-workers", "0", "--output-dir", str(tmp_path)])
        trainer = mod.main(exp, args)
        torch.cuda.synchronize()
        assert trainer.run_steps == 2 and len(seen) == 2 and isinstance(trainer.transform, lens.LensTransform)
        assert trainer.ring_timeouts() == 0
        assert [m.size for m in trainer.transform.models] == [(320, 320), (640, 640)]
        twin = lens.LensTransform([LensModel.from_json(files[0]), LensModel.from_json(files[1])], seed=5)
        twin.models[0].size = (320, 320)
        for it, (img, lab) in enumerate(seen):
            items = [exp.dataset[4 * it + j] for j in range(4)]
            twin.set_position(0, it)
            want = twin.batch([x[0] for x in items], [x[1] for x in items], (320, 320))
            assert torch.equal(img, want[0]) and torch.equal(lab, want[1])
            assert bool(torch.isfinite(lab).all()) and bool(lab.any()) and bool((img != 114).any()) and bool((img == 114).any())
    finally:
        sys.path.remove(Y24)


# --------------------------------------------------------------------------------------------------------------- bad arguments
def test_bad_arguments_launch_nothing():
    from ep24 import _lib, lens
    from ep24._lib import call, ptr, stream_ptr
    from ep24.augment import _rot
    m, _ = both((60.0, 60.0, 63.5, 47.5), (52.0, 52.0, 47.5, 39.5))
    tab = m.table()
    pts = torch.zeros(4, 2, dtype=torch.float64, device=DEV)
    out = torch.full((4, 2), -7.0, dtype=torch.float64, device=DEV)
    good = (ptr(pts), 4, tab.ctypes.data, 0, ptr(out))
    for i, bad in ((0, None), (4, None), (2, None), (1, -1), (3, 2), (3, -1)):
        args = list(good)
        args[i] = bad
        with pytest.raises(_lib.Ep24Error, match="lens_points"):
            call("lens_points", *args, stream_ptr())
    for i, v in ((0, 0.0), (5, -1.0), (12, 1.6), (12, 0.0), (9, float("nan")), (13, float("inf"))):
        t = tab.copy()
        t[i] = v
        with pytest.raises(_lib.Ep24Error, match="lens_points"):
            call("lens_points", ptr(pts), 4, t.ctypes.data, 0, ptr(out), stream_ptr())
    call("lens_points", None, 0, None, 0, None, stream_ptr())                            # nothing to do is not an error
    torch.cuda.synchronize()
    assert bool((out == -7.0).all())

    # the image launches
    src = torch.zeros(8 * 8 * 3, dtype=torch.uint8, device=DEV)
    desc = torch.tensor([[0, 8, 8]], dtype=torch.int64, device=DEV)
    table = torch.from_numpy(np.concatenate([tab, [0, 8, 8, 0]])).to(DEV)
    u8 = torch.full((8, 8, 3), 9, dtype=torch.uint8, device=DEV)
    f32 = torch.full((1, 3, 8, 8), -7.0, dtype=torch.float32, device=DEV)
    good = (ptr(src), ptr(desc), ptr(table), 1, 64, ptr(u8), 114)
    for i, bad in ((0, None), (1, None), (2, None), (5, None), (3, -1), (3, 65536), (4, 0), (6, 256), (6, -1)):
        args = list(good)
        args[i] = bad
        with pytest.raises(_lib.Ep24Error, match="lens_warp_u8"):
            call("lens_warp_u8", *args, stream_ptr())
    good = (ptr(src), ptr(desc), ptr(table), 1, ptr(f32), 8, 8, 114)
    for i, bad in ((0, None), (1, None), (2, None), (4, None), (3, -1), (3, 65536), (5, 0), (6, -8), (7, 300), (5, 1 << 30)):
        args = list(good)
        args[i] = bad
        with pytest.raises(_lib.Ep24Error, match="lens_preproc_u8"):
            call("lens_preproc_u8", *args, stream_ptr())
    call("lens_warp_u8", None, None, None, 0, 0, None, 114, stream_ptr())
    call("lens_preproc_u8", None, None, None, 0, None, 8, 8, 114, stream_ptr())
    img = np.zeros((8, 8, 3), dtype=np.uint8)
    for bad_images in ([img.astype(np.float32)], [img[..., 0]], [img[:, :, :2]], [torch.zeros(8, 8, 3, dtype=torch.int16)]):
        with pytest.raises(ValueError, match="uint8"):
            lens.warp_images(bad_images, m, "distort", (8, 8))
        with pytest.raises(ValueError, match="uint8"):
            lens.preproc_images(bad_images, m, "distort", (8, 8), out=f32)
    with pytest.raises(ValueError, match="lens models"):
        lens.warp_images([img, img], [m], "distort", (8, 8))
    with pytest.raises(ValueError, match="sizes"):
        lens.warp_images([img, img], m, "distort", [(8, 8)])
    with pytest.raises(ValueError, match="direction"):
        lens.warp_images([img], m, "sideways", (8, 8))
    with pytest.raises(ValueError, match="fill"):
        lens.preproc_images([img], m, "distort", (8, 8), fill=300, out=f32)
    for bad_out in (torch.full((1, 3, 8, 16), -7.0, device=DEV)[..., ::2], torch.full((1, 3, 8, 8), -7.0, dtype=torch.float64, device=DEV),
                    torch.full((2, 3, 8, 8), -7.0, device=DEV)):
        with pytest.raises(ValueError, match="contiguous fp32"):
            lens.preproc_images([img], m, "distort", (8, 8), out=bad_out)
        assert bool((bad_out == -7.0).all())
    torch.cuda.synchronize()
    assert bool((u8 == 9).all()) and bool((f32 == -7.0).all())

    # the label launches
    n, ml = 2, 4
    dbl = torch.zeros(n * 22 + 51, dtype=torch.float64, device=DEV)
    cand = torch.empty(n, ml, 51, dtype=torch.float32, device=DEV)
    keep = torch.empty(n, ml, dtype=torch.int32, device=DEV)
    lab = torch.full((n, ml, 51), -7.0, dtype=torch.float32, device=DEV)
    cnt = torch.full((n,), -7, dtype=torch.int32, device=DEV)
    flg = torch.full((n, ml), -7, dtype=torch.int32, device=DEV)
    good = (ptr(dbl, n * 22), ptr(dbl), ptr(_rot(torch.device(DEV))), n, ml, ptr(cand), ptr(keep), ptr(lab), ptr(cnt), ptr(flg))
    for i, bad in ((0, None), (1, None), (2, None), (5, None), (6, None), (7, None), (8, None), (9, None), (3, -1), (3, 65536), (4, 0),
                   (4, -2)):
        args = list(good)
        args[i] = bad
        with pytest.raises(_lib.Ep24Error, match="lens_labels"):
            call("lens_labels", *args, stream_ptr())
    call("lens_labels", None, None, None, 0, ml, None, None, None, None, None, stream_ptr())
    rows = F.blob_rows(np.random.RandomState(0), 2, 8, 8, 1.0, 2.0)
    nan_rows = rows.copy()
    nan_rows[1, 7] = float("nan")
    with pytest.raises(ValueError, match="non-finite"):
        lens.warp_labels([rows, nan_rows], [(8, 8)] * 2, m, "distort", (8, 8), ml, out=lab)
    with pytest.raises(ValueError, match="sizes"):
        lens.warp_labels([rows, rows], [(8, 8)], m, "distort", (8, 8), ml, out=lab)
    with pytest.raises(ValueError, match="lens models"):
        lens.warp_labels([rows, rows], [(8, 8)] * 2, [m], "distort", (8, 8), ml, out=lab)
    with pytest.raises(ValueError, match="scales"):
        lens.warp_labels([rows, rows], [(8, 8)] * 2, m, "distort", (8, 8), ml, out=lab, scales=[1.0])
    with pytest.raises(ValueError, match="contiguous fp32"):
        lens.warp_labels([rows, rows], [(8, 8)] * 2, m, "distort", (8, 8), ml, out=lab.double())
    with pytest.raises(ValueError, match="contiguous fp32"):
        lens.warp_labels([rows, rows], [(8, 8)] * 2, m, "distort", (8, 8), ml, out=torch.full((n, ml, 102), -7.0, device=DEV)[..., ::2])
    with pytest.raises(ValueError, match="max_labels"):
        lens.warp_labels([rows, rows], [(8, 8)] * 2, m, "distort", (8, 8), 0)
    torch.cuda.synchronize()
    assert bool((lab == -7.0).all()) and bool((cnt == -7).all()) and bool((flg == -7).all())
    # the same table with no rows at all: every image comes out empty
    call("lens_labels", *good, stream_ptr())
    torch.cuda.synchronize()
    assert not lab.any() and not cnt.any() and not flg.any()
