"""CPU half of the augmentation tests: the numpy oracle (tests/augment_oracle.py) against closed forms, the decision margins
of the seeded cases that tests/test_gpu_augment.py demands equality on, and the host API (``sample_params``, ``--augment``)."""
import math
import os
import sys

import numpy as np
import pytest
import torch

import augment_oracle as ao

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
Y24 = os.path.join(ROOT, "exploration-of-potential_amd", "yolox_24p")


def make_source(h, w, num_gt, seed, star=False):
    """A raw item as a decoder + txt reader hand it over: uint8 HWC image, label rows [k,51] normalised by width / height."""
    from ep24 import synth
    img = np.random.RandomState(seed).randint(0, 256, (h, w, 3)).astype(np.uint8)
    lab = synth.make_labels(1, [num_gt], size=(h, w), seed=seed + 1000, star=star)[0][:num_gt].double().numpy()
    lab[:, 1::2] /= float(w)
    lab[:, 2::2] /= float(h)
    return img, lab.reshape(-1, 51) if num_gt else np.zeros((0, 51))


# (h, w, objects, star): unequal source sizes, star objects, one image without labels
SOURCES = [(480, 640, 12, False), (360, 500, 12, True), (640, 480, 0, False), (333, 517, 12, True), (600, 600, 12, False),
           (240, 320, 3, False)]
INPUT_SIZE = (320, 416)                 # rectangular
MAX_LABELS = 6                          # small, so that a mosaic of 12-object sources has more survivors than rows
SEEDS = (7, 11)                         # the seeds of the GPU parity tests; their margins are asserted below


def seeded_case(seed, hsv=False):
    from ep24 import augment as aug
    items = [make_source(h, w, k, 100 * seed + 7 * j, star) for j, (h, w, k, star) in enumerate(SOURCES)]
    images, targets = [it[0] for it in items], [it[1] for it in items]
    params = aug.sample_params(aug.position_rng(seed, 0, 0), [im.shape[:2] for im in images], INPUT_SIZE, mosaic_prob=0.85)
    if not hsv:
        params.hsv_on[:] = False
    return images, targets, params


def simple_case(n=3, size=(256, 320)):
    items = [make_source(200 + 40 * j, 300 + 25 * j, 3 + j, 50 + j, star=j % 2 == 1) for j in range(n)]
    return [it[0] for it in items], [it[1] for it in items], size


def radii(table_row):
    return np.hypot(table_row[3::2] - table_row[1], table_row[4::2] - table_row[2])


# ------------------------------------------------------------------------------------------------ oracle vs closed forms

def test_identity_is_the_plain_transform():
    from ep24 import augment as aug
    from oracle import input as oin
    images, targets, size = simple_case()
    p = aug.identity_params(len(images))
    got, owner, margin = ao.sample_u8(images, p, size)
    table, counts, info = ao.augment_labels(targets, [im.shape[:2] for im in images], p, size)
    assert margin == 0.5
    for i, (im, tg) in enumerate(zip(images, targets)):
        w_img, w_lab = oin.train_transform(im, tg, size)
        assert np.array_equal(got[i], w_img)
        assert counts[i] == len(tg)
        assert np.abs(table[i] - w_lab).max() <= 1e-3
    assert all((h == 1).all() for h in info["hits"])


def test_mirror_only_reverses_the_rays():
    from ep24 import augment as aug
    images, targets, size = simple_case()
    p = aug.identity_params(len(images))
    base, _, _ = ao.sample_u8(images, p, size)
    plain, _, _ = ao.augment_labels(targets, [im.shape[:2] for im in images], p, size)
    p.mirror[:] = True
    got, _, _ = ao.sample_u8(images, p, size)
    table, counts, _ = ao.augment_labels(targets, [im.shape[:2] for im in images], p, size)
    assert np.array_equal(got, base[..., ::-1])
    for i, tg in enumerate(targets):
        assert counts[i] == len(tg)
        for j in range(len(tg)):
            assert abs(table[i, j, 1] - (size[1] - plain[i, j, 1])) <= 1e-3 and abs(table[i, j, 2] - plain[i, j, 2]) <= 1e-3
            old, new = radii(plain[i, j]), radii(table[i, j])
            np.testing.assert_allclose(new, old[(12 - np.arange(24)) % 24], atol=2e-3)


def _one_object(size=(640, 640), centre=(400.0, 300.0), star=False, seed=5):
    rs = np.random.RandomState(seed)
    r = rs.uniform(30, 90, 24)
    if star:
        r[1::2] *= 0.35
    row = np.zeros(51)
    row[0] = 7
    row[1], row[2] = centre[0] / size[1], centre[1] / size[0]
    row[3::2] = (centre[0] + r * ao.RAY[:, 0]) / size[1]
    row[4::2] = (centre[1] + r * ao.RAY[:, 1]) / size[0]
    return np.zeros((size[0], size[1], 3), dtype=np.uint8), row.reshape(1, 51), r


@pytest.mark.parametrize("star", [False, True])
def test_rotation_by_one_ray_shifts_the_radii(star):
    from ep24 import augment as aug
    size = (640, 640)
    img, rows, r = _one_object(size, star=star)
    p = aug.identity_params(1)
    # rotate by +15 degrees in image coordinates (x right, y down) about the object's centre: old ray k lands on ray k + 1
    c, s = math.cos(math.radians(15)), math.sin(math.radians(15))
    cx, cy = 400.0, 300.0
    p.set_matrix(0, [[c, -s, cx - (c * cx - s * cy)], [s, c, cy - (s * cx + c * cy)]])
    table, counts, info = ao.augment_labels([rows], [size], p, size)
    assert counts[0] == 1 and abs(table[0, 0, 1] - cx) <= 1e-3 and abs(table[0, 0, 2] - cy) <= 1e-3 and table[0, 0, 0] == 7
    np.testing.assert_allclose(radii(table[0, 0]), np.roll(r, 1), atol=2e-3)


def test_uniform_scale_halves_the_radii():
    from ep24 import augment as aug
    size = (640, 640)
    img, rows, r = _one_object(size, star=True)
    p = aug.identity_params(1)
    p.set_matrix(0, [[0.5, 0.0, 10.0], [0.0, 0.5, 20.0]])
    table, counts, _ = ao.augment_labels([rows], [size], p, size)
    assert counts[0] == 1 and abs(table[0, 0, 1] - 210.0) <= 1e-3 and abs(table[0, 0, 2] - 170.0) <= 1e-3
    np.testing.assert_allclose(radii(table[0, 0]), 0.5 * r, atol=2e-3)


def test_objects_whose_centre_leaves_are_dropped_and_rays_are_cut():
    from ep24 import augment as aug
    size = (640, 640)
    img, rows, r = _one_object(size, centre=(400.0, 300.0))
    p = aug.identity_params(1)
    p.set_matrix(0, [[1.0, 0.0, 300.0], [0.0, 1.0, 0.0]])            # centre to x = 700: outside the output
    assert ao.augment_labels([rows], [size], p, size)[1][0] == 0
    p.set_matrix(0, [[1.0, 0.0, 238.5], [0.0, 1.0, 0.0]])            # x = 638.5: inside, but closer than min_margin
    assert ao.augment_labels([rows], [size], p, size)[1][0] == 0
    assert ao.augment_labels([rows], [size], p, size, min_margin=1.0)[1][0] == 1
    p.set_matrix(0, [[1.0, 0.0, 220.0], [0.0, 1.0, 0.0]])            # x = 620: kept, the rays to the right end at the border
    table, counts, _ = ao.augment_labels([rows], [size], p, size)
    assert counts[0] == 1 and abs(radii(table[0, 0])[0] - 20.0) <= 1e-3 and table[0, 0, 3::2].max() <= 640.0 + 1e-4
    # a mosaic whose centre cuts the object off from its own tile: the top-left tile ends at xc
    p = aug.identity_params(1)
    p.mosaic[0], p.centre[0] = True, (390, 640)                      # tile 0 = [0,390) x [0,640): the centre x = 400 - 250 = 150
    table, counts, info = ao.augment_labels([rows], [size], p, size)
    assert counts[0] == 1 and abs(table[0, 0, 1] - 150.0) <= 1e-3      # padw = 390 - 640
    p.centre[0] = (245, 640)                                          # padw = -395: the centre lands at x = 5, tile = [0,245)
    table, counts, info = ao.augment_labels([rows], [size], p, size)
    assert counts[0] == 1 and table[0, 0, 3::2].min() >= -1e-4
    p.centre[0] = (241, 640)                                          # centre at x = 1 < min_margin
    assert ao.augment_labels([rows], [size], p, size)[1][0] == 0


def test_hsv_zero_gains_round_trip_and_known_colours():
    b, g, r = np.array([10.0, 200.0, 0.0, 114.0]), np.array([20.0, 100.0, 0.0, 114.0]), np.array([250.0, 50.0, 0.0, 114.0])
    b2, g2, r2 = ao.hsv_shift(b, g, r, 0, 0, 0)
    np.testing.assert_allclose(np.stack([b2, g2, r2]), np.stack([b, g, r]), atol=1e-9)
    # pure red, hue + 60 (H is half degrees: 30) -> yellow; value gain clips at 255
    b2, g2, r2 = ao.hsv_shift(np.array([0.0]), np.array([0.0]), np.array([255.0]), 30, 0, 40)
    np.testing.assert_allclose([b2[0], g2[0], r2[0]], [0.0, 255.0, 255.0], atol=1e-9)
    b2, g2, r2 = ao.hsv_shift(np.array([0.0]), np.array([0.0]), np.array([200.0]), -30, -255, 0)      # saturation to 0: grey
    np.testing.assert_allclose([b2[0], g2[0], r2[0]], [200.0, 200.0, 200.0], atol=1e-9)


# ------------------------------------------------------------------------------------------------ the GPU tests' seeds

@pytest.mark.parametrize("seed", SEEDS)
def test_seeded_cases_are_away_from_their_thresholds(seed):
    """What tests/test_gpu_augment.py compares for equality must not sit on a knife edge: centre margin, extent filter and
    pixel ownership are further than 1e-6 from their thresholds (float32 evaluation of the image coordinates is not required
    to agree), every re-cast ray meets exactly one edge, and the case covers what the issue lists."""
    images, targets, params = seeded_case(seed)
    sizes = [im.shape[:2] for im in images]
    _, owner, pix_margin = ao.sample_u8(images, params, INPUT_SIZE)
    table, counts, info = ao.augment_labels(targets, sizes, params, INPUT_SIZE, MAX_LABELS)
    print("seed %d: pixel margin %.3g, centre margin %.3g, extent margin %.3g, survivors %s" %
          (seed, pix_margin, info["centre_margin"], info["extent_margin"], counts.tolist()))
    assert pix_margin > 1e-6 and info["centre_margin"] > 1e-6 and info["extent_margin"] > 1e-6
    assert all((h == 1).all() for h in info["hits"]) and np.isfinite(table).all()
    assert params.mosaic.any() and counts.max() > MAX_LABELS and (owner >= 0).any() and (owner < 0).any()
    assert any(len(t) == 0 for t in targets) and len({s for s in sizes}) == len(sizes)


def test_seeded_cases_between_them_cover_mirror_plain_and_empty_images():
    got = {"mirror": False, "plain": False, "zero": False, "tiles": set()}
    for seed in SEEDS:
        images, targets, params = seeded_case(seed)
        _, owner, _ = ao.sample_u8(images, params, INPUT_SIZE)
        _, counts, _ = ao.augment_labels(targets, [im.shape[:2] for im in images], params, INPUT_SIZE, MAX_LABELS)
        got["mirror"] |= bool(params.mirror.any() and not params.mirror.all())
        got["plain"] |= bool((~params.mosaic).any())
        got["zero"] |= bool((counts == 0).any())
        got["tiles"] |= set(np.unique(owner[params.mosaic]).tolist())
    assert got["mirror"] and got["plain"] and got["zero"] and got["tiles"] >= {-1, 0, 1, 2, 3}, got


# ------------------------------------------------------------------------------------------------ host API

def test_sample_params_ranges_and_draw_order():
    from ep24 import augment as aug
    sizes, S = [(480, 640)] * 64, (320, 416)
    p = aug.sample_params(aug.position_rng(1, 2, 3), sizes, S)
    assert p.mosaic.all() and p.hsv_on.all() and 0 < p.mirror.sum() < 64                 # defaults: mosaic 1.0, hsv 1.0, flip 0.5
    assert (p.centre[:, 0] >= 208).all() and (p.centre[:, 0] < 624).all() and (p.centre[:, 1] >= 160).all() and (p.centre[:, 1] < 480).all()
    assert (p.partners[:, 0] == np.arange(64)).all() and (p.partners >= 0).all() and (p.partners < 64).all()
    assert (np.abs(p.M[:, 0, 2]) <= 41.6).all() and (np.abs(p.M[:, 1, 2]) <= 32.0).all()
    for i in range(64):
        A = p.M[i][:, :2]
        det = np.linalg.det(A)
        assert 0.2 < det < 2.4                                                             # scale in (0.5, 1.5), shear <= 2 degrees
        np.testing.assert_allclose(A @ p.Minv[i][:, :2], np.eye(2), atol=1e-12)
        np.testing.assert_allclose(A @ p.Minv[i][:, 2] + p.M[i][:, 2], 0, atol=1e-9)
    assert (p.hsv == np.trunc(p.hsv)).all() and (np.abs(p.hsv[:, 0]) <= 5).all() and (np.abs(p.hsv[:, 1:]) <= 30).all()
    assert (p.hsv == 0).any() and (p.hsv != 0).any()
    # the matrix is get_affine_matrix's: rotation * scale about the origin, then shear, then translation
    M = aug.affine_matrix(10.0, 1.25, 0.0, 0.0, 3.0, -4.0)
    a, b = 1.25 * math.cos(math.radians(10)), 1.25 * math.sin(math.radians(10))
    np.testing.assert_allclose(M, [[a, b, 3.0], [-b, a, -4.0]], atol=1e-15)
    M = aug.affine_matrix(0.0, 1.0, 2.0, -1.0, 0.0, 0.0)
    np.testing.assert_allclose(M, [[1.0, math.tan(math.radians(-1.0)), 0], [math.tan(math.radians(2.0)), 1.0, 0]], atol=1e-15)
    # same position, same parameters; another iteration, epoch or seed: others
    q = aug.sample_params(aug.position_rng(1, 2, 3), sizes, S)
    for k in ("mosaic", "centre", "partners", "M", "Minv", "mirror", "hsv_on", "hsv"):
        assert np.array_equal(getattr(p, k), getattr(q, k)), k
    for other in ((1, 2, 4), (1, 3, 3), (2, 2, 3)):
        assert not np.array_equal(aug.sample_params(aug.position_rng(*other), sizes, S).M, p.M)
    # draw order: 20 numbers per image whatever the coins say, so image i does not depend on the probabilities of the others
    off = aug.sample_params(aug.position_rng(1, 2, 3), sizes, S, mosaic_prob=0.0, flip_prob=0.0, hsv_prob=0.0)
    assert not off.mosaic.any() and not off.mirror.any() and not off.hsv_on.any()
    assert np.array_equal(off.M, aug.identity_params(64).M) and np.array_equal(off.hsv, p.hsv)
    rng2, rng3 = aug.position_rng(1, 2, 3), aug.position_rng(1, 2, 3)
    aug.sample_params(rng2, sizes[:5], S, mosaic_prob=0.9, flip_prob=0.1)
    aug.sample_params(rng3, sizes[:5], S, mosaic_prob=0.3, hsv_prob=0.0)
    assert rng2.random_sample() == rng3.random_sample()                                      # both generators are in the same state


def test_mosaic_transform_positions_and_no_cpu_fallback():
    from ep24 import augment as aug
    from ep24._lib import Ep24Error
    tr = aug.MosaicTransform(seed=5)
    sizes, S = [(100, 120)] * 4, (64, 96)
    tr.set_position(2, 7)
    a = tr.sample(sizes, S)
    tr.set_position(2, 8)
    b = tr.sample(sizes, S)
    tr.set_position(2, 7)
    c = tr.sample(sizes, S)
    assert np.array_equal(a.M, c.M) and np.array_equal(a.partners, c.partners) and not np.array_equal(a.M, b.M)
    assert tr.position == (2, 7)
    if not torch.cuda.is_available():
        img = np.zeros((100, 120, 3), dtype=np.uint8)
        for enabled in (True, False):
            tr.enabled = enabled
            with pytest.raises(Ep24Error):
                tr.batch([img], [np.zeros((0, 51))], S)
        with pytest.raises(Ep24Error):
            aug.mosaic_batch([img], [np.zeros((0, 51))], aug.identity_params(1), S)


def test_augment_flag_exp_attributes_and_reexport():
    sys.path.insert(0, Y24)
    try:
        import importlib
        mod = importlib.import_module("train_24p")
        assert mod.make_parser().parse_args([]).augment is False
        a = mod.make_parser().parse_args(["--augment", "--augment-seed", "4"])
        assert a.augment is True and a.augment_seed == 4
        from exp import get_exp
        exp = get_exp(os.path.join(Y24, "load_train", "yolox_24p_train.py"))
        assert (exp.mosaic_prob, exp.degrees, exp.translate, tuple(exp.mosaic_scale), exp.shear, exp.flip_prob, exp.hsv_prob) == \
            (1.0, 10.0, 0.1, (0.5, 1.5), 2.0, 0.5, 1.0)
        import datasets
        from ep24 import augment as aug
        assert datasets.MosaicTransform is aug.MosaicTransform and issubclass(aug.MosaicTransform, datasets.TrainTransform)
        tr = aug.MosaicTransform.from_exp(exp, seed=3)
        assert (tr.mosaic_prob, tr.degrees, tr.shear, tr.flip_prob, tr.seed, tr.enabled) == (1.0, 10.0, 2.0, 0.5, 3, True)
    finally:
        sys.path.remove(Y24)
