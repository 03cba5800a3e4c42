"""CPU half of the mixup tests: the numpy oracle (tests/mixup_oracle.py) against closed forms, the decision margins and the
coverage of the seeded cases that tests/test_gpu_mixup.py demands equality on, and the host API (``sample_mixup``, ``--mixup``)."""
import os
import sys

import numpy as np
import pytest

import augment_oracle as ao
import mixup_oracle as mo
from test_augment_oracle import INPUT_SIZE, MAX_LABELS, Y24, _one_object, radii, seeded_case, simple_case

MIX_SEEDS = (7, 11)                     # the seeds of the GPU parity tests; what they cover is asserted below
MIX_PROB = 0.7


def seeded_mix_case(seed, hsv=False):
    """``seeded_case(seed)`` with the mixup fields drawn by ``sample_mixup`` at the same position."""
    from ep24 import augment as aug
    images, targets, params = seeded_case(seed, hsv=hsv)
    aug.sample_mixup(aug.mixup_rng(seed, 0, 0), params, [im.shape[:2] for im in images], [len(t) for t in targets], INPUT_SIZE,
                     mixup_prob=MIX_PROB)
    return images, targets, params


def _mosaic_params(n):
    """Image 0 a mosaic of sources 0, 1, 2, 0 under a mild affine map; the others plain."""
    from ep24 import augment as aug
    p = aug.identity_params(n)
    p.mosaic[0], p.centre[0], p.partners[0] = True, (300, 260), (0, 1, 2, 0)
    p.set_matrix(0, aug.affine_matrix(4.0, 0.8, 1.0, -1.0, -60.0, -40.0))
    return p


def _set_mix(p, i, partner, jit=1.0, flip=False, off=(0, 0)):
    p.mixup[i], p.mix_partner[i], p.mix_jit[i], p.mix_flip[i], p.mix_off[i] = True, partner, jit, flip, off


# ------------------------------------------------------------------------------------------------ oracle vs closed forms

def test_unit_jitter_is_the_average_with_the_plain_letterbox():
    from oracle import input as oin
    images, targets, size = simple_case()
    sizes = [im.shape[:2] for im in images]
    p = _mosaic_params(len(images))
    a, _, _ = ao.sample_u8(images, p, size)
    own, own_counts, _ = ao.augment_labels(targets, sizes, p, size)
    _set_mix(p, 0, 1)
    got, cls, owner, _, mix_margin = mo.sample_u8(images, p, size)
    table, counts, info = mo.augment_labels(targets, sizes, p, size)
    w_img, w_lab = oin.train_transform(images[1], targets[1], size)
    assert mix_margin == 0.5                                                    # u = px exactly
    assert np.array_equal(got[0], ((a[0].astype(np.int64) + w_img.astype(np.int64)) >> 1).astype(np.float32))
    assert np.array_equal(got[1:], a[1:]) and (cls[1:] != mo.PARTNER).all()
    assert not (cls[0] == mo.BLACK).any() and (cls[0] == mo.PARTNER).any() and (cls[0] == mo.TILE).any()
    k0, k1 = int(own_counts[0]), len(targets[1])
    assert 0 < k0 and k0 + k1 <= 50 and counts[0] == k0 + k1 and info["partner_kept"][0] == k1
    assert np.array_equal(table[0, :k0], own[0, :k0])                            # the image's own rows first, untouched
    assert np.abs(table[0, k0:k0 + k1] - w_lab[:k1]).max() <= 1e-3               # then the partner's, as the plain transform has them
    assert not table[0, k0 + k1:].any()
    assert np.array_equal(table[1:], own[1:]) and np.array_equal(counts[1:], own_counts[1:])


def _object_case(centre=(400.0, 300.0)):
    """Two 640 x 640 sources on a 640 x 640 input (letterbox scale 1): a noise image without labels and a black one with one
    object.  Image 0 is plain; the tests blend source 1 into it."""
    from ep24 import augment as aug
    size = (640, 640)
    img, rows, r = _one_object(size, centre=centre, star=True)
    noise = np.random.RandomState(3).randint(0, 256, (640, 640, 3)).astype(np.uint8)
    return [noise, img], [np.zeros((0, 51)), rows], aug.identity_params(2), size, r


def test_half_jitter_leaves_black_outside_and_halves_the_radii():
    images, targets, p, size, r = _object_case()
    a, _, _ = ao.sample_u8(images, p, size)
    _set_mix(p, 0, 1, jit=0.5)
    got, cls, _, _, _ = mo.sample_u8(images, p, size)
    ys, xs = np.mgrid[0:640, 0:640]
    outside = (xs >= 320) | (ys >= 320)
    assert np.array_equal(got[0][:, outside], (a[0][:, outside].astype(np.int64) >> 1).astype(np.float32))
    assert np.array_equal(got[0][:, ~outside], (a[0][:, ~outside].astype(np.int64) >> 1).astype(np.float32))   # the partner is black
    assert (cls[0][~outside] == mo.PARTNER).all() and (cls[0][outside] == mo.TILE).all()
    table, counts, _ = mo.augment_labels(targets, [(640, 640)] * 2, p, size)
    assert counts[0] == 1 and abs(table[0, 0, 1] - 200.0) <= 1e-3 and abs(table[0, 0, 2] - 150.0) <= 1e-3 and table[0, 0, 0] == 7
    np.testing.assert_allclose(radii(table[0, 0]), 0.5 * r, atol=2e-3)


def test_flip_mirrors_the_centre_and_reverses_the_rays():
    images, targets, p, size, r = _object_case()
    _set_mix(p, 0, 1, jit=1.0, flip=True)
    table, counts, _ = mo.augment_labels(targets, [(640, 640)] * 2, p, size)
    assert counts[0] == 1 and abs(table[0, 0, 1] - (640.0 - 400.0)) <= 1e-3 and abs(table[0, 0, 2] - 300.0) <= 1e-3
    np.testing.assert_allclose(radii(table[0, 0]), r[(12 - np.arange(24)) % 24], atol=2e-3)
    # pixels: the partner's columns reversed
    images[1] = np.random.RandomState(4).randint(0, 256, (640, 640, 3)).astype(np.uint8)
    a, _, _ = ao.sample_u8(images, p, size)
    got, _, _, _, _ = mo.sample_u8(images, p, size)
    want = (a[0].astype(np.int64) + images[1].transpose(2, 0, 1)[:, :, ::-1].astype(np.int64)) >> 1
    assert np.array_equal(got[0], want.astype(np.float32))
    # with the jitter too: Wj = 480, the centre goes to 0.75 * 400 = 300 and then to 480 - 300
    _set_mix(p, 0, 1, jit=0.75, flip=True)
    table, counts, _ = mo.augment_labels(targets, [(640, 640)] * 2, p, size)
    assert counts[0] == 1 and abs(table[0, 0, 1] - 180.0) <= 1e-3 and abs(table[0, 0, 2] - 225.0) <= 1e-3
    np.testing.assert_allclose(radii(table[0, 0]), 0.75 * r[(12 - np.arange(24)) % 24], atol=2e-3)


def test_crop_drops_objects_whose_centre_leaves_and_cuts_rays_at_the_border():
    images, targets, p, size, r = _object_case(centre=(100.0, 300.0))
    sizes = [(640, 640)] * 2
    _set_mix(p, 0, 1, jit=1.5, off=(0, 0))                                       # Wj = Hj = 960: the centre goes to (150, 450)
    table, counts, _ = mo.augment_labels(targets, sizes, p, size)
    assert counts[0] == 1 and abs(table[0, 0, 1] - 150.0) <= 1e-3 and abs(table[0, 0, 2] - 450.0) <= 1e-3
    np.testing.assert_allclose(radii(table[0, 0]), 1.5 * r, atol=3e-3)
    _set_mix(p, 0, 1, jit=1.5, off=(200, 0))                                     # x = -50: cropped away
    assert mo.augment_labels(targets, sizes, p, size)[1][0] == 0
    _set_mix(p, 0, 1, jit=1.5, off=(149, 0))                                     # x = 1: inside, but closer than min_margin
    assert mo.augment_labels(targets, sizes, p, size)[1][0] == 0
    assert mo.augment_labels(targets, sizes, p, size, min_margin=0.5)[1][0] == 1
    _set_mix(p, 0, 1, jit=1.5, off=(130, 200))                                   # (20, 250): kept, the rays to the left end at x = 0
    table, counts, _ = mo.augment_labels(targets, sizes, p, size)
    assert counts[0] == 1 and abs(table[0, 0, 1] - 20.0) <= 1e-3 and abs(table[0, 0, 2] - 250.0) <= 1e-3
    assert 1.5 * r[12] > 20.0 and abs(radii(table[0, 0])[12] - 20.0) <= 1e-3 and table[0, 0, 3::2].min() >= -1e-4
    np.testing.assert_allclose(radii(table[0, 0])[0], 1.5 * r[0], atol=3e-3)     # the ray to the right is not cut
    # the image's final mirror applies to the partner's rows as to all others
    p.mirror[0] = True
    table, counts, _ = mo.augment_labels(targets, sizes, p, size)
    assert counts[0] == 1 and abs(table[0, 0, 1] - 620.0) <= 1e-3 and abs(radii(table[0, 0])[0] - 20.0) <= 1e-3
    # pixels of that case: black beyond the jittered canvas does not occur (960 - 130 > 640), the crop shifts the partner
    got, cls, _, _, _ = mo.sample_u8(images, p, size)
    assert not (cls[0] == mo.BLACK).any()


def test_empty_jittered_canvas_is_an_error():
    from ep24 import augment as aug
    images, targets, p, size, _ = _object_case()
    _set_mix(p, 0, 1, jit=0.001)
    with pytest.raises(ValueError):
        mo.sample_u8(images, p, size)
    with pytest.raises(ValueError):
        aug.mixup_layout(p, 0, [(640, 640)] * 2, size)
    with pytest.raises(ValueError):
        aug.mixup_canvas(0.0, size)
    assert aug.mixup_canvas(0.5, (320, 416)) == (208, 160)
    _set_mix(p, 0, 1, jit=1.0, off=(-1, 0))
    with pytest.raises(ValueError):
        aug.mixup_layout(p, 0, [(640, 640)] * 2, size)


@pytest.mark.parametrize("seed", MIX_SEEDS)
def test_mixup_off_is_the_augment_oracle(seed):
    images, targets, params = seeded_case(seed, hsv=True)
    sizes = [im.shape[:2] for im in images]
    assert not params.mixup.any()
    want, owner, margin = ao.augment_images(images, params, INPUT_SIZE)
    got, cls, owner2, tile_margin, mix_margin = mo.augment_images(images, params, INPUT_SIZE)
    assert np.array_equal(got, want) and np.array_equal(owner, owner2) and tile_margin == margin and mix_margin == np.inf
    assert np.array_equal(cls == mo.TILE, owner >= 0) and np.array_equal(cls == mo.PLAIN_PAD, owner < 0)
    wt, wc, _ = ao.augment_labels(targets, sizes, params, INPUT_SIZE, MAX_LABELS)
    gt, gc, info = mo.augment_labels(targets, sizes, params, INPUT_SIZE, MAX_LABELS)
    assert np.array_equal(gt, wt) and np.array_equal(gc, wc) and info["partner_kept"] == [0] * len(images)


# ------------------------------------------------------------------------------------------------ the GPU tests' seeds

@pytest.mark.parametrize("seed", MIX_SEEDS)
def test_seeded_mix_cases_are_away_from_their_thresholds(seed):
    """What tests/test_gpu_mixup.py compares for equality must not sit on a knife edge: pixel ownership in both maps, centre
    margin and extent filter are further than 1e-6 from their thresholds and every re-cast ray meets exactly one edge."""
    images, targets, params = seeded_mix_case(seed)
    sizes = [im.shape[:2] for im in images]
    _, cls, owner, tile_margin, mix_margin = mo.sample_u8(images, params, INPUT_SIZE)
    table, counts, info = mo.augment_labels(targets, sizes, params, INPUT_SIZE, MAX_LABELS)
    print("seed %d: pixel margins %.3g (tiles) %.3g (partner), centre margin %.3g, extent margin %.3g, survivors %s, of the partner %s"
          % (seed, tile_margin, mix_margin, info["centre_margin"], info["extent_margin"], counts.tolist(), info["partner_kept"]))
    assert params.mixup.any()
    assert tile_margin > 1e-6 and mix_margin > 1e-6 and info["centre_margin"] > 1e-6 and info["extent_margin"] > 1e-6
    assert all((h == 1).all() for h in info["hits"]) and np.isfinite(table).all()


def test_seeded_mix_cases_between_them_cover_what_the_issue_lists():
    got = dict(jit_lo=False, jit_hi=False, flip=False, noflip=False, x_off=False, y_off=False, odd_wj=False, classes=set(),
               mosaic_plain=False, non_mosaic=False, partner_rows=False, overflow=False, mirrored=False, unmirrored=False)
    for seed in MIX_SEEDS:
        images, targets, params = seeded_mix_case(seed)
        sizes = [im.shape[:2] for im in images]
        on = params.mixup
        _, cls, _, _, _ = mo.sample_u8(images, params, INPUT_SIZE)
        table, counts, info = mo.augment_labels(targets, sizes, params, INPUT_SIZE, MAX_LABELS)
        assert not (on & ~params.mosaic).any()
        got["jit_lo"] |= bool((params.mix_jit[on] < 1).any())
        got["jit_hi"] |= bool((params.mix_jit[on] > 1).any())
        got["flip"] |= bool(params.mix_flip[on].any())
        got["noflip"] |= bool((~params.mix_flip[on]).any())
        got["mirrored"] |= bool(params.mirror[on].any())                      # the partner is placed in the frame before the final mirror
        got["unmirrored"] |= bool((~params.mirror[on]).any())
        got["x_off"] |= bool((params.mix_off[on][:, 0] != 0).any())
        got["y_off"] |= bool((params.mix_off[on][:, 1] != 0).any())
        got["odd_wj"] |= any(int(INPUT_SIZE[1] * j) % 4 != 0 for j in params.mix_jit[on])
        got["classes"] |= set(np.unique(cls[on]).tolist())
        got["mosaic_plain"] |= bool((params.mosaic & ~on).any())
        got["non_mosaic"] |= bool((~params.mosaic).any())
        # partner rows that reach the table: a (4, row) among the first MAX_LABELS survivors
        got["partner_rows"] |= any(any(t == 4 for t, _ in kept[:MAX_LABELS]) for kept in info["kept"])
        got["overflow"] |= bool((counts[on] > MAX_LABELS).any())
    assert got.pop("classes") >= {mo.TILE, mo.PARTNER, mo.PARTNER_PAD, mo.BLACK}
    assert all(got.values()), got


# ------------------------------------------------------------------------------------------------ host API

def test_sample_mixup_draw_count_order_and_ranges():
    from ep24 import augment as aug
    n, S = 64, (320, 416)
    sizes, counts = [(480, 640)] * n, [3] * n
    base = aug.sample_params(aug.position_rng(1, 2, 3), sizes, S)
    p = aug.sample_params(aug.position_rng(1, 2, 3), sizes, S)
    assert not p.mixup.any() and (p.mix_jit == 1).all() and not p.mix_off.any()          # off by default
    assert aug.sample_mixup(aug.mixup_rng(1, 2, 3), p, sizes, counts, S) is p
    for k in ("mosaic", "centre", "partners", "M", "Minv", "mirror", "hsv_on", "hsv"):    # sample_params' output is not touched
        assert np.array_equal(getattr(p, k), getattr(base, k)), k
    assert p.mixup.all() and 0 < p.mix_flip.sum() < n                                    # defaults: mixup_prob 1.0
    assert (p.mix_jit >= 0.5).all() and (p.mix_jit < 1.5).all() and (p.mix_partner >= 0).all() and (p.mix_partner < n).all()
    for i in range(n):
        Wj, Hj = int(416 * p.mix_jit[i]), int(320 * p.mix_jit[i])
        x_off, y_off = p.mix_off[i]
        assert 0 <= x_off <= max(Wj - 416 - 1, 0) and 0 <= y_off <= max(Hj - 320 - 1, 0)
        assert (x_off == 0 and y_off == 0) or p.mix_jit[i] > 1
    assert (p.mix_off[:, 0] > 0).any() and (p.mix_off[:, 1] > 0).any()
    # the six draws in their order, replayed by hand
    rng = aug.mixup_rng(1, 2, 3)
    for i in range(n):
        u_mix, jit, u_flip, partner = rng.random_sample(), rng.uniform(0.5, 1.5), rng.random_sample(), int(rng.randint(0, n))
        u_y, u_x = rng.random_sample(), rng.random_sample()
        Wj, Hj = int(416 * jit), int(320 * jit)
        assert p.mix_jit[i] == jit and p.mix_flip[i] == (u_flip > 0.5) and p.mix_partner[i] == partner
        assert tuple(p.mix_off[i]) == (int(u_x * (Wj - 416)) if Wj > 416 else 0, int(u_y * (Hj - 320)) if Hj > 320 else 0)
    # a generator of its own: seeded with [seed, epoch, it, 1]
    assert aug.mixup_rng(1, 2, 3).random_sample() == np.random.RandomState(np.array([1, 2, 3, 1], dtype=np.uint32)).random_sample()
    assert aug.mixup_rng(1, 2, 3).random_sample() != aug.position_rng(1, 2, 3).random_sample()
    # same position, same parameters; another position: others
    q = aug.sample_mixup(aug.mixup_rng(1, 2, 3), aug.sample_params(aug.position_rng(1, 2, 3), sizes, S), sizes, counts, S)
    for k in ("mixup", "mix_partner", "mix_jit", "mix_flip", "mix_off"):
        assert np.array_equal(getattr(p, k), getattr(q, k)), k
    for other in ((1, 2, 4), (1, 3, 3), (2, 2, 3)):
        o = aug.sample_mixup(aug.mixup_rng(*other), aug.sample_params(aug.position_rng(1, 2, 3), sizes, S), sizes, counts, S)
        assert not np.array_equal(o.mix_jit, p.mix_jit)
    # 6 numbers per image whatever the coins say: both generators end in the same state
    rng2, rng3 = aug.mixup_rng(1, 2, 3), aug.mixup_rng(1, 2, 3)
    some = aug.sample_mixup(rng2, aug.sample_params(aug.position_rng(1, 2, 3), sizes[:5], S), sizes[:5], counts[:5], S, mixup_prob=0.5)
    none = aug.sample_mixup(rng3, aug.sample_params(aug.position_rng(1, 2, 3), sizes[:5], S, mosaic_prob=0.0), sizes[:5], [0] * 5, S,
                            mixup_prob=0.0, mixup_scale=(0.9, 1.1))
    assert rng2.random_sample() == rng3.random_sample()
    assert not none.mixup.any()
    off = aug.sample_mixup(aug.mixup_rng(1, 2, 3), aug.sample_params(aug.position_rng(1, 2, 3), sizes, S), sizes, counts, S, mixup_prob=0.0)
    assert not off.mixup.any()
    half = aug.sample_mixup(aug.mixup_rng(1, 2, 3), aug.sample_params(aug.position_rng(1, 2, 3), sizes, S), sizes, counts, S, mixup_prob=0.5)
    assert 0 < half.mixup.sum() < n and np.array_equal(half.mix_jit[half.mixup], p.mix_jit[half.mixup])


def test_sample_mixup_conditions():
    from ep24 import augment as aug
    n, S = 8, (320, 416)
    sizes = [(480, 640)] * n

    def drawn(counts, **kw):
        p = aug.sample_params(aug.position_rng(5, 0, 0), sizes, S, **kw)
        return aug.sample_mixup(aug.mixup_rng(5, 0, 0), p, sizes, counts, S)

    full = drawn([2] * n)
    assert full.mixup.all()
    # the partner walk: cyclically forward from the drawn index to the next image with label rows
    counts = [0, 0, 3, 0, 0, 0, 1, 0]
    p = drawn(counts)
    for i in range(n):
        want = int(full.mix_partner[i])
        while counts[want] == 0:
            want = (want + 1) % n
        tiles_have_labels = any(counts[int(j)] > 0 for j in p.partners[i])
        assert p.mixup[i] == tiles_have_labels                                   # the stand-in for len(mosaic_labels) != 0
        if p.mixup[i]:
            assert p.mix_partner[i] == want and counts[p.mix_partner[i]] > 0
    assert p.mixup.any() and not p.mixup.all() and set(p.mix_partner[p.mixup].tolist()) <= {2, 6}
    assert any(counts[int(full.mix_partner[i])] == 0 for i in range(n) if p.mixup[i])   # the walk really moved one
    # no image of the batch has labels: no mixup
    assert not drawn([0] * n).mixup.any()
    # no mixup on an image that is not a mosaic
    assert not drawn([2] * n, mosaic_prob=0.0).mixup.any()
    some = drawn([2] * n, mosaic_prob=0.5)
    assert np.array_equal(some.mixup, some.mosaic) and 0 < some.mosaic.sum() < n
    with pytest.raises(ValueError):
        aug.sample_mixup(aug.mixup_rng(5, 0, 0), aug.identity_params(3), sizes, [1] * n, S)


def test_mosaic_transform_mixup_positions():
    from ep24 import augment as aug
    sizes, counts, S = [(100, 120)] * 4, [2, 0, 1, 3], (64, 96)
    plain, zero, mix = aug.MosaicTransform(seed=5), aug.MosaicTransform(seed=5, mixup_prob=0.0), aug.MosaicTransform(seed=5, mixup_prob=1.0)
    assert (plain.mixup_prob, plain.mixup_scale, mix.mixup_scale) == (0.0, (0.5, 1.5), (0.5, 1.5))
    for tr in (plain, zero, mix):
        tr.set_position(2, 7)
    a, z, m = plain.sample(sizes, S), zero.sample(sizes, S, counts), mix.sample(sizes, S, counts)
    for k in ("mosaic", "centre", "partners", "M", "Minv", "mirror", "hsv_on", "hsv"):    # mixup_prob = 0 samples what it samples today
        assert np.array_equal(getattr(a, k), getattr(z, k)) and np.array_equal(getattr(a, k), getattr(m, k)), k
    assert not a.mixup.any() and not z.mixup.any() and m.mixup.any()
    want = aug.sample_mixup(aug.mixup_rng(5, 2, 7), aug.sample_params(aug.position_rng(5, 2, 7), sizes, S), sizes, counts, S)
    for k in ("mixup", "mix_partner", "mix_jit", "mix_flip", "mix_off"):
        assert np.array_equal(getattr(m, k), getattr(want, k)), k
    mix.set_position(2, 8)
    b = mix.sample(sizes, S, counts)
    mix.set_position(2, 7)                                                       # set_position reseeds both generators
    c = mix.sample(sizes, S, counts)
    assert np.array_equal(c.mix_jit, m.mix_jit) and np.array_equal(c.M, m.M) and not np.array_equal(b.mix_jit, m.mix_jit)


def test_mixup_flag_exp_attributes_and_from_exp():
    sys.path.insert(0, Y24)
    try:
        import importlib
        mod = importlib.import_module("train_24p")
        assert mod.make_parser().parse_args([]).mixup is False
        a = mod.make_parser().parse_args(["--augment", "--mixup"])
        assert a.mixup is True and a.augment is True
        mod.check_mixup_args(a)
        mod.check_mixup_args(mod.make_parser().parse_args(["--augment"]))
        with pytest.raises(SystemExit) as e:
            mod.check_mixup_args(mod.make_parser().parse_args(["--mixup"]))
        assert "--augment" in str(e.value)
        from exp import get_exp
        exp = get_exp(os.path.join(Y24, "load_train", "yolox_24p_train.py"))
        assert (exp.enable_mixup, exp.mixup_prob, tuple(exp.mixup_scale)) == (True, 1.0, (0.5, 1.5))
        from ep24 import augment as aug
        tr = aug.MosaicTransform.from_exp(exp, seed=3)
        assert (tr.mixup_prob, tr.mixup_scale) == (0.0, (0.5, 1.5))                # not read without mixup=True
        exp.mixup_prob, exp.mixup_scale = 0.6, (0.8, 1.6)
        tr = aug.MosaicTransform.from_exp(exp, seed=3, mixup=True)
        assert (tr.mixup_prob, tr.mixup_scale, tr.seed, tr.mosaic_prob) == (0.6, (0.8, 1.6), 3, 1.0)
        assert aug.MosaicTransform.from_exp(exp, seed=3).mixup_prob == 0.0
    finally:
        sys.path.remove(Y24)
