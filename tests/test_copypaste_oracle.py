"""CPU half of the copy-paste tests: the numpy oracle (tests/copypaste_oracle.py) against hand-computed cases, and the cases that
tests/test_gpu_copypaste.py demands EQUALITY on - what they cover between them and that none of their decisions is a close call
(|IoA - thr| >= 1e-6, every margin / inside decision at least 1e-3 px from its threshold).  Those are conditions on the inputs,
checked here with the oracle alone; they are not tolerances on the GPU."""
import functools

import numpy as np
import pytest

import copypaste_oracle as co
import poly24_oracle as P

MIN_MARGIN, THR = 2.0, 0.30
SIZES = ((48, 80), (50, 70))            # (S_h, S_w): tails that are no multiple of a wave, a tile or four pixels
N = 5
SEEDED = (("seed37", 37, SIZES[0]), ("seed6", 6, SIZES[1]), ("seed34", 34, SIZES[1]))     # three accepted candidates each
CASES = ("hand",) + tuple(name for name, _, _ in SEEDED)
TAGS = {"flip_on", "flip_off", "dx_neg", "dx_pos", "dy_neg", "dy_pos", "outside", "margin", "veto_existing", "veto_accepted_only",
        "select", "cap", "overflow", "self_flip", "zero_area", "off"}


def square_row(cls, cx, cy, h):
    row = np.zeros(51, dtype=np.float32)
    row[0], row[1], row[2] = cls, cx, cy
    row[3:] = P.square64(float(cx), float(cy), float(h)).reshape(48)
    return row


def descriptor(on, partner, flip, dx, dy, select=-1):
    return np.array([on, partner, flip, dx, dy, select, 0, 0], dtype=np.int64)


def table(rows_per_image, max_labels, counts=None):
    n = len(rows_per_image)
    lab = np.zeros((n, max_labels, 51), dtype=np.float32)
    for i, rows in enumerate(rows_per_image):
        for r, row in enumerate(rows[:max_labels]):
            lab[i, r] = row
    cnt = np.array([len(r) for r in rows_per_image] if counts is None else counts, dtype=np.int32)
    return lab, cnt


def lopsided(seed, lo=6.0, hi=7.0):
    return np.random.RandomState(seed).uniform(lo, hi, 24)


def hand_case():
    """S = 48 x 80, n = 5, max_labels = 6.  What each image is there for:
      0  pastes from 1, no flip, dx > 0, dy < 0: candidate 0 vetoed by an existing row, 1 accepted (next to a zero-area existing
         row), 2 vetoed only by the accepted candidate 1, 3 has its select bit cleared, 4 is partly outside, 5 has its centre inside
         the margin;
      1  off: out == pre;
      2  pastes from 3, flip, dx < 0, dy > 0: four rows of its own, the cap of six is reached after two of three acceptable candidates;
      3  pastes from ITSELF, flip: its three rows mirrored beside the originals;
      4  pre_count = 9 > max_labels: nothing is pasted."""
    S, max_labels = SIZES[0], 6
    zero = np.zeros(51, dtype=np.float32)
    zero[0], zero[1:] = 3, np.tile(np.array([60.0, 20.0], dtype=np.float32), 25)               # every vertex at the centre: area 0
    img0 = [co.polygon_row(1, 20, 24, 8.0), zero]
    img1 = [co.polygon_row(2, 12, 26, lopsided(1, 6.5, 7.5)), co.polygon_row(4, 45, 28, lopsided(2, 7.5, 8.5)),
            co.polygon_row(5, 50, 30, lopsided(3, 6.5, 7.5)), co.polygon_row(6, 30, 14, 6.0), co.polygon_row(7, 66.5, 24, 8.0),
            co.polygon_row(8, 69, 30, 6.0)]
    img2 = [co.polygon_row(9, 8, 8, 6.0), co.polygon_row(10, 8, 24, 6.0), co.polygon_row(11, 8, 40, 6.0), co.polygon_row(12, 24, 8, 6.0)]
    img3 = [co.polygon_row(13, 35, 20, lopsided(4)), co.polygon_row(14, 15, 20, lopsided(5)), co.polygon_row(15, 35, 36, lopsided(6))]
    img4 = [co.polygon_row(16 + k, 10 + 11 * k, 24, 6.0) for k in range(6)]
    lab, cnt = table([img0, img1, img2, img3, img4], max_labels, counts=[2, 6, 4, 3, 9])
    paste = np.stack([descriptor(1, 1, 0, 10, -4, ~(1 << 3)), descriptor(0, 0, 0, 0, 0), descriptor(1, 3, 1, -5, 3),
                      descriptor(1, 3, 1, 4, 0), descriptor(1, 0, 0, 3, 3)])
    return dict(name="hand", S=S, max_labels=max_labels, pre_labels=lab, pre_count=cnt, paste=paste, seed=1000)


def seeded_case(name, seed, S):
    """n = 5, max_labels = 50: 0 .. 8 lopsided polygons of radius 6 - 15 px per image, descriptors from ``sample_paste`` at
    probability 1 (the draws of the host side), one image switched off."""
    from ep24 import augment as aug
    rs = np.random.RandomState(seed)
    S_h, S_w = S
    images = []
    for i in range(N):
        rows = []
        for _ in range(int(rs.randint(0, 9))):
            base = rs.uniform(6.0, 15.0)
            r = np.clip(base * rs.uniform(0.8, 1.2, 24), 6.0, 15.0)
            rows.append(co.polygon_row(int(rs.randint(0, 80)), rs.uniform(12.0, S_w - 12.0), rs.uniform(12.0, S_h - 12.0), r))
        images.append(rows)
    lab, cnt = table(images, 50)
    p = aug.sample_paste(aug.paste_rng(seed, 0, 0), aug.AugParams(N), N, S, 1.0)
    p.paste[seed % N] = False
    return dict(name=name, S=S, max_labels=50, pre_labels=lab, pre_count=cnt, paste=aug.paste_descriptors(p), seed=seed)


@functools.lru_cache(maxsize=None)
def case(name):
    """The inputs of a case and the oracle's answer, computed once per process and shared (nobody writes to them)."""
    c = hand_case() if name == "hand" else seeded_case(*[s for s in SEEDED if s[0] == name][0])
    rows, counts, ranges, decisions = co.paste_labels(c["pre_labels"], c["pre_count"], c["paste"], c["S"], MIN_MARGIN, THR,
                                                      c["max_labels"])
    c.update(rows=rows, counts=counts, ranges=ranges, decisions=decisions)
    c["pre_images"] = np.random.RandomState(c["seed"] + 77).randint(0, 256, (N, 3) + tuple(c["S"])).astype(np.float32)
    for v in c.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return c


def coverage(c):
    tags = set()
    E = np.minimum(c["pre_count"], c["max_labels"])
    for i, d in enumerate(c["paste"]):
        on, j, flip, dx, dy = (int(v) for v in d[:5])
        if not on:
            tags.add("off")
            continue
        tags.add("flip_on" if flip else "flip_off")
        tags.update(t for t, hit in (("dx_neg", dx < 0), ("dx_pos", dx > 0), ("dy_neg", dy < 0), ("dy_pos", dy > 0)) if hit)
        if j == i and flip:
            tags.add("self_flip")
    by_cand = {}
    for d in c["decisions"]:
        by_cand.setdefault((d["image"], d["cand"]), []).append(d)
    for (i, k), ds in by_cand.items():
        for d in ds:
            if d["kind"] in ("select", "cap", "overflow"):
                tags.add(d["kind"])
            if d["kind"] == "margin" and not d["passed"]:
                tags.add("margin")
            if d["kind"] == "inside" and not d["passed"]:
                tags.add("outside")
        vetoes = [d["row"] for d in ds if d["kind"] == "ioa" and not d["passed"]]
        if vetoes:
            tags.add("veto_existing" if min(vetoes) < E[i] else "veto_accepted_only")
        if any(d["kind"] == "inside" and d["passed"] for d in ds) and E[i] > 0 and \
                (co.areas(c["pre_labels"][i, :E[i], 3:].reshape(-1, 24, 2)) == 0).any():
            tags.add("zero_area")
    return tags


# ------------------------------------------------------------------------------------------------ oracle vs hand-computed cases

def _two_images(existing, candidate, d):
    lab, cnt = table([[existing], [candidate]], 6)
    paste = np.stack([d, descriptor(0, 0, 0, 0, 0)])
    return co.paste_labels(lab, cnt, paste, SIZES[0], MIN_MARGIN, THR, 6)


def test_square_pasted_beside_a_square():
    existing, cand = square_row(1, 20, 24, 8), square_row(2, 20, 24, 8)
    rows, counts, ranges, dec = _two_images(existing, cand, descriptor(1, 1, 0, 20, 0))
    assert counts.tolist() == [2, 1] and ranges.tolist() == [[1, 2], [1, 1]]
    assert np.array_equal(rows[0, 0], existing) and np.array_equal(rows[1, 0], cand) and not rows[0, 2:].any() and not rows[1, 1:].any()
    # x + 20: the sides (integers) move exactly and the squares share the line x = 28; a vertex between the corners is the fp32
    # value plus 20 rounded again, within an ulp of 48 (3.8e-6) of the square built at 40
    np.testing.assert_allclose(rows[0, 1], square_row(2, 40, 24, 8), rtol=0, atol=4e-6)
    assert rows[0, 1, 3::2].min() == 32 and rows[0, 1, 3::2].max() == 48 and np.array_equal(rows[0, 1, 4::2], cand[4::2])
    ioa = [d for d in dec if d["kind"] == "ioa"]
    assert len(ioa) == 1 and abs(ioa[0]["value"]) <= 1e-12 and ioa[0]["passed"]
    assert co.accepted(dec) == {(0, 0)}


@pytest.mark.parametrize("shift, share, pasted", [((8, 8), 0.25, True), ((8, 0), 0.50, False)])
def test_square_covering_a_quarter_and_a_half(shift, share, pasted):
    """Side 16 squares: shifted by (8, 8) the pasted one hides 8 x 8 of 256 = 25 % of the existing one (< 30 %: pasted), shifted by
    (8, 0) it hides 8 x 16 = 50 % (vetoed)."""
    existing, cand = square_row(1, 30, 24, 8), square_row(2, 30, 24, 8)
    rows, counts, ranges, dec = _two_images(existing, cand, descriptor(1, 1, 0, shift[0], shift[1]))
    ioa = [d for d in dec if d["kind"] == "ioa"]
    assert len(ioa) == 1 and abs(ioa[0]["value"] - share) <= 1e-12 and ioa[0]["passed"] == pasted
    assert abs(ioa[0]["distance"] - abs(share - THR)) <= 1e-12
    assert counts.tolist() == [2 if pasted else 1, 1] and ranges.tolist() == [[1, 2 if pasted else 1], [1, 1]]
    assert rows[0, 1].any() == pasted
    if pasted:
        np.testing.assert_allclose(rows[0, 1], square_row(2, 30 + shift[0], 24 + shift[1], 8), rtol=0, atol=4e-6)


def test_flip_maps_vertex_k_to_12_minus_k():
    """A lopsided polygon (radius 6 + 0.3 k on ray k) mirrored about the image: the point on the ray of 15 k degrees lands on the
    ray of 180 - 15 k degrees, i.e. vertex (12 - k) mod 24 of the pasted row has the radius of source vertex k, and every vertex of
    the pasted row is on its own ray again."""
    r = 6.0 + 0.3 * np.arange(24)
    cand = co.polygon_row(7, 30, 24, r)
    lab, cnt = table([[], [cand]], 6)
    paste = np.stack([descriptor(1, 1, 1, 3, -2), descriptor(0, 0, 0, 0, 0)])
    rows, counts, ranges, dec = co.paste_labels(lab, cnt, paste, SIZES[0], MIN_MARGIN, THR, 6)
    assert counts.tolist() == [1, 1] and ranges.tolist() == [[0, 1], [1, 1]]
    row = rows[0, 0].astype(np.float64)
    assert row[0] == 7 and row[1] == 80 - 30 + 3 and row[2] == 24 - 2
    vx, vy = row[3::2] - row[1], row[4::2] - row[2]
    np.testing.assert_allclose(np.hypot(vx, vy), r[(12 - np.arange(24)) % 24], atol=1e-5)
    ang = np.degrees(np.arctan2(vy, vx)) % 360.0
    np.testing.assert_allclose(ang, 15.0 * np.arange(24), atol=1e-3)
    # the same points, mirrored: vertex m of the new row is source vertex (12 - m) mod 24 at (80 - x + 3, y - 2)
    src = cand[3:].reshape(24, 2)[(12 - np.arange(24)) % 24].astype(np.float64)
    assert np.array_equal(rows[0, 0, 3::2], (80.0 - src[:, 0] + 3.0).astype(np.float32))
    assert np.array_equal(rows[0, 0, 4::2], (src[:, 1] - 2.0).astype(np.float32))


def test_pixels_of_a_pasted_square():
    """The square [32, 48) x [16, 32) pasted from image 1 at dx = 20, mirrored: exactly its 16 x 16 pixel centres are taken, from
    the mirrored and shifted source columns."""
    existing, cand = square_row(1, 10, 10, 4), square_row(2, 60, 24, 8)
    lab, cnt = table([[existing], [cand]], 6)
    paste = np.stack([descriptor(1, 1, 1, 20, 0), descriptor(0, 0, 0, 0, 0)])
    S_h, S_w = SIZES[0]
    rows, counts, ranges, _ = co.paste_labels(lab, cnt, paste, SIZES[0], MIN_MARGIN, THR, 6)
    assert counts.tolist() == [2, 1] and rows[0, 1, 1] == 80 - 60 + 20
    pre = np.random.RandomState(0).randint(0, 256, (2, 3, S_h, S_w)).astype(np.float32)
    out, pasted = co.paste_u8(pre, rows, ranges, paste)
    want = np.zeros((S_h, S_w), dtype=bool)
    want[16:32, 32:48] = True
    assert np.array_equal(pasted[0], want) and not pasted[1].any() and np.array_equal(out[1], pre[1])
    xs = S_w - 1 - (np.arange(32, 48) - 20)
    assert np.array_equal(out[0][:, 16:32, 32:48], pre[1][:, 16:32, :][:, :, xs])
    assert np.array_equal(out[0][:, ~want], pre[0][:, ~want])


# ------------------------------------------------------------------------------------------------ the cases of the GPU tests

def test_hand_case_is_what_its_docstring_says():
    c = case("hand")
    assert c["counts"].tolist() == [3, 6, 6, 6, 9] and c["ranges"].tolist() == [[2, 3], [6, 6], [4, 6], [3, 6], [6, 6]]
    assert co.accepted(c["decisions"]) == {(0, 1), (2, 0), (2, 1), (3, 0), (3, 1), (3, 2)}
    kinds = {(d["image"], d["cand"]): d["kind"] for d in c["decisions"] if not d["passed"]}
    assert kinds[(0, 0)] == "ioa" and kinds[(0, 2)] == "ioa" and kinds[(0, 3)] == "select" and kinds[(0, 4)] == "inside"
    assert kinds[(0, 5)] == "margin" and kinds[(2, 2)] == "cap" and kinds[(4, None)] == "overflow"
    assert coverage(c) == TAGS


def test_cases_cover_the_list_between_them():
    got = set()
    for name in CASES:
        tags = coverage(case(name))
        print(name, "accepted", sorted(co.accepted(case(name)["decisions"])), "covers", sorted(tags))
        got |= tags
    assert got == TAGS
    for name, _, _ in SEEDED:                                                      # the seeded ones are not idle
        c = case(name)
        assert len(co.accepted(c["decisions"])) >= 2 and "off" in coverage(c)
    assert {"veto_existing", "veto_accepted_only", "self_flip"} <= set().union(*(coverage(case(name)) for name, _, _ in SEEDED))
    assert {case(name)["S"] for name in CASES} == set(SIZES)


@pytest.mark.parametrize("name", CASES)
def test_no_decision_is_a_close_call(name):
    c = case(name)
    ioa = [d["distance"] for d in c["decisions"] if d["kind"] == "ioa"]
    geo = [d["distance"] for d in c["decisions"] if d["kind"] in ("margin", "inside")]
    print(name, "decisions: %d IoA (closest %.3g), %d margin / inside (closest %.3g px)" %
          (len(ioa), min(ioa, default=np.inf), len(geo), min(geo, default=np.inf)))
    assert ioa and geo
    assert min(ioa) >= 1e-6 and min(geo) >= 1e-3


@pytest.mark.parametrize("name", CASES)
def test_pasted_pixels_exist_and_only_they_change(name):
    c = case(name)
    out, pasted = co.paste_u8(c["pre_images"], c["rows"], c["ranges"], c["paste"])
    for i in range(N):
        assert (pasted[i].sum() > 0) == (c["ranges"][i, 1] > c["ranges"][i, 0]), (name, i)
        assert np.array_equal(out[i][:, ~pasted[i]], c["pre_images"][i][:, ~pasted[i]])


def test_sample_paste_draws_the_same_count_whatever_the_outcome():
    """69 variates per image: the generator's state after n images does not depend on the probabilities, and the fields of image
    i do not depend on what was decided for the images before it."""
    from ep24 import augment as aug
    S = (64, 96)
    a, b = aug.paste_rng(5, 1, 2), aug.paste_rng(5, 1, 2)
    pa = aug.sample_paste(a, aug.AugParams(4), 4, S, 1.0, obj_prob=1.0)
    pb = aug.sample_paste(b, aug.AugParams(4), 4, S, 0.0, obj_prob=0.0)
    assert a.random_sample() == b.random_sample()
    assert pa.paste.all() and not pb.paste.any()
    assert np.array_equal(pa.paste_partner, pb.paste_partner) and np.array_equal(pa.paste_off, pb.paste_off)
    assert np.array_equal(pa.paste_flip, pb.paste_flip)
    assert (pa.paste_select == np.uint64(2 ** 64 - 1)).all() and (pb.paste_select == 0).all()
    assert (np.abs(pa.paste_off[:, 0]) <= 48).all() and (np.abs(pa.paste_off[:, 1]) <= 32).all()
    # its own stream: the other two generators at the same position draw what they drew
    assert aug.paste_rng(5, 1, 2).random_sample() != aug.mixup_rng(5, 1, 2).random_sample() != aug.position_rng(5, 1, 2).random_sample()
    d = aug.paste_descriptors(pa)
    assert d.shape == (4, 8) and d.dtype == np.int64 and (d[:, 5] == -1).all() and (d[:, 6:] == 0).all()
    pa.paste_partner[2] = 4
    with pytest.raises(Exception, match="EP24_E_ARG"):
        aug.paste_descriptors(pa)
