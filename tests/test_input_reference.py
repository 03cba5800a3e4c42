"""tests/input_reference.py without a GPU: its references agree with what the repository already has (the committed goldens g14_input
and g8_sector, oracle/input.py, oracle/sector.py, augment_oracle, mixup_oracle, fisheye_oracle, resize_oracle) on the new cases; every
case reaches the path it is there for, computed from the kernels' constants as restated in input_reference; and each of the twelve
mutants changes the expected output of at least one case."""
import os
import sys
import zlib

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import augment_oracle as ao  # noqa: E402
import copypaste_oracle as co  # noqa: E402
import fisheye_oracle as fo  # noqa: E402
import input_reference as R  # noqa: E402
import mixup_oracle as mo  # noqa: E402
import resize_oracle as ro  # noqa: E402
from oracle import input as oin  # noqa: E402
from oracle import sector as osec  # noqa: E402
from test_oracle_input import INPUT_CASES, input_case  # noqa: E402

SMALL_PREPROC = [k for k in R.PREPROC_CASES if k != "cap"]


def differs(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return a.shape != b.shape or not np.array_equal(a, b, equal_nan=True)


# ---------------------------------------------------------------------------------------------------------------------------
# the references against what exists
def test_preproc_reference_is_the_golden_and_the_oracle(golden):
    """one buffer, rows 3 * w apart: g14_input's checksums, and oracle.input.preproc on every image of the new cases that has the
    letterbox's own size and a plain stride"""
    z = golden("g14_input")
    for i, (tag, h, w, size, k) in enumerate(INPUT_CASES):
        img, targets = input_case(tag, h, w, k, 140 + i)
        r, rh, rw = R.letterbox(h, w, *size)
        desc = np.array([[0, h, w, 3 * w, rh, rw]], dtype=np.int64)
        scales = np.array([[1.0 / (rw / w), 1.0 / (rh / h)]])
        out = R.preproc_u8_ref(img.reshape(-1), desc, scales, *size)[0]
        assert zlib.crc32(out.tobytes()) == int(z[tag + "_crc"]), tag
        rows = targets.reshape(-1, 51) if targets.size else np.zeros((0, 51))
        lab = R.preproc_labels_ref(rows, np.array([0, len(rows)]), np.array([[w, h, r]], dtype=np.float64), 50)[0]
        assert np.array_equal(lab, z[tag + "_labels"]), tag
    for name in SMALL_PREPROC:
        c = R.preproc_case(name)
        out = R.preproc_u8_ref(c["buf"], c["desc"], c["scales"], c["S_h"], c["S_w"])
        for i, (img, d) in enumerate(zip(c["images"], c["desc"])):
            _, rh, rw = R.letterbox(img.shape[0], img.shape[1], c["S_h"], c["S_w"])
            if (rh, rw) == (int(d[4]), int(d[5])) and rh > 0:
                assert np.array_equal(out[i], oin.preproc(img, (c["S_h"], c["S_w"]))[0]), (name, i)
            elif rh > 0:                                                  # a resized size of the test's own: the resize itself
                rh, rw = int(d[4]), int(d[5])
                assert np.array_equal(out[i][:, :rh, :rw], osec.resize_linear_u8(img, rw, rh).transpose(2, 0, 1))
                assert (out[i][:, rh:] == 114).all() and (out[i][:, :, rw:] == 114).all()


@pytest.mark.parametrize("max_labels", R.LABEL_MAX)
def test_label_reference_is_the_oracle(max_labels):
    c = R.labels_case(max_labels)
    out = R.preproc_labels_ref(c["rows"], c["row_off"], c["whr"], max_labels)
    for i in range(4):
        lo, hi = c["row_off"][i:i + 2]
        w, h, r = c["whr"][i]
        t = c["rows"][lo:hi].copy()
        t[:, 1::2] = t[:, 1::2] * w                                       # train_transform's own order: boxes * w, then boxes *= r
        t[:, 2::2] = t[:, 2::2] * h
        t[:, 1:] *= r
        want = np.zeros((max_labels, 51))
        want[:min(len(t), max_labels)] = t[:max_labels]
        assert np.array_equal(out[i], want.astype(np.float32))


def descriptors_of(images, targets, params, S_h, S_w):
    """the tables ``ep24.augment.mosaic_batch`` uploads, for a batch given as the existing oracles take it"""
    from ep24 import augment as aug
    n = len(images)
    sizes = [im.shape[:2] for im in images]
    offs = np.concatenate([[0], np.cumsum([im.size for im in images])])
    row_off = np.concatenate([[0], np.cumsum([len(t) for t in targets])])
    tiles, tscale = np.zeros((n, 4, 16), dtype=np.int64), np.zeros((n, 4, 3))
    par, flags = np.zeros((n, 16)), np.zeros((n, 2), dtype=np.int32)
    mixi, mixd = np.zeros((n, 16), dtype=np.int64), np.zeros((n, 12))
    for i in range(n):
        for q, (j, rw, rh, (lx1, ly1, lx2, ly2), padw, padh) in enumerate(aug.tile_layout(params, i, sizes, (S_h, S_w))):
            h, w = sizes[j]
            if rw <= 0 or rh <= 0 or lx2 <= lx1 or ly2 <= ly1:
                continue
            tiles[i, q, :14] = (offs[j], h, w, 3 * w, rw, rh, lx1, ly1, lx2, ly2, padw, padh, row_off[j], row_off[j + 1])
            tscale[i, q] = (1.0 / (rw / w), 1.0 / (rh / h), min(S_h / h, S_w / w))
        par[i, 0:6], par[i, 6:12], par[i, 12:15] = params.M[i].reshape(6), params.Minv[i].reshape(6), params.hsv[i]
        flags[i] = (int(params.mirror[i]), int(params.hsv_on[i]))
        if params.mixup[i]:
            j = int(params.mix_partner[i])
            mixi[i], mixd[i] = aug.mixup_layout(params, i, sizes, (S_h, S_w))
            mixi[i, 1], mixi[i, 12], mixi[i, 13] = offs[j], row_off[j], row_off[j + 1]
    buf = np.concatenate([im.reshape(-1) for im in images])
    rows = np.concatenate([np.asarray(t, dtype=np.float64).reshape(-1, 51) for t in targets] + [np.zeros((1, 51))])
    return buf, rows, tiles, tscale, par, flags, mixi, mixd


@pytest.fixture(scope="module")
def seeded():
    """a seeded mosaic of test_augment_oracle with mixup drawn on top, small enough for the float64 oracles"""
    from ep24 import augment as aug
    from test_augment_oracle import make_source
    items = [make_source(h, w, k, 70 + j, star) for j, (h, w, k, star) in enumerate([(90, 120, 7, False), (100, 70, 5, True), (64, 64, 0, False),
                                                                                      (75, 130, 8, True)])]
    images, targets = [it[0] for it in items], [it[1] for it in items]
    sizes = [im.shape[:2] for im in images]
    S = (96, 128)
    params = aug.sample_params(aug.position_rng(3, 0, 0), sizes, S, mosaic_prob=0.8)
    aug.sample_mixup(aug.mixup_rng(3, 0, 0), params, sizes, [len(t) for t in targets], S, mixup_prob=0.7)
    return images, targets, sizes, S, params


def test_augment_references_are_the_oracles(seeded):
    images, targets, sizes, S, params = seeded
    assert params.mosaic.any() and params.mixup.any() and not params.mixup.all() and params.mirror.any()
    buf, rows, tiles, tscale, par, flags, mixi, mixd = descriptors_of(images, targets, params, *S)
    got, owned = R.augment_u8_ref(buf, tiles, tscale, par, flags, mixi, mixd, *S)
    want, cls, owner, _, _ = mo.sample_u8(images, params, S)
    assert np.array_equal(got, want.astype(np.float64))
    assert np.array_equal(owned, (cls == mo.TILE) | (cls == mo.PARTNER))
    plain = type(params)(len(images))
    for k in ("mosaic", "centre", "partners", "M", "Minv", "mirror"):
        setattr(plain, k, getattr(params, k))
    got, owned = R.augment_u8_ref(buf, tiles, tscale, par, flags, None, None, *S)
    want, owner, _ = ao.sample_u8(images, plain, S)
    assert np.array_equal(got, want.astype(np.float64)) and np.array_equal(owned, owner >= 0)
    for dt in (np.float32, np.float64):
        got, _ = R.augment_u8_ref(buf, tiles, tscale, par, flags, mixi, mixd, *S, hsv_dtype=dt)
        want = mo.augment_images(images, params, S, dt)[0]
        assert params.hsv_on.any() and np.array_equal(got, want.astype(np.float64))
    for ml in (3, 50):
        table, counts, info = R.augment_labels_ref(rows, tiles, tscale, par, flags, mixi, mixd, *S, 2.0, ml)
        want, wcounts, winfo = mo.augment_labels(targets, sizes, params, S, ml, 2.0)
        assert counts.tolist() == wcounts.tolist() and counts.max() > 3
        assert np.array_equal(table.astype(np.float32), want)
        assert [len(k) for k in info["kept"]] == [len(k) for k in winfo["kept"]]


def test_resize_and_sector_references_are_the_oracles(golden):
    x = np.random.RandomState(0).randn(3, 5, 7).astype(np.float32)
    assert np.array_equal(R.resize_bilinear_ref(x, 33, 29), ro.resize(x, 33, 29))
    # the gather against the winner map of the oracle, which g8_sector pins: the key of a pixel is a * T + r of the last writer
    z = golden("g8_sector")
    theta, h, w = 60, 427, 640
    src_map, (y0, y1, x0, x1), T = osec.winner_map(theta, h, w)
    key = "t%d_%dx%d_" % (theta, h, w)
    assert zlib.crc32(np.ascontiguousarray(src_map).tobytes()) == int(z[key + "src_crc"])
    ok = src_map >= 0
    row, col = src_map // osec.N_ANG, src_map % osec.N_ANG
    winner = np.where(ok, (osec.N_ANG - 1 - col) * T + (T - 1 - row), -1).astype(np.int32)
    _, flat = R.sector_gather_ref(None, winner.reshape(-1), winner.shape[1], 0, 0, winner.shape[0], winner.shape[1], T, osec.N_ANG, 0)
    assert np.array_equal(flat, src_map)
    g = R.gather_case()
    dst, flat = R.sector_gather_ref(g["src"].reshape(-1), g["winner"].reshape(-1), g["cw"], g["y0"], g["x0"], g["oh"], g["ow"], g["T"], g["n_ang"], 114)
    assert np.array_equal(dst, osec.apply(flat, g["src"], 114))
    assert R.mask_bbox_ref(np.zeros((4, 5, 3), np.uint8), [9, 9, -1, -1]) == [9, 9, -1, -1]
    m = np.zeros((6, 7, 3), np.uint8)
    m[2:4, 1:6] = 255
    box = R.mask_bbox_ref(m, [2 ** 31 - 1, 2 ** 31 - 1, -1, -1])
    assert [box[0], box[1], box[2] - box[0], box[3] - box[1]] == osec.mask_bbox(m)


@pytest.mark.parametrize("max_labels", (5, 50))
def test_sector_label_reference_is_the_oracle(max_labels):
    c = R.sector_case(max_labels)
    cand, keep, out, counts, flags, margins = R.sector_labels_ref(c["rows"], c["geo"], max_labels)
    targets = [c["rows"][int(G[10]):int(G[10]) + int(G[11])] for G in c["geo"]]
    table, wcounts, wflags, _ = fo.warp_labels(targets, [R.geo_dict(G) for G in c["geo"]], R.SECTOR_S, max_labels)
    assert np.array_equal(out.astype(np.float32), table) and counts.tolist() == wcounts.tolist() and np.array_equal(flags, wflags)


# ---------------------------------------------------------------------------------------------------------------------------
# every case reaches what it claims
def test_grid_caps_are_crossed():
    c = R.preproc_case("cap")
    assert c["S_h"] * c["S_w"] // 4 > R.PRE_WG * R.PRE_THREADS and c["S_w"] % 4 == 0
    assert all(c["S_h"] * c["S_w"] // 4 <= R.PRE_WG * R.PRE_THREADS for c in map(R.preproc_case, SMALL_PREPROC))
    for name in ("cap", "cap_mix"):
        a = R.augment_case(name)
        assert a["S_h"] * a["S_w"] // 4 > R.PRE_WG * R.PRE_THREADS
    assert (R.SCALE_CAP_ROWS - 1) * 51 <= R.SCALE_WG * R.SCALE_THREADS < R.SCALE_CAP_ROWS * 51 and R.SCALE_CAP_ROWS == 10281
    # resize_bilinear_f32: none of the existing shapes leaves the first trip or has more planes than grid.y (tests/test_gpu_multiscale.py
    # runs them with 2 x 3 planes); the added one does both
    for src, dst in ro.SHAPES:
        bx, by = R.resize_grid(6, *dst)
        assert dst[0] * dst[1] <= R.RESIZE_WG * 256 and by == 6
    n, src, dst = R.RESIZE_CAP
    bx, by = R.resize_grid(n, *dst)
    assert dst[0] * dst[1] > R.RESIZE_WG * 256 and bx == R.RESIZE_WG and by < n
    # the sector family: the full warps tests/test_gpu_sector.py runs cross every cap, so no large case is added for them
    # (each of them runs as resize + gather and as the fused warp, image and mask, with mask_bbox behind)
    pixels = []
    for theta, h, w in R.SECTOR_FULL:
        g = fo.geometry(theta, h, w)
        pixels.append(g["oh"] * g["ow"])
        print("sector %d deg %d x %d: %d x %d = %d pixels, T = %d" % (theta, h, w, g["oh"], g["ow"], pixels[-1], g["T"]))
        assert pixels[-1] > R.BBOX_WG * 256 and g["T"] * fo.N > R.RESIZE_U8_WG * 256
    assert max(pixels) > R.WARP_WG * 256 > R.GATHER_WG * 256


def test_preproc_cases_reach_their_paths():
    seen = dict(right=False, below=False, both=False, none=False, cut=False, flat=False, pad=False, offsets=False)
    for name in SMALL_PREPROC:
        c = R.preproc_case(name)
        offs = []
        for (off, h, w, ld, rh, rw) in c["desc"].tolist():
            seen["right"] |= 0 < rw < c["S_w"] and rh == c["S_h"]
            seen["below"] |= 0 < rh < c["S_h"] and rw == c["S_w"]
            seen["both"] |= 0 < rh < c["S_h"] and 0 < rw < c["S_w"]
            seen["none"] |= rh == c["S_h"] and rw == c["S_w"]
            seen["cut"] |= rw % 4 != 0 and rh > 0
            seen["flat"] |= rh == 0 or rw == 0
            seen["pad"] |= ld > 3 * w
            offs.append(off % 16)
        seen["offsets"] |= len(offs) > 1 and len(set(offs)) == len(offs)
    assert all(seen.values()), seen
    c = R.preproc_case("flat")
    assert c["desc"][0].tolist()[1:3] == [1, 4000] and c["desc"][0][4] == 0
    assert R.preproc_case("narrow")["S_w"] == 4
    assert [d[1:3] for d in R.preproc_case("1x1")["desc"].tolist()] == [[1, 1]]
    assert R.LABEL_MAX == (1, 5, 6, 50) and [m * 51 for m in R.LABEL_MAX[:3]] == [51, 255, 306]          # below, one short of, beyond 256
    for m in R.LABEL_MAX:
        assert R.labels_case(m)["counts"][:3] == [m, 0, m + 3]


def test_augment_image_cases_reach_their_paths():
    c = R.augment_case("meet")
    S_h, S_w = c["S_h"], c["S_w"]
    ys, xs = np.mgrid[0:S_h, 0:S_w]
    P = c["params"][0]
    u, v = P[6] * xs + P[7] * ys + P[8], P[9] * xs + P[10] * ys + P[11]
    d = c["tiles"][0]
    assert ((u == d[1][6] - 0.5) & (v == d[2][7] - 0.5)).sum() == 1                 # one pixel exactly on the corner where four regions meet
    assert d[0][10] < 0 and d[0][6] == 0                                             # tile 0 is cropped on the negative side
    assert all(int(t[3]) > 3 * int(t[2]) for t in d) and c["flags"][:, 0].tolist() == [0, 1]
    _, owned = R.augment_u8_ref(c["buf"], c["tiles"], c["tscale"], c["params"], c["flags"], None, None, S_h, S_w)
    own = [((u >= t[6] - 0.5) & (u < t[8] - 0.5) & (v >= t[7] - 0.5) & (v < t[9] - 0.5)).sum() for t in d]
    assert all(o > 0 for o in own) and not owned[0].all()                            # all four tiles and padding are on the image
    c = R.augment_case("mix")
    assert c["mixi"][:, 0].tolist() == [1, 0, 1] and c["mixi"][0, 11] == 1 and c["mixi"][2, 11] == 0
    out, owned = R.augment_u8_ref(c["buf"], c["tiles"], c["tscale"], c["params"], c["flags"], c["mixi"], c["mixd"], S_h, S_w)
    base, towned = R.augment_u8_ref(c["buf"], c["tiles"], c["tscale"], c["params"], c["flags"], None, None, S_h, S_w)
    X = c["mixi"][0]
    assert X[7] < S_w and X[8] < S_h and X[9] == 0 and X[10] == 0                    # the jittered canvas lies inside the window
    free = ~towned[0]
    assert (out[0][0][free] == 57).any() and (out[0][0][free & ~owned[0]] == 114).any() and (owned[0] & free).any()
    assert np.array_equal(out[1], base[1])                                           # the image without a partner is the plain one


def test_hsv_case_holds_every_kind_of_pixel():
    c = R.hsv_case()
    base, owned = R.augment_u8_ref(c["buf"], c["tiles"], c["tscale"], c["params"], c["flags"], None, None, c["S_h"], c["S_w"])
    assert np.array_equal(base[0][:, :, :8], c["image"].transpose(2, 0, 1)) and (base[0][:, :, 8:] == 114).all()      # shown 1 : 1
    assert np.array_equal(base[1][:, :, ::-1][:, :, :8], c["image"].transpose(2, 0, 1))
    b, g, r = (c["image"][..., k].reshape(-1).astype(np.float64) for k in range(3))
    v, mn = np.maximum(np.maximum(b, g), r), np.minimum(np.minimum(b, g), r)
    assert ((v == mn) & (v > 0)).any() and (v == 0).any()
    with np.errstate(all="ignore"):
        h = np.where(v == mn, -1, np.where(v == r, (60 * (g - b) / (v - mn)) % 360, np.where(v == g, 120 + 60 * (b - r) / (v - mn), 240 + 60 * (r - g) / (v - mn))))
        s = np.where(v > 0, (v - mn) * 255 / np.maximum(v, 1), 0)
    assert {int(x // 60) for x in h[h >= 0]} == {0, 1, 2, 3, 4, 5}
    for dh, ds, dv in c["params"][:, 12:15]:
        if ds > 0:
            assert (s + ds > 255).any() and (v + dv > 255).any() or dv < 0
        else:
            assert (s + ds < 0).any()
    assert any((v + p[14] < 0).any() for p in c["params"]) and any((v + p[14] > 255).any() for p in c["params"])
    o32, _ = R.augment_u8_ref(c["buf"], c["tiles"], c["tscale"], c["params"], c["flags"], None, None, c["S_h"], c["S_w"], hsv_dtype=np.float32)
    o64, _ = R.augment_u8_ref(c["buf"], c["tiles"], c["tscale"], c["params"], c["flags"], None, None, c["S_h"], c["S_w"], hsv_dtype=np.float64)
    measured = float(np.abs(o32 - o64).max())
    print("hsv case: float32 vs float64 oracle %.3g -> bound %.3g" % (measured, 4 * measured))
    assert 0 < measured < 1e-2 and np.abs(o64 - base).max() > 10 and np.array_equal(o64[~np.stack([owned] * 3, 1)], base[~np.stack([owned] * 3, 1)])


@pytest.mark.parametrize("max_labels", sorted(R.LAB_BATCH))
def test_label_cases_reach_their_paths(max_labels):
    """candidates and survivors are what the patterns say, no decision is near its threshold, every ray meets one edge"""
    c = R.label_case(max_labels)
    table, counts, info = R.augment_labels_ref(c["rows"], c["tiles"], c["tscale"], c["params"], c["flags"], c["mixi"], c["mixd"], c["S_h"], c["S_w"],
                                               R.LAB_MARGIN, max_labels)
    want = R.label_expectation(max_labels)
    print("max_labels %d: candidates %s survivors %s; centre margin %.3g, extent margin %.3g" %
          (max_labels, info["cands"], counts.tolist(), info["centre_margin"], info["extent_margin"]))
    assert info["cands"] == [w[0] for w in want] and info["kept"] == [w[1] for w in want]
    assert info["centre_margin"] > 1e-3 and info["extent_margin"] > 1e-3 and all((h == 1).all() for h in info["hits"])
    assert np.abs(table[..., 1:]).max() < 1024                                       # an fp32 ulp of a coordinate is at most 6.1e-5
    cands = set(info["cands"])
    if max_labels >= 6:
        assert {0, 9, 10, 11, 20, 21} <= cands
        assert any(cnt > max_labels for cnt in counts)                               # survivors exceed the rows
    if max_labels == 6:
        kept = info["kept"][6]
        assert kept[max_labels - 1] < R.CHUNK - 1 and kept[max_labels] == R.CHUNK - 1 and kept[max_labels + 1] == R.CHUNK      # the overflow straddles a chunk
    assert any(int(t[13] - t[12]) > max_labels for T in c["tiles"] for t in T)       # a tile holds more rows than max_labels
    first_partner = [sum(min(int(t[13] - t[12]), max_labels) for t in T) for T, X in zip(c["tiles"], c["mixi"]) if X[0]]
    assert first_partner and all(f % R.CHUNK != 0 for f in first_partner)            # the partner's rows start mid-chunk
    assert any(9 in k and any(j > 9 for j in k) for k in info["kept"]) or max_labels == 1


@pytest.mark.parametrize("max_labels", R.SECTOR_MAX)
def test_sector_cases_reach_their_paths(max_labels):
    c = R.sector_case(max_labels)
    cand, keep, out, counts, flags, margins = R.sector_labels_ref(c["rows"], c["geo"], max_labels)
    print("max_labels %d: kept %s, margins %s" % (max_labels, counts.tolist(), margins))
    assert min(margins.values()) > 1e-6
    assert [int(G[11]) for G in c["geo"]] == [0, 1, max_labels, max_labels + 3]
    assert keep[1, 0] == 3                                                           # the single row: kept, centre fell back
    if max_labels >= 5:
        k = keep[2]
        assert (k == 0).any() and (k == 1).any() and (k == 3).any()                  # dropped, kept, kept with fell_back, interleaved
        assert (k[:-1] != k[1:]).sum() > max_labels // 3
    if max_labels > R.COMPACT_PASS:
        assert (keep[2, R.COMPACT_PASS:] & 1).any() and (keep[2, :R.COMPACT_PASS] & 1).sum() > 100        # both passes pack
        assert max_labels < 300 or (keep[2, R.COMPACT_PASS:] == 3).any()                 # a flagged row in the second pass
    assert (max_labels % R.ROWS_PER_WG != 0) == (max_labels in (1, 2, 3, 5, 50, 257))
    assert np.abs(out[np.isfinite(out)]).max() < 2048 if counts.any() else True


def test_paste_cases_reach_what_the_existing_ones_do_not():
    """tests/test_copypaste_oracle.py's CASES run S = 48 x 80 (VEC) and 50 x 70 (VEC = false by S_w % 4, both tile edges cut, 6 columns
    and 2 rows left) with max_labels 6 and 50 and fewer than 64 candidates.  Added: one column / one row left, VEC = false by
    alignment alone, max_labels = 256 with candidates 64 .. 69, and a pasted pixel whose source column does not exist."""
    from test_copypaste_oracle import SIZES
    assert sorted(SIZES) == [(48, 80), (50, 70)] and 70 % R.TW == 6 and 50 % R.TH == 2
    c = R.paste_case("cut")
    assert c["S"][1] % R.TW == 1 and c["S"][0] % R.TH == 1 and not R.paste_vec(c["S"][1], 0, 0)
    c = R.paste_case("shifted")
    assert R.paste_vec(c["S"][1], 0, 0) and not R.paste_vec(c["S"][1], 4, 4)
    for name in R.PASTE_NEW:
        c = R.paste_case(name)
        rows, counts, ranges, dec = co.paste_labels(c["pre_labels"], c["pre_count"], c["paste"], c["S"], R.PASTE_MARGIN, R.PASTE_THR, c["max_labels"])
        close = [d for d in dec if d["distance"] is not None and d["distance"] < (1e-6 if d["kind"] == "ioa" else 1e-3)]
        assert not close, (name, close[:2])
        img, pasted = R.paste_u8_ref(c["pre_images"], rows, ranges, c["paste"])
        print(name, "ranges", ranges.tolist(), "pasted pixels", pasted.sum((1, 2)).tolist())
        if name in ("cut", "shifted"):
            assert ranges.tolist() == [[0, 2], [2, 2], [0, 2]]
            assert pasted[0][:, -1].any() and pasted[0][-1].any() and pasted[2][:, 0].any()      # the last column, the last row, the first column
        if name == "rows256":
            assert c["max_labels"] == R.MAX_ROWS and c["pre_count"].tolist() == [3, 70, 256, 0]
            acc = co.accepted(dec)
            vetoed = {d["cand"] for d in dec if d["image"] == 0 and d["kind"] == "ioa" and not d["passed"]}
            assert vetoed == {12, 37} and {k for i, k in acc if i == 0} == set(range(64)) - vetoed
            assert ranges.tolist() == [[3, 65], [70, 70], [256, 256], [0, 3]] and counts.tolist() == [65, 70, 256, 3]
            assert any(d["kind"] == "select" and d["cand"] >= 64 for d in dec if d["image"] == 0)
        if name == "nosource":
            inside = co.centres_inside(rows[0, 0, 3:], *c["S"])
            assert ranges.tolist() == [[0, 1], [1, 2]] and (inside & ~pasted[0]).any() and pasted[0].any()


# ---------------------------------------------------------------------------------------------------------------------------
# the mutants
def _preproc(mutant):
    return [R.preproc_u8_ref(c["buf"], c["desc"], c["scales"], c["S_h"], c["S_w"], mutant) for c in map(R.preproc_case, SMALL_PREPROC)]


def _aug(mutant):
    out = []
    for name in ("meet", "mix"):
        c = R.augment_case(name)
        out.append(R.augment_u8_ref(c["buf"], c["tiles"], c["tscale"], c["params"], c["flags"], c["mixi"], c["mixd"], c["S_h"], c["S_w"], mutant=mutant)[0])
    return out


def _aug_labels(mutant):
    out = []
    for ml in sorted(R.LAB_BATCH):
        c = R.label_case(ml)
        t, cnt, _ = R.augment_labels_ref(c["rows"], c["tiles"], c["tscale"], c["params"], c["flags"], c["mixi"], c["mixd"], c["S_h"], c["S_w"], R.LAB_MARGIN,
                                         ml, mutant)
        out += [t, cnt]
    return out


def _pre_labels(mutant):
    out = [R.preproc_labels_ref(c["rows"], c["row_off"], c["whr"], m, mutant) for m, c in ((m, R.labels_case(m)) for m in R.LABEL_MAX)]
    lab = np.random.RandomState(1).rand(3, 51).astype(np.float32)
    return out + [R.scale_labels_ref(lab, *R.SCALES, mutant)]


def _resize(mutant):
    x = np.random.RandomState(2).randn(2, 5, 7).astype(np.float32)
    return [R.resize_bilinear_ref(x, 64, 96, mutant)]


def _sector(mutant):
    out = []
    for ml in (5, 257):
        c = R.sector_case(ml)
        out += list(R.sector_labels_ref(c["rows"], c["geo"], ml, mutant)[2:5])
    return out


def _paste(mutant):
    out = []
    for name in ("cut", "nosource"):
        c = R.paste_case(name)
        rows, _, ranges, _ = co.paste_labels(c["pre_labels"], c["pre_count"], c["paste"], c["S"], R.PASTE_MARGIN, R.PASTE_THR, c["max_labels"])
        out.append(R.paste_u8_ref(c["pre_images"], rows, ranges, c["paste"], mutant)[0])
    return out


FAMILIES = dict(preproc=_preproc, augment=_aug, augment_labels=_aug_labels, labels=_pre_labels, resize=_resize, sector=_sector, paste=_paste)
KILLED_BY = dict(last_quad=("preproc", "augment"), x1_clamp=("resize",), pixel_mirror=("augment",), label_mirror=("augment_labels",),
                 tile_cap=("augment_labels",), slot_chunk=("augment_labels",), overflow_written=("augment_labels",),
                 tail=("labels", "augment_labels", "sector"), compact_carry=("sector",), stride=("preproc", "augment"), xy_swap=("labels",),
                 edge_column=("paste",))


@pytest.fixture(scope="module")
def clean():
    return {k: f(None) for k, f in FAMILIES.items()}


@pytest.mark.parametrize("mutant", R.MUTANTS)
def test_every_mutant_changes_an_expected_output(clean, mutant):
    assert set(KILLED_BY) == set(R.MUTANTS)
    for fam in KILLED_BY[mutant]:
        got = FAMILIES[fam](mutant)
        changed = [i for i, (a, b) in enumerate(zip(got, clean[fam])) if differs(a, b)]
        print("%s on %s: outputs changed %s" % (mutant, fam, changed))
        assert changed, (mutant, fam)


def test_mutants_touch_nothing_else(clean):
    """a mutant leaves the families it does not belong to bit-identical: each name means one mistake"""
    for mutant in R.MUTANTS:
        for fam, f in FAMILIES.items():
            if fam not in KILLED_BY[mutant]:
                assert not any(differs(a, b) for a, b in zip(f(mutant), clean[fam])), (mutant, fam)
