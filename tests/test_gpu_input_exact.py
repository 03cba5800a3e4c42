"""The kernels in front of the network - csrc/preproc.hip (ep24_preproc_u8, ep24_preproc_labels, ep24_scale_labels,
ep24_resize_bilinear_f32), csrc/augment.hip (ep24_augment_u8, ep24_augment_mix_u8, ep24_augment_labels, ep24_augment_mix_labels),
csrc/sector.hip (ep24_sector_labels, ep24_sector_gather, ep24_sector_warp_u8, ep24_resize_linear_u8, ep24_mask_bbox) and csrc/paste.hip
(ep24_paste_labels, ep24_paste_u8) - against tests/input_reference.py, through the C ABI.  tests/test_input_reference.py shows without a
GPU that the references equal the committed goldens and the existing oracles, that every case reaches what it claims, and that twelve
mutants are rejected on these inputs.

Every buffer, inputs included, sits between two guards of 64 sentinel elements and whole buffers are compared: the 114 fill right of
and below the resized area, label rows beyond the count, out_count, keep, out_flags, paste_range, cand rows the kernel must not
write, and every input a call must leave alone.  Outputs start as the sentinel, so an element a loop skipped shows.

Bit for bit: everything, except
  HSV             |got - float64 oracle| <= 4 x max |float32 oracle - float64 oracle| on the case's own pixels (the rule of
                  tests/test_gpu_augment.py: the margin is for instruction order, and it is not taken from the kernel);
  re-cast labels  coordinates of ep24_augment_labels / ep24_augment_mix_labels / ep24_sector_labels within 1e-3 px of the float64
                  reference (the bound the repository has), their class column, counts, row order, flags and zero tails exact.

The sizes come from the constants of the .hip files (restated in tests/input_reference.py):
  preproc_u8, augment_u8<MIX>   4096 workgroups x 256 quads: 2048 x 2052 = 1 050 624 quads, one image
  preproc_labels                256 threads over max_labels x 51: max_labels 1 (51), 5 (255), 6 (306), 50
  scale_labels                  2048 x 256 elements: 10 281 rows
  resize_bilinear_f32           2048 workgroups, grid.y = 8192 / grid.x: 5 planes of 725 x 724 (none of resize_oracle.SHAPES leaves the
                                first trip, and tests/test_gpu_multiscale.py's 6 planes never exceed grid.y)
  augment_labels                CHUNK = 10: 0, 9, 10, 11, 20, 21 candidates at max_labels 6 and 50, an overflow across a chunk boundary,
                                a tile with more rows than max_labels, the partner's rows from the middle of a chunk; max_labels 1
  sector_labels / compact       4 rows per workgroup, 256 row slots per pass: max_labels 1, 2, 3, 5, 50, 256, 257, 300
  sector_gather, sector_warp_u8, resize_linear_u8, mask_bbox: the full warps of tests/test_gpu_sector.py already cross their caps
                                (test_grid_caps_are_crossed); here small crafted maps, plus a 257 x 259 mask for mask_bbox's 65 536 threads
  paste_u8                      64 x 16 tiles: S = 17 x 65; VEC = false by alignment alone; max_labels = 256 (53 248 bytes of LDS)

No case found a kernel or launcher bug, so csrc/ is unchanged.  The three places the issue names: ep24_paste_labels / ep24_paste_u8 at
max_labels = 256 run and are exact (test_paste[rows256]: 62 rows pasted, candidates 64 .. 69 left alone, a full table takes nothing) and
refuse 257; ep24_preproc_labels with a null ``rows`` and no row in the batch reads nothing through it and writes zeros (the host cannot
refuse it: the counts are in device memory); ep24_sector_labels refuses n > 65535 before any launch.

50 cases; on an MI355X the file takes 4.5 s, its slowest cases 1.06 s (test_paste[rows256]: the host's sequential walk over 64
candidates), 0.54 s (augment_mix_u8 beyond its cap), 0.49 s (preproc_u8 beyond its cap), 0.36 s (augment_u8 beyond its cap).
Largest figures, printed as INPUT-ERR before each assertion and measured against the float64 references:
  HSV                 6.46e-5 against a bound of 2.58e-4 (float32 oracle vs float64 oracle 6.46e-5), both instantiations
  augment labels      7.6e-6 px = 0.500 fp32 ulp (max_labels 1, 6, 50, with and without partner rows): the correctly rounded value
  sector labels       1.53e-5 px = 0.500 fp32 ulp (max_labels 256 .. 300; 7.6e-6 px at the smaller tables)
"""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import augment_oracle as ao  # noqa: E402
import copypaste_oracle as co  # noqa: E402
import input_reference as R  # noqa: E402
import update_reference as U  # noqa: E402
from oracle import sector as osec  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
E_ARG = -1
I32_SENT = 0x5A5A5A5A
LABEL_TOL = 1e-3                     # px: the bound of tests/test_gpu_augment.py and tests/test_gpu_fisheye.py


def _abi():
    from ep24._lib import call, lib, stream_ptr
    return call, stream_ptr, lib()


def G(n, kind, fill=None):
    return U.Guarded(n, kind, DEV, fill)


def Gf64(a):
    return G(np.asarray(a).size, "f64", R.f64bits(a).reshape(-1))


def Gi64(a):
    return G(np.asarray(a).size, "i64", np.asarray(a, dtype=np.int64).reshape(-1))


def Gi32(a):
    return G(np.asarray(a).size, "i32", np.asarray(a, dtype=np.int32).reshape(-1))


def Gu8(a):
    return G(np.asarray(a).size, "u8", np.asarray(a, dtype=np.uint8).reshape(-1))


def Gf32(a):
    return G(np.asarray(a).size, "f32", R.f32bits(a).reshape(-1))


def sync():
    torch.cuda.synchronize()


def unchanged(*bufs):
    """input buffers and their guards are as they were uploaded"""
    for k, b in enumerate(bufs):
        if b is not None:
            b.check(b.host[U.GUARD:U.GUARD + b.n], "input %d" % k)


def guards(buf, what):
    """only the guards (the window is compared under a bound by the caller) -> the window as float32"""
    win = buf.check(buf.read()[0], what)
    return U.from_bits32(win)


def report(what, **figures):
    print("INPUT-ERR %s: %s" % (what, ", ".join("%s %.3g" % kv for kv in figures.items())))


def ulps(got32, want64):
    """the largest |got - want| in units of the fp32 spacing at want"""
    want64 = np.asarray(want64, dtype=np.float64)
    sp = np.spacing(np.maximum(np.abs(want64), 2.0 ** -20).astype(np.float32)).astype(np.float64)
    return float((np.abs(np.asarray(got32, dtype=np.float64) - want64) / sp).max()) if want64.size else 0.0


# ---------------------------------------------------------------------------------------------------------------------------
# csrc/preproc.hip
@pytest.mark.parametrize("name", list(R.PREPROC_CASES))
def test_preproc_u8(name):
    call, sp, _ = _abi()
    c = R.preproc_case(name)
    n, S_h, S_w = len(c["desc"]), c["S_h"], c["S_w"]
    buf, desc, scales = Gu8(c["buf"]), Gi64(c["desc"]), Gf64(c["scales"])
    out = G(n * 3 * S_h * S_w, "f32")
    call("preproc_u8", buf.ptr(), desc.ptr(), scales.ptr(), n, out.ptr(), S_h, S_w, sp())
    sync()
    out.check(R.f32bits(R.preproc_u8_ref(c["buf"], c["desc"], c["scales"], S_h, S_w)).reshape(-1), "preproc_u8 %s" % name)
    unchanged(buf, desc, scales)


def test_preproc_u8_refusals():
    """EP24_E_ARG before any launch: S_w % 4 != 0, an output 4 bytes off a 16-byte boundary, n > 65535, null pointers, sizes <= 0;
    n = 0 is not an error and launches nothing"""
    _, sp, lib = _abi()
    fn = lib.fn["ep24_preproc_u8"]
    c = R.preproc_case("narrow")
    buf, desc, scales = Gu8(c["buf"]), Gi64(c["desc"]), Gf64(c["scales"])
    out = G(2 * 3 * 5 * 8 + 4, "f32")
    good = dict(images=buf.ptr(), desc=desc.ptr(), scales=scales.ptr(), n=2, out=out.ptr(), S_h=5, S_w=4)
    for bad in (dict(S_w=6), dict(S_w=5), dict(out=out.ptr(1)), dict(n=65536), dict(n=-1), dict(images=None), dict(desc=None), dict(scales=None),
                dict(out=None), dict(S_h=0), dict(S_w=0)):
        a = dict(good, **bad)
        assert fn(a["images"], a["desc"], a["scales"], a["n"], a["out"], a["S_h"], a["S_w"], sp()) == E_ARG, bad
    assert fn(None, None, None, 0, None, 5, 4, sp()) == 0
    sync()
    out.check(np.full(out.n, U.SENT32, dtype=np.uint32), "a refused call wrote")


@pytest.mark.parametrize("max_labels", R.LABEL_MAX)
def test_preproc_labels(max_labels):
    """counts max_labels, 0, max_labels + 3, min(2, max_labels) in one launch: bit for bit (float)((t * w) * r), zero behind the count"""
    call, sp, _ = _abi()
    c = R.labels_case(max_labels)
    rows, off, whr = Gf64(c["rows"]), Gi64(c["row_off"]), Gf64(c["whr"])
    out = G(4 * max_labels * 51, "f32")
    call("preproc_labels", rows.ptr(), off.ptr(), whr.ptr(), 4, out.ptr(), max_labels, sp())
    sync()
    out.check(R.f32bits(R.preproc_labels_ref(c["rows"], c["row_off"], c["whr"], max_labels)).reshape(-1), "preproc_labels %d" % max_labels)
    unchanged(rows, off, whr)


def test_preproc_labels_without_rows_and_refusals():
    """a batch without a single row: the one-row dummy the wrapper uploads, and no row table at all (nothing is read through it)"""
    call, sp, lib = _abi()
    off, whr = Gi64(np.zeros(4)), Gf64(R.labels_case(5)["whr"][:3])
    dummy = Gf64(np.full(51, 0.25))
    for rows in (dummy.ptr(), None):
        out = G(3 * 5 * 51, "f32")
        call("preproc_labels", rows, off.ptr(), whr.ptr(), 3, out.ptr(), 5, sp())
        sync()
        out.check(np.zeros(out.n, dtype=np.uint32), "labels of a batch without rows")
    fn = lib.fn["ep24_preproc_labels"]
    out = G(3 * 5 * 51, "f32")
    good = dict(rows=dummy.ptr(), off=off.ptr(), whr=whr.ptr(), n=3, out=out.ptr(), ml=5)
    for bad in (dict(off=None), dict(whr=None), dict(out=None), dict(ml=0), dict(ml=-4), dict(n=-1)):
        a = dict(good, **bad)
        assert fn(a["rows"], a["off"], a["whr"], a["n"], a["out"], a["ml"], sp()) == E_ARG, bad
    assert fn(None, None, None, 0, None, 5, sp()) == 0
    sync()
    out.check(np.full(out.n, U.SENT32, dtype=np.uint32), "a refused call wrote")
    unchanged(off, whr, dummy)


@pytest.mark.parametrize("rows", R.SCALE_ROWS)
def test_scale_labels(rows):
    """out of place and in place, scales 1.3 and 0.7 as the ABI's floats; the table holds negative values, zeros and a NaN"""
    call, sp, lib = _abi()
    rng = np.random.RandomState(rows)
    lab = (rng.rand(rows, 51) * 1280 - 100).astype(np.float32)
    lab[rng.rand(rows, 51) < 0.1] = 0.0
    lab[0, 7] = np.nan
    sx, sy = U.f32(R.SCALES[0]), U.f32(R.SCALES[1])
    want = R.f32bits(R.scale_labels_ref(lab, sx, sy)).reshape(-1)
    src, dst = Gf32(lab), G(rows * 51, "f32")
    call("scale_labels", src.ptr(), dst.ptr(), rows, sx, sy, sp())
    sync()
    dst.check(want, "scale_labels %d rows" % rows)
    unchanged(src)
    call("scale_labels", src.ptr(), src.ptr(), rows, sx, sy, sp())
    sync()
    src.check(want, "scale_labels %d rows in place" % rows)
    fn = lib.fn["ep24_scale_labels"]
    for bad in ((None, dst.ptr(), rows), (src.ptr(), None, rows), (src.ptr(), dst.ptr(), 0), (src.ptr(), dst.ptr(), -1)):
        assert fn(bad[0], bad[1], bad[2], sx, sy, sp()) == E_ARG, bad


def test_resize_bilinear_beyond_its_cap():
    call, sp, _ = _abi()
    n, (sh, sw), (dh, dw) = R.RESIZE_CAP
    x = np.random.RandomState(4).randn(n, sh, sw).astype(np.float32)
    src, dst = Gf32(x), G(n * dh * dw, "f32")
    call("resize_bilinear_f32", src.ptr(), n, sh, sw, dst.ptr(), dh, dw, sp())
    sync()
    dst.check(R.f32bits(R.resize_bilinear_ref(x, dh, dw)).reshape(-1), "resize_bilinear_f32 %d planes -> %d x %d" % (n, dh, dw))
    unchanged(src)


# ---------------------------------------------------------------------------------------------------------------------------
# csrc/augment.hip: the image half
def _augment_u8(c, mix):
    call, sp, _ = _abi()
    n, S_h, S_w = len(c["tiles"]), c["S_h"], c["S_w"]
    ins = [Gu8(c["buf"]), Gi64(c["tiles"]), Gf64(c["tscale"]), Gf64(c["params"]), Gi32(c["flags"])]
    out = G(n * 3 * S_h * S_w, "f32")
    if mix:
        mixi = c["mixi"] if c["mixi"] is not None else np.zeros((n, R.MIX_I), dtype=np.int64)
        mixd = c["mixd"] if c["mixd"] is not None else np.zeros((n, R.MIX_D))
        ins += [Gi64(mixi), Gf64(mixd)]
        call("augment_mix_u8", *[b.ptr() for b in ins], n, out.ptr(), S_h, S_w, sp())
    else:
        call("augment_u8", *[b.ptr() for b in ins], n, out.ptr(), S_h, S_w, sp())
    sync()
    unchanged(*ins)
    return out


@pytest.mark.parametrize("name,mix", [("meet", False), ("meet", True), ("mix", True), ("cap", False), ("cap_mix", True)])
def test_augment_u8_without_hsv(name, mix):
    """hand-built descriptors, bit for bit; "meet" through ep24_augment_mix_u8 with every partner off is the plain instantiation's image"""
    c = R.augment_case(name)
    want, _ = R.augment_u8_ref(c["buf"], c["tiles"], c["tscale"], c["params"], c["flags"], c["mixi"], c["mixd"], c["S_h"], c["S_w"])
    _augment_u8(c, mix).check(R.f32bits(want.astype(np.float32)).reshape(-1), "augment_u8 %s" % name)


@pytest.mark.parametrize("mix", [False, True])
def test_augment_u8_hsv(mix):
    c = R.hsv_case()
    args = (c["buf"], c["tiles"], c["tscale"], c["params"], c["flags"], None, None, c["S_h"], c["S_w"])
    base, owned = R.augment_u8_ref(*args)
    o32, _ = R.augment_u8_ref(*args, hsv_dtype=np.float32)
    o64, _ = R.augment_u8_ref(*args, hsv_dtype=np.float64)
    bound = 4.0 * float(np.abs(o32 - o64).max())
    got = guards(_augment_u8(c, mix), "augment_u8 hsv").astype(np.float64).reshape(o64.shape)
    err = float(np.abs(got - o64).max())
    report("hsv mix %d" % mix, float32_vs_float64=bound / 4, bound=bound, gpu_vs_float64=err)
    free = ~np.stack([owned] * 3, 1)
    assert np.array_equal(got[free], base[free])                                     # padding keeps 114 exactly
    assert 0 < bound < 4e-2 and err <= bound


def test_augment_u8_refusals():
    _, sp, lib = _abi()
    c = R.augment_case("meet")
    ins = [Gu8(c["buf"]), Gi64(c["tiles"]), Gf64(c["tscale"]), Gf64(c["params"]), Gi32(c["flags"]), Gi64(np.zeros((2, 16))), Gf64(np.zeros((2, 12)))]
    out = G(2 * 3 * 24 * 32 + 4, "f32")
    p = [b.ptr() for b in ins]
    plain, mixed = lib.fn["ep24_augment_u8"], lib.fn["ep24_augment_mix_u8"]
    for S_w, n, o in ((30, 2, out.ptr()), (32, 2, out.ptr(1)), (32, 65536, out.ptr()), (32, 2, None), (0, 2, out.ptr())):
        assert plain(*p[:5], n, o, 24, S_w, sp()) == E_ARG and mixed(*p, n, o, 24, S_w, sp()) == E_ARG, (S_w, n)
    for k in range(7):
        q = list(p)
        q[k] = None
        assert mixed(*q, 2, out.ptr(), 24, 32, sp()) == E_ARG and (k >= 5 or plain(*q[:5], 2, out.ptr(), 24, 32, sp()) == E_ARG), k
    sync()
    out.check(np.full(out.n, U.SENT32, dtype=np.uint32), "a refused call wrote")


# ---------------------------------------------------------------------------------------------------------------------------
# the label half
def check_table(got, want64, counts, max_labels, what):
    """class column, occupied rows and the zero tail exactly; coordinates under the bound -> (largest difference in px, in fp32 ulp)"""
    n = len(counts)
    got = got.reshape(n, max_labels, 51)
    filled = np.minimum(np.asarray(counts), max_labels)
    err = ulp = 0.0
    for i in range(n):
        k = int(filled[i])
        assert not U.bits32(got[i, k:]).any(), "%s: image %d, the rows behind %d are not +0" % (what, i, k)
        assert np.array_equal(got[i, :k, 0], want64[i, :k, 0].astype(np.float32)), "%s: image %d, class column / row order" % (what, i)
        if k:
            err = max(err, float(np.abs(got[i, :k].astype(np.float64) - want64[i, :k]).max()))
            ulp = max(ulp, ulps(got[i, :k, 1:], want64[i, :k, 1:]))
    return err, ulp


@pytest.mark.parametrize("mix", [False, True])
@pytest.mark.parametrize("max_labels", sorted(R.LAB_BATCH))
def test_augment_labels(max_labels, mix):
    """the candidate counts and overflow patterns of LAB_BATCH; without ``mix`` the same batch through ep24_augment_labels, which has
    no partner rows"""
    call, sp, _ = _abi()
    c = R.label_case(max_labels)
    n, S_h, S_w = len(c["tiles"]), c["S_h"], c["S_w"]
    mixi, mixd = (c["mixi"], c["mixd"]) if mix else (None, None)
    want, counts, info = R.augment_labels_ref(c["rows"], c["tiles"], c["tscale"], c["params"], c["flags"], mixi, mixd, S_h, S_w, R.LAB_MARGIN, max_labels)
    ins = [Gf64(c["rows"]), Gi64(c["tiles"]), Gf64(c["tscale"]), Gf64(c["params"]), Gi32(c["flags"])]
    if mix:
        ins += [Gi64(mixi), Gf64(mixd)]
    rot = Gf64(ao.RAY)
    out, cnt = G(n * max_labels * 51, "f32"), G(n, "i32")
    call("augment_mix_labels" if mix else "augment_labels", *[b.ptr() for b in ins], rot.ptr(), n, S_h, S_w, R.LAB_MARGIN, out.ptr(), cnt.ptr(),
         max_labels, sp())
    sync()
    cnt.check(counts.astype(np.int32), "out_count (survivors, those beyond max_labels included)")
    err, ulp = check_table(guards(out, "augment_labels"), want, counts, max_labels, "augment_labels %d mix %d" % (max_labels, mix))
    report("augment_labels max_labels %d mix %d" % (max_labels, mix), px=err, ulp=ulp, survivors=float(counts.sum()))
    assert err <= LABEL_TOL
    unchanged(rot, *ins)


def test_augment_labels_refusals():
    _, sp, lib = _abi()
    c = R.label_case(1)
    n = len(c["tiles"])
    ins = [Gf64(c["rows"]), Gi64(c["tiles"]), Gf64(c["tscale"]), Gf64(c["params"]), Gi32(c["flags"]), Gi64(c["mixi"]), Gf64(c["mixd"]), Gf64(ao.RAY)]
    out, cnt = G(n * 51, "f32"), G(n, "i32")
    p = [b.ptr() for b in ins]
    plain, mixed = lib.fn["ep24_augment_labels"], lib.fn["ep24_augment_mix_labels"]
    S_h, S_w = c["S_h"], c["S_w"]
    for k in range(8):
        q = list(p)
        q[k] = None
        assert mixed(*q, n, S_h, S_w, 2.0, out.ptr(), cnt.ptr(), 1, sp()) == E_ARG, k
        if k not in (5, 6):
            assert plain(*q[:5], q[7], n, S_h, S_w, 2.0, out.ptr(), cnt.ptr(), 1, sp()) == E_ARG, k
    for nn, sh, margin, o, k, ml in ((-1, S_h, 2.0, out.ptr(), cnt.ptr(), 1), (n, 0, 2.0, out.ptr(), cnt.ptr(), 1), (n, S_h, -1.0, out.ptr(), cnt.ptr(), 1),
                                     (n, S_h, 2.0, None, cnt.ptr(), 1), (n, S_h, 2.0, out.ptr(), None, 1), (n, S_h, 2.0, out.ptr(), cnt.ptr(), 0)):
        assert mixed(*p, nn, sh, S_w, margin, o, k, ml, sp()) == E_ARG and plain(*p[:5], p[7], nn, sh, S_w, margin, o, k, ml, sp()) == E_ARG
    sync()
    out.check(np.full(out.n, U.SENT32, dtype=np.uint32), "a refused call wrote")
    cnt.check(np.full(n, I32_SENT, dtype=np.int32), "a refused call wrote")


# ---------------------------------------------------------------------------------------------------------------------------
# csrc/sector.hip
@pytest.mark.parametrize("max_labels", R.SECTOR_MAX)
def test_sector_labels(max_labels):
    """four images with 0, 1, max_labels and max_labels + 3 rows: keep words, counts and flags whole, the packed table's class column,
    row order and zero tail exactly, coordinates under the bound; cand is written where a row is kept and nowhere else"""
    call, sp, _ = _abi()
    c = R.sector_case(max_labels)
    n = len(c["geo"])
    cand64, keep, want, counts, flags, _ = R.sector_labels_ref(c["rows"], c["geo"], max_labels)
    rows, geo, rot = Gf64(c["rows"]), Gf64(c["geo"]), Gf64(ao.RAY)
    cand, kp = G(n * max_labels * 51, "f32"), G(n * max_labels, "i32")
    out, cnt, fl = G(n * max_labels * 51, "f32"), G(n, "i32"), G(n * max_labels, "i32")
    call("sector_labels", rows.ptr(), geo.ptr(), rot.ptr(), n, max_labels, cand.ptr(), kp.ptr(), out.ptr(), cnt.ptr(), fl.ptr(), sp())
    sync()
    kp.check(keep.reshape(-1), "keep")
    cnt.check(counts, "out_count")
    fl.check(flags.reshape(-1), "out_flags")
    err, ulp = check_table(guards(out, "sector_labels out"), want, counts, max_labels, "sector_labels %d" % max_labels)
    got_cand = cand.check(cand.read()[0], "cand").reshape(n, max_labels, 51)
    written = (keep & 1).astype(bool)
    assert (got_cand[~written] == np.uint32(U.SENT32)).all(), "cand: a row that is not kept was written"
    if written.any():
        err = max(err, float(np.abs(U.from_bits32(got_cand[written]).astype(np.float64) - cand64[written]).max()))
    report("sector_labels max_labels %d" % max_labels, px=err, ulp=ulp, kept=float(counts.sum()))
    assert err <= LABEL_TOL
    unchanged(rows, geo, rot)


def test_sector_labels_refuses_a_batch_beyond_the_grid():
    _, sp, lib = _abi()
    c = R.sector_case(2)
    rows, geo, rot = Gf64(c["rows"]), Gf64(c["geo"]), Gf64(ao.RAY)
    bufs = [G(4 * 2 * 51, "f32"), G(8, "i32"), G(4 * 2 * 51, "f32"), G(4, "i32"), G(8, "i32")]
    fn = lib.fn["ep24_sector_labels"]
    for n, ml in ((65536, 2), (-1, 2), (4, 0)):
        assert fn(rows.ptr(), geo.ptr(), rot.ptr(), n, ml, *[b.ptr() for b in bufs], sp()) == E_ARG, (n, ml)
    sync()
    for b in bufs:
        b.check(np.full(b.n, b.sent).astype(U._NP[b.kind]), "a refused call wrote")


def test_sector_gather_warp_and_resize():
    """a crafted winner map with -1 at the crop's first and last pixel: gather with and without src_index, the index-only call, the
    fused warp against resize + gather, the stand-alone resize at sizes down to one row or column"""
    call, sp, lib = _abi()
    g = R.gather_case()
    T, n_ang, cw, y0, x0, oh, ow = g["T"], g["n_ang"], g["cw"], g["y0"], g["x0"], g["oh"], g["ow"]
    win, src, img = Gi32(g["winner"]), Gu8(g["src"]), Gu8(g["img"])
    want_dst, want_idx = R.sector_gather_ref(g["src"].reshape(-1), g["winner"].reshape(-1), cw, y0, x0, oh, ow, T, n_ang, 114)
    assert want_idx[0, 0] == -1 and want_idx[-1, -1] == -1 and (want_idx >= 0).sum() > oh * ow // 2
    for with_dst, with_idx in ((True, True), (True, False), (False, True)):
        dst, idx = G(oh * ow * 3, "u8"), G(oh * ow, "i32")
        call("sector_gather", src.ptr() if with_dst else None, win.ptr(), cw, y0, x0, oh, ow, T, n_ang, dst.ptr() if with_dst else None, 114,
             idx.ptr() if with_idx else None, sp())
        sync()
        dst.check(want_dst.reshape(-1) if with_dst else np.full(dst.n, U.SENT8, dtype=np.uint8), "sector_gather dst %d %d" % (with_dst, with_idx))
        idx.check(want_idx.reshape(-1) if with_idx else np.full(idx.n, I32_SENT, dtype=np.int32), "sector_gather src_index %d %d" % (with_dst, with_idx))
    sh, sw = g["img"].shape[:2]
    for fill in (114, 0):
        dst = G(oh * ow * 3, "u8")
        call("sector_warp_u8", img.ptr(), sh, sw, win.ptr(), cw, y0, x0, oh, ow, T, n_ang, dst.ptr(), fill, sp())
        sync()
        dst.check(R.sector_warp_ref(g["img"], g["winner"].reshape(-1), cw, y0, x0, oh, ow, T, n_ang, fill).reshape(-1), "sector_warp_u8 fill %d" % fill)
    unchanged(win, src, img)
    rng = np.random.RandomState(12)
    for (h, w), (dh, dw) in R.RESIZE_U8_SHAPES:
        a = rng.randint(0, 256, (h, w, 3)).astype(np.uint8)
        s, d = Gu8(a), G(dh * dw * 3, "u8")
        call("resize_linear_u8", s.ptr(), h, w, d.ptr(), dh, dw, sp())
        sync()
        d.check(osec.resize_linear_u8(a, dw, dh).reshape(-1), "resize_linear_u8 %dx%d -> %dx%d" % (h, w, dh, dw))
        unchanged(s)
    # refusals
    dst, idx = G(oh * ow * 3, "u8"), G(oh * ow, "i32")
    fn = lib.fn["ep24_sector_gather"]
    for a in ((src.ptr(), None, dst.ptr(), idx.ptr(), oh, T), (src.ptr(), win.ptr(), None, None, oh, T), (None, win.ptr(), dst.ptr(), None, oh, T),
              (src.ptr(), win.ptr(), dst.ptr(), idx.ptr(), 0, T), (src.ptr(), win.ptr(), dst.ptr(), idx.ptr(), oh, 0)):
        assert fn(a[0], a[1], cw, y0, x0, a[4], ow, a[5], n_ang, a[2], 114, a[3], sp()) == E_ARG, a
    fn = lib.fn["ep24_sector_warp_u8"]
    for a in ((None, win.ptr(), dst.ptr(), sh), (img.ptr(), None, dst.ptr(), sh), (img.ptr(), win.ptr(), None, sh), (img.ptr(), win.ptr(), dst.ptr(), 0)):
        assert fn(a[0], a[3], sw, a[1], cw, y0, x0, oh, ow, T, n_ang, a[2], 114, sp()) == E_ARG, a
    fn = lib.fn["ep24_resize_linear_u8"]
    for a in ((None, dst.ptr(), 6, 5), (img.ptr(), None, 6, 5), (img.ptr(), dst.ptr(), 0, 5), (img.ptr(), dst.ptr(), 6, 0)):
        assert fn(a[0], a[2], 8, a[1], a[3], 9, sp()) == E_ARG, a
    sync()
    dst.check(np.full(dst.n, U.SENT8, dtype=np.uint8), "a refused call wrote")
    idx.check(np.full(idx.n, I32_SENT, dtype=np.int32), "a refused call wrote")


@pytest.mark.parametrize("h,w", [(5, 7), (257, 259)])
def test_mask_bbox(h, w):
    """an empty mask leaves the box as it was; one pixel at each corner, alone and together; channel 0 alone counts"""
    call, sp, lib = _abi()
    init = [2 ** 31 - 1, 2 ** 31 - 1, -1, -1]
    corners = [(0, 0), (0, w - 1), (h - 1, 0), (h - 1, w - 1)]
    masks = [[]] + [[p] for p in corners] + [corners, [(h // 2, w // 3), (h // 3, w // 2)]]
    for pts in masks:
        m = np.zeros((h, w, 3), dtype=np.uint8)
        m[..., 1:] = 255                                             # the other channels do not count
        for y, x in pts:
            m[y, x, 0] = 1
        mk, box = Gu8(m), Gi32(init)
        call("mask_bbox", mk.ptr(), h, w, box.ptr(), sp())
        sync()
        box.check(np.array(R.mask_bbox_ref(m, init), dtype=np.int32), "mask_bbox %s" % (pts,))
        unchanged(mk)
    fn = lib.fn["ep24_mask_bbox"]
    for a in ((None, box.ptr(), h, w), (mk.ptr(), None, h, w), (mk.ptr(), box.ptr(), 0, w), (mk.ptr(), box.ptr(), h, 0)):
        assert fn(a[0], a[2], a[3], a[1], sp()) == E_ARG


# ---------------------------------------------------------------------------------------------------------------------------
# csrc/paste.hip: what tests/test_gpu_copypaste.py's CASES do not reach
@pytest.mark.parametrize("name", R.PASTE_NEW)
def test_paste(name):
    call, sp, _ = _abi()
    c = R.paste_case(name)
    (S_h, S_w), ml, n = c["S"], c["max_labels"], c["n"]
    shift = 1 if name == "shifted" else 0                            # both image buffers start 4 bytes off a 16-byte boundary
    sent = np.full(shift, U.SENT32, dtype=np.uint32)
    pre = G(c["pre_images"].size + shift, "f32", np.concatenate([sent, R.f32bits(c["pre_images"]).reshape(-1)]))
    lab, cnt, desc = Gf32(c["pre_labels"]), Gi32(c["pre_count"]), Gi64(c["paste"])
    o_lab, o_cnt, o_rng = G(n * ml * 51, "f32"), G(n, "i32"), G(2 * n, "i32")
    o_img = G(c["pre_images"].size + shift, "f32")
    assert R.paste_vec(S_w, pre.ptr(shift), o_img.ptr(shift)) == (name == "rows256" or name == "nosource")
    call("paste_labels", lab.ptr(), cnt.ptr(), desc.ptr(), n, S_h, S_w, R.PASTE_MARGIN, R.PASTE_THR, o_lab.ptr(), o_cnt.ptr(), o_rng.ptr(), ml, sp())
    call("paste_u8", pre.ptr(shift), o_lab.ptr(), o_rng.ptr(), desc.ptr(), n, o_img.ptr(shift), S_h, S_w, ml, sp())
    sync()
    rows, counts, ranges, _ = co.paste_labels(c["pre_labels"], c["pre_count"], c["paste"], c["S"], R.PASTE_MARGIN, R.PASTE_THR, ml)
    o_cnt.check(counts, "out_count")
    o_rng.check(ranges.reshape(-1), "paste_range")
    o_lab.check(R.f32bits(rows).reshape(-1), "out_labels")
    want, pasted = R.paste_u8_ref(c["pre_images"], rows, ranges, c["paste"])
    print(name, "ranges", ranges.tolist(), "pasted pixels", pasted.sum((1, 2)).tolist())
    o_img.check(np.concatenate([sent, R.f32bits(want).reshape(-1)]), "out_images")
    unchanged(pre, lab, cnt, desc)


def test_paste_refusals():
    _, sp, lib = _abi()
    c = R.paste_case("cut")
    (S_h, S_w), n = c["S"], c["n"]
    pre, lab, cnt, desc = Gf32(c["pre_images"]), Gf32(np.zeros((n, 257, 51))), Gi32(c["pre_count"]), Gi64(c["paste"])
    o_lab, o_cnt, o_rng, o_img = G(n * 257 * 51, "f32"), G(n, "i32"), G(2 * n, "i32"), G(pre.n, "f32")
    fl, fu = lib.fn["ep24_paste_labels"], lib.fn["ep24_paste_u8"]
    for ml in (257, 0, -1):
        assert fl(lab.ptr(), cnt.ptr(), desc.ptr(), n, S_h, S_w, 2.0, 0.3, o_lab.ptr(), o_cnt.ptr(), o_rng.ptr(), ml, sp()) == E_ARG, ml
        assert fu(pre.ptr(), o_lab.ptr(), o_rng.ptr(), desc.ptr(), n, o_img.ptr(), S_h, S_w, ml, sp()) == E_ARG, ml
    assert "256" in lib.last_error()
    assert fl(lab.ptr(), cnt.ptr(), desc.ptr(), -1, S_h, S_w, 2.0, 0.3, o_lab.ptr(), o_cnt.ptr(), o_rng.ptr(), 6, sp()) == E_ARG
    assert fl(lab.ptr(), cnt.ptr(), desc.ptr(), n, S_h, S_w, 2.0, 0.3, lab.ptr(), o_cnt.ptr(), o_rng.ptr(), 6, sp()) == E_ARG
    assert fu(pre.ptr(), o_lab.ptr(), o_rng.ptr(), desc.ptr(), n, pre.ptr(), S_h, S_w, 6, sp()) == E_ARG
    assert fu(pre.ptr(), o_lab.ptr(), o_rng.ptr(), desc.ptr(), n, o_img.ptr(), 0, S_w, 6, sp()) == E_ARG
    sync()
    for b in (o_lab, o_img):
        b.check(np.full(b.n, U.SENT32, dtype=np.uint32), "a refused call wrote")
    for b in (o_cnt, o_rng):
        b.check(np.full(b.n, I32_SENT, dtype=np.int32), "a refused call wrote")
