"""The stratified 24-point evaluation on the GPU (csrc/evalstrata.hip, ep24.evaluate strata) against its numpy oracle
(tests/eval24_strata_oracle.py) on the shared scenes (tests/eval24_strata_scenes.py), fed with the kernels' own IoU matrices: measures,
records, npig, precision and recall bit-equal."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import eval24_strata_oracle as SO  # noqa: E402
import eval24_strata_scenes as SC  # noqa: E402
import segmeval_oracle as SEG  # noqa: E402
from ep24 import evaluate as E, infer, synth  # noqa: E402
from ep24._lib import Ep24Error, call, ptr, stream_ptr  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
Y24 = os.path.join(ROOT, "exploration-of-potential_amd", "yolox_24p")
pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


# ---- measure -------------------------------------------------------------------------------------------
def test_measure_bit_equal_to_the_oracle():
    rng = np.random.RandomState(3)
    zt = np.concatenate([E.no_zones(1), E.radius_zones([(1280, 960)], (640, 640)), E.lens_zones([SC.LENS_A, SC.LENS_B])])
    scales = np.array([1.0, 0.5, 0.8, 1.25])
    lab = np.stack(SC.random_gts(2000, [0, 1, 2], rng))
    # the principal points themselves, points beyond either field, the far corner
    special = [(319.5, 319.5), (300.0, 330.0), (5.0, 5.0), (639.0, 2.0), (239.5, 319.5), (0.0, 0.0)]
    lab = np.concatenate([lab] + [np.stack([SC.gt_row(1, x, y, 12.0, rng) for x, y in special])] * 4)
    det = np.concatenate([SC.false_positives(2000, [0, 1], rng)] + [np.stack([SC.det_of(SC.gt_row(1, x, y, 9.0, rng)) for x, y in special])] * 4)
    for rows, kind, fn in ((lab, "label", SO.measure_labels), (det, "det", SO.measure_dets)):
        n = len(rows)
        image = np.concatenate([np.arange(n - 24) % 4, np.repeat(np.arange(4), 6)])
        got = E.measure(dev(rows), kind, image, scales, zt).cpu().numpy()
        want = fn(rows, image, scales, zt)
        assert got.shape == want.shape == (n, 2)
        for col, name in ((0, "area"), (1, "zone")):
            bad = np.flatnonzero(bits(got[:, col]) != bits(want[:, col]))
            assert bad.size == 0, (kind, name, len(bad), image[bad[:4]], got[bad[:4], col], want[bad[:4], col])
        z = want[:, 1]
        assert (z[image == 0] == 0).all() and np.isinf(z[image >= 2]).any() and (z[(image >= 2)] == 0).sum() >= 2
        assert (z[image == 1] >= 0).all() and (z[image == 1] == 0).sum() == 1 and (want[:, 0] > 0).all()      # the content's centre itself
    assert E.measure(dev(lab[:0]), "label", np.zeros(0, np.int64), scales, zt).shape == (0, 2)
    with pytest.raises(ValueError, match="image"):
        E.measure(dev(lab[:3]), "label", [0, 1, 4], scales, zt)
    with pytest.raises(ValueError, match="kind"):
        E.measure(dev(lab[:3]), "gt", [0, 1, 2], scales, zt)


# ---- records and tables -------------------------------------------------------------------------------
def gpu_iou(iou_type):
    return lambda gt50, det26: E.pairwise_iou(dev(gt50), dev(det26), iou_type).cpu().numpy()


def run_gpu(scene, strata, zones, C, iou_type, max_dets, splits, legacy=False):
    ev = E.Evaluator24(C, iou_type=iou_type) if legacy else E.Evaluator24(C, iou_type=iou_type, max_dets=max_dets, strata=strata)
    lo = 0
    for s in splits:
        d = [None if x is None else dev(x) for x in scene["dets"][lo:lo + s]]
        extra = () if legacy else (scene["scales"][lo:lo + s], zones[lo:lo + s])
        ev.update_detections(d, dev(scene["labels"][lo:lo + s]), *extra)
        lo += s
    assert lo == len(scene["dets"])
    return ev, ev.summarize()


def check(ev, st, want):
    rec, wr = ev.records(), want["records"]
    assert len(rec["cls"]) == len(wr["cls"])
    for k in ("cls", "seq", "p", "rank", "m"):
        assert np.array_equal(rec[k], wr[k]), k
    assert np.array_equal(rec["score"].view(np.uint32), wr["score"].view(np.uint32))
    assert np.array_equal(bits(rec["area"]), bits(wr["area"])) and np.array_equal(bits(rec["zone"]), bits(wr["zone"]))
    assert np.array_equal(ev.npig(), want["npig"])
    assert np.array_equal(bits(st["precision"]), bits(want["precision"]))
    assert np.array_equal(bits(st["recall"]), bits(want["recall"]))


CASES = [  # B, L, C, configuration, maxDets, IoU type
    (5, 256, 120, "coco+lens", (1, 10, 100), "rect"),
    (5, 256, 120, "coco+lens", (128,), "poly24"),
    (5, 256, 1, "radius3", (1, 10, 100), "circle24"),
    (1, 256, 120, "all", (128,), "circle24"),
    (5, 1, 120, "coco+lens", (1, 10, 100), "poly24"),
    (1, 1, 1, "radius3", (128,), "rect"),
]


@pytest.mark.parametrize("B,L,C,cfg,max_dets,iou_type", CASES)
def test_scenes_bit_equal_to_the_oracle(B, L, C, cfg, max_dets, iou_type):
    scene = SC.make_scene(B, L)
    strata, zones = SC.config(scene, cfg)
    ev, st = run_gpu(scene, strata, zones, C, iou_type, max_dets, [B])
    want = SO.evaluate(SC.oracle_images(scene, zones, gpu_iou(iou_type)), C, SC.strata_rows(strata), max_dets)
    check(ev, st, want)
    assert st["precision"].shape == (10, 101, C, len(strata), len(max_dets)) and set(st["strata"]) == {s.name for s in strata}
    if B == 5 and L == 256:
        assert (want["records"]["m"] >> 16).any() or cfg == "all"
        assert 0.0 < st["AP"] < 1.0
        for a, s in enumerate(strata):
            assert st["strata"][s.name]["npig"] == int(want["npig"][:, a].sum()) > 0


def test_batch_split_and_repeat_invariance():
    scene = SC.make_scene()
    strata, zones = SC.config(scene, "coco+lens")
    ref = None
    for splits in ([5], [2, 3], [1] * 5, [5]):
        ev, st = run_gpu(scene, strata, zones, 120, "circle24", (1, 10, 100), splits)
        tabs = (st["precision"], st["recall"], ev.npig(), ev.records()["m"])
        if ref is None:
            ref = tabs
        assert all(np.array_equal(a, b) for a, b in zip(tabs, ref))


def test_no_strata_equals_the_all_stratum_equals_the_single_range_evaluator():
    scene = SC.make_scene()
    strata, zones = SC.config(scene, "all")
    old, so = run_gpu(scene, None, None, 120, "circle24", None, [5], legacy=True)
    new, sn = run_gpu(scene, strata, zones, 120, "circle24", (100,), [5])
    dflt = E.Evaluator24(120, strata=strata)                                  # default tables: scale 1, no zones
    dflt.update_detections([None if x is None else dev(x) for x in scene["dets"]], dev(scene["labels"]))
    sd = dflt.summarize()
    assert old.strata is None and so["precision"].shape == (10, 101, 120)
    for s in (sn, sd):
        assert np.array_equal(bits(s["precision"][:, :, :, 0, 0]), bits(so["precision"]))
        assert np.array_equal(bits(s["recall"][:, :, 0, 0]), bits(so["recall"]))
        assert (s["AP"], s["AP50"], s["AP75"], s["AR100"]) == (so["AP"], so["AP50"], so["AP75"], so["AR100"])
    ro, rn = old.records(), new.records()
    for k in ro:
        assert np.array_equal(ro[k], rn[k]), k
    assert np.array_equal(rn["m"][:, 0], ro["tp"]) and np.array_equal(new.npig()[:, 0], old.npig())
    assert old.summary == E.format_summary(so, 100) and new.summary == old.summary


def test_update_equals_update_detections_of_postprocess():
    B, S, C = 4, 320, 80
    pred = synth.decode_head(synth.make_raw_head(B, S, seed=21, num_classes=C), S)
    pred[..., 26:] = torch.sigmoid(pred[..., 26:])
    pred = pred.to(DEV)
    labels = synth.make_labels(B, [6, 0, 12, 3], size=S, seed=22).to(DEV)
    sizes = [(480, 640), (320, 320), (200, 320), (640, 640)]
    scales = E.letterbox_scales(sizes, (S, S))
    lens = SC.LENS_A.scaled(0.5)
    strata = E.coco_area_strata() + E.zone_strata([0, 30, 60, 90], "deg")
    zones = E.lens_zones([lens] * B)
    for iou_type in ("circle24", "poly24"):
        a = E.Evaluator24(C, iou_type=iou_type, max_dets=(1, 10, 100), strata=strata)
        a.update(pred, labels, scales, zones)
        b = E.Evaluator24(C, iou_type=iou_type, max_dets=(1, 10, 100), strata=strata)
        b.update_detections(infer.postprocess(pred, C, conf_thre=0.01, nms_thre=0.65), labels, scales, zones)
        sa, sb = a.summarize(), b.summarize()
        assert a.n_records == b.n_records > 0
        ra, rb = a.records(), b.records()
        for k in ra:
            assert np.array_equal(ra[k], rb[k]), k
        assert np.array_equal(sa["precision"], sb["precision"]) and np.array_equal(sa["recall"], sb["recall"])
        assert np.array_equal(a.npig(), b.npig()) and a.summary == b.summary


def test_accumulate_across_chunk_boundaries():
    """Hand-made records with TP and ignore bits, classes of 1 023, 1 024, 1 025 and 2 049 records (sums and maxima carried over the
    accumulate kernel's chunks of 1 024), NA = 8, NM = 3: every table against the oracle, nothing written outside them."""
    from test_gpu_segmeval import framed, frames_intact
    rng = np.random.RandomState(31)
    counts, NA, md = (1023, 1024, 1025, 2049), 8, (5, 60, 128)
    K = len(counts)
    cls = np.concatenate([np.full(c, k, dtype=np.int64) for k, c in enumerate(counts)])
    i = np.concatenate([np.arange(c, dtype=np.int64) for c in counts])
    n = len(cls)
    tp = rng.randint(0, 1024, size=(n, NA))
    ig = np.zeros((n, NA), dtype=np.int64)
    for t in range(10):
        ig |= (rng.rand(n, NA) < 0.15).astype(np.int64) << t
    perm = rng.permutation(n)
    rec = {"cls": cls[perm], "seq": (i // 128)[perm], "rank": (i % 128)[perm], "score": (rng.randint(1, 100, n) / 100.0)[perm],
           "m": (tp | (ig << 16)).astype(np.int32)[perm], "npig": rng.randint(1, 3000, size=(K, NA)).astype(np.int64)}
    rec["npig"][2, 5] = 0                                                      # a class without GTs in one stratum: -1
    want_p, want_r = SEG.accumulate(rec, K, md)
    ranks = SEG.score_ranks(rec["score"]).astype(np.uint64)
    key = dev(((ranks << np.uint64(32)) | (rec["seq"].astype(np.uint64) << np.uint64(7)) | rec["rank"].astype(np.uint64)).view(np.int64))
    c32, m32, npig = dev(rec["cls"].astype(np.int32)), dev(rec["m"]), dev(rec["npig"].astype(np.int32))
    order = E.sort_records(key, c32, 7 + int(rec["seq"].max()).bit_length(), max(K - 1, 1).bit_length())
    npr, nrc = 10 * 101 * K * NA * 3, 10 * K * NA * 3
    p_big, prec, f64 = framed(npr, torch.float64)
    r_big, recl, _ = framed(nrc, torch.float64)
    ctp = torch.full((NA * 3 * n,), -1, dtype=torch.int32, device=DEV)
    env = torch.full((NA * 3 * n,), float("nan"), dtype=torch.float64, device=DEV)
    md_d, rthr = dev(np.array(md, dtype=np.int32)), dev(SEG.REC_THRS.copy())
    call("eval_accumulate_strata", ptr(order), ptr(key), ptr(c32), ptr(m32), n, ptr(npig), K, NA, ptr(md_d), 3, ptr(rthr), ptr(ctp), ptr(env),
         ptr(prec), ptr(recl), stream_ptr())
    assert frames_intact(p_big, npr, f64) and frames_intact(r_big, nrc, f64)
    assert np.array_equal(bits(prec.cpu().numpy().reshape(want_p.shape)), bits(want_p))
    assert np.array_equal(bits(recl.cpu().numpy().reshape(want_r.shape)), bits(want_r))
    assert (want_p[:, :, 2, 5] == -1).all() and ((want_p > 0) & (want_p < 0.99)).any()


def test_bad_arguments_launch_nothing():
    scene = SC.make_scene(2, 8)
    strata, zones = SC.config(scene, "coco+lens")
    labels = dev(scene["labels"])
    dets = [dev(x) for x in scene["dets"]]
    ev = E.Evaluator24(120, strata=strata)
    for kw, name in ((dict(scales=[1.0, -2.0], zones=zones), "scales"), (dict(scales=[1.0], zones=zones), "scales"),
                     (dict(scales=None, zones=np.where(np.arange(16) == 0, 7.0, zones)), "zones"), (dict(zones=zones[:1]), "zones")):
        with pytest.raises(ValueError, match=name):
            ev.update_detections(dets, labels, **kw)
    assert ev.seq == 0 and ev.n_records == 0 and (ev._npig is None or int(ev._npig.sum()) == 0)
    # the C entry points: every output pre-filled and unchanged, the message names the argument
    rows = torch.cat(dets)
    n = rows.shape[0]
    cs, thr, rthr = E._device_consts(rows.device)
    row_off = dev(np.array([0, dets[0].shape[0]], dtype=np.int64))
    count = dev(np.array([d.shape[0] for d in dets], dtype=np.int32))
    sc, zt = dev(scene["scales"]), dev(zones)
    good = np.array(SC.strata_rows(strata), dtype=np.float64)
    bad_rng = good.copy()
    bad_rng[2, :2] = (9.0, 4.0)
    many = np.tile(good[:1], (9, 1))

    def match(L, strata_rows, NA, max_dets, name):
        out = [torch.full((n * 8,), -7, dtype=dt, device=DEV) for dt in (torch.int64, torch.int32, torch.int32, torch.int32)]
        val = torch.full((n * 2,), -7.0, dtype=torch.float64, device=DEV)
        cnt, npig, err = (torch.full((k,), -7, dtype=torch.int32, device=DEV) for k in (1, 120 * 8, 1))
        sort = torch.full((2 * 256,), -7, dtype=torch.int64, device=DEV)
        with pytest.raises(Ep24Error, match=name):
            call("eval_match_strata", ptr(labels), L, 2, ptr(rows), 29, ptr(row_off), None, 0, ptr(count), None, None, 120, 0, ptr(cs),
                 ptr(thr), max_dets, 0, ptr(sort), 256, ptr(sc), ptr(zt), strata_rows.ctypes.data, NA, ptr(out[0]), ptr(out[1]), ptr(out[2]),
                 ptr(out[3]), ptr(val), ptr(cnt), ptr(npig), ptr(err), stream_ptr())
        torch.cuda.synchronize()
        assert all(bool((t == -7).all()) for t in out + [val, cnt, npig, err, sort]), name

    match(8, many, 9, 100, "NA=9")
    match(8, good, 0, 100, "NA=0")
    match(8, bad_rng, 8, 100, r"strata\[2\]")
    match(8, good, 8, 129, "max_dets=129")
    match(257, good, 8, 100, "L=257")
    out = torch.full((8,), -7.0, dtype=torch.float64, device=DEV)
    for NA, NM, name in ((9, 1, "NA=9"), (8, 5, "NM=5")):
        with pytest.raises(Ep24Error, match=name):
            call("eval_accumulate_strata", None, None, None, None, 0, ptr(count), 1, NA, ptr(count), NM, ptr(rthr), None, None, ptr(out), ptr(out),
                 stream_ptr())
    with pytest.raises(Ep24Error, match="row_kind"):
        call("eval_measure", ptr(rows), 29, 2, ptr(count), 2, ptr(sc), ptr(zt), 2, ptr(cs), ptr(out), stream_ptr())
    torch.cuda.synchronize()
    assert bool((out == -7.0).all())


# ---- the two instances of the one match kernel, at C level ---------------------------------------------
def _match_sources():
    """{name: (labels, rows, ncols, row_off, keep, keep_stride, count, conf, cls, C, P, cap)}: the scene as ``update_detections``
    hands it over (29 columns, no keep / conf / cls) and a B = 2, 320^2 synthetic head as ``update`` does (rows through post_nms'
    keep, class and confidence from post_prepare's arrays)."""
    scene = SC.make_scene(5, 256)
    counts = [0 if d is None else len(d) for d in scene["dets"]]
    rows = dev(np.concatenate([d for d in scene["dets"] if d is not None]))
    off = np.zeros(5, dtype=np.int64)
    off[1:] = np.cumsum(counts)[:-1]
    src = {"update_detections": (dev(scene["labels"]), rows, 29, dev(off), None, 0, dev(np.array(counts, dtype=np.int32)), None, None, 120,
                                 E._pow2(max(counts)), sum(counts))}
    B, S, C = 2, 320, 80
    pred = synth.decode_head(synth.make_raw_head(B, S, seed=21, num_classes=C), S)
    pred[..., 26:] = torch.sigmoid(pred[..., 26:])
    pred = pred.to(DEV).float().contiguous()
    labels = synth.make_labels(B, [6, 12], size=S, seed=22).to(DEV).float().contiguous()
    E.Evaluator24(C, conf_thre=0.01).update(pred, labels)       # post_prepare + post_nms: their outputs stay in the scratch
    A = pred.shape[1]
    ws = infer._scratch[(B, A, str(pred.device))]
    src["update"] = (labels, pred, 27 + C, E._row_offs[(B, A, str(pred.device))], ws.keep, A, ws.count, ws.conf, ws.cls, C, E._pow2(A), B * A)
    return src


def test_plain_and_one_stratum_instances_agree_at_c_level():
    """ep24_eval_match and ep24_eval_match_strata (one all-inclusive stratum, scale 1, no zones) on the same buffers: the same
    records, TP bits, GT counts, no ignore bit, for every IoU type and both detection sources."""
    cs, thr, _ = E._device_consts(torch.device(DEV))
    one = np.array([E.Stratum("all").row()], dtype=np.float64)
    for name, (labels, rows, ncols, row_off, keep, stride, count, conf, cls, C, P, cap) in _match_sources().items():
        B = labels.shape[0]
        sc, zt = torch.ones(B, dtype=torch.float64, device=DEV), dev(E.no_zones(B))
        for iou_type in ("circle24", "rect", "poly24"):
            got = []
            for strata in (False, True):
                key = torch.zeros(cap, dtype=torch.int64, device=DEV)
                rcls, rp, rm = (torch.zeros(cap, dtype=torch.int32, device=DEV) for _ in range(3))
                cnt, npig, err = (torch.zeros(k, dtype=torch.int32, device=DEV) for k in (1, C, 1))
                sort = torch.zeros(B * P, dtype=torch.int64, device=DEV)
                head = [ptr(labels), labels.shape[1], B, ptr(rows), ncols, ptr(row_off), ptr(keep), stride, ptr(count), ptr(conf), ptr(cls), C,
                        E.IOU_TYPES[iou_type], ptr(cs), ptr(thr), 100, 0, ptr(sort), P]
                recs, tail = [ptr(key), ptr(rcls), ptr(rp), ptr(rm)], [ptr(cnt), ptr(npig), ptr(err), stream_ptr()]
                if strata:
                    call("eval_match_strata", *head, ptr(sc), ptr(zt), one.ctypes.data, 1, *recs, None, *tail)
                else:
                    call("eval_match", *head, *recs, *tail)
                n = int(cnt.item())
                k, c, p, m = (t[:n].cpu().numpy() for t in (key, rcls, rp, rm))
                o = np.lexsort((k, c))
                got.append((n, k[o], c[o], p[o], m[o], npig.cpu().numpy(), int(err.item())))
            (n0, k0, c0, p0, tp, g0, e0), (n1, k1, c1, p1, m, g1, e1) = got
            what = (name, iou_type)
            assert n0 == n1 > 0 and e0 == 0 and e1 == 0, what
            assert np.array_equal(k0, k1) and np.array_equal(c0, c1) and np.array_equal(p0, p1), what
            assert np.array_equal(tp, m & 0x3FF) and not (m >> 16).any(), what
            assert tp.any() or name == "update", what                                 # the random head need not hit a GT
            assert np.array_equal(g0, g1) and g0.sum() > 0, what


def test_plain_match_bad_arguments_launch_nothing():
    """The counterpart of the eval_match_strata cases above for ep24_eval_match: every output and scratch buffer pre-filled and
    unchanged, the message names the argument as name=value."""
    scene = SC.make_scene(2, 8)
    labels = dev(scene["labels"])
    dets = [dev(x) for x in scene["dets"]]
    rows = torch.cat(dets)
    n = rows.shape[0]
    cs, thr, _ = E._device_consts(rows.device)
    row_off = dev(np.array([0, dets[0].shape[0]], dtype=np.int64))
    count = dev(np.array([d.shape[0] for d in dets], dtype=np.int32))
    conf = torch.ones(n, dtype=torch.float32, device=DEV)

    def match(name, L=8, max_dets=100, P=256, conf=None, iou_type=0):
        out = [torch.full((n,), -7, dtype=dt, device=DEV) for dt in (torch.int64, torch.int32, torch.int32, torch.int32)]
        cnt, npig, err = (torch.full((k,), -7, dtype=torch.int32, device=DEV) for k in (1, 120, 1))
        sort = torch.full((2 * 256,), -7, dtype=torch.int64, device=DEV)
        with pytest.raises(Ep24Error, match=name):
            call("eval_match", ptr(labels), L, 2, ptr(rows), 29, ptr(row_off), None, 0, ptr(count), ptr(conf), None, 120, iou_type, ptr(cs),
                 ptr(thr), max_dets, 0, ptr(sort), P, ptr(out[0]), ptr(out[1]), ptr(out[2]), ptr(out[3]), ptr(cnt), ptr(npig), ptr(err),
                 stream_ptr())
        torch.cuda.synchronize()
        assert all(bool((t == -7).all()) for t in out + [cnt, npig, err, sort]), name

    match("L=257", L=257)
    match("max_dets=129", max_dets=129)
    match("P=192", P=192)
    match("cls=null", conf=conf)
    match("iou_type=3", iou_type=3)


# ---- entry points --------------------------------------------------------------------------------------
def _small_exp():
    sys.path.insert(0, Y24)
    from exp import get_exp
    exp = get_exp(os.path.join(Y24, "load_train", "yolox_24p_train.py"))
    exp.depth, exp.width = 0.33, 0.25
    exp.test_size = (320, 320)
    exp.eval_len = 10
    return exp


def test_exp_eval_with_strata_equals_the_decomposed_path():
    from ep24.input import TrainTransform
    from ep24.lens import LensModel, image_model
    exp = _small_exp()
    lens = LensModel.equidistant((320, 320), (320, 320), 150.0)
    exp.eval_areas, exp.eval_zones, exp.eval_lens = True, "lens", lens
    torch.manual_seed(0)
    model = exp.get_model().to(DEV)
    ev = exp.get_evaluator(4)
    ap, ap50, summary = exp.eval(model, ev, False)
    assert model.training and summary.count("Average") == 12 and len(ev.strata) == 7 and ev.max_dets == (1, 10, 100)
    assert sum("deg" in ln for ln in summary.splitlines()) == 3, summary      # one table row per zone
    strata = E.coco_area_strata() + E.zone_strata([0, 30, 60, 90], "deg")
    ref = E.Evaluator24(exp.num_classes, max_dets=(1, 10, 100), conf_thre=exp.test_conf, nms_thre=exp.nmsthre, strata=strata)
    model.eval()
    tt = TrainTransform(max_labels=50)
    with torch.no_grad():
        for images, targets, _, _ in exp.get_eval_loader(4):
            sizes = [tuple(im.shape[:2]) for im in images]
            imgs, labs = tt.batch(images, targets, (320, 320))
            eng = model.engine(imgs.shape[0], 320)
            ref.update(eng.forward_eval(imgs), labs, E.letterbox_scales(sizes, (320, 320)),
                       E.lens_zones([image_model(lens, h, w, (320, 320)) for h, w in sizes]))
    st = ref.summarize()
    model.train()
    assert ref.seq == 10 and ev.seq == 10
    assert np.array_equal(st["precision"], ev.stats["precision"]) and np.array_equal(st["recall"], ev.stats["recall"])
    assert (ap, ap50) == (st["AP"], st["AP50"]) and ev.summary == ref.summary and ev.stats["strata"] == st["strata"]


def test_eval_24p_on_a_trained_checkpoint(tmp_path):
    env = dict(os.environ)
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK"):
        env.pop(k, None)
    exp_file = os.path.join(Y24, "load_train", "yolox_24p_train.py")
    out = str(tmp_path / "run")
    cmd = [sys.executable, os.path.join(Y24, "train_24p.py"), "-f", exp_file, "-b", "4", "-l", "0.01", "--synthetic", "--synthetic-len", "8",
           "--steps", "2", "--log-interval", "1", "--loader-workers", "0", "--output-dir", out]
    p = subprocess.run(cmd, cwd=Y24, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=900)
    assert p.returncode == 0, p.stdout[-4000:]
    ckpt = os.path.join(out, "yolox_24p", "last_epoch_ckpt.pth")
    assert os.path.exists(ckpt)
    js = str(tmp_path / "stats.json")
    cmd = [sys.executable, os.path.join(Y24, "eval_24p.py"), "-f", exp_file, "-c", ckpt, "-b", "8", "--synthetic", "--eval-areas",
           "--eval-zones", "radius", "--out", js]
    p = subprocess.run(cmd, cwd=Y24, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=900)
    assert p.returncode == 0, p.stdout[-4000:]
    lines = p.stdout.splitlines()
    assert len([ln for ln in lines if ln.startswith(" Average Precision")]) == 6, p.stdout[-3000:]
    assert len([ln for ln in lines if ln.startswith(" Average Recall")]) == 6
    for area in ("all", "small", "medium", "large"):
        assert any("area=%6s" % area in ln for ln in lines), area
    stats = json.load(open(js))
    names = ["all", "small", "medium", "large"] + [s.name for s in E.zone_strata([0, 1 / 3, 2 / 3, float("inf")], "r")]
    assert list(stats["strata"]) == names and stats["max_dets"] == [1, 10, 100]
    for nm in names:
        assert set(stats["strata"][nm]) == {"AP", "AP50", "AP75", "AR1", "AR10", "AR100", "npig"}
        assert any(ln.split()[:1] == [nm] for ln in lines) or nm in ("all", "small", "medium", "large")
    assert stats["strata"]["all"]["npig"] > 0 and len(stats["per_class_AP"]) > 0 and stats["images"] == 64
    env["WORLD_SIZE"] = "2"
    p = subprocess.run(cmd, cwd=Y24, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=900)
    assert p.returncode != 0 and "WORLD_SIZE" in p.stdout
