"""The ep24_segm_* kernels and ep24.segmeval.SegmEvaluator on the GPU against tests/segmeval_oracle.py, everything exact:
mask statistics and crowd-aware IoU on random bit masks of mixed sizes inside sentinel frames, the matcher on the recorded
scene's IoU blocks (whole and split over two calls) and on groups of more than 64 GTs, the accumulator on the oracle's records
and on classes longer than its chunk of 1 024 records, the evaluator end to end on a dataset built here (three chunk sizes, three input forms) and eval_segm.py in a child process."""
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import cocomask_oracle as cmo
import segmeval_oracle as ora
from test_cocomask_oracle import fixture_annotation
from test_segmeval_oracle import scene, scene_groups, scene_records

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FRAME, SENTINEL = 16, 0x5A
WIDTHS, HEIGHTS = (1, 31, 32, 33, 64, 65), (1, 7, 40)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def framed(n, dtype):
    """n elements between two frames, every byte of all three the sentinel: (whole buffer, the n elements, a frame's value)."""
    big = torch.empty(n + 2 * FRAME, dtype=dtype, device=DEV)
    big.view(torch.uint8).fill_(SENTINEL)
    return big, big[FRAME:FRAME + n], big[0].item()


def frames_intact(big, n, fill):
    b = big.cpu()
    return bool((b[:FRAME] == fill).all()) and bool((b[FRAME + n:] == fill).all())


def pack_bits(m):
    """bool [H, W] -> uint32 [H, ceil(W / 32)]: pixel x is bit x & 31 of word x >> 5, the bits at x >= W zero."""
    H, W = m.shape
    WW = (W + 31) // 32
    p = np.zeros((H, WW * 32), dtype=np.uint8)
    p[:, :W] = m
    return np.packbits(p, axis=1, bitorder="little").view("<u4").reshape(H, WW)


def want_stats(m):
    ys, xs = np.nonzero(m)
    if len(xs) == 0:
        return [m.shape[1], m.shape[0], -1, -1], 0
    return [int(xs.min()), int(ys.min()), int(xs.max()), int(ys.max())], len(xs)


@functools.lru_cache(maxsize=None)
def mask_groups():
    """One group per size of WIDTHS x HEIGHTS plus one without GTs and one without detections: (masks, crowd flags per mask,
    groups = (H, W, GT mask indices, DT mask indices)).  Per size: random masks, an empty and a full one on either side, and two
    masks in disjoint halves of the canvas; every second GT is crowd."""
    rng = np.random.RandomState(11)
    masks, crowd, groups = [], [], []

    def add(ms, cr=None):
        first = len(masks)
        masks.extend(ms)
        crowd.extend(cr if cr is not None else [0] * len(ms))
        return list(range(first, len(masks)))

    def half(H, W, second):
        m = np.zeros((H, W), dtype=bool)
        r = rng.rand(H, W) < 0.7
        if W > 1:
            m[:, W // 2:] = r[:, W // 2:]
            if not second:
                m = np.zeros((H, W), dtype=bool)
                m[:, :W // 2] = r[:, :W // 2]
        elif H > 1:
            if second:
                m[H // 2:] = r[H // 2:]
            else:
                m[:H // 2] = r[:H // 2]
        return m

    sizes = [(H, W) for W in WIDTHS for H in HEIGHTS]
    for n, (H, W) in enumerate(sizes):
        gts = [rng.rand(H, W) < 0.5, np.zeros((H, W), dtype=bool), np.ones((H, W), dtype=bool), half(H, W, False), rng.rand(H, W) < 0.2]
        dts = [rng.rand(H, W) < 0.5, np.ones((H, W), dtype=bool), half(H, W, True), np.zeros((H, W), dtype=bool)][: 3 + n % 2]
        g = add(gts, [k % 2 for k in range(len(gts))])
        groups.append((H, W, g, add(dts)))
        if n == 4:
            groups.append((7, 33, [], add([rng.rand(7, 33) < 0.5])))                       # G = 0
        if n == 9:
            groups.append((40, 65, add([rng.rand(40, 65) < 0.5], [1]), []))                # D = 0
    return masks, crowd, groups


def test_mask_stats_and_iou_equal_the_oracle_on_mixed_sizes():
    from ep24._lib import call, ptr, stream_ptr
    masks, crowd, groups = mask_groups()
    N = len(masks)
    packed = [pack_bits(m) for m in masks]
    words = np.concatenate([[0], np.cumsum([p.size for p in packed])])
    tab = np.stack([words[:-1], [m.shape[0] for m in masks], [m.shape[1] for m in masks], np.zeros(N, dtype=np.int64)], 1).astype(np.int64)
    bits = dev(np.concatenate([p.reshape(-1) for p in packed]).view(np.int32))
    tab_t = dev(tab)
    s = stream_ptr()
    bb_big, bbox, f32 = framed(4 * N, torch.int32)
    ar_big, area, _ = framed(N, torch.int32)
    call("segm_mask_stats", ptr(bits), ptr(tab_t), N, ptr(bbox), ptr(area), s)
    want = [want_stats(m) for m in masks]
    assert bbox.cpu().view(N, 4).tolist() == [w[0] for w in want]
    assert area.cpu().tolist() == [w[1] for w in want]
    assert frames_intact(bb_big, 4 * N, f32) and frames_intact(ar_big, N, f32)
    assert any(w[1] == 0 for w in want) and any(w[1] == m.size for w, m in zip(want, masks))
    # the group table: the IoU blocks follow each other from a base of 5; masks of several sizes in one call
    base, rows, off = 5, [], 5
    for H, W, g, d in groups:
        rows.append([H, W, g[0] if g else 0, len(g), d[0] if d else 0, len(d), off, 0])
        off += len(g) * len(d)
    pairs = off - base
    assert any(r[3] == 0 for r in rows) and any(r[5] == 0 for r in rows) and len({(r[0], r[1]) for r in rows}) == 18
    grp = dev(np.array(rows, dtype=np.int64))
    crowd_t = dev(np.array(crowd, dtype=np.uint8))
    io_big, iou, f64 = framed(off, torch.float64)
    in_big, inter, i64 = framed(off, torch.int64)
    call("segm_iou", ptr(bits), ptr(tab_t), N, ptr(bbox), ptr(area), ptr(crowd_t), ptr(grp), len(rows), pairs, ptr(iou), ptr(inter), s)
    got_iou, got_inter = iou.cpu().numpy(), inter.cpu().numpy()
    assert frames_intact(io_big, off, f64) and frames_intact(in_big, off, i64)
    assert np.all(got_iou[:base].view(np.int64) == np.float64(f64).view(np.int64)) and np.all(got_inter[:base] == i64)      # before the base: untouched
    disjoint = crowd_pairs = 0
    for (H, W, g, d), r in zip(groups, rows):
        if not g or not d:
            continue
        w_inter, w_iou = ora.mask_iou([masks[k] for k in d], [masks[k] for k in g], [crowd[k] for k in g])
        o = r[6]
        assert got_inter[o:o + w_inter.size].reshape(w_inter.shape).tolist() == w_inter.tolist(), (H, W)
        assert np.array_equal(got_iou[o:o + w_iou.size].view(np.int64), w_iou.reshape(-1).view(np.int64)), (H, W)
        disjoint += int((w_inter[2] == 0).sum())
        crowd_pairs += int((w_iou[:, 1::2] > 0).sum())
    assert disjoint > 0 and crowd_pairs > 0
    # without the optional inter table the IoUs are the same
    io2_big, iou2, _ = framed(off, torch.float64)
    call("segm_iou", ptr(bits), ptr(tab_t), N, ptr(bbox), ptr(area), ptr(crowd_t), ptr(grp), len(rows), pairs, ptr(iou2), None, s)
    assert torch.equal(iou2.view(torch.int64), iou.view(torch.int64))


# ------------------------------------------------------------------------------------------------- the matcher
def match_inputs(groups):
    """Oracle groups -> the device arrays of ep24_segm_match and its table (numpy)."""
    G = np.array([len(g["gt_area"]) for g in groups], dtype=np.int64)
    D = np.array([len(g["dt_area"]) for g in groups], dtype=np.int64)
    gfirst, dfirst = np.concatenate([[0], np.cumsum(G)]), np.concatenate([[0], np.cumsum(D)])
    ioff = np.concatenate([[0], np.cumsum(G * D)])
    mgrp = np.stack([gfirst[:-1], G, dfirst[:-1], D, ioff[:-1], [g["cls"] for g in groups], [g["seq"] for g in groups], np.zeros(len(G))], 1)
    cat = lambda key, dt: np.concatenate([np.asarray(g[key], dtype=dt).reshape(-1) for g in groups] + [np.zeros(1, dtype=dt)])
    rank = ora.score_ranks(cat("dt_score", np.float64)[:-1]).astype(np.int32)
    return {"mgrp": mgrp.astype(np.int64), "iou": cat("iou", np.float64), "crowd": cat("gt_crowd", np.uint8), "ign0": cat("gt_ignore0", np.uint8),
            "gt_area": cat("gt_area", np.float64), "dt_area": cat("dt_area", np.float64), "rank": np.concatenate([rank, np.zeros(1, np.int32)]),
            "nG": int(G.sum()), "nD": int(D.sum())}


def run_match(inp, K, area_ranges, splits):
    """ep24_segm_match over the table rows [a, b) of every split, into one set of record buffers; -> (m, key, cls, npig) numpy."""
    from ep24._lib import call, ptr, stream_ptr
    NA, n = len(area_ranges), inp["nD"]
    t = {k: dev(v) for k, v in inp.items() if isinstance(v, np.ndarray)}
    rng, thr = dev(np.array(area_ranges, dtype=np.float64)), dev(ora.IOU_THRS.copy())
    m_big, m, fm = framed(n * NA, torch.int32)
    k_big, key, fk = framed(n, torch.int64)
    c_big, cls, _ = framed(n, torch.int32)
    scratch = torch.full((max(inp["nG"], 1),), -1, dtype=torch.int64, device=DEV)            # garbage: the kernel zeroes what it uses
    npig = torch.zeros(K * NA, dtype=torch.int32, device=DEV)
    for a, b in splits:
        call("segm_match", ptr(t["mgrp"], a * 8), b - a, ptr(t["iou"]), ptr(t["crowd"]), ptr(t["ign0"]), ptr(t["gt_area"]), ptr(t["dt_area"]),
             ptr(t["rank"]), ptr(rng), NA, ptr(thr), K, ptr(scratch), ptr(m), ptr(key), ptr(cls), ptr(npig), stream_ptr())
    assert frames_intact(m_big, n * NA, fm) and frames_intact(k_big, n, fk) and frames_intact(c_big, n, fm)
    return m.cpu().numpy().reshape(n, NA), key.cpu().numpy().view(np.uint64), cls.cpu().numpy(), npig.cpu().numpy().reshape(K, NA)


def check_records(got, rec, ranks):
    m, key, cls, npig = got
    assert m.tolist() == rec["m"].tolist()
    assert cls.tolist() == rec["cls"].tolist()
    assert (key >> np.uint64(32)).tolist() == ranks.tolist()
    assert ((key >> np.uint64(7)) & np.uint64((1 << 25) - 1)).tolist() == rec["seq"].tolist()
    assert (key & np.uint64(127)).tolist() == rec["rank"].tolist()
    assert npig.tolist() == rec["npig"].tolist()


def test_match_on_the_scene_whole_and_split_over_two_calls():
    sc = scene()
    groups, _, _ = scene_groups()
    rec, _, _ = scene_records()
    inp = match_inputs(groups)
    ranges = [tuple(r) for r in sc["area_ranges"]]
    whole = run_match(inp, sc["num_classes"], ranges, [(0, len(groups))])
    check_records(whole, rec, inp["rank"][:-1])
    assert (whole[0] >> 16).any() and (whole[0] & 0x3FF).any() and whole[3][2].tolist() == [0] * 4
    h = len(groups) // 2
    split = run_match(inp, sc["num_classes"], ranges, [(h, len(groups)), (0, h)])
    for a, b in zip(whole, split):
        assert np.array_equal(a, b)


def test_match_with_more_than_64_gts_and_ties():
    """G = 70 and 130 (the matched bits of GTs beyond the first 64 live in scratch), 1 and 65; IoUs on a grid of 1 / 8 so that equal
    IoUs, IoUs exactly at thresholds and contested GTs are common; crowd, ignore and areas at the range bounds at random."""
    rng = np.random.RandomState(5)
    groups = []
    for n, (G, D) in enumerate(((70, 40), (130, 128), (1, 3), (65, 9), (0, 4), (64, 20))):
        crowd = (rng.rand(G) < 0.1).astype(int)
        groups.append({"cls": n % 2, "seq": n, "iou": rng.randint(0, 9, size=(D, G)) / 8.0 * (rng.rand(D, G) < 0.3),
                       "gt_crowd": crowd.tolist(), "gt_ignore0": (crowd | (rng.rand(G) < 0.15)).astype(int).tolist(),
                       "gt_area": rng.choice([100.0, 1024.0, 1025.0, 9216.0, 20000.0], size=G).tolist(),
                       "dt_area": rng.choice([100.0, 1024.0, 5000.0, 9216.0, 9217.0], size=D).tolist(),
                       "dt_score": np.sort(rng.randint(0, 50, size=D) / 50.0)[::-1].tolist()})
    rec = ora.records(groups, 2)
    inp = match_inputs(groups)
    check_records(run_match(inp, 2, ora.AREA_RANGES, [(0, len(groups))]), rec, inp["rank"][:-1])
    # fewer area ranges: the bits of a range do not depend on its neighbours
    two = run_match(inp, 2, ora.AREA_RANGES[2:], [(0, len(groups))])
    assert two[0].tolist() == rec["m"][:, 2:].tolist() and two[3].tolist() == rec["npig"][:, 2:].tolist()


# ------------------------------------------------------------------------------------------------- the accumulator
def run_accumulate(rec, K, max_dets):
    from ep24._lib import call, ptr, stream_ptr
    from ep24.evaluate import sort_records
    n, NA, NM = len(rec["cls"]), rec["m"].shape[1], len(max_dets)
    ranks = ora.score_ranks(rec["score"]).astype(np.uint64)
    key = dev(((ranks << np.uint64(32)) | (rec["seq"].astype(np.uint64) << np.uint64(7)) | rec["rank"].astype(np.uint64)).view(np.int64))
    cls, m = dev(rec["cls"].astype(np.int32)), dev(rec["m"].astype(np.int32))
    npig = dev(rec["npig"].astype(np.int32))
    s = stream_ptr()
    order = sort_records(key, cls, 7 + int(rec["seq"].max()).bit_length(), max(K - 1, 1).bit_length())
    npr, nrc = 10 * 101 * K * NA * NM, 10 * K * NA * NM
    p_big, prec, f64 = framed(npr, torch.float64)
    r_big, recl, _ = framed(nrc, torch.float64)
    rng_ = torch.full((2 * K,), -7, dtype=torch.int64, device=DEV)
    ctp = torch.full((NA * NM * n,), -1, dtype=torch.int32, device=DEV)
    env = torch.full((NA * NM * n,), float("nan"), dtype=torch.float64, device=DEV)
    md, rthr = dev(np.array(max_dets, dtype=np.int32)), dev(ora.REC_THRS.copy())           # held: a temporary's block would be reused
    call("segm_accumulate", ptr(order), ptr(key), ptr(cls), ptr(m), n, ptr(npig), K, NA, ptr(md), NM, ptr(rthr), ptr(rng_), ptr(ctp),
         ptr(env), ptr(prec), ptr(recl), s)
    assert frames_intact(p_big, npr, f64) and frames_intact(r_big, nrc, f64)
    return prec.cpu().numpy().reshape(10, 101, K, NA, NM), recl.cpu().numpy().reshape(10, K, NA, NM)


def test_accumulate_on_the_oracle_records():
    """The scene's records with a fourth class that has GTs and no record at all: class 2 (no GT) gives -1, class 3 zeros."""
    sc = scene()
    rec, _, _ = scene_records()
    rec = dict(rec, npig=np.concatenate([rec["npig"], [[5, 0, 2, 3]]]))
    want_p, want_r = ora.accumulate(rec, 4, tuple(sc["max_dets"]))
    got_p, got_r = run_accumulate(rec, 4, sc["max_dets"])
    assert np.array_equal(got_p.view(np.int64), want_p.view(np.int64))
    assert np.array_equal(got_r.view(np.int64), want_r.view(np.int64))
    assert np.all(got_p[:, :, 2] == -1) and np.all(got_r[:, 2] == -1)
    assert np.all(got_p[:, :, 3, 0] == 0) and np.all(got_r[:, 3, 0] == 0) and np.all(got_p[:, :, 3, 1] == -1)
    assert (got_p == 1.0 / (1.0 + ora.EPS)).any() and ((got_p > 0) & (got_p < 0.99)).any()
    # another set of maxDets, two of them: the position filter
    want_p, want_r = ora.accumulate(rec, 4, (3, 128))
    got_p, got_r = run_accumulate(rec, 4, [3, 128])
    assert np.array_equal(got_p.view(np.int64), want_p.view(np.int64)) and np.array_equal(got_r.view(np.int64), want_r.view(np.int64))


CHUNK_K, CHUNK_MAX_DETS = 5, (3, 100, 128)


@functools.lru_cache(maxsize=None)
def chunk_records():
    """Synthetic records (no masks, no matcher) whose classes straddle the accumulate kernel's chunk of 1 024 records: class 0 two
    full chunks and a tail of 452, class 1 exactly one chunk, class 2 one chunk and a tail of one, class 3 GTs and no record, class 4
    records and no GT.  Two area ranges, ranks up to 124, scores on a grid of 0.01 (many ties), random TP bits and sparse ignore
    bits disjoint from them; the records stand in a random order.  -> (records, the oracle's tables at CHUNK_MAX_DETS); shared, not
    to be modified."""
    rng = np.random.RandomState(23)
    counts = (2500, 1024, 1025, 0, 37)
    cls = np.concatenate([np.full(c, k, dtype=np.int64) for k, c in enumerate(counts)])
    i = np.concatenate([np.arange(c, dtype=np.int64) for c in counts])
    n = len(cls)
    tp = rng.randint(0, 1024, size=(n, 2))
    ig = np.zeros((n, 2), dtype=np.int64)
    for t in range(10):
        ig |= (rng.rand(n, 2) < 0.1).astype(np.int64) << t
    ig &= ~tp
    o = rng.permutation(n)
    rec = {"cls": cls[o], "score": np.round(rng.rand(n), 2)[o], "seq": (i // 125)[o], "rank": (i % 125)[o],
           "m": (tp | (ig << 16)).astype(np.int32)[o], "npig": np.array([[2507, 2500], [1024, 1030], [1025, 1026], [5, 3], [0, 0]], dtype=np.int64)}
    return rec, ora.accumulate(rec, CHUNK_K, CHUNK_MAX_DETS)


def test_accumulate_across_chunk_boundaries():
    """Classes of 2 500, 1 024 and 1 025 records: the running sums and the running maximum cross from one chunk of 1 024 to the next."""
    rec, (want_p, want_r) = chunk_records()
    assert np.bincount(rec["cls"], minlength=CHUNK_K).tolist() == [2500, 1024, 1025, 0, 37] and rec["rank"].max() == 124
    assert (rec["m"] >> 16).any() and not ((rec["m"] >> 16) & rec["m"] & 0x3FF).any()
    got_p, got_r = run_accumulate(rec, CHUNK_K, list(CHUNK_MAX_DETS))
    assert np.array_equal(got_p.view(np.int64), want_p.view(np.int64))
    assert np.array_equal(got_r.view(np.int64), want_r.view(np.int64))
    assert np.all(got_p[:, :, 3] == 0) and np.all(got_r[:, 3] == 0) and np.all(got_p[:, :, 4] == -1) and np.all(got_r[:, 4] == -1)
    assert ((got_p > 0) & (got_p < 0.99)).any()


# ------------------------------------------------------------------------------------------------- end to end
def moved(poly, dx, dy, s):
    return [v * s + (dx if i % 2 == 0 else dy) for i, v in enumerate(poly)]


def rle_of(poly, h, w, compress):
    counts = cmo.rle_from_poly(poly, h, w)
    return {"size": [h, w], "counts": cmo.rle_to_string(counts) if compress else counts}


@functools.lru_cache(maxsize=None)
def dataset():
    """Three images (33 x 31, 64 x 65, 427 x 640), three categories -> (gt dict, result list, the oracle's evaluation of it)."""
    an, fh, fw = fixture_annotation()
    big = an["segmentation"][0]
    sizes = {1: (33, 31), 2: (64, 65), 3: (fh, fw)}
    assert (fh, fw) == (427, 640)
    tri, quad, bar = [3.0, 4.0, 25.0, 6.0, 12.0, 28.0], [5.0, 5.0, 28.0, 7.0, 26.0, 30.0, 4.0, 24.0], [10.0, 40.0, 60.0, 42.0, 58.0, 60.0, 12.0, 58.0]
    out = []                                                                       # the crowd: columns 20..49 of image 2, rows 8..39, as uncompressed runs
    flat = np.zeros(64 * 65, dtype=np.uint8)
    for x in range(20, 50):
        flat[x * 64 + 8:x * 64 + 40] = 1
    prev, cnt = 0, 0
    for v in flat:
        if v != prev:
            out.append(cnt)
            cnt, prev = 0, v
        cnt += 1
    out.append(cnt)
    gt = {"images": [{"id": i, "height": h, "width": w} for i, (h, w) in sizes.items()],
          "categories": [{"id": 7}, {"id": 1}, {"id": 3}],
          "annotations": [
              {"id": 1, "image_id": 3, "category_id": 7, "segmentation": [big], "area": an["area"], "iscrowd": 0},
              {"id": 2, "image_id": 2, "category_id": 1, "segmentation": {"size": [64, 65], "counts": [int(c) for c in out]}, "area": 960.0, "iscrowd": 1},
              {"id": 3, "image_id": 2, "category_id": 1, "segmentation": [bar], "area": 1024.0, "iscrowd": 0},
              {"id": 4, "image_id": 1, "category_id": 1, "segmentation": [tri], "area": 250.0, "iscrowd": 0},
              {"id": 5, "image_id": 1, "category_id": 3, "segmentation": [quad, tri], "area": 500.0, "iscrowd": 0},
              {"id": 6, "image_id": 1, "category_id": 3, "segmentation": [moved(tri, 2.0, 1.0, 0.5)], "area": 60.0, "iscrowd": 0, "ignore": 1},
              {"id": 7, "image_id": 3, "category_id": 1, "segmentation": [moved(big, 0.0, 100.0, 0.5)], "area": 9216.0, "iscrowd": 0}]}
    res = []

    def det(img, cat, seg, score):
        res.append({"image_id": img, "category_id": cat, "segmentation": seg, "score": score})
    h, w = sizes[3]
    det(3, 7, rle_of(moved(big, 4.0, 3.0, 1.0), h, w, True), 0.9)
    det(3, 7, rle_of(moved(big, 20.0, 30.0, 0.9), h, w, False), 0.6)
    det(3, 7, [moved(big, -3.0, 2.0, 1.02)], 0.6)                                  # a polygon list; equal scores
    det(3, 1, rle_of(moved(big, 2.0, 101.0, 0.5), h, w, True), 0.8)
    det(3, 3, rle_of(moved(big, 0.0, 0.0, 0.3), h, w, True), 0.5)                  # a category without GT in this image
    h, w = sizes[2]
    for k in range(4):
        det(2, 1, rle_of([22.0 + 6 * k, 10.0 + 5 * k, 30.0 + 6 * k, 10.0 + 5 * k, 30.0 + 6 * k, 22.0 + 5 * k, 22.0 + 6 * k, 22.0 + 5 * k], h, w, k % 2 == 0),
            0.7 - 0.1 * k)                                                         # inside the crowd region
    det(2, 1, rle_of(moved(bar, 1.0, 0.0, 1.0), h, w, True), 0.7 + 1e-12)
    det(2, 1, rle_of(moved(bar, 0.0, -25.0, 0.5), h, w, True), 0.3)
    h, w = sizes[1]
    det(1, 1, rle_of(moved(tri, 1.0, 0.0, 1.0), h, w, True), 0.85)
    det(1, 1, rle_of(moved(tri, 0.0, 1.0, 0.9), h, w, False), 0.4)
    det(1, 3, rle_of(moved(quad, 1.0, 1.0, 0.95), h, w, True), 0.75)
    det(1, 3, rle_of(moved(tri, 2.0, 1.0, 0.5), h, w, True), 0.65)                # on the ignore GT
    det(1, 3, [moved(quad, 0.0, 0.0, 0.4)], 0.2)
    det(99, 1, rle_of(tri, 33, 31, True), 0.99)                                    # an image the GT file does not have
    det(1, 55, rle_of(tri, 33, 31, True), 0.99)                                    # a category it does not have
    # the oracle's side: masks by tests/cocomask_oracle.py, grouping in plain Python
    img_ids, cat_ids = sorted(sizes), sorted(c["id"] for c in gt["categories"])
    mask = lambda seg, i: np.array(cmo.ann_to_mask(seg, *sizes[i]), dtype=bool)
    groups = []
    for seq, i in enumerate(img_ids):
        for k, c in enumerate(cat_ids):
            G = [a for a in gt["annotations"] if a["image_id"] == i and a["category_id"] == c]
            D = [r for r in res if r["image_id"] == i and r["category_id"] == c]
            if not G and not D:
                continue
            D = sorted(D, key=lambda r: -r["score"])[:100]
            dm, gm = [mask(r["segmentation"], i) for r in D], [mask(a["segmentation"], i) for a in G]
            crowd = [int(a.get("iscrowd", 0)) for a in G]
            _, iou = ora.mask_iou(dm, gm, crowd)
            groups.append({"cls": k, "seq": seq, "iou": iou, "gt_crowd": crowd,
                           "gt_ignore0": [int(bool(a.get("ignore", 0)) or bool(a.get("iscrowd", 0))) for a in G],
                           "gt_area": [float(a["area"]) for a in G], "dt_area": [float(m.sum()) for m in dm],
                           "dt_score": [r["score"] for r in D]})
    return gt, res, ora.evaluate(groups, len(cat_ids))


def tables_equal(st, want):
    stats, lines, precision, recall, _ = want
    return (st["stats"] == stats and np.array_equal(st["precision"].view(np.int64), precision.view(np.int64))
            and np.array_equal(st["recall"].view(np.int64), recall.view(np.int64)))


def test_evaluator_end_to_end(tmp_path):
    from ep24.results import SegmResults
    from ep24.segmeval import SegmEvaluator
    gt, res, want = dataset()
    stats, lines, precision, recall, rec = want
    assert len(stats) == 12 and 0 < stats[0] < 1 and (precision == -1).any() and (rec["m"] >> 16).any()
    ev = SegmEvaluator(gt)
    assert ev.add_results(res) == len(res)
    st = ev.evaluate()
    assert st["chunks"] == 1 and st["dropped"] == 2 and st["records"] == len(res) - 2 and st["category_ids"] == [1, 3, 7]
    assert tables_equal(st, want)
    assert ev.summary == "\n".join(lines) + "\n"
    assert st["per_class_AP"].tolist() == [float(np.mean(precision[:, :, k, 0, 2][precision[:, :, k, 0, 2] > -1])) for k in range(3)]
    # three chunks (one image each) give the same tables as one
    ev3 = SegmEvaluator(gt, chunk_bytes=1)
    ev3.add_results(res)
    st3 = ev3.evaluate()
    assert st3["chunks"] == 3 and tables_equal(st3, want) and ev3.summary == ev.summary
    # the same results as a file and as a SegmResults
    path = tmp_path / "segm.json"
    path.write_text(json.dumps(res))
    gpath = tmp_path / "gt.json"
    gpath.write_text(json.dumps(gt))
    evf = SegmEvaluator(str(gpath))
    evf.add_results(str(path))
    assert tables_equal(evf.evaluate(), want)
    sr = SegmResults()
    sr.records = list(res)
    evs = SegmEvaluator(gt)
    evs.add_results(sr)
    assert tables_equal(evs.evaluate(), want)
    # results added in two parts keep their input order
    ev2 = SegmEvaluator(gt)
    ev2.add_results(res[:7])
    ev2.add_results(res[7:])
    assert tables_equal(ev2.evaluate(), want)


def test_evaluator_without_results():
    """No result at all (and only foreign ones): every class with GTs scores 0, the others -1; no record reaches the sort."""
    from ep24.segmeval import SegmEvaluator
    gt, res, _ = dataset()
    groups = []
    for seq, i in enumerate((1, 2, 3)):
        for k, c in enumerate((1, 3, 7)):
            G = [a for a in gt["annotations"] if a["image_id"] == i and a["category_id"] == c]
            if G:
                groups.append({"cls": k, "seq": seq, "iou": np.zeros((0, len(G))), "gt_crowd": [int(a.get("iscrowd", 0)) for a in G],
                               "gt_ignore0": [int(bool(a.get("ignore", 0)) or bool(a.get("iscrowd", 0))) for a in G],
                               "gt_area": [float(a["area"]) for a in G], "dt_area": [], "dt_score": []})
    want = ora.evaluate(groups, 3)
    for results in ([], [r for r in res if r["image_id"] == 99]):
        ev = SegmEvaluator(gt)
        ev.add_results(results)
        st = ev.evaluate()
        assert st["records"] == 0 and tables_equal(st, want) and ev.summary == "\n".join(want[1]) + "\n"
    assert want[0][0] == 0.0 and (want[2] == -1).any()


def test_eval_segm_entry_point(tmp_path):
    gt, res, want = dataset()
    (tmp_path / "gt.json").write_text(json.dumps(gt))
    (tmp_path / "dt.json").write_text(json.dumps(res))
    out = tmp_path / "stats.json"
    p = subprocess.run([sys.executable, "eval_segm.py", "--gt", str(tmp_path / "gt.json"), "--dt", str(tmp_path / "dt.json"), "--out", str(out)],
                       cwd=os.path.join(ROOT, "exploration-of-potential_amd", "yolox_24p"), capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    lines = [l for l in p.stdout.splitlines() if l.startswith(" Average ")]
    assert lines == want[1] and len(lines) == 12
    got = json.loads(out.read_text())
    assert got["stats"] == want[0] and got["max_dets"] == [1, 10, 100] and got["dropped"] == 2
    assert sorted(got["per_class_AP"]) == ["1", "3", "7"]
