"""ep24.cocomask.encode / encode_buffer and ep24.results on the GPU: run lengths, offsets and compressed strings equal to
the literal rleEncode / rleToString (tests/rle_encode_oracle.py) at every strip and word tail, inside sentinel frames, two runs
bytewise identical, across the 65 535 grid cap, decode and encode checking each other, the sample annotation, the segm
records of synthetic detections and ``show_24p.py --save-segm`` in a child process."""
import functools
import glob
import hashlib
import json
import os

import numpy as np
import pytest
import torch

import rle_encode_oracle as ora
from test_cocomask_oracle import fixture_annotation
from test_rle_host import PATTERNS, SIZES, pattern

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
FRAME, SLACK, SENTINEL = 16, 40, 0x5A


@functools.lru_cache(maxsize=None)
def size_cases(h, w):
    """The nine patterns of one size and the oracle's counts for them, computed once."""
    ms = [pattern(p, h, w) for p in PATTERNS]
    return ms, [ora.rle_encode(m.tolist()) for m in ms]


def pack(ms):
    from ep24 import masks
    return masks.pack(torch.from_numpy(np.stack(ms)).to(DEV))


def check(rl, want, sizes):
    """offsets, counts and strings of a RunLengths against lists of oracle counts."""
    off, cnt = rl.offsets.cpu().numpy(), rl.counts.cpu().numpy()
    assert rl.offsets.dtype == torch.int64 and rl.counts.dtype == torch.int32 and rl.offsets.is_cuda and rl.counts.is_cuda
    assert off.tolist() == np.concatenate([[0], np.cumsum([len(c) for c in want])]).tolist()
    assert cnt.tolist() == [v for c in want for v in c]
    coco = rl.to_coco()
    assert coco == [{"size": [h, w], "counts": ora.rle_to_string(c)} for c, (h, w) in zip(want, sizes)]
    assert rl.to_coco(compress=False) == [{"size": [h, w], "counts": c} for c, (h, w) in zip(want, sizes)]
    return coco


@pytest.mark.parametrize("h, w", SIZES)
def test_every_pattern_alone_equals_rle_encode(h, w):
    from ep24 import cocomask
    ms, want = size_cases(h, w)
    for name, m, c in zip(PATTERNS, ms, want):
        rl = cocomask.encode(pack([m]))
        assert rl.size == (h, w) and len(rl) == 1, name
        check(rl, [c], [(h, w)])
    assert want[0] == [h * w] and want[1] == [0, h * w] and want[2][0] == 0          # zeros, ones, pixel (0, 0) set


@pytest.mark.parametrize("h, w", SIZES)
def test_mixed_batch_and_decode_round_trip(h, w):
    """One call over all patterns: an empty mask between two full ones, the masks with the most runs first and last."""
    from ep24 import cocomask
    ms, want = size_cases(h, w)
    most = max(range(len(ms)), key=lambda i: len(want[i]))
    z, o = PATTERNS.index("zeros"), PATTERNS.index("ones")
    order = [most] + [i for i in range(len(ms)) if i not in (z, o)] + [o, z, o, most]
    batch, cnts = [ms[i] for i in order], [want[i] for i in order]
    coco = check(cocomask.encode(pack(batch)), cnts, [(h, w)] * len(batch))
    buf, desc = cocomask.decode_batch(coco, [(h, w)] * len(batch))          # decode and encode check each other
    got = buf[:len(batch) * h * w].view(len(batch), h, w).cpu().numpy()
    assert np.array_equal(got, np.stack(batch))


def framed(n, dtype, fill):
    big = torch.full((n + 2 * FRAME,), fill, dtype=dtype, device=DEV)
    return big, big[FRAME:FRAME + n]


def test_output_stays_inside_a_sentinel_frame_and_repeats_bytewise():
    from ep24 import _lib, cocomask
    batch, want = [], []
    for h, w in ((65, 33), (65, 33)):
        ms, cs = size_cases(h, w)
        batch, want = batch + ms, want + cs
    pm = pack(batch)
    total = sum(len(c) for c in want)
    s64, s32 = int.from_bytes(bytes([SENTINEL]) * 8, "little"), int.from_bytes(bytes([SENTINEL]) * 4, "little")
    images = []
    for _ in range(2):
        big_o, off = framed(len(batch) + 1 + SLACK, torch.int64, s64)
        big_c, cnt = framed(total + SLACK, torch.int32, s32)
        rl = cocomask.encode(pm, out=(off, cnt))
        torch.cuda.synchronize()
        assert rl.offsets.data_ptr() == off.data_ptr() and rl.offsets.numel() == len(batch) + 1
        assert rl.counts.data_ptr() == cnt.data_ptr() and rl.counts.numel() == total
        check(rl, want, [(65, 33)] * len(batch))
        o, c = big_o.cpu().numpy(), big_c.cpu().numpy()
        assert (o[:FRAME] == s64).all() and (o[FRAME + len(batch) + 1:] == s64).all(), "the offsets' frame or slack was written"
        assert (c[:FRAME] == s32).all() and (c[FRAME + total:] == s32).all(), "the counts' frame or slack was written"
        images.append(o.tobytes() + c.tobytes())
    assert images[0] == images[1]
    with pytest.raises(_lib.Ep24Error, match="hold"):
        cocomask.encode(pm, out=(torch.zeros(len(batch) + 1, dtype=torch.int64, device=DEV),
                                 torch.zeros(total - 1, dtype=torch.int32, device=DEV)))


def test_no_masks_and_more_masks_than_a_grid_axis():
    from ep24 import cocomask, masks
    empty = masks.pack(torch.zeros(0, 5, 7, dtype=torch.uint8, device=DEV))
    big_o, off = framed(1, torch.int64, -3)
    rl = cocomask.encode(empty, out=(off, torch.zeros(0, dtype=torch.int32, device=DEV)))
    assert len(rl) == 0 and big_o.cpu().tolist() == [-3] * FRAME + [0] + [-3] * FRAME and rl.counts.numel() == 0
    assert cocomask.encode(empty).to_coco() == []
    n = 70000                                                                # above the 65 535 masks of one launch
    m = (np.random.default_rng(70000).random((n, 2, 3)) < 0.5).astype(np.uint8)
    # rleEncode of 2 x 3 masks in numpy: the column-major pixels with a 0 in front, the changes, their distances
    flat = np.concatenate([np.zeros((n, 1), np.uint8), m.transpose(0, 2, 1).reshape(n, 6)], 1)
    change = flat[:, 1:] != flat[:, :-1]
    runs = change.sum(1) + 1
    want_off = np.concatenate([[0], np.cumsum(runs)])
    rl = cocomask.encode(masks.pack(torch.from_numpy(m).to(DEV)))
    assert rl.offsets.cpu().numpy().tolist() == want_off.tolist()
    cnt = rl.counts.cpu().numpy()
    for i in list(range(40)) + list(range(65500, 65600)) + list(range(n - 40, n)):
        assert cnt[want_off[i]:want_off[i + 1]].tolist() == ora.rle_encode(m[i].tolist()), i
    pos = np.where(change, np.arange(6), 6)
    pos = np.concatenate([np.sort(pos, 1), np.full((n, 1), 6)], 1)           # the ends, then 6s; the first runs[i] are the mask's
    keep = np.arange(7) < runs[:, None]
    prev = np.concatenate([np.zeros((n, 1), np.int64), pos[:, :-1]], 1)
    assert cnt.tolist() == (pos - prev)[keep].tolist()


def byte_buffer(ms):
    from ep24 import cocomask
    desc, nbytes = cocomask._descriptors([m.shape for m in ms])
    flat = np.concatenate([m.reshape(-1) for m in ms] + [np.zeros((-nbytes) % 4, np.uint8)])
    return torch.from_numpy(flat).to(DEV), torch.from_numpy(desc).to(DEV), desc


def test_encode_buffer_masks_of_different_sizes():
    from ep24 import cocomask
    ms, want = [], []
    for k, (h, w) in enumerate(SIZES):
        cs, cw = size_cases(h, w)
        for i in (PATTERNS.index("random"), (k % len(PATTERNS))):
            ms.append(cs[i])
            want.append(cw[i])
    buf, desc, d = byte_buffer(ms)
    assert {int(o) % 4 for o in d[:, 0]} == {0, 1, 2, 3}                     # masks start at every byte offset of a word
    rl = cocomask.encode_buffer(buf, desc)
    sizes = [m.shape for m in ms]
    assert rl.size == sizes
    coco = check(rl, want, sizes)
    back, _ = cocomask.decode_batch(coco, sizes)
    assert torch.equal(back, buf)
    check(cocomask.encode_buffer(buf, d), want, sizes)                       # the table as a numpy array
    assert cocomask.encode_buffer(buf[:0], desc[:0]).to_coco() == []
    # non-zero bytes are set pixels, and a row stride above w is honoured
    wide = np.zeros((9, 12), np.uint8)
    wide[:, :7] = pattern("random", 9, 7) * 255
    stride = np.array([[0, 9, 7, 11, 57, 12]])
    check(cocomask.encode_buffer(torch.from_numpy(wide.reshape(-1)).to(DEV), stride), [ora.rle_encode((wide[:, :7] > 0).tolist())], [(9, 7)])


def test_sample_annotation_through_decode_encode_and_string():
    from ep24 import cocomask
    an, h, w = fixture_annotation()
    other = pattern("rect", 33, 125)
    buf, desc = cocomask.decode_batch([an["segmentation"], {"size": [33, 125], "counts": ora.rle_encode(other.tolist())}],
                                      [(h, w), (33, 125)])
    rl = cocomask.encode_buffer(buf, desc)
    first, second = rl.to_coco()
    mask = buf[:h * w].view(h, w).cpu().numpy()
    want = ora.rle_encode(mask.tolist())
    counts = rl.to_coco(compress=False)[0]["counts"]
    assert (h, w) == (427, 640) and first["size"] == [427, 640] and counts == want
    assert ora.rle_area(counts) == int(mask.sum()) == 32513 and len(counts) == 1131 and max(counts) == 26184
    s = first["counts"]
    assert s == ora.rle_to_string(want) and len(s) == 1158
    assert hashlib.sha256(s.encode("ascii")).hexdigest().startswith("529b61e97f6e2767")
    assert second == {"size": [33, 125], "counts": ora.rle_to_string(ora.rle_encode(other.tolist()))}


def detection(cx, cy, r, obj, conf, cls, wobble=0.0):
    radii = [r * (1.0 + wobble * ((k * 7) % 5 - 2) / 2.0) for k in range(24)]
    return [cx, cy] + radii + [obj, conf, cls]


@pytest.mark.parametrize("ratio", [1.0, 0.5])
def test_segm_results_of_synthetic_detections(ratio, tmp_path):
    from ep24 import masks, results
    from ep24.labels24 import COCO_IDS
    h, w = 50, 70
    rows = np.array([detection(30, 25, 12, 0.9, 0.8, 3, 0.2),               # inside the canvas
                     detection(66, 8, 15, 0.7, 0.6, 79),                     # clipped by the right and the top border
                     detection(200, 200, 10, 0.5, 0.4, 0)], dtype=np.float32)      # outside: the empty record
    rows[:, :26] *= ratio                                                    # detections live in the letterboxed input
    dets = torch.from_numpy(rows).to(DEV)
    res = results.SegmResults(COCO_IDS)
    assert res.add(7, None, ratio, (h, w)) == 0 and res.add(8, dets[:0], ratio, (h, w)) == 0 and len(res) == 0
    assert res.add(9, dets, ratio, (h, w)) == 3 and res.add("no_digits", dets[1:], ratio, (h, w)) == 2
    got = json.load(open(res.dump(str(tmp_path / "segm.json"))))
    assert got == res.records and [r["image_id"] for r in got] == [9, 9, 9, "no_digits", "no_digits"]
    assert [r["category_id"] for r in got] == [4, 90, 1, 90, 1]
    truth = masks.unpack(masks.detections_to_masks(dets, ratio, (h, w))).cpu().numpy().astype(np.uint8)
    for r, j in zip(got, [0, 1, 2, 1, 2]):
        assert sorted(r) == ["area", "bbox", "category_id", "image_id", "score", "segmentation"]
        assert r["segmentation"]["size"] == [h, w] and isinstance(r["segmentation"]["counts"], str)
        counts = ora.rle_from_string(r["segmentation"]["counts"])
        assert counts == ora.rle_encode(truth[j].tolist())
        assert np.array_equal(np.array(ora.rle_decode(counts, h, w), dtype=np.uint8), truth[j])
        assert r["bbox"] == ora.rle_to_bbox(counts, h, w) and r["area"] == ora.rle_area(counts) == int(truth[j].sum())
        assert r["score"] == float(np.float32(rows[j, 26]) * np.float32(rows[j, 27]))
    inside, clipped, outside = got[:3]
    x, y, bw, bh = inside["bbox"]
    assert inside["area"] > 300 and x > 0 and y > 0 and x + bw < w and y + bh < h
    x, y, bw, bh = clipped["bbox"]
    assert clipped["area"] > 100 and y == 0 and x + bw == w
    assert outside["area"] == 0 and outside["bbox"] == [0, 0, 0, 0] and ora.rle_from_string(outside["segmentation"]["counts"]) == [h * w]
    plain = results.SegmResults()
    plain.add(1, dets, ratio, (h, w))
    assert [r["category_id"] for r in plain.records] == [3, 79, 0]


def test_label_script_saves_the_decoded_masks_as_rle(tmp_path):
    from test_cocomask_host import load_script
    from test_cocomask_oracle import FIXTURE
    mod = load_script()
    an, h, w = fixture_annotation()
    (tmp_path / "images").mkdir()
    (tmp_path / "images" / (str(an["image_id"]).zfill(12) + ".jpg")).write_bytes(b"")
    out = tmp_path / "rle.json"
    poly = mod.Polygon_24("Cord", FIXTURE, str(tmp_path / "images"), str(tmp_path / "labels"), decoder="gpu", save_rle=str(out))
    poly.json_anno_process()
    got = json.load(open(out))
    assert list(got) == [str(an["id"])] and got[str(an["id"])]["size"] == [h, w]
    assert hashlib.sha256(got[str(an["id"])]["counts"].encode("ascii")).hexdigest().startswith("529b61e97f6e2767")


def test_show_24p_saves_segm_results(tmp_path):
    """``show_24p.py --save-segm`` in a fresh process, the small Exp with its initial parameters: one record per detection kept,
    every ``counts`` a mask of its image's size."""
    from ep24 import cocomask
    from test_gpu_show24p import _run
    in_dir, out_dir, segm = tmp_path / "images", str(tmp_path / "shown"), str(tmp_path / "segm.json")
    in_dir.mkdir()
    rng = np.random.default_rng(0)
    shapes = {"000000000139.npy": (96, 80), "b_small.npy": (48, 64)}
    for name, (h, w) in shapes.items():
        np.save(str(in_dir / name), rng.integers(0, 256, (h, w, 3), dtype=np.uint8))
    log = _run("show_24p.py", "-p", str(in_dir), "-b", "2", "--conf", "1e-5", "--draw-conf", "0", "--output-dir", out_dir, "--save-segm",
               segm, "--segm-category-ids", "coco")
    runs = glob.glob(os.path.join(out_dir, "*"))
    assert len(runs) == 1, (runs, log[-2000:])
    got = json.load(open(segm))
    at = 0
    for name, image_id in (("000000000139.npy", 139), ("b_small.npy", "b_small")):
        h, w = shapes[name]
        rows = np.load(os.path.join(runs[0], name + ".dets.npy"))
        recs = got[at:at + len(rows)]
        at += len(rows)
        assert len(recs) == len(rows) and all(r["image_id"] == image_id and r["segmentation"]["size"] == [h, w] for r in recs)
        for r, row in zip(recs, rows):
            assert r["score"] == float(row[26] * row[27]) and 1 <= r["category_id"] <= 90
        if recs:
            buf, _ = cocomask.decode_batch([r["segmentation"] for r in recs], [(h, w)] * len(recs))      # raises unless they sum to h * w
            areas = buf[:len(recs) * h * w].view(len(recs), h * w).sum(1, dtype=torch.int64).cpu().tolist()
            assert areas == [r["area"] for r in recs]
    assert at == len(got) > 0, "no detection at conf 1e-5: nothing was exported"
