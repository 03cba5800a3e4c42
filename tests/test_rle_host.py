"""Host side of the mask -> COCO RLE direction without a GPU: the vectorised ``rle_string_from_counts`` against the oracle's
rleToString and as the inverse of the parser, ``SegmResults`` on hand-made records, the new C entry points in the header,
argument errors before any device call and the refusal without a GPU - and the count / scan / emit / counts kernels of
csrc/rle.hip walked through lane by lane in numpy against the literal rleEncode (tests/rle_encode_oracle.py)."""
import json

import numpy as np
import pytest
import torch

import rle_encode_oracle as ora
from test_cocomask_host import load_script

SIZES = [(1, 1), (1, 9), (9, 1), (2, 3), (63, 31), (64, 32), (65, 33), (130, 65), (33, 125), (128, 64), (7, 97)]
PATTERNS = ["zeros", "ones", "first", "last", "checker", "columns", "rows", "random", "rect"]


def pattern(name, h, w, seed=0):
    """uint8 [h, w] of 0 / 1."""
    y, x = np.mgrid[0:h, 0:w]
    m = np.zeros((h, w), dtype=np.uint8)
    if name == "ones":
        m[:] = 1
    elif name == "first":
        m[0, 0] = 1
    elif name == "last":
        m[h - 1, w - 1] = 1
    elif name == "checker":
        m = ((x + y) & 1).astype(np.uint8)
    elif name == "columns":
        m = (x & 1).astype(np.uint8)
    elif name == "rows":
        m = (y & 1).astype(np.uint8)
    elif name == "random":
        m = (np.random.default_rng(1000 * h + w + seed).random((h, w)) < 0.5).astype(np.uint8)
    elif name == "rect":
        m[h // 4:h - h // 4, w // 4:w - w // 4] = 1
    else:
        assert name == "zeros"
    return m


def pack_rows(m):
    """uint8 [h, w] -> uint32 [h, ceil(w / 32)]: pixel x is bit x & 31 of word x >> 5."""
    h, w = m.shape
    ww = (w + 31) // 32
    p = np.zeros((h, ww * 32), dtype=np.uint64)
    p[:, :w] = m
    return (p.reshape(h, ww, 32) << np.arange(32, dtype=np.uint64)).sum(2).astype(np.uint32)


def strips(bits, H, W, xw):
    """rle.hip's traversal of one word column: per strip of 64 rows the transition words t[64] (uint32), lane = row."""
    valid = np.uint32(0xFFFFFFFF if W - 32 * xw >= 32 else (1 << (W - 32 * xw)) - 1)
    last = bits[H - 1]
    carry = np.uint32((int(last[xw]) << 1 | (int(last[xw - 1]) >> 31 if xw else 0)) & 0xFFFFFFFF)
    for y0 in range(0, H, 64):
        cur = np.zeros(64, dtype=np.uint32)
        k = min(64, H - y0)
        cur[:k] = bits[y0:y0 + k, xw]
        prev = np.roll(cur, 1)
        prev[0] = carry
        carry = cur[63]
        t = (cur ^ prev) & valid
        t[k:] = 0
        yield y0, t


def model_encode(batch):
    """batch: list of uint8 [h, w] -> (offsets [n + 1], counts) by the kernels' steps, one mask = one table row."""
    colprefix, runs = [], []
    packed = [pack_rows(m) for m in batch]
    for m, bits in zip(batch, packed):                                       # count, then the per-mask scan
        H, W = m.shape
        cnt = np.zeros(((W + 31) // 32) * 32, dtype=np.int64)
        for xw in range((W + 31) // 32):
            for _, t in strips(bits, H, W, xw):
                for b in range(32):
                    cnt[32 * xw + b] += int(((t >> np.uint32(b)) & np.uint32(1)).sum())
        assert not cnt[W:].any()
        cnt = cnt[:W]
        colprefix.append(np.cumsum(cnt) - cnt)
        runs.append(int(cnt.sum()) + 1)
    offsets = np.concatenate([[0], np.cumsum(runs)]).astype(np.int64)
    ends = np.full(offsets[-1], -7, dtype=np.int64)
    for n, (m, bits) in enumerate(zip(batch, packed)):                       # emit
        H, W = m.shape
        for xw in range((W + 31) // 32):
            base = np.zeros(32, dtype=np.int64)
            k = min(32, W - 32 * xw)
            base[:k] = offsets[n] + colprefix[n][32 * xw:32 * xw + k]
            for y0, t in strips(bits, H, W, xw):
                for b in range(32):
                    seg = ((t >> np.uint32(b)) & np.uint32(1)).astype(np.int64)
                    if not seg.any():
                        continue
                    rank = np.cumsum(seg) - seg
                    for lane in np.flatnonzero(seg):
                        at = base[b] + rank[lane]
                        assert offsets[n] <= at < offsets[n + 1] - 1 and ends[at] == -7
                        ends[at] = (32 * xw + b) * H + y0 + lane
                    base[b] += seg.sum()
    counts = np.zeros(offsets[-1], dtype=np.int64)
    for n, m in enumerate(batch):                                            # counts
        for i in range(offsets[n], offsets[n + 1]):
            end = ends[i] if i < offsets[n + 1] - 1 else m.size
            counts[i] = end - (ends[i - 1] if i > offsets[n] else 0)
    return offsets, counts


def test_kernel_steps_in_numpy_equal_rle_encode():
    batch = [pattern(p, h, w) for h, w in SIZES for p in PATTERNS]
    offsets, counts = model_encode(batch)
    most = 0
    for n, m in enumerate(batch):
        want = ora.rle_encode(m.tolist())
        assert counts[offsets[n]:offsets[n + 1]].tolist() == want, (n, m.shape)
        assert ora.rle_area(want) == int(m.sum())
        most = max(most, len(want))
    assert most == 8450                                                      # alternate rows at 130 x 65: every pixel a run
    assert ora.rle_encode([[0, 0], [0, 0]]) == [4] and ora.rle_encode([[1, 1], [1, 1]]) == [0, 4]
    assert ora.rle_encode([[1, 0], [0, 0]]) == [0, 1, 3]


def from_differences(first, diffs):
    """counts whose stored values from the fourth on are ``diffs``."""
    c = list(first)
    for d in diffs:
        c.append(c[-2] + d)
    assert min(c) >= 0
    return c


EDGES = [15, 16, 511, 512, 16383, 16384, 524287, 524288, 2 ** 24 - 1, 2 ** 24, 2 ** 29 - 1, 2 ** 29]      # last value of k characters, first of k + 1
STRING_CASES = [
    from_differences([1, 1, 1], EDGES),
    from_differences([2 ** 30, 2 ** 30, 2 ** 30], [-d - 1 for d in EDGES]),
    [12], [0, 12], [3, 1025, 2, 1, 1500, 1500, 31, 32, 15, 16], [0, 5, 3, 2000, 7, 1, 40000, 2, 1],
    [5, 4, 3, 2, 1, 0, 7],                                                   # negative differences
    [0, 1, 2, 15, 16, 17, 527, 528, 529],                                    # 1 / 2 character boundaries (+15 / +16, -16 / -17)
    [2 ** 31 - 1, 7, 1, 7, 2 ** 31 - 1, 7, 0, 7, 2 ** 29, 7, 2 ** 29 - 2 ** 24 - 1, 7, 0],   # large negative differences
]


def test_string_writer_is_the_oracles_and_inverts_the_parser():
    from ep24 import cocomask
    lengths = set()
    for cnts in STRING_CASES:
        s = cocomask.rle_string_from_counts(cnts)
        assert isinstance(s, str) and s == ora.rle_to_string(cnts)
        assert cocomask.rle_counts_from_string(s) == cnts == ora.rle_from_string(s)
        assert cocomask.rle_string_from_counts(np.array(cnts, dtype=np.int32)) == s
        for i, c in enumerate(cnts):                                         # characters per value, from the oracle
            lengths.add(len(ora.rle_to_string([c - (cnts[i - 2] if i > 2 else 0)])))
    assert lengths >= {1, 2, 3, 4, 5, 6, 7}
    # several masks at once: the difference rule restarts with every mask
    flat = np.concatenate([np.array(c, dtype=np.int64) for c in STRING_CASES])
    off = np.concatenate([[0], np.cumsum([len(c) for c in STRING_CASES])])
    assert cocomask.rle_string_from_counts(flat, off) == [ora.rle_to_string(c) for c in STRING_CASES]
    rng = np.random.default_rng(3)
    many = [rng.integers(0, 3000, rng.integers(1, 40)).tolist() for _ in range(50)]
    off = np.concatenate([[0], np.cumsum([len(c) for c in many])])
    assert cocomask.rle_string_from_counts(np.concatenate(many), off) == [ora.rle_to_string(c) for c in many]
    assert cocomask.rle_string_from_counts([], [0]) == [] and cocomask.rle_string_from_counts([], [0, 0]) == [""]
    assert cocomask.rle_string_from_counts([]) == ""
    for bad in ([1, 3], [0, 2], [0, 2, 1, 3]):
        with pytest.raises(ValueError):
            cocomask.rle_string_from_counts([1, 2, 3], bad)


def test_run_lengths_to_coco_on_host_tensors():
    from ep24 import cocomask
    a, b = [0, 5, 3, 2, 20, 1, 11], [12]
    rl = cocomask.RunLengths(torch.tensor([0, 7, 8]), torch.tensor(a + b, dtype=torch.int32), [(6, 7), (4, 3)])
    assert len(rl) == 2 and rl.sizes == [(6, 7), (4, 3)]
    assert rl.to_coco() == [{"size": [6, 7], "counts": ora.rle_to_string(a)}, {"size": [4, 3], "counts": ora.rle_to_string(b)}]
    assert rl.to_coco(compress=False) == [{"size": [6, 7], "counts": a}, {"size": [4, 3], "counts": b}]
    assert cocomask.RunLengths(torch.tensor([0, 1, 2]), torch.tensor([12, 12], dtype=torch.int32), (4, 3)).sizes == [(4, 3)] * 2


def test_segm_results_records_and_dump(tmp_path):
    from ep24 import results
    from ep24.labels24 import COCO_IDS
    assert load_script().COCO_IDS is COCO_IDS and len(COCO_IDS) == 80 and COCO_IDS[0] == 1 and COCO_IDS[79] == 90 and COCO_IDS[11] == 13
    m = np.zeros((5, 4), dtype=np.uint8)
    m[1:4, 2:4] = 1
    cnts = ora.rle_encode(m.tolist())
    segs = [{"size": [5, 4], "counts": ora.rle_to_string(cnts)}, {"size": [5, 4], "counts": ora.rle_to_string([20])}]
    res = results.SegmResults(COCO_IDS)
    res.add_records(139, segs, [[2, 1, 3, 3], [4, 5, -1, -1]], [6, 0], np.array([0.75, 0.5], dtype=np.float32), [0, 79])
    res.add_records("street", segs[:1], [[2, 1, 3, 3]], [6], [0.25], [11])
    assert len(res) == 3
    path = res.dump(str(tmp_path / "segm.json"))
    got = json.load(open(path))
    assert got == [
        {"image_id": 139, "category_id": 1, "segmentation": segs[0], "score": 0.75, "bbox": ora.rle_to_bbox(cnts, 5, 4), "area": 6},
        {"image_id": 139, "category_id": 90, "segmentation": segs[1], "score": 0.5, "bbox": [0, 0, 0, 0], "area": 0},
        {"image_id": "street", "category_id": 13, "segmentation": segs[0], "score": 0.25, "bbox": [2, 1, 2, 3], "area": 6}]
    assert ora.rle_to_bbox([20], 5, 4) == [0, 0, 0, 0] and ora.rle_area(cnts) == 6
    plain = results.SegmResults()
    plain.add_records(1, segs[:1], [[2, 1, 3, 3]], [6], [1.0], [57])
    assert plain.records[0]["category_id"] == 57
    with pytest.raises(IndexError):
        res.add_records(1, segs[:1], [[2, 1, 3, 3]], [6], [1.0], [80])
    with pytest.raises(ValueError):
        res.add_records(1, segs, [[2, 1, 3, 3]], [6], [1.0], [0])


def test_header_declares_the_rle_entry_points():
    from ep24 import _lib
    protos = _lib.parse_header()
    for name in ("ep24_rle_pack_bytes", "ep24_rle_count", "ep24_rle_scan", "ep24_rle_emit", "ep24_rle_counts"):
        assert name in protos and protos[name][0] == "int" and protos[name][1][-1] == ("void*", "stream"), name
    assert [a for _, a in protos["ep24_rle_count"][1]] == ["bits", "tab", "N", "H", "W", "colcnt", "stream"]


def _packed(bits, size):
    from ep24 import masks
    n = bits.shape[0]
    return masks.PackedMasks(bits, torch.zeros(n, 4, dtype=torch.int32), torch.zeros(n, dtype=torch.int32), size)


def test_argument_errors_come_before_the_gpu(monkeypatch):
    from ep24 import _lib, cocomask, results

    def no_gpu(*a, **k):
        raise AssertionError("the GPU was touched")
    monkeypatch.setattr(_lib, "require_gpu", no_gpu)
    monkeypatch.setattr(cocomask, "call", no_gpu)
    good = _packed(torch.zeros(2, 5, 1, dtype=torch.int32), (5, 7))
    with pytest.raises(IndexError):
        cocomask.encode(torch.zeros(2, 5, 7, dtype=torch.uint8))             # not PackedMasks
    with pytest.raises(IndexError):
        cocomask.encode(_packed(torch.zeros(2, 5, 2, dtype=torch.int32), (5, 7)))      # words per row
    with pytest.raises(IndexError):
        cocomask.encode(_packed(torch.zeros(2, 5, 1, dtype=torch.int64), (5, 7)))
    with pytest.raises(_lib.Ep24Error, match="UNSUPPORTED"):
        cocomask.encode(_packed(torch.zeros(0, 1, 1, dtype=torch.int32), (65536, 32768)))   # H * W = 2^31
    for out in ((torch.zeros(2, dtype=torch.int64), torch.zeros(9, dtype=torch.int32)),    # offsets too short
                (torch.zeros(3, dtype=torch.int32), torch.zeros(9, dtype=torch.int32)),
                (torch.zeros(3, dtype=torch.int64), torch.zeros(9, dtype=torch.int64)),
                torch.zeros(3, dtype=torch.int64)):
        with pytest.raises(ValueError):
            cocomask.encode(good, out=out)
    buf = torch.zeros(40, dtype=torch.uint8)
    for desc in ([[0, 5, 7, 8, 43, 7, 1]], [[0, 5, 9, 8, 43, 9]], [[8, 5, 7, 8, 43, 7]], [[0, 0, 7, 8, 43, 7]], [[-1, 5, 7, 8, 43, 7]],
                 [[0, 5, 7, 8, 43, 6]]):
        with pytest.raises(ValueError):
            cocomask.encode_buffer(buf, np.array(desc))
    with pytest.raises(ValueError):
        cocomask.encode_buffer(buf.view(5, 8), np.array([[0, 5, 7, 8, 43, 7]]))
    with pytest.raises(IndexError):
        results.SegmResults().add(1, torch.zeros(3, 26), 1.0, (8, 8))


def test_encode_refuses_to_run_without_a_gpu():
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    from ep24 import _lib, cocomask, results
    with pytest.raises(_lib.Ep24Error):
        cocomask.encode(_packed(torch.zeros(2, 5, 1, dtype=torch.int32), (5, 7)))
    with pytest.raises(_lib.Ep24Error):
        cocomask.encode_buffer(torch.zeros(36, dtype=torch.uint8), np.array([[0, 5, 7, 8, 43, 7]]))
    with pytest.raises(_lib.Ep24Error):
        results.SegmResults().add(1, torch.zeros(3, 29), 1.0, (8, 8))


def test_label_script_refuses_save_rle_without_the_gpu_decoder(tmp_path):
    mod = load_script()
    with pytest.raises(ValueError, match="--decoder gpu"):
        mod.Polygon_24("Cord", str(tmp_path / "none.json"), str(tmp_path), str(tmp_path / "out"), save_rle=str(tmp_path / "rle.json"))
    import os
    import subprocess
    import sys
    from conftest import PKG
    r = subprocess.run([sys.executable, os.path.join("datasets", "labels_create_24p.py"), "--json", "x.json", "--images", "x",
                        "--save-rle", str(tmp_path / "rle.json")], cwd=os.path.join(PKG, "yolox_24p"), capture_output=True, text=True)
    assert r.returncode == 2 and "--decoder gpu" in r.stderr and not (tmp_path / "rle.json").exists()


def test_show_24p_segm_flags():
    from test_draw24_api import _show24p
    mod = _show24p()
    a = mod.make_parser().parse_args([])
    assert a.save_segm is None and a.segm_category_ids == "index"
    a = mod.make_parser().parse_args(["--save-segm", "r.json", "--segm-category-ids", "coco"])
    assert a.save_segm == "r.json" and a.segm_category_ids == "coco"
    with pytest.raises(SystemExit):
        mod.make_parser().parse_args(["--segm-category-ids", "names"])
