"""ep24.cocomask on the GPU: every decoded mask bit-equal to tests/cocomask_oracle.py inside a sentinel-framed buffer,
two runs bytewise identical, the decoded buffer fed to the rays without leaving the device, and the label script with
``decoder="gpu"`` writing the rows the oracle's masks give."""
import functools
import json
import os

import numpy as np
import pytest
import torch

import cocomask_oracle as ora
from test_cocomask_host import load_script
from test_cocomask_oracle import FIXTURE, TABLE, fixture_annotation, random_polygons

pytestmark = pytest.mark.gpu

FRAME, SENTINEL = 64, 0xA5
RLE_COUNTS = [0, 5, 3, 2, 20, 1, 11]                                # 6 x 7, the first run empty


@functools.lru_cache(maxsize=None)
def batch():
    """(name, segmentation, h, w) of every case, and the oracle's masks for them, computed once."""
    cases = [(c[0], c[1], c[2], c[3]) for c in TABLE]
    cases += [("random%d" % i, [xy], h, w) for i, (xy, h, w) in enumerate(random_polygons(200, seed=2024))]
    many = [xy for xy, _, _ in random_polygons(17, seed=6)]
    cases += [("polygons%d" % n, many[:n], 23, 31) for n in (7, 8, 9, 14, 15, 17)]     # 7 polygons to a round
    tri = [-2.0, -1.5, 9.3, 2.2, 3.1, 11.7]
    cases += [("w1", [tri], 9, 1), ("h1", [tri], 1, 9), ("w_not_4", [tri], 5, 7), ("w_not_4b", [tri], 6, 9)]
    an, h, w = fixture_annotation()
    cases.append(("fixture", an["segmentation"], h, w))
    long_counts = [3, 1025, 2, 1, 1500, 1500, 31, 32, 15, 16]                          # 4125 = 33 x 125
    cases += [("rle_list", {"size": [6, 7], "counts": RLE_COUNTS}, 6, 7),
              ("rle_string", {"size": [6, 7], "counts": ora.rle_to_string(RLE_COUNTS)}, 6, 7),
              ("rle_long", {"size": [33, 125], "counts": ora.rle_to_string(long_counts)}, 33, 125),
              ("rle_zeros", {"size": [4, 3], "counts": [12]}, 4, 3),
              ("rle_ones", {"size": [4, 3], "counts": [0, 12]}, 4, 3),
              ("rle_empty_runs", {"size": [4, 3], "counts": [2, 0, 3, 4, 0, 0, 3]}, 4, 3)]
    cases.append(("after_rle", [[0.5, 0.5, 4.5, 0.5, 4.5, 2.5]], 3, 5))                # an odd offset behind the RLE masks
    want = [np.array(ora.ann_to_mask(seg, h, w), dtype=np.uint8).reshape(h, w) for _, seg, h, w in cases]
    return cases, want


def decode_framed(cases):
    from ep24 import cocomask
    nbytes = sum(h * w for _, _, h, w in cases)
    total = (nbytes + 3) // 4 * 4
    big = torch.full((total + 2 * FRAME,), SENTINEL, dtype=torch.uint8, device="cuda:0")
    buf, desc = cocomask.decode_batch([c[1] for c in cases], [(c[2], c[3]) for c in cases], out=big[FRAME:FRAME + total])
    torch.cuda.synchronize()
    assert buf.data_ptr() == big.data_ptr() + FRAME and buf.numel() == total
    return big.cpu().numpy(), desc.cpu().numpy(), nbytes, total


def test_masks_bit_equal_to_the_oracle_inside_a_frame():
    cases, want = batch()
    big, desc, nbytes, total = decode_framed(cases)
    assert (big[:FRAME] == SENTINEL).all() and (big[FRAME + total:] == SENTINEL).all(), "the frame was written"
    assert (big[FRAME + nbytes:FRAME + total] == 0).all()
    buf = big[FRAME:FRAME + total]
    offsets = set()
    for (name, _, h, w), d, m in zip(cases, desc, want):
        assert list(d[1:3]) == [h, w] and d[5] == w
        got = buf[d[0]:d[0] + h * w].reshape(h, w)
        assert np.array_equal(got, m), (name, int((got != m).sum()))
        offsets.add(int(d[0]) % 4)
    assert offsets == {0, 1, 2, 3}                                   # masks share 32-bit words at every byte offset
    assert int(want[[c[0] for c in cases].index("fixture")].sum()) == 32513


def test_two_runs_are_bytewise_identical():
    cases, _ = batch()
    a, b = decode_framed(cases)[0], decode_framed(cases)[0]
    assert a.tobytes() == b.tobytes()


def test_decode_batch_allocates_and_ann_to_mask():
    from ep24 import cocomask
    cases, want = batch()
    pick = [i for i, c in enumerate(cases) if c[0] in ("two_squares", "polygons17", "rle_string", "w1")]
    buf, desc = cocomask.decode_batch([cases[i][1] for i in pick], [(cases[i][2], cases[i][3]) for i in pick])
    assert buf.dtype == torch.uint8 and buf.is_cuda and buf.numel() % 4 == 0 and desc.dtype == torch.int64 and desc.shape == (4, 6)
    for j, i in enumerate(pick):
        _, seg, h, w = cases[i]
        off = int(desc[j, 0])
        assert np.array_equal(buf[off:off + h * w].view(h, w).cpu().numpy(), want[i])
        m = cocomask.ann_to_mask(seg, h, w)
        assert isinstance(m, np.ndarray) and m.dtype == np.uint8 and m.shape == (h, w) and set(np.unique(m)) <= {0, 1}
        assert np.array_equal(m, want[i])
    empty, d0 = cocomask.decode_batch([], [])
    assert empty.numel() == 0 and d0.shape == (0, 6)


def test_rays_from_the_decoded_buffer_equal_rays_from_host_masks():
    from ep24 import cocomask, labels24
    cases, want = batch()
    centres = [[w / 2 + 0.25, h / 2] for _, _, h, w in cases]
    buf, desc = cocomask.decode_batch([c[1] for c in cases], [(c[2], c[3]) for c in cases])
    pts, rad = labels24.rays_from_buffer(buf, desc, centres)
    want_p, want_r = labels24.rays_batch(want, centres)
    assert pts.shape == (len(cases), 24, 2) and torch.equal(pts, want_p) and torch.equal(rad, want_r)
    assert bool((pts >= 0).all(dim=2).any())


def test_label_script_with_the_gpu_decoder(tmp_path):
    from ep24 import labels24
    mod = load_script()
    with open(FIXTURE) as f:
        d = json.load(f)
    real = d["annotations"][0]
    octagon = [200, 100, 300, 100, 360, 160, 360, 260, 300, 320, 200, 320, 140, 260, 140, 160]
    crowd = dict(real, id=2, iscrowd=1, segmentation={"size": [427, 640], "counts": [1000, 500, 427 * 640 - 1500]})
    d["annotations"] = [real,
                        dict(real, id=3, segmentation=[octagon], area=41200.0, bbox=[140, 100, 220, 220], category_id=90),
                        crowd,
                        dict(real, id=4, area=0.5),
                        dict(real, id=5, image_id=7)]                # its image file is missing
    d["images"].append(dict(d["images"][0], id=7, file_name="000000000007.jpg", height=300, width=400))
    (tmp_path / "images").mkdir()
    (tmp_path / "images" / "000000130566.jpg").write_bytes(b"")
    with open(tmp_path / "ann.json", "w") as f:
        json.dump(d, f)
    for mode, width in (("Cord", 51), ("Radius", 27)):
        out = tmp_path / ("labels_" + mode)
        poly = mod.Polygon_24(mode, str(tmp_path / "ann.json"), str(tmp_path / "images"), str(out), decoder="gpu")
        poly.json_anno_process()
        poly.save_24r_to_txt()
        # the same two annotations through the oracle's host masks
        kept = d["annotations"][:2]
        masks = [np.array(ora.ann_to_mask(a["segmentation"], 427, 640), dtype=np.uint8) for a in kept]
        centres = [(a["bbox"][0] + a["bbox"][2] / 2, a["bbox"][1] + a["bbox"][3] / 2) for a in kept]
        pts, rad = labels24.rays_batch(masks, centres)
        keep, cord, radius = labels24.label_rows([poly.coco_id2idx[str(a["category_id"])] for a in kept], centres,
                                                 [m.shape for m in masks], pts, rad, labels24.hull_areas(pts), [a["area"] for a in kept])
        rows = cord if mode == "Cord" else radius
        assert rows.shape == (int(keep.sum()), width) and keep[1]     # the octagon passes the hull-area filter
        labels24.save_rows(tmp_path / "want.txt", rows)
        assert sorted(os.listdir(out)) == ["000000000007.txt", "000000130566.txt"]
        assert (out / "000000130566.txt").read_text() == (tmp_path / "want.txt").read_text() != ""
        assert (out / "000000000007.txt").read_text() == ""
        got = labels24.load_rows(out / "000000130566.txt")
        assert got.shape == rows.shape and got[-1, 0] == 79
