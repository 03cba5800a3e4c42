"""Host side of ep24.cocomask without a GPU: argument errors are raised before any device call, the RLE string parser
agrees with the oracle's, and the launch tables (_plan) decode to the oracle's masks when the three kernels of
csrc/cocomask.hip are walked through sequentially in Python."""
import importlib.util
import math
import os
import sys

import numpy as np
import pytest

import cocomask_oracle as ora
from conftest import PKG
from test_cocomask_oracle import TABLE, random_polygons


def edge_point(e, d):
    xs, ys, xe, ye = (int(v) for v in e[:4])
    dx, dy = abs(xe - xs), abs(ye - ys)
    if dx == 0 and dy == 0:
        return xs, ys
    flip = (dx >= dy and xs > xe) or (dx < dy and ys > ye)
    if flip:
        xs, xe, ys, ye = xe, xs, ye, ys
    if dx >= dy:
        t = dx - d if flip else d
        return t + xs, int(ys + float(ye - ys) / dx * t + .5)
    t = dy - d if flip else d
    return int(xs + float(xe - xs) / dy * t + .5), t + ys


def run_plan(plan):
    """poly_xor, poly_scan and rle of csrc/cocomask.hip, one thread after the other."""
    desc, total = plan["desc"], plan["total"]
    buf = [0] * total
    for e0, e1, items, max_w in plan["rounds"]:
        edges, start = plan["edges"][e0:e1], plan["start"][e0:e1 + 1]
        assert edges[0][6] == 1 and max_w >= max(desc[it >> 1][2] for it in items)
        for lo in range(e1 - e0):
            e = edges[lo]
            for d in range(int(start[lo + 1] - start[lo])):
                if d == 0 and e[6]:
                    continue
                a = edge_point(e, d)
                b = edge_point(e, d - 1) if d else edge_point(edges[lo - 1], int(start[lo] - start[lo - 1]) - 1)
                if a[0] == b[0]:
                    continue
                xd = (float(a[0] if a[0] < b[0] else a[0] - 1) + .5) / 5 - .5
                off, H, W, _, _, ld = (int(v) for v in desc[e[4]])
                if math.floor(xd) != xd or xd < 0 or xd > W - 1:
                    continue
                y = math.ceil(min(max((float(min(a[1], b[1])) + .5) / 5 - .5, 0.0), float(H)))
                if y >= H:
                    continue
                assert 0 <= e[5] < 7
                buf[off + y * ld + int(xd)] ^= 1 << int(e[5])
        for it in items:
            off, H, W, _, _, ld = (int(v) for v in desc[it >> 1])
            for x in range(W):
                run = 0
                for y in range(H):
                    v = buf[off + y * ld + x]
                    run ^= v & 0x7f
                    on = int(run != 0) | (v >> 7)
                    buf[off + y * ld + x] = on if it & 1 else on << 7
    if plan["runs"] is not None:
        for a, first, n in plan["runs"]:
            off, H, W, _, _, ld = (int(v) for v in desc[a])
            end = plan["ends"][first:first + n]
            assert plan["max_w"] >= W and end[-1] == H * W
            for x in range(W):
                lo = int(np.searchsorted(end, x * H, side="right"))
                for y in range(H):
                    while end[lo] <= x * H + y:
                        lo += 1
                    buf[off + y * ld + x] = lo & 1
    return buf


def masks_of(buf, desc):
    return [[buf[off + y * ld: off + y * ld + W] for y in range(H)] for off, H, W, _, _, ld in (map(int, d) for d in desc)]


def test_plan_decodes_to_the_oracle():
    from ep24 import cocomask
    rnd = random_polygons(40, seed=5)
    many = [xy for xy, _, _ in random_polygons(17, seed=6)]
    segs = [c[1] for c in TABLE] + [[xy] for xy, _, _ in rnd] + [many[:7], many[:8], many[:9], many[:14], many[:15], many]
    sizes = [(c[2], c[3]) for c in TABLE] + [(h, w) for _, h, w in rnd] + [(23, 31)] * 6
    cnts = [0, 5, 3, 2, 20, 1, 11]
    segs += [{"size": [6, 7], "counts": cnts}, {"size": [6, 7], "counts": ora.rle_to_string(cnts)}, {"counts": [42]}]
    sizes += [(6, 7)] * 3
    plan = cocomask._plan(segs, sizes)
    assert plan["total"] % 4 == 0 and 0 <= plan["total"] - plan["nbytes"] < 4
    assert len(plan["rounds"]) == 3 and [len(r[2]) for r in plan["rounds"]] == [len(TABLE) + 46, 5, 2]
    got = masks_of(run_plan(plan), plan["desc"])
    for i, (seg, (h, w)) in enumerate(zip(segs, sizes)):
        assert got[i] == ora.ann_to_mask(seg, h, w), i


def test_descriptors_are_ray24s():
    from ep24 import cocomask
    sizes = [(427, 640), (1, 1), (3, 5), (480, 640), (333, 500)]
    desc, nbytes = cocomask._descriptors(sizes)
    off = 0
    for d, (H, W) in zip(desc.tolist(), sizes):
        L = int(np.sqrt(np.power(H, 2) + np.power(W, 2)))                     # the scalar forms of labels24.rays_batch
        assert d == [off, H, W, L, int(np.ceil((L - 0) / 0.2)), W]
        off += H * W
    assert nbytes == off and desc[0, 3] == 769


def test_rle_string_parser_is_the_oracles():
    from ep24 import cocomask
    for cnts in ([0, 5, 3, 2000, 7, 1, 40000, 2, 1], [12], [3, 1025, 2, 1, 1500, 1500, 31, 32, 15, 16]):
        s = ora.rle_to_string(cnts)
        assert cocomask.rle_counts_from_string(s) == cnts and cocomask.rle_counts_from_string(s.encode()) == cnts
    with pytest.raises(ValueError):
        cocomask.rle_counts_from_string("5P")                       # ends inside a number
    with pytest.raises(ValueError):
        cocomask.rle_counts_from_string("5 3")


@pytest.mark.parametrize("seg, size", [
    ([[1, 1, 5, 1, 5]], (8, 8)),                                    # odd coordinate count
    ([], (8, 8)),                                                   # no polygon
    ([[]], (8, 8)),                                                 # a polygon without vertices
    ([[1, 1, float("nan"), 2]], (8, 8)),
    ([[1, 1, 3e6, 2]], (8, 8)),
    ({"size": [8, 8], "counts": [10, 20, 33]}, (8, 8)),             # counts do not sum to h * w
    ({"size": [8, 8], "counts": [70, -6]}, (8, 8)),
    ({"size": [8, 9], "counts": [64]}, (8, 8)),
    ([[1, 1, 5, 1, 5, 5]], (12000, 12000)),                         # H + W + L >= 32768
    ([[1, 1, 5, 1, 5, 5]], (0, 8)),
])
def test_argument_errors_come_before_the_gpu(seg, size, monkeypatch):
    from ep24 import _lib, cocomask

    def no_gpu(*a, **k):
        raise AssertionError("the GPU was touched")
    monkeypatch.setattr(_lib, "require_gpu", no_gpu)
    monkeypatch.setattr(cocomask, "call", no_gpu)
    with pytest.raises(ValueError):
        cocomask.decode_batch([seg], [size])
    with pytest.raises(ValueError):
        cocomask.ann_to_mask(seg, size[0], size[1])


def load_script():
    d = os.path.join(PKG, "yolox_24p")
    sys.path.insert(0, d)
    try:
        spec = importlib.util.spec_from_file_location("labels_create_24p", os.path.join(d, "datasets", "labels_create_24p.py"))
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
    finally:
        sys.path.remove(d)
    return mod


def test_pycocotools_decoder_is_unchanged():
    mod = load_script()
    try:
        import pycocotools  # noqa: F401
    except ImportError:
        with pytest.raises(ImportError, match="pycocotools"):
            mod.Polygon_24()
    with pytest.raises(ValueError):
        mod.Polygon_24(decoder="host")
    assert mod.Polygon_24.__init__.__defaults__[-1] == "pycocotools"


def test_script_starts_from_its_documented_directory():
    """``cd yolox_24p && python datasets/labels_create_24p.py``: Python puts datasets/ on the path, not yolox_24p/."""
    import subprocess
    r = subprocess.run([sys.executable, os.path.join("datasets", "labels_create_24p.py"), "--help"],
                       cwd=os.path.join(PKG, "yolox_24p"), capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert "--decoder" in r.stdout and "pycocotools" in r.stdout and "gpu" in r.stdout
