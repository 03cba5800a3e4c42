"""ep24_mask_boundary, ep24_segm_iou_min, ``SegmEvaluator(iou_type="boundary")``, ``eval_segm.py --iou-type boundary`` and
``ep24.masks.boundary`` on the GPU against tests/boundary_oracle.py, everything exact: the bands word for word on masks of mixed
sizes and radii inside sentinel frames (one table call, the uniform form, the wide, tall and very tall shapes where the kernel takes
another path), the contract's edges, and the evaluator end to end on the scene of tests/test_gpu_segmeval.py."""
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import boundary_oracle as bo
import cocomask_oracle as cmo
from test_boundary_oracle import boundary_want, dataset_masks
from test_cocomask_oracle import fixture_annotation
from test_gpu_segmeval import DEV, ROOT, dataset, dev, framed, frames_intact, pack_bits, tables_equal, want_stats

pytestmark = pytest.mark.gpu

E_ARG, E_UNSUPPORTED = -1, -3
WIDTHS, HEIGHTS, RADII = (1, 31, 32, 33, 64, 65, 97), (1, 7, 40), (1, 2, 5, 33, 40)


def kinds(H, W, rng):
    """The mask kinds of one size: random at three densities, empty, full, full minus one interior pixel, one pixel in each corner,
    a filled rectangle that touches two image edges."""
    out = [rng.rand(H, W) < p for p in (0.5, 0.9, 0.98)]
    out += [np.zeros((H, W), dtype=bool), np.ones((H, W), dtype=bool)]
    m = np.ones((H, W), dtype=bool)
    m[H // 2, W // 2] = False
    out.append(m)
    for y, x in ((0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1)):
        m = np.zeros((H, W), dtype=bool)
        m[y, x] = True
        out.append(m)
    m = np.zeros((H, W), dtype=bool)
    m[:(2 * H + 2) // 3, :(3 * W + 3) // 4] = True
    out.append(m)
    return out


@functools.lru_cache(maxsize=None)
def mixed():
    """-> (masks, radii): every size of WIDTHS x HEIGHTS with every mask kind and the radii of RADII in turn (every size meets every
    radius), the wide row, the tall mask with d > W, a mask of 9 000 rows (two bands of rows), one wide enough for tiles of word
    columns, and the 427 x 640 fixture annotation at d = 15 and 38."""
    rng = np.random.RandomState(17)
    masks, radii = [], []
    k = 0
    for W in WIDTHS:
        for H in HEIGHTS:
            ms = kinds(H, W, rng)
            for j, m in enumerate(ms):
                masks.append(m)
                radii.append(RADII[(k + j) % len(RADII)])
            for d in RADII:                                                        # a dense random mask at every radius
                masks.append(rng.rand(H, W) < 0.995)
                radii.append(d)
            k += 1
    for H, W, d in ((3, 2100, 70), (300, 5, 100), (300, 5, 2), (9000, 3, 1), (70, 4200, 30)):
        for m in (rng.rand(H, W) < 0.999, np.ones((H, W), dtype=bool)):
            masks.append(m)
            radii.append(d)
    an, fh, fw = fixture_annotation()
    big = np.array(cmo.ann_to_mask(an["segmentation"], fh, fw), dtype=bool)
    assert (fh, fw) == (427, 640)
    masks += [big, big]
    radii += [15, 38]
    return masks, radii


@functools.lru_cache(maxsize=None)
def mixed_want():
    masks, radii = mixed()
    return [pack_bits(bo.boundary(m, min(d, max(m.shape)))) for m, d in zip(masks, radii)]       # d >= max(H, W): the whole mask


def table_of(masks, radii):
    packed = [pack_bits(m) for m in masks]
    words = np.concatenate([[0], np.cumsum([p.size for p in packed])])
    tab = np.stack([words[:-1], [m.shape[0] for m in masks], [m.shape[1] for m in masks], radii], 1).astype(np.int64)
    return packed, words, tab


def test_bands_of_mixed_sizes_and_radii_in_one_table_call():
    from ep24._lib import call, ptr, stream_ptr
    masks, radii = mixed()
    want = mixed_want()
    N = len(masks)
    packed, words, tab = table_of(masks, radii)
    total = int(words[-1])
    bits = dev(np.concatenate([p.reshape(-1) for p in packed]).view(np.int32))
    tab_t = dev(tab)
    Hm, Wm = int(tab[:, 1].max()), int(tab[:, 2].max())
    big, out, fill = framed(total, torch.int32)
    call("mask_boundary", ptr(bits), ptr(tab_t), N, Hm, Wm, 0, ptr(out), stream_ptr())
    got = out.cpu().numpy().view(np.uint32)
    assert frames_intact(big, total, fill)
    eroded = whole = 0
    for n in range(N):
        g = got[words[n]:words[n + 1]].reshape(want[n].shape)
        assert np.array_equal(g, want[n]), (masks[n].shape, radii[n], n)
        eroded += int(not np.array_equal(want[n], packed[n]))
        whole += int(np.array_equal(want[n], packed[n]) and masks[n].any())
    assert eroded > 20 and whole > 20
    # a second call writes the same words
    big2, out2, _ = framed(total, torch.int32)
    call("mask_boundary", ptr(bits), ptr(tab_t), N, Hm, Wm, 0, ptr(out2), stream_ptr())
    assert torch.equal(out2, out) and frames_intact(big2, total, fill)


def test_very_tall_mask_with_a_radius_beyond_the_lds_arrays():
    """9 000 x 3 at d = 4 500: 2 d + 1 rows do not fit the kernel's LDS arrays and it walks the rows directly.  The oracle's 4 500
    literal iterations would take seconds, and the definition gives the answer outright: d >= W, so every pixel's window reaches
    outside the image, nothing survives the erosion and the band is the mask itself.  (d = 1 on this shape is in ``mixed``.)"""
    from ep24._lib import call, ptr, stream_ptr
    rng = np.random.RandomState(19)
    masks = [rng.rand(9000, 3) < 0.999, np.ones((9000, 3), dtype=bool), np.zeros((9000, 3), dtype=bool)]
    assert not bo.erode(masks[1][:40], 3).any()                                     # the same argument at a size the oracle walks
    packed, words, tab = table_of(masks, [4500, 4500, 4500])
    total = int(words[-1])
    bits = dev(np.concatenate([p.reshape(-1) for p in packed]).view(np.int32))
    tab_t = dev(tab)
    big, out, fill = framed(total, torch.int32)
    call("mask_boundary", ptr(bits), ptr(tab_t), 3, 9000, 3, 0, ptr(out), stream_ptr())
    assert torch.equal(out, bits) and frames_intact(big, total, fill)
    big2, out2, _ = framed(total, torch.int32)
    call("mask_boundary", ptr(bits), None, 3, 9000, 3, 4500, ptr(out2), stream_ptr())
    assert torch.equal(out2, bits) and frames_intact(big2, total, fill)


@pytest.mark.parametrize("H,W,d", ((40, 65, 2), (7, 97, 33), (40, 33, 100)))
def test_uniform_form_gives_the_same_words(H, W, d):
    from ep24._lib import call, ptr, stream_ptr
    rng = np.random.RandomState(23)
    masks = [rng.rand(H, W) < p for p in (0.5, 0.9, 0.98, 0.999)] + [np.ones((H, W), dtype=bool)]
    N = len(masks)
    packed, words, tab = table_of(masks, [d] * N)
    bits = dev(np.concatenate([p.reshape(-1) for p in packed]).view(np.int32))
    total = int(words[-1])
    big, out, fill = framed(total, torch.int32)
    call("mask_boundary", ptr(bits), None, N, H, W, d, ptr(out), stream_ptr())
    want = np.concatenate([pack_bits(bo.boundary(m, min(d, max(H, W)))).reshape(-1) for m in masks])
    assert np.array_equal(out.cpu().numpy().view(np.uint32), want) and frames_intact(big, total, fill)
    tab_t = dev(tab)
    big2, out2, _ = framed(total, torch.int32)
    call("mask_boundary", ptr(bits), ptr(tab_t), N, H, W, 0, ptr(out2), stream_ptr())
    assert torch.equal(out2, out) and frames_intact(big2, total, fill)


def test_contract_edges():
    from ep24._lib import Ep24Error, call, ptr, stream_ptr
    rng = np.random.RandomState(29)
    masks = [rng.rand(40, 65) < 0.95 for _ in range(6)]
    packed, words, tab = table_of(masks, [2] * 6)
    tab[1, 0] = -1                                                                 # skipped rows: a negative word, H = 0, d = 0
    tab[3, 1] = 0
    tab[4, 3] = 0
    skipped = (1, 3, 4)
    bits = dev(np.concatenate([p.reshape(-1) for p in packed]).view(np.int32))
    total = int(words[-1])
    s = stream_ptr()
    big, out, fill = framed(total, torch.int32)
    tab_t = dev(tab)
    call("mask_boundary", ptr(bits), ptr(tab_t), 0, 40, 65, 0, ptr(out), s)       # N == 0 writes nothing
    call("mask_boundary", None, None, 0, 40, 65, 2, None, s)
    assert bool((big == fill).all())
    call("mask_boundary", ptr(bits), ptr(tab_t), 6, 40, 65, 0, ptr(out), s)
    got = out.cpu().numpy()
    for n in range(6):
        g = got[words[n]:words[n + 1]]
        if n in skipped:
            assert (g == fill).all(), n
        else:
            assert np.array_equal(g.view(np.uint32), pack_bits(bo.boundary(masks[n], 2)).reshape(-1)), n
    assert frames_intact(big, total, fill)

    def code(*args):
        with pytest.raises(Ep24Error) as e:
            call("mask_boundary", *args)
        return "(%d)" % E_ARG in str(e.value), "(%d)" % E_UNSUPPORTED in str(e.value)
    assert code(ptr(bits), ptr(tab_t), 6, 40, 65, 0, ptr(bits), s) == (True, False)             # out == bits
    assert code(None, ptr(tab_t), 6, 40, 65, 0, ptr(out), s) == (True, False)
    assert code(ptr(bits), ptr(tab_t), 6, 40, 65, 0, None, s) == (True, False)
    assert code(ptr(bits), None, 6, 40, 65, 0, ptr(out), s) == (False, True)                    # the uniform form's d
    assert code(ptr(bits), ptr(tab_t), -1, 40, 65, 0, ptr(out), s) == (False, True)
    assert code(ptr(bits), ptr(tab_t), 6, 0, 65, 0, ptr(out), s) == (False, True)
    assert code(ptr(bits), None, 6, 40, 0, 2, ptr(out), s) == (False, True)
    assert frames_intact(big, total, fill)


def test_iou_min_equals_numpy():
    from ep24._lib import call, ptr, stream_ptr
    rng = np.random.RandomState(31)
    n = 1000
    a, b = rng.rand(n), rng.rand(n)
    b[::3] = a[::3]                                                                # equal pairs
    a[5::7] = 0.0
    b[2::11] = 0.0
    a[-1], b[-1] = 1.0, 1.0
    big, iou, fill = framed(n, torch.float64)
    iou.copy_(dev(a))
    other = dev(b)
    call("segm_iou_min", ptr(iou), ptr(other), 0, stream_ptr())                    # n == 0: nothing moves
    assert np.array_equal(iou.cpu().numpy().view(np.int64), a.view(np.int64))
    call("segm_iou_min", ptr(iou), ptr(other), n, stream_ptr())
    assert np.array_equal(iou.cpu().numpy().view(np.int64), np.minimum(a, b).view(np.int64))
    assert np.array_equal(other.cpu().numpy().view(np.int64), b.view(np.int64))
    assert frames_intact(big, n, fill)
    assert (np.minimum(a, b) == a).any() and (np.minimum(a, b) != a).any()


# ------------------------------------------------------------------------------------------------- end to end
@pytest.mark.parametrize("ratio", (0.02, 0.05))
def test_boundary_evaluator_end_to_end(ratio):
    from ep24.segmeval import SegmEvaluator
    gt, res, want_segm, _ = dataset_masks()
    want, _ = boundary_want(ratio)
    assert bo.dilation(427, 640, ratio) == (15 if ratio == 0.02 else 38)
    ev = SegmEvaluator(gt, iou_type="boundary", dilation_ratio=ratio)
    ev.add_results(res)
    st = ev.evaluate()
    assert tables_equal(st, want) and ev.summary == "\n".join(want[1]) + "\n"
    assert st["iou_type"] == "boundary" and st["dilation_ratio"] == ratio and st["chunks"] == 1
    assert st["stats"] != want_segm[0]
    ev3 = SegmEvaluator(gt, chunk_bytes=1, iou_type="boundary", dilation_ratio=ratio)
    ev3.add_results(res)
    st3 = ev3.evaluate()
    assert st3["chunks"] == 3 and tables_equal(st3, want) and ev3.summary == ev.summary


def test_segm_stays_the_default_and_bad_arguments_raise():
    from ep24.segmeval import SegmEvaluator
    gt, res, want = dataset()
    ev = SegmEvaluator(gt)
    ev.add_results(res)
    st = ev.evaluate()
    assert tables_equal(st, want) and ev.summary == "\n".join(want[1]) + "\n"
    assert st["iou_type"] == "segm" and st["dilation_ratio"] == 0.02
    with pytest.raises(ValueError):
        SegmEvaluator(gt, iou_type="bbox")
    for bad in (0.0, -0.02, float("inf"), float("nan")):
        with pytest.raises(ValueError):
            SegmEvaluator(gt, iou_type="boundary", dilation_ratio=bad)


def test_eval_segm_boundary_entry_point(tmp_path):
    gt, res, want_segm = dataset()
    want, _ = boundary_want(0.02)
    (tmp_path / "gt.json").write_text(json.dumps(gt))
    (tmp_path / "dt.json").write_text(json.dumps(res))
    cwd = os.path.join(ROOT, "exploration-of-potential_amd", "yolox_24p")
    base = [sys.executable, "eval_segm.py", "--gt", str(tmp_path / "gt.json"), "--dt", str(tmp_path / "dt.json")]
    out = tmp_path / "boundary.json"
    p = subprocess.run(base + ["--out", str(out), "--iou-type", "boundary"], cwd=cwd, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    lines = [l for l in p.stdout.splitlines() if l.startswith(" Average ")]
    assert lines == want[1] and len(lines) == 12
    got = json.loads(out.read_text())
    assert got["stats"] == want[0] and got["iou_type"] == "boundary" and got["dilation_ratio"] == 0.02
    out2 = tmp_path / "segm.json"
    p = subprocess.run(base + ["--out", str(out2)], cwd=cwd, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    got2 = json.loads(out2.read_text())
    assert sorted(got2) == ["dropped", "images", "max_dets", "per_class_AP", "results", "stats"] and got2["stats"] == want_segm[0]
    assert sorted(got) == sorted(list(got2) + ["iou_type", "dilation_ratio"])


def test_masks_boundary():
    from ep24 import masks as M
    rng = np.random.RandomState(37)
    H, W = 40, 65
    ms = [rng.rand(H, W) < p for p in (0.9, 0.98, 0.999)] + [np.ones((H, W), dtype=bool), np.zeros((H, W), dtype=bool)]
    pm = M.pack(dev(np.stack(ms).astype(np.uint8)))
    for d, want_d in ((3, 3), (None, bo.dilation(H, W, 0.02)), (1000, 65)):
        band = M.boundary(pm, d)
        assert isinstance(band, M.PackedMasks) and band.size == (H, W) and len(band) == len(ms)
        got = band.bits.cpu().numpy().view(np.uint32)
        for n, m in enumerate(ms):
            b = bo.boundary(m, want_d)
            assert np.array_equal(got[n], pack_bits(b)), (d, n)
            box, area = want_stats(b)
            assert band.bbox[n].tolist() == box and int(band.area[n]) == area, (d, n)
    assert bo.dilation(H, W, 0.02) == 2
    wide = M.boundary(pm, dilation_ratio=0.1)                                       # round(0.1 * 76.32) = 8
    assert np.array_equal(wide.bits.cpu().numpy().view(np.uint32)[0], pack_bits(bo.boundary(ms[0], 8)))
    assert M.unpack(M.boundary(pm, 3))[0].cpu().numpy().tolist() == bo.boundary(ms[0], 3).tolist()
