"""The mask kernels (csrc/mask.hip, ep24.masks) against the numpy oracle (tests/poly24_oracle.py): the rasteriser bit for bit,
packing round trips, mask IoU in integers, and the two polygon geometries (area IoU, raster IoU) against each other."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import poly24_oracle as P  # noqa: E402
from ep24 import evaluate as E, masks as M  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SIZES = [(40, 1), (40, 31), (40, 32), (40, 33), (37, 65)]


def _u32(t):
    return t.cpu().numpy().view(np.uint32)


def _polygons():
    """12 polygons: stars, integer vertices (rows pass exactly through a vertex), horizontal edges, partly and wholly outside
    the canvas (negative coordinates, beyond W and H), zero radius, one that covers everything, a clockwise one."""
    rng = np.random.default_rng(3)
    th = np.arange(24) * (np.pi / 12)
    cases = [
        P.regular(16.0, 20.0, rng.uniform(3.0, 15.0, 24)),
        P.regular(33.25, 17.5, rng.uniform(2.0, 30.0, 24)),
        np.stack([np.round(16 + 11 * np.cos(th)), np.round(19 + 13 * np.sin(th))], -1),      # integer vertices
        P.square64(12.0, 18.0, 7.0),                                             # horizontal edges on the rows 11 and 25
        P.regular(-3.0, 5.0, 9.0),                                               # partly left / above
        P.regular(30.0, 38.0, 12.5),                                             # partly right / below
        P.regular(-40.0, -40.0, 6.0),                                            # wholly outside
        P.regular(200.0, 20.0, 10.0),
        P.regular(10.0, 10.0, 0.0),                                              # zero radius
        P.regular(10.5, 10.5, 0.25),                                             # between pixel centres: empty
        P.regular(20.0, 20.0, 500.0),                                            # covers the canvas
        P.regular(40.0, 12.0, rng.uniform(3.0, 20.0, 24))[::-1],                 # clockwise
    ]
    return np.ascontiguousarray(np.stack(cases).astype(np.float32))


@pytest.mark.parametrize("H,W", SIZES)
def test_raster_bit_exact_against_the_oracle(H, W):
    polys = _polygons()
    N = len(polys)
    assert N == 12
    out = M.PackedMasks(torch.full((N, H, (W + 31) // 32), -1, dtype=torch.int32, device=DEV),
                        torch.full((N, 4), -1, dtype=torch.int32, device=DEV), torch.full((N,), -1, dtype=torch.int32, device=DEV), (H, W))
    pm = M.rasterize(torch.from_numpy(polys).to(DEV), (H, W), out=out)
    assert pm is out and pm.size == (H, W)
    words, bbox, area = P.rasterize(polys, H, W)
    got = _u32(pm.bits)
    assert got.shape == words.shape
    if W % 32:
        assert not (got[..., -1] >> np.uint32(W % 32)).any()                     # bits at x >= W are zero
    assert np.array_equal(got, words)
    assert np.array_equal(pm.bbox.cpu().numpy(), bbox) and np.array_equal(pm.area.cpu().numpy(), area)
    assert area[6] == area[7] == area[8] == area[9] == 0 and area[10] == H * W and (W < 8 or area[0] > 0)
    # a fresh allocation gives the same, and so does the per-pixel statement of the rule
    again = M.rasterize(torch.from_numpy(polys).to(DEV), (H, W))
    assert torch.equal(again.bits, pm.bits) and torch.equal(again.bbox, pm.bbox) and torch.equal(again.area, pm.area)
    pix = np.stack([P.raster_pixels(p, H, W) for p in polys])
    assert np.array_equal(M.unpack(pm).cpu().numpy(), pix)


def test_raster_of_no_polygons():
    pm = M.rasterize(torch.zeros(0, 24, 2, device=DEV), (40, 33))
    assert tuple(pm.bits.shape) == (0, 40, 2) and tuple(pm.bbox.shape) == (0, 4) and tuple(pm.area.shape) == (0,) and len(pm) == 0
    assert tuple(M.unpack(pm).shape) == (0, 40, 33)


@pytest.mark.parametrize("H,W", SIZES)
def test_pack_unpack_round_trip(H, W):
    rng = np.random.default_rng(H * 100 + W)
    m = (rng.random((6, H, W)) < 0.3).astype(np.uint8) * rng.integers(1, 256, (6, H, W)).astype(np.uint8)
    m[4] = 0                                                                     # an empty mask
    m[5] = 255
    pm = M.pack(torch.from_numpy(m).to(DEV))
    bbox, area = P.boxes_areas(m)
    assert np.array_equal(_u32(pm.bits), P.pack_bits(m))
    assert np.array_equal(pm.bbox.cpu().numpy(), bbox) and np.array_equal(pm.area.cpu().numpy(), area)
    back = M.unpack(pm)
    assert back.dtype == torch.bool and np.array_equal(back.cpu().numpy(), m != 0)
    pb = M.pack(torch.from_numpy(m != 0).to(DEV))                                # bool input
    assert torch.equal(pb.bits, pm.bits)


def test_mask_iou_against_integer_counts():
    H, W = 37, 65
    rng = np.random.default_rng(9)
    a = np.zeros((5, H, W), bool)
    b = np.zeros((7, H, W), bool)
    a[0, 3:20, 5:40] = rng.random((17, 35)) < 0.7
    a[1, 10:30, 30:65] = True
    a[2] = rng.random((H, W)) < 0.5
    a[3, 0:5, 0:5] = True                                                        # box disjoint from most of b
    b[0] = a[0]                                                                  # identical
    b[1, 12:37, 0:33] = True
    b[2] = rng.random((H, W)) < 0.5
    b[3, 30:37, 50:65] = True
    b[4, 0, 0] = True                                                            # one pixel
    b[5, 20:30, 31:33] = True                                                    # straddles a word boundary
    # a[4] and b[6] stay empty
    pa, pb = M.pack(torch.from_numpy(a).to(DEV)), M.pack(torch.from_numpy(b).to(DEV))
    inter, iou = M.mask_iou(pa, pb)
    wi, wu = P.mask_iou(a, b)
    assert inter.dtype == torch.int64 and iou.dtype == torch.float64
    assert np.array_equal(inter.cpu().numpy(), wi)
    assert np.array_equal(iou.cpu().numpy().view(np.uint64), wu.view(np.uint64))
    assert wu[0, 0] == 1.0 and wi[3, 3] == 0 and wu[4, 6] == 0.0 and wi[1, 5] == 20
    e = M.pack(torch.zeros(0, H, W, dtype=torch.uint8, device=DEV))
    i0, u0 = M.mask_iou(e, pb)
    assert tuple(i0.shape) == (0, 7) and tuple(u0.shape) == (0, 7)
    i1, u1 = M.mask_iou(pa, e)
    assert tuple(i1.shape) == (5, 0) and tuple(u1.shape) == (5, 0)
    with pytest.raises(IndexError):
        M.mask_iou(pa, M.pack(torch.zeros(1, H, W + 1, dtype=torch.uint8, device=DEV)))


def test_area_iou_and_raster_iou_agree():
    """The 40 generator pairs: polygon IoU of the pairs as they are against the mask IoU of their vertices scaled by 16 on a
    1024 x 1024 canvas.  1e-3 is the raster's discretisation at 16 x (tests/test_poly24_oracle.py measures 2e-4 for the oracle)."""
    rows = P.generator_pairs()
    a, b = torch.from_numpy(rows[:, 0].copy()).to(DEV), torch.from_numpy(rows[:, 1].copy()).to(DEV)
    va, vb = M.detection_polygons(a), M.detection_polygons(b)
    assert np.array_equal(va.cpu().numpy(), P.det_polygons(rows[:, 0])) and np.array_equal(vb.cpu().numpy(), P.det_polygons(rows[:, 1]))
    gt50 = torch.cat([a[:, :2], va.reshape(-1, 48)], 1)                          # polygon A as a GT row: centre + vertices
    exact = E.pairwise_iou(gt50, b, "poly24").diagonal().cpu().numpy()
    ma, mb = M.rasterize(va * 16.0, (1024, 1024)), M.rasterize(vb * 16.0, (1024, 1024))
    _, iou = M.mask_iou(ma, mb)
    got = iou.diagonal().cpu().numpy()
    worst = float(np.abs(got - exact).max())
    print("mask IoU at 16x vs poly24: worst |diff| = %.3e" % worst)
    assert worst <= 1e-3
    assert float(exact.max()) > 0.4 and float(exact.min()) < 0.1                 # the pairs span small and large overlaps


def test_detections_to_masks():
    rng = np.random.default_rng(4)
    n, ratio, hw = 9, 0.5, (97, 130)
    det = np.zeros((n, 29), np.float32)
    det[:, 0] = rng.uniform(-5.0, 70.0, n)                                       # letterboxed coordinates: the image is 65 x 48.5 there
    det[:, 1] = rng.uniform(-5.0, 55.0, n)
    det[:, 2:26] = rng.uniform(1.0, 14.0, (n, 24))
    det[:, 26:] = rng.random((n, 3))
    pm = M.detections_to_masks(torch.from_numpy(det).to(DEV), ratio, hw)
    polys = P.det_polygons(det, ratio=ratio)
    words, bbox, area = P.rasterize(polys, *hw)
    assert pm.size == hw and np.array_equal(_u32(pm.bits), words)
    assert np.array_equal(pm.bbox.cpu().numpy(), bbox) and np.array_equal(pm.area.cpu().numpy(), area) and area.max() > 100
    p26 = M.detections_to_masks(torch.from_numpy(det[:, :26].copy()).to(DEV), ratio, hw)
    assert torch.equal(p26.bits, pm.bits)
    for empty in (None, torch.zeros(0, 29, device=DEV)):
        e = M.detections_to_masks(empty, ratio, hw)
        assert isinstance(e, M.PackedMasks) and len(e) == 0 and e.size == hw and tuple(e.bits.shape) == (0, 97, 5)
        assert e.bits.is_cuda and tuple(e.bbox.shape) == (0, 4) and tuple(e.area.shape) == (0,)


def test_shape_errors():
    with pytest.raises(IndexError):
        M.rasterize(torch.zeros(3, 24, 3, device=DEV), (8, 8))
    with pytest.raises(IndexError):
        M.detection_polygons(torch.zeros(3, 27, device=DEV))
    with pytest.raises(IndexError):
        M.pack(torch.zeros(3, 8, 8, device=DEV))                                 # fp32 masks
    with pytest.raises(M.Ep24Error):
        M.rasterize(torch.zeros(1, 24, 2, device=DEV), (0, 8))
