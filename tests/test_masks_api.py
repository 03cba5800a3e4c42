"""The polygon feature's surface that needs no GPU: the new C ABI entries, the "poly24" IoU type, ep24.masks' input checks and
the trainer's --eval-iou flag."""
import ctypes
import os
import sys

import pytest
import torch

from ep24 import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
Y24 = os.path.join(ROOT, "exploration-of-potential_amd", "yolox_24p")
MASK_SYMBOLS = ["ep24_poly24_vertices", "ep24_poly24_raster", "ep24_mask_pack_u8", "ep24_mask_unpack_u8", "ep24_mask_iou"]


def test_mask_symbols_are_declared_and_exported():
    protos = _lib.parse_header()
    cdll = ctypes.CDLL(_lib.LIB_PATH)
    for name in MASK_SYMBOLS:
        assert name in protos, name
        assert hasattr(cdll, name), name
        assert protos[name][1][-1] == ("void*", "stream"), name                 # raw pointers, sizes and a stream
    assert _lib.lib().fn["ep24_abi_version"]() == 3                              # additions only: the version stays


def test_poly24_is_an_iou_type():
    from ep24 import evaluate
    assert evaluate.IOU_TYPES == {"circle24": 0, "rect": 1, "poly24": 2}
    ev = evaluate.Evaluator24(80, iou_type="poly24")
    assert (ev.iou_type, ev._t, ev.max_dets) == ("poly24", 2, 100)
    with pytest.raises(ValueError):
        evaluate.Evaluator24(80, iou_type="polygon")


def test_exp_passes_the_iou_type_on():
    sys.path.insert(0, Y24)
    try:
        from exp import get_exp
        exp = get_exp(os.path.join(Y24, "load_train", "yolox_24p_train.py"))
        assert exp.eval_iou_type == "circle24"
        exp.eval_iou_type = "poly24"
        assert exp.get_evaluator(4).iou_type == "poly24"
    finally:
        sys.path.remove(Y24)


def test_masks_take_gpu_tensors_only():
    """CPU tensors are refused with or without a GPU in the machine: there is no CPU path."""
    from ep24 import masks
    assert {"PackedMasks", "detection_polygons", "rasterize", "pack", "unpack", "mask_iou", "detections_to_masks"} <= set(dir(masks))
    with pytest.raises(_lib.Ep24Error):
        masks.detection_polygons(torch.zeros(3, 26))
    with pytest.raises(_lib.Ep24Error):
        masks.rasterize(torch.zeros(3, 24, 2), (16, 16))
    with pytest.raises(_lib.Ep24Error):
        masks.pack(torch.zeros(2, 8, 8, dtype=torch.uint8))
    with pytest.raises(_lib.Ep24Error):
        masks.detections_to_masks(torch.zeros(3, 29), 0.5, (16, 16))
    cpu = masks.PackedMasks(torch.zeros(1, 8, 1, dtype=torch.int32), torch.zeros(1, 4, dtype=torch.int32), torch.zeros(1, dtype=torch.int32),
                            (8, 8))
    assert len(cpu) == 1 and cpu.size == (8, 8)
    with pytest.raises(_lib.Ep24Error):
        masks.unpack(cpu)
    with pytest.raises(_lib.Ep24Error):
        masks.mask_iou(cpu, cpu)
    with pytest.raises(IndexError):
        masks.unpack("not masks")


def test_eval_iou_flag():
    sys.path.insert(0, Y24)
    try:
        import importlib
        mod = importlib.import_module("train_24p")
        assert mod.make_parser().parse_args([]).eval_iou is None
        for name in ("circle24", "rect", "poly24"):
            assert mod.make_parser().parse_args(["--eval-iou", name]).eval_iou == name
        with pytest.raises(SystemExit):
            mod.make_parser().parse_args(["--eval-iou", "polygon"])
    finally:
        sys.path.remove(Y24)
