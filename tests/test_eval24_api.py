"""The evaluator's surface that needs no GPU: the ep24_eval_* C ABI, ep24.evaluate, Exp.get_evaluator / eval and the
trainer's --eval-interval flag."""
import ctypes
import os
import subprocess
import sys

import pytest
import torch

from ep24 import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
Y24 = os.path.join(ROOT, "exploration-of-potential_amd", "yolox_24p")
EVAL_SYMBOLS = ["ep24_eval_iou", "ep24_eval_match", "ep24_eval_sort", "ep24_eval_accumulate"]


def test_eval_symbols_are_declared_and_exported():
    protos = _lib.parse_header()
    cdll = ctypes.CDLL(_lib.LIB_PATH)
    for name in EVAL_SYMBOLS:
        assert name in protos, name
        assert hasattr(cdll, name), name
    assert _lib.lib().fn["ep24_abi_version"]() == 3


def test_evaluator_imports_and_refuses_to_run_without_gpu():
    from ep24 import evaluate
    ev = evaluate.Evaluator24(80)
    assert (ev.iou_type, ev.max_dets, ev.conf_thre, ev.nms_thre) == ("circle24", 100, 0.01, 0.65)
    with pytest.raises(ValueError):
        evaluate.Evaluator24(80, iou_type="polygon")
    with pytest.raises(_lib.Ep24Error):
        evaluate.Evaluator24(80, max_dets=129)
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    with pytest.raises(_lib.Ep24Error):
        ev.update(torch.zeros(1, 10, 107), torch.zeros(1, 50, 51))
    with pytest.raises(_lib.Ep24Error):
        ev.update_detections([None], torch.zeros(1, 50, 51))
    with pytest.raises(_lib.Ep24Error):
        evaluate.pairwise_iou(torch.zeros(2, 50), torch.zeros(3, 26))


def test_ray_table_is_float64_rounded():
    import numpy as np
    from ep24 import evaluate
    cs = evaluate.ray_cos_sin()
    assert cs.dtype == np.float32 and cs.shape == (48,)
    assert cs[0] == 1.0 and cs[24] == 0.0 and cs[6] == np.float32(np.cos(np.pi / 2))
    assert list(evaluate.IOU_THRS) == list(np.linspace(0.5, 0.95, 10))


def test_exp_has_the_evaluator_factory():
    sys.path.insert(0, Y24)
    try:
        from exp import get_exp
        exp = get_exp(os.path.join(Y24, "load_train", "yolox_24p_train.py"))
        for name in ("get_eval_loader", "get_evaluator", "eval"):
            assert callable(getattr(exp, name, None)), name
        ev = exp.get_evaluator(4)
        assert (ev.conf_thre, ev.nms_thre, ev.num_classes) == (exp.test_conf, exp.nmsthre, exp.num_classes)
        images, rows, _, _ = next(iter(ev.dataloader))
        assert len(images) == 4 and images[0].dtype == torch.uint8 and rows[0].shape[1] == 51
        with pytest.raises(_lib.Ep24Error):
            exp.get_evaluator(4, is_distributed=True)
    finally:
        sys.path.remove(Y24)


def test_eval_interval_defaults_off_and_is_refused_when_distributed(tmp_path):
    sys.path.insert(0, Y24)
    try:
        import importlib
        mod = importlib.import_module("train_24p")
        assert mod.make_parser().parse_args([]).eval_interval == 0
        assert mod.make_parser().parse_args(["--eval-interval", "2"]).eval_interval == 2
    finally:
        sys.path.remove(Y24)
    env = dict(os.environ, WORLD_SIZE="8", RANK="0", LOCAL_RANK="0")
    p = subprocess.run([sys.executable, os.path.join(Y24, "train_24p.py"), "-f", os.path.join(Y24, "load_train", "yolox_24p_train.py"),
                        "-b", "1", "--synthetic", "--steps", "1", "--eval-interval", "1", "--output-dir", str(tmp_path)], cwd=Y24, env=env,
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    assert p.returncode != 0 and "--eval-interval" in p.stdout and "distributed evaluation" in p.stdout, p.stdout[-2000:]
