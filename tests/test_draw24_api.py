"""The drawing feature's surface that needs no GPU: the two C ABI entries, ep24.draw's argument checks and show_24p.py's parser."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

from ep24 import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
Y24 = os.path.join(ROOT, "exploration-of-potential_amd", "yolox_24p")
DRAW_SYMBOLS = ["ep24_draw24_prepare", "ep24_draw24_paint"]


def test_draw_symbols_are_declared_and_exported():
    protos = _lib.parse_header()
    cdll = ctypes.CDLL(_lib.LIB_PATH)
    for name in DRAW_SYMBOLS:
        assert name in protos, name
        assert hasattr(cdll, name), name
        assert protos[name][1][-1] == ("void*", "stream"), name                 # raw pointers, sizes and a stream last
    assert _lib.lib().fn["ep24_abi_version"]() == 3                              # additions only: the version stays
    hdr = open(_lib.HEADER_PATH).read()
    from ep24 import draw
    for macro, value in (("EP24_DRAW_REC_WORDS", draw.REC_WORDS), ("EP24_DRAW_MAX_SIDE", draw.MAX_SIDE),
                         ("EP24_DRAW_MAX_FONT_SCALE", draw.MAX_FONT_SCALE)):
        assert "#define %s %d" % (macro, value) in hdr, macro


def test_library_refuses_bad_sizes_without_a_launch():
    """The size checks of the two entry points answer before any pointer is used or anything is launched.  The calls run on a thread
    of their own: the library's last-error text is per thread, and other tests expect this thread's to stay empty."""
    import threading
    fn = _lib.lib().fn
    E_ARG, E_UNSUPPORTED = -1, -3
    prep = lambda n=1, ratio=1.0, conf=0.0, H=8, W=8, C=3, s=2: fn["ep24_draw24_prepare"](None, n, ratio, conf, None, H, W, None, C, None,
                                                                                         None, s, 0, None, None)
    paint = lambda n=1, H=8, W=8, a=0, s=2: fn["ep24_draw24_paint"](None, H, W, None, n, None, a, s, None)
    got = {}

    def calls():
        got["prep_arg"] = [prep(n=-1), prep(C=0), prep(ratio=0.0), prep(ratio=float("inf")), prep(ratio=float("nan")),
                           prep(conf=float("nan")), prep()]                       # the last: null pointers with n > 0
        got["prep_uns"] = [prep(H=0), prep(W=16385), prep(s=0), prep(s=1025)]
        got["prep_ok"] = [prep(n=0), prep(n=0, H=16384, W=16384)]                 # nothing to do: no launch
        got["paint_arg"] = [paint(a=256), paint(a=-1), paint(n=-1), paint()]
        got["paint_uns"] = [paint(H=16385), paint(W=0), paint(s=0)]
        got["paint_ok"] = [paint(n=0)]
        got["text"] = _lib.lib().last_error()
    th = threading.Thread(target=calls)
    th.start()
    th.join()
    assert got["prep_arg"] == [E_ARG] * 7 and got["paint_arg"] == [E_ARG] * 4
    assert got["prep_uns"] == [E_UNSUPPORTED] * 4 and got["paint_uns"] == [E_UNSUPPORTED] * 3
    assert got["prep_ok"] == [0, 0] and got["paint_ok"] == [0]
    assert "draw24" in got["text"]
    assert _lib.lib().last_error() == ""


def test_draw_takes_gpu_tensors_only():
    """CPU tensors are refused with or without a GPU in the machine: there is no CPU path."""
    from ep24 import draw
    assert {"draw_detections", "palette", "label_table", "FONT"} <= set(dir(draw))
    img = torch.zeros(16, 20, 3, dtype=torch.uint8)
    with pytest.raises(_lib.Ep24Error):
        draw.draw_detections(img, torch.zeros(2, 29))
    with pytest.raises(_lib.Ep24Error):
        draw.draw_detections(img, None)
    with pytest.raises(_lib.Ep24Error):
        draw.draw_detections(img, torch.zeros(0, 29), out=torch.zeros(16, 20, 3, dtype=torch.uint8))


def test_draw_checks_arguments_before_the_gpu():
    """Shape and argument errors come first - on CPU tensors they are raised instead of the GPU refusal."""
    from ep24 import draw
    img, det = torch.zeros(16, 20, 3, dtype=torch.uint8), torch.zeros(2, 29)
    for bad in (torch.zeros(16, 20, dtype=torch.uint8), torch.zeros(16, 20, 4, dtype=torch.uint8), torch.zeros(3, 16, 20, dtype=torch.uint8),
                torch.zeros(0, 20, 3, dtype=torch.uint8), np.zeros((16, 20, 3), dtype=np.uint8)):
        with pytest.raises(IndexError):
            draw.draw_detections(bad, det)
    with pytest.raises(ValueError):
        draw.draw_detections(img.float(), det)                                   # wrong image dtype
    for bad in (torch.zeros(2, 26), torch.zeros(29), torch.zeros(1, 2, 29)):
        with pytest.raises(IndexError):
            draw.draw_detections(img, bad)
    with pytest.raises(ValueError):
        draw.draw_detections(img, det.to(torch.int32))                           # wrong detection dtype
    for alpha in (-1, 256, 0.5):
        with pytest.raises(ValueError):
            draw.draw_detections(img, det, fill_alpha=alpha)
    for scale in (0, -2, 1.5, 1025):
        with pytest.raises(ValueError):
            draw.draw_detections(img, det, font_scale=scale)
    for ratio in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            draw.draw_detections(img, det, ratio=ratio)
    with pytest.raises(ValueError):
        draw.draw_detections(img, det, conf=float("nan"))
    with pytest.raises(ValueError):
        draw.draw_detections(img, det, num_classes=0)
    with pytest.raises(ValueError):
        draw.draw_detections(img, det, num_classes=3, class_names=["a", "b"])
    with pytest.raises(IndexError):
        draw.draw_detections(img, det, num_classes=3, colors=torch.zeros(4, 3, dtype=torch.uint8))
    with pytest.raises(ValueError):
        draw.draw_detections(img, det, num_classes=3, colors=torch.zeros(3, 3))
    with pytest.raises(IndexError):
        draw.draw_detections(img, det, out=torch.zeros(16, 21, 3, dtype=torch.uint8))
    with pytest.raises(ValueError):
        draw.draw_detections(img, det, out=torch.zeros(16, 20, 3))
    with pytest.raises(ValueError):
        draw.draw_detections(img, det, out=torch.zeros(16, 3, 20, dtype=torch.uint8).permute(0, 2, 1))      # not contiguous


def _show24p():
    import importlib
    sys.path.insert(0, Y24)
    try:
        return importlib.import_module("show_24p")
    finally:
        sys.path.remove(Y24)


def test_show_24p_parser():
    mod = _show24p()
    a = mod.make_parser().parse_args([])
    # the reference's six flags and their defaults
    assert (a.batch_size, a.start_device, a.devices, a.exp_file, a.load_path, a.weights) == (64, 0, 1, None, None, None)
    # the additions
    assert (a.output_dir, a.conf, a.nms, a.nms_iou, a.draw_conf, a.fill_alpha, a.show_scores, a.class_names, a.device) == \
        (None, 0.01, 0.3, "rect", 1e-4, 0, False, None, "cuda")
    a = mod.make_parser().parse_args(["-f", "e.py", "-p", "dir", "-w", "ck.pth", "-b", "2", "-s", "1", "-d", "1", "--nms-iou", "poly24",
                                      "--conf", "1e-5", "--draw-conf", "0", "--fill-alpha", "96", "--show-scores", "--output-dir", "o",
                                      "--class-names", "n.txt", "--device", "cuda:1", "--nms", "0.5"])
    assert (a.exp_file, a.load_path, a.weights, a.batch_size, a.nms_iou, a.conf, a.draw_conf, a.fill_alpha, a.show_scores) == \
        ("e.py", "dir", "ck.pth", 2, "poly24", 1e-5, 0.0, 96, True)
    for name in ("rect", "poly24"):
        assert mod.make_parser().parse_args(["--nms-iou", name]).nms_iou == name
    with pytest.raises(SystemExit):
        mod.make_parser().parse_args(["--nms-iou", "circle24"])


def test_show_24p_starts_nothing_else():
    """The entry point neither replaces the process's program nor starts other processes."""
    src = open(os.path.join(Y24, "show_24p.py")).read()
    for word in ("os.exec", "subprocess", "os.system", "os.spawn", "multiprocessing", "os.fork", "popen"):
        assert word not in src, word


def test_show_24p_image_files(tmp_path):
    mod = _show24p()
    rng = np.random.default_rng(0)
    img = rng.integers(0, 256, (5, 7, 3), dtype=np.uint8)
    for name in ("a.ppm", "b.npy"):
        mod.write_image(str(tmp_path / name), img)
        assert np.array_equal(mod.read_image(str(tmp_path / name)), img)
    (tmp_path / "c.ppm").write_bytes(b"P6\n# a comment\n7 5\n255\n" + img.tobytes())
    assert np.array_equal(mod.read_image(str(tmp_path / "c.ppm")), img)
    np.save(str(tmp_path / "b.npy.dets.npy"), np.zeros((0, 29), dtype=np.float32))
    (tmp_path / "notes.txt").write_text("x")
    folder, files = mod.list_images(str(tmp_path))
    assert folder == str(tmp_path) and files == ["a.ppm", "b.npy", "c.ppm"]      # results of an earlier run are not inputs
    assert mod.list_images(str(tmp_path / "a.ppm")) == (str(tmp_path), ["a.ppm"])
    with pytest.raises(SystemExit):
        np.save(str(tmp_path / "f.npy"), np.zeros((4, 4), dtype=np.float32))
        mod.read_image(str(tmp_path / "f.npy"))
