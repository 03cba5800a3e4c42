"""Multiscale training without a GPU: the numpy restatement of the resize rule (tests/resize_oracle.py) against the float64
formula and against the reference's ``Exp.preprocess`` (``F.interpolate`` on CPU tensors), ``ep24.multiscale.size_for``, the two
new C ABI entries and the trainer's refusals."""
import ctypes
import os
import random
import sys
import types

import numpy as np
import pytest
import torch

import resize_oracle as ro
from ep24 import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
Y24 = os.path.join(ROOT, "exploration-of-potential_amd", "yolox_24p")
SYMBOLS = ["ep24_resize_bilinear_f32", "ep24_scale_labels"]


def integer_planes(shape, seed):
    return np.random.default_rng(seed).integers(0, 256, (2, 3) + tuple(shape)).astype(np.float32)


def make_exp(input_size=(128, 128), multiscale_range=1):
    sys.path.insert(0, Y24)
    try:
        from exp import get_exp
        exp = get_exp(os.path.join(Y24, "load_train", "yolox_24p_train.py"))
    finally:
        sys.path.remove(Y24)
    exp.input_size, exp.multiscale_range = input_size, multiscale_range
    return exp


@pytest.mark.parametrize("src,dst", ro.SHAPES)
def test_oracle_matches_the_float64_formula(src, dst):
    """Nine float32 roundings of at most 2^-17 each on 0..255 data (four products, two sums per row pair, two products and the final
    sum: each result is below 256, half an ulp is 2^-17 = 7.6e-6) plus the two weight roundings (2^-25 * 255 each): <= 1e-4."""
    x = integer_planes(src, 1)
    got = ro.resize(x, *dst)
    assert got.shape == (2, 3) + tuple(dst) and got.dtype == np.float32
    err = float(np.abs(got.astype(np.float64) - ro.resize_f64(x, *dst)).max())
    print("oracle vs float64", src, dst, err)
    assert err <= 1e-4
    if src == dst:
        assert np.array_equal(got, x)


@pytest.mark.parametrize("src,dst", ro.SHAPES)
def test_oracle_matches_the_reference_preprocess_images(src, dst):
    """``Exp.preprocess`` on CPU tensors is the reference's ``F.interpolate``; ATen computes the coordinates in float32, so a few
    ulps of a coordinate (8 * 2^-24 * the larger source side) times the data range 255 are allowed."""
    exp = make_exp(input_size=src)
    x = integer_planes(src, 2)
    labels = torch.zeros(2, 4, 51)
    want, _ = exp.preprocess(torch.from_numpy(x.copy()), labels, dst)
    got = ro.resize(x, *dst)
    bound = 255 * 8 * 2.0 ** -24 * max(src)
    err = float(np.abs(got - want.numpy()).max())
    print("oracle vs F.interpolate", src, dst, err, "bound", bound)
    assert tuple(want.shape) == (2, 3) + tuple(dst)
    assert err <= bound


@pytest.mark.parametrize("input_size,tsize", [((128, 128), (96, 96)), ((128, 128), (160, 160)), ((96, 160), (64, 128))])
def test_oracle_matches_the_reference_preprocess_labels(input_size, tsize):
    exp = make_exp(input_size=input_size)
    rng = np.random.default_rng(3)
    lab = rng.uniform(0.0, 160.0, (2, 50, 51)).astype(np.float32)
    lab[:, :, 0] = rng.integers(0, 80, (2, 50))
    lab[:, 7:] = 0.0                                                            # padding rows
    x = torch.zeros(2, 3, *input_size)
    _, want = exp.preprocess(x, torch.from_numpy(lab.copy()), tsize)
    got = ro.scale_labels(lab, tsize[1] / input_size[1], tsize[0] / input_size[0])
    assert np.array_equal(got, want.numpy())
    assert np.array_equal(got[..., 0], lab[..., 0]) and not np.array_equal(got[:, :7, 1:], lab[:, :7, 1:])


def test_preprocess_identity_returns_its_arguments():
    exp = make_exp()
    x, lab = torch.zeros(1, 3, 128, 128), torch.zeros(1, 50, 51)
    a, b = exp.preprocess(x, lab, (128, 128))
    assert a is x and b is lab
    a, b = exp.preprocess(x, lab, (128, 128), out=None)
    assert a is x and b is lab


def test_size_for_follows_from_seed_and_draw_alone():
    from ep24.multiscale import size_for
    exp = make_exp(input_size=(640, 640), multiscale_range=5)
    first = [size_for(exp, 7, k) for k in range(50)]
    random.seed(123)                                                            # the module-level generator plays no part
    again = [size_for(make_exp(input_size=(640, 640), multiscale_range=5), 7, k) for k in reversed(range(50))][::-1]
    assert first == again
    assert [size_for(exp, 8, k) for k in range(50)] != first
    assert len(set(first)) > 1
    lo, hi = 32 * (640 // 32 - 5), 32 * (640 // 32 + 5)
    for h, w in first:
        assert h % 32 == 0 and w % 32 == 0 and lo <= h <= hi and h == w


def test_size_for_keeps_the_aspect_of_a_rectangular_input():
    from ep24.multiscale import size_for
    exp = make_exp(input_size=(320, 640), multiscale_range=3)
    sizes = [size_for(exp, 0, k) for k in range(50)]
    assert len(set(sizes)) > 1
    for h, w in sizes:
        assert h % 32 == 0 and w == 2 * h and 32 * (10 - 3) <= h <= 32 * (10 + 3)


def test_random_resize_without_rng_draws_from_the_module_generator():
    exp = make_exp(input_size=(640, 640), multiscale_range=5)
    random.seed(5)
    a = [exp.random_resize() for _ in range(20)]
    random.seed(5)
    b = [exp.random_resize(None, None) for _ in range(20)]
    random.seed(5)
    want = [(32 * s, 32 * s) for s in (random.randint(15, 25) for _ in range(20))]
    assert a == b == want and len(set(a)) > 1


def test_multiscale_symbols_are_declared_and_exported():
    protos = _lib.parse_header()
    cdll = ctypes.CDLL(_lib.LIB_PATH)
    for name in SYMBOLS:
        assert name in protos, name
        assert hasattr(cdll, name), name
        assert protos[name][1][-1] == ("void*", "stream"), name
    assert [t for t, _ in protos["ep24_resize_bilinear_f32"][1]] == ["const float*", "int", "int", "int", "float*", "int", "int", "void*"]
    assert [t for t, _ in protos["ep24_scale_labels"][1]] == ["const float*", "float*", "int64_t", "float", "float", "void*"]
    assert _lib.lib().fn["ep24_abi_version"]() == 3                              # additions only: the version stays


def test_entry_points_refuse_bad_arguments():
    """Null pointers and non-positive sizes are refused before anything is launched (no GPU needed to see it).  The calls run on a
    thread of their own: the library's last-error text is per thread, and other tests expect this thread's to stay empty."""
    import threading
    L = _lib.lib()
    resize, scale = L.fn["ep24_resize_bilinear_f32"], L.fn["ep24_scale_labels"]
    one = ctypes.c_void_p(16)                                                   # any non-null address: nothing is dereferenced
    got = {}

    def calls():
        got["null"] = [resize(None, 3, 8, 8, one, 8, 8, None)]
        got["null_text"] = L.last_error()
        got["null"].append(resize(one, 3, 8, 8, None, 8, 8, None))
        got["sizes"] = [resize(one, n, sh, sw, one, dh, dw, None) for n, sh, sw, dh, dw in
                        ((0, 8, 8, 8, 8), (-1, 8, 8, 8, 8), (3, 0, 8, 8, 8), (3, 8, -1, 8, 8), (3, 8, 8, 0, 8), (3, 8, 8, 8, 0))]
        got["plane"] = [resize(one, 3, 65536, 65536, one, 8, 8, None), resize(one, 3, 8, 8, one, 65536, 65536, None)]
        got["plane_text"] = L.last_error()
        got["labels"] = [scale(None, one, 4, 1.0, 1.0, None), scale(one, None, 4, 1.0, 1.0, None), scale(one, one, 0, 1.0, 1.0, None),
                         scale(one, one, -3, 1.0, 1.0, None), scale(one, one, 1 << 41, 1.0, 1.0, None)]
        got["labels_text"] = L.last_error()
    th = threading.Thread(target=calls)
    th.start()
    th.join()
    for key in ("null", "sizes", "plane", "labels"):
        assert all(rc != 0 for rc in got[key]), (key, got[key])
    assert "resize_bilinear_f32" in got["null_text"] and "31-bit" in got["plane_text"] and "scale_labels" in got["labels_text"]
    assert L.last_error() == ""


def test_resize_batch_takes_gpu_tensors_only():
    from ep24 import multiscale
    with pytest.raises(_lib.Ep24Error):
        multiscale.resize_batch(torch.zeros(2, 3, 64, 64), torch.zeros(2, 50, 51), (32, 32))
    with pytest.raises(IndexError):
        multiscale.resize_batch(torch.zeros(2, 1, 64, 64), torch.zeros(2, 50, 51), (32, 32))
    with pytest.raises(IndexError):
        multiscale.resize_batch(torch.zeros(2, 3, 64, 64), torch.zeros(2, 50, 50), (32, 32))
    with pytest.raises(IndexError):
        multiscale.resize_batch(torch.zeros(2, 3, 64, 64), torch.zeros(3, 50, 51), (32, 32))


def test_trainer_refuses_what_multiscale_cannot_do():
    sys.path.insert(0, Y24)
    try:
        import importlib
        mod = importlib.import_module("train_24p")
    finally:
        sys.path.remove(Y24)
    parse = mod.make_parser().parse_args
    d = parse([])
    assert (d.multiscale, d.multiscale_interval, d.multiscale_seed, d.multiscale_plans) == (False, 10, 0, 0)
    a = parse(["--multiscale", "--multiscale-interval", "2", "--multiscale-seed", "9", "--multiscale-plans", "3"])
    assert (a.multiscale, a.multiscale_interval, a.multiscale_seed, a.multiscale_plans) == (True, 2, 9, 3)
    exp = make_exp()
    mod.check_multiscale_args(a, exp, 1)                                        # fine
    mod.check_multiscale_args(parse(["--no-graph"]), exp, 8)                    # without the flag nothing is checked
    with pytest.raises(SystemExit, match="no-graph"):
        mod.check_multiscale_args(parse(["--multiscale", "--no-graph"]), exp, 1)
    with pytest.raises(SystemExit, match="out of scope"):
        mod.check_multiscale_args(parse(["--multiscale"]), exp, 2)
    flat = types.SimpleNamespace(multiscale_range=0, input_size=(128, 128))
    with pytest.raises(SystemExit, match="multiscale_range"):
        mod.check_multiscale_args(parse(["--multiscale"]), flat, 1)
    flat.random_size = (3, 5)                                                   # an explicit range stands in for multiscale_range
    mod.check_multiscale_args(parse(["--multiscale"]), flat, 1)
