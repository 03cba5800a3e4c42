"""The feature-map study's surface that needs no GPU: the four C ABI entries, ep24.featmap's argument checks (all raised before the
GPU is touched), the colour ramp, the host half of the study and demo_featuremap.py's parser."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

from ep24 import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
Y24 = os.path.join(ROOT, "exploration-of-potential_amd", "yolox_24p")
SYMBOLS = ["ep24_featmap_mean_bf16", "ep24_featmap_range", "ep24_featmap_render", "ep24_featmap_response"]
BF = torch.bfloat16


def test_featmap_symbols_are_declared_and_exported():
    protos = _lib.parse_header()
    cdll = ctypes.CDLL(_lib.LIB_PATH)
    for name in SYMBOLS:
        assert name in protos, name
        assert hasattr(cdll, name), name
        assert protos[name][1][-1] == ("void*", "stream"), name
    assert [t for t, _ in protos["ep24_featmap_mean_bf16"][1]] == ["const void*", "int64_t", "int64_t", "int", "float*", "void*"]
    assert len(protos["ep24_featmap_render"][1]) == 11 and len(protos["ep24_featmap_response"][1]) == 12
    assert _lib.lib().fn["ep24_abi_version"]() == 3                              # additions only: the version stays
    hdr = open(_lib.HEADER_PATH).read()
    from ep24 import featmap
    assert "E4  feature-map response" in hdr
    assert "#define EP24_FEATMAP_MAX_SCALE %d" % featmap.MAX_SCALE in hdr
    assert "#define EP24_DRAW_MAX_SIDE %d" % featmap.MAX_SIDE in hdr


def test_library_refuses_bad_arguments_without_a_launch():
    """Every refusal of the four entry points answers before a pointer is used or anything is launched (null pointers throughout).
    On a thread of its own: the library's last-error text is per thread."""
    import threading
    fn = _lib.lib().fn
    E_ARG, E_UNS = -1, -3
    mean = lambda x=None, ld=8, M=1, C=8: fn["ep24_featmap_mean_bf16"](x, ld, M, C, None, None)
    rng = lambda N=1, cells=4: fn["ep24_featmap_range"](None, N, cells, None, None)
    ren = lambda N=1, H=2, W=2, s=1, a=128: fn["ep24_featmap_render"](None, N, H, W, s, None, None, None, a, None, None)
    res = lambda B=1, H=4, W=4, st=8, L=1, mode=0: fn["ep24_featmap_response"](None, B, H, W, st, None, L, mode, None, None, None, None)
    got = {}

    def calls():
        got["mean_arg"] = [mean(M=-1), mean()]                                   # the last: null pointers with M > 0
        got["mean_uns"] = [mean(C=0), mean(C=4), mean(C=12, ld=16), mean(C=16, ld=8), mean(C=8, ld=12), mean(x=8), mean(x=2, M=0)]
        got["mean_ok"] = [mean(M=0), mean(M=0, C=1024, ld=2048)]
        got["rng_arg"] = [rng(N=-1), rng(cells=-1), rng()]
        got["rng_ok"] = [rng(N=0)]
        got["ren_arg"] = [ren(N=-1), ren(a=-1), ren(a=256), ren()]
        got["ren_uns"] = [ren(s=0), ren(s=65), ren(H=0), ren(W=0), ren(H=257, s=64), ren(W=16385)]
        got["ren_ok"] = [ren(N=0), ren(N=0, H=256, W=256, s=64)]
        got["res_arg"] = [res(B=-1), res(L=-1), res(st=0), res(mode=2), res(mode=-1), res()]
        got["res_uns"] = [res(H=0), res(W=16385)]
        got["res_ok"] = [res(B=0), res(L=0)]
        got["text"] = _lib.lib().last_error()
    th = threading.Thread(target=calls)
    th.start()
    th.join()
    for key, val in got.items():
        if key.endswith("_arg"):
            assert val == [E_ARG] * len(val), (key, val)
        elif key.endswith("_uns"):
            assert val == [E_UNS] * len(val), (key, val)
        elif key.endswith("_ok"):
            assert val == [0] * len(val), (key, val)
    assert "featmap" in got["text"]
    assert _lib.lib().last_error() == ""


def test_colormap_has_256_distinct_rows():
    from ep24 import featmap
    c = featmap.colormap()
    assert c.dtype == torch.uint8 and tuple(c.shape) == (256, 3)
    assert len({tuple(r) for r in c.tolist()}) == 256
    assert c[0].tolist() == [0, 0, 0] and c[255].tolist() == [255, 255, 255]
    assert torch.equal(c, featmap.colormap())


def test_featmap_takes_gpu_tensors_only():
    """Well-formed CPU tensors are refused with or without a GPU in the machine: there is no CPU path."""
    from ep24 import featmap
    maps, labels = torch.zeros(2, 4, 4), torch.zeros(2, 3, 51)
    with pytest.raises(_lib.Ep24Error):
        featmap.channel_mean(torch.zeros(2, 4, 4, 16, dtype=BF))
    with pytest.raises(_lib.Ep24Error):
        featmap.value_range(maps)
    with pytest.raises(_lib.Ep24Error):
        featmap.render(maps, 4)
    with pytest.raises(_lib.Ep24Error):
        featmap.response([maps], labels, strides=(8,))


def test_channel_mean_checks_arguments_before_the_gpu():
    from ep24 import featmap
    dense = torch.zeros(2, 4, 4, 32, dtype=BF)
    for bad in (torch.zeros(4, 4, 16, dtype=BF), np.zeros((2, 4, 4, 16)), None):
        with pytest.raises(IndexError):
            featmap.channel_mean(bad)
    with pytest.raises(ValueError):
        featmap.channel_mean(torch.zeros(2, 4, 4, 16))                           # fp32
    for bad in (torch.zeros(2, 4, 4, 12, dtype=BF),                              # C no multiple of 8
                dense[..., 4:20],                                                # a slice that starts inside a 16-byte chunk
                torch.zeros(2, 4, 4, 20, dtype=BF)[..., :16],                    # row stride no multiple of 8
                dense.permute(0, 2, 1, 3),                                       # not NHWC-dense
                dense[:, ::2],                                                   # rows skipped
                torch.zeros(2, 16, 4, 4, dtype=BF).permute(0, 2, 3, 1)):         # an NCHW tensor viewed as NHWC
        with pytest.raises(ValueError):
            featmap.channel_mean(bad)
    good = dense[..., 8:24]
    with pytest.raises(IndexError):
        featmap.channel_mean(good, out=torch.zeros(2, 4, 5))
    with pytest.raises(ValueError):
        featmap.channel_mean(good, out=torch.zeros(2, 4, 4, dtype=torch.float64))
    with pytest.raises(_lib.Ep24Error):
        featmap.channel_mean(good)                                               # well-formed, but on the CPU


def test_render_checks_arguments_before_the_gpu():
    from ep24 import featmap
    maps = torch.zeros(2, 4, 5)
    for bad in (torch.zeros(4, 5), torch.zeros(1, 2, 4, 5), np.zeros((2, 4, 5), np.float32)):
        with pytest.raises(IndexError):
            featmap.render(bad, 2)
        with pytest.raises(IndexError):
            featmap.value_range(bad)
    with pytest.raises(ValueError):
        featmap.render(maps.double(), 2)
    with pytest.raises(ValueError):
        featmap.value_range(maps.double())
    with pytest.raises(ValueError):
        featmap.render(torch.zeros(2, 5, 4).permute(0, 2, 1), 2)                 # not contiguous
    for scale in (0, 65, 1.5, True):
        with pytest.raises(ValueError):
            featmap.render(maps, scale)
    for alpha in (-1, 256, 0.5):
        with pytest.raises(ValueError):
            featmap.render(maps, 2, alpha=alpha)
    with pytest.raises(IndexError):
        featmap.render(torch.zeros(1, 300, 4), 64)                               # 19 200 rows
    for kw in ({"vmin": float("nan")}, {"vmax": float("inf")}):
        with pytest.raises(ValueError):
            featmap.render(maps, 2, **kw)
    with pytest.raises(IndexError):
        featmap.render(maps, 2, base=torch.zeros(2, 3, 8, 11))
    with pytest.raises(ValueError):
        featmap.render(maps, 2, base=torch.zeros(2, 3, 8, 10, dtype=torch.float64))
    with pytest.raises(IndexError):
        featmap.render(maps, 2, lut=torch.zeros(255, 3, dtype=torch.uint8))
    with pytest.raises(ValueError):
        featmap.render(maps, 2, lut=torch.zeros(256, 3))
    with pytest.raises(IndexError):
        featmap.render(maps, 2, out=torch.zeros(2, 8, 10, 4, dtype=torch.uint8))
    with pytest.raises(ValueError):
        featmap.render(maps, 2, out=torch.zeros(2, 8, 10, 3))


def test_response_checks_arguments_before_the_gpu():
    from ep24 import featmap
    maps, labels = [torch.zeros(2, 4, 4), torch.zeros(2, 2, 2)], torch.zeros(2, 3, 51)
    with pytest.raises(ValueError):
        featmap.response(maps, labels, strides=(8, 16), region="circle24")
    with pytest.raises(IndexError):
        featmap.response(maps, labels, strides=(8, 16, 32))
    with pytest.raises(IndexError):
        featmap.response([], labels, strides=())
    for st in ((8, 0), (8, 1.5), (-8, 16)):
        with pytest.raises(ValueError):
            featmap.response(maps, labels, strides=st)
    for bad in (torch.zeros(2, 3, 50), torch.zeros(3, 51), np.zeros((2, 3, 51), np.float32)):
        with pytest.raises(IndexError):
            featmap.response(maps, bad, strides=(8, 16))
    with pytest.raises(ValueError):
        featmap.response(maps, labels.double(), strides=(8, 16))
    with pytest.raises(IndexError):
        featmap.response([torch.zeros(3, 4, 4), maps[1]], labels, strides=(8, 16))       # another batch size
    with pytest.raises(IndexError):
        featmap.response([torch.zeros(2, 4), maps[1]], labels, strides=(8, 16))
    with pytest.raises(ValueError):
        featmap.response([maps[0].double(), maps[1]], labels, strides=(8, 16))


def test_return_fpn_is_an_eval_mode_option():
    from ep24 import nn as enn
    m = enn.YOLOX(enn.YOLOPAFPN(0.33, 0.125), enn.YOLOXHead(80, 0.125))
    with pytest.raises(ValueError):
        m(torch.zeros(1, 3, 64, 64), train=True, return_fpn=True)               # before the GPU is asked for


def test_shifted_inputs():
    """The host half of the study: shift onto a 114 canvas, labels move along, a centre outside the image drops its row, isolate."""
    from ep24 import featmap
    h, w = 40, 32
    rng = np.random.default_rng(0)
    img = rng.integers(0, 114, (h, w, 3), dtype=np.uint8)                        # never 114 itself
    a = np.arange(24) * (15.0 * np.pi / 180.0)
    row = np.zeros((1, 51))
    row[0, 0], row[0, 1], row[0, 2] = 3, 16 / w, 12 / h
    row[0, 3::2], row[0, 4::2] = (16 + 6 * np.cos(a)) / w, (12 + 6 * np.sin(a)) / h
    images, targets = featmap.shifted_inputs(img, row, (-20, -5, 0, 7, 30), isolate=False)
    assert np.array_equal(images[2], img) and np.array_equal(targets[2], row)
    assert np.array_equal(images[3][7:], img[:h - 7]) and (images[3][:7] == 114).all()
    assert np.array_equal(images[1][:h - 5], img[5:]) and (images[1][h - 5:] == 114).all()
    assert np.allclose(targets[3][0, 2::2], row[0, 2::2] + 7 / h) and np.array_equal(targets[3][0, 1::2], row[0, 1::2])
    assert [len(t) for t in targets] == [0, 1, 1, 1, 0]                          # centre rows 12 - 20 and 12 + 30 leave the image
    iso, _ = featmap.shifted_inputs(img, row, (0,), isolate=True)
    kept = (iso[0] != 114).any(axis=2)
    yy, xx = np.mgrid[0:h, 0:w]
    assert kept[12, 16] and not kept[0, 0]
    assert kept[(xx - 16) ** 2 + (yy - 12) ** 2 <= 25].all() and not kept[(xx - 16) ** 2 + (yy - 12) ** 2 >= 49].any()
    assert np.array_equal(iso[0][kept], img[kept])
    with pytest.raises(IndexError):
        featmap.shifted_inputs(img[:, :, 0], row, (0,))
    with pytest.raises(ValueError):
        featmap.shifted_inputs(img, np.full((1, 51), np.nan), (0,))


def test_study_checks_arguments_before_the_gpu():
    from ep24 import featmap
    img, row = np.zeros((32, 32, 3), np.uint8), np.zeros((0, 51))
    with pytest.raises(IndexError):
        featmap.study(None, img, row, 100)
    with pytest.raises(ValueError):
        featmap.study(None, img, row, 64, thetas=(10,))
    with pytest.raises(ValueError):
        featmap.study(None, img, row, 64, offsets=())


def _demo():
    import importlib
    sys.path.insert(0, Y24)
    try:
        return importlib.import_module("demo_featuremap")
    finally:
        sys.path.remove(Y24)


def test_demo_featuremap_parser():
    mod = _demo()
    a = mod.make_parser().parse_args([])
    # the reference's flags and their defaults (yolox/demo_featuremap.py:46-61)
    assert (a.backbone, a.vis, a.ckpt, a.conf, a.nms, a.tsize, a.exp_file) == (None, False, None, 0.25, 0.45, 640, None)
    assert (a.path, a.labels, a.synthetic, a.offsets, a.thetas, a.region, a.output_dir, a.device) == \
        (None, None, False, [-100, -50, 0, 50, 100], list(range(30, 95, 5)), "rect", None, "cuda")
    a = mod.make_parser().parse_args(["--backbone", "resnet", "-c", "ck.pth", "-f", "e.py", "--tsize", "320", "--conf", "0.1", "--nms", "0.5",
                                      "--vis", "-p", "o.npy", "--labels", "o.txt", "--offsets", "-50", "0", "50", "--thetas", "30", "90",
                                      "--region", "poly24", "--output-dir", "out", "--device", "cuda:1"])
    assert (a.backbone, a.ckpt, a.exp_file, a.tsize, a.conf, a.nms, a.vis) == ("resnet", "ck.pth", "e.py", 320, 0.1, 0.5, True)
    assert (a.path, a.labels, a.offsets, a.thetas, a.region, a.output_dir, a.device) == \
        ("o.npy", "o.txt", [-50, 0, 50], [30, 90], "poly24", "out", "cuda:1")
    for name in ("darknet", "vgg", "resnet", "densenet"):
        assert mod.make_parser().parse_args(["--backbone", name]).backbone == name
    with pytest.raises(SystemExit):
        mod.make_parser().parse_args(["--backbone", "mobilenet"])
    assert mod.make_parser().parse_args(["--synthetic", "--thetas"]).thetas == []


def test_demo_featuremap_tables_and_synthetic_object():
    mod = _demo()
    img, rows = mod.synthetic_object(320, 0)
    assert img.shape == (320, 320, 3) and img.dtype == np.uint8 and rows.shape == (1, 51)
    assert 0 < rows[0, 1] < 1 and 0 < rows[0, 2] < 1
    lev = lambda m: {"rect": {"mean": [m], "count": [4]}, "poly24": {"mean": [], "count": []}}
    result = {"thetas": [30], "offsets": [-50, 0], "strides": [8], "map_sizes": [[40, 40]],
              "AP": {"none": {"AP": 0.5}, "theta_30": {"AP": -1.0}},
              "table": {"offset_-50_none": {"levels": [lev(0.25)]}, "offset_000_none": {"levels": [lev(0.5)]},
                        "offset_-50_theta_30": {"levels": [lev(1.0)]}, "offset_000_theta_30": {"levels": [lev(2.0)]}}}
    text = mod.format_tables(result, "rect").splitlines()
    assert "40x40" in text[0] and text[2].split() == ["none", "0.25000", "0.50000", "0.500"]
    assert text[3].split() == ["theta_30", "1.00000", "2.00000", "-1.000"]
    assert mod.format_tables(result, "poly24").splitlines()[2].split() == ["none", "-", "-", "0.500"]
