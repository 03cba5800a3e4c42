"""ep24.jpeg's writer on the GPU: ep24_jpeg_sample + ep24_jpeg_fdct against libjpeg's forward path (tests/jpeg_encode_oracle.py, itself
pinned to the committed Pillow files by tests/test_jpeg_encode_oracle.py) in every coefficient, ``encode`` against the committed files
byte for byte, batches, strided input, the round trip through the project's own decoder, and show_24p.py without PIL."""
import glob
import importlib
import os
import sys

import numpy as np
import pytest
import torch

import jpeg_encode_fixtures as ef
from ep24 import _lib, jpeg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
Y24 = os.path.join(ROOT, "exploration-of-potential_amd", "yolox_24p")
pytestmark = pytest.mark.gpu


def _kw(name):
    c = ef.case(name)
    return dict(quality=c["quality"], subsampling="4:2:0" if c["sampling"] == "grey" else c["sampling"], restart_interval=c["restart_interval"])


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


@pytest.mark.parametrize("name", ef.names())
def test_every_fixture_alone(name):
    px, want, kw = ef.pixels(name), ef.oracle_coefficients(name), _kw(name)
    grey = px.ndim == 2
    got = jpeg.forward([_dev(px)], bgr=False, **kw)
    assert len(got) == 1 and got[0].coef.dtype == np.int16 and got[0].coef.shape == want.shape
    assert np.array_equal(got[0].coef, want), "%d coefficients differ" % int((got[0].coef != want).sum())
    assert got[0].header.ncomp == (1 if grey else 3) and got[0].shape == (px.shape[0], px.shape[1], 3)
    data = jpeg.encode([_dev(px)], bgr=False, **kw)
    assert data == [ef.data(name)]
    if grey:                                                 # [h, w] and [h, w, 1] are the same one-component image, whatever bgr says
        assert jpeg.encode([_dev(px[:, :, None])], **kw) == [ef.data(name)]
    else:                                                    # BGR is the default: what ep24.jpeg.decode hands out
        assert jpeg.encode([_dev(px[:, :, ::-1])], **kw) == [ef.data(name)]


def test_all_fixtures_in_one_call_in_two_orders():
    """The cumulative tables and the binary search: the pixels of all 100 fixtures - six sizes, the scene and the photo, one- and
    three-component images mixed - in ONE call per sampling, in two orders; every result equals that of the image alone."""
    names = ef.names()
    order_b = list(np.random.RandomState(3).permutation(names))
    assert names != order_b
    dev = {n: _dev(ef.pixels(n)) for n in names}
    for sampling in ("4:4:4", "4:2:2", "4:2:0"):
        single = {}
        for n in names:
            c = ef.case(n)
            key = (c["source"], c["sampling"] == "grey")
            if key not in single:
                single[key] = jpeg.forward([dev[n]], quality=75, subsampling=sampling, bgr=False)[0].coef.copy()
            if c["quality"] == 75 and c["sampling"] in (sampling, "grey"):
                assert np.array_equal(single[key], ef.oracle_coefficients(n)), n
        for order in (names, order_b):
            out = jpeg.forward([dev[n] for n in order], quality=75, subsampling=sampling, bgr=False)
            assert len(out) == len(order)
            for n, it in zip(order, out):
                assert np.array_equal(it.coef, single[(ef.case(n)["source"], ef.case(n)["sampling"] == "grey")]), n


def test_strided_input_is_read_where_it_lies():
    rs = np.random.RandomState(11)
    wide = torch.from_numpy(rs.randint(0, 256, (40, 70, 3)).astype(np.uint8)).cuda()
    view = wide[3:36, 9:59]                                  # 33 x 50, row stride 210 > 150, a start that is not 4-byte aligned
    assert not view.is_contiguous() and view.stride(0) == 210
    for sampling in ("4:4:4", "4:2:2", "4:2:0"):
        assert jpeg.encode([view], quality=75, subsampling=sampling) == jpeg.encode([view.contiguous()], quality=75, subsampling=sampling)
    g = wide[:, :, 1]                                        # one component, pixel stride 3: not packed, copied by forward
    assert jpeg.encode([g]) == jpeg.encode([g.contiguous()])
    g2 = wide.view(40, 210)[5:22, 7:30]                      # one component, packed pixels, row stride 210
    assert jpeg.encode([g2]) == jpeg.encode([g2.contiguous()])


@pytest.mark.parametrize("name", ["enc_420_q95_33x50", "enc_422_q75_17x23", "enc_444_q10_40x7", "enc_grey_q75_5x3", "enc_rst5_420_q75_33x50"])
def test_own_round_trip(name):
    mine = jpeg.decode(jpeg.encode([_dev(ef.pixels(name))], bgr=False, **_kw(name)), bgr=False)[0]
    theirs = jpeg.decode([ef.data(name)], bgr=False)[0]
    assert torch.equal(mine, theirs) and tuple(mine.shape) == (ef.case(name)["height"], ef.case(name)["width"], 3)


def test_explicit_tables_and_quality_are_the_same():
    px = _dev(ef.pixels("enc_420_q75_17x23"))
    assert jpeg.encode([px], quality=jpeg.quality_tables(75), bgr=False) == [ef.data("enc_420_q75_17x23")]


def test_zero_input_launches_nothing():
    assert jpeg.forward([]) == [] and jpeg.encode([]) == []
    L = _lib.lib()
    s = _lib.stream_ptr()
    assert L.fn["ep24_jpeg_sample"](None, 0, 0, None, 0, s) == 0
    assert L.fn["ep24_jpeg_fdct"](None, 0, None, 0, None, 0, 0, None, s) == 0
    buf = torch.zeros(256, dtype=torch.uint8, device="cuda")
    assert L.fn["ep24_jpeg_sample"](buf.data_ptr(), 0, 5, buf.data_ptr(), 64, s) == 0          # no image: nothing to do
    assert L.fn["ep24_jpeg_sample"](buf.data_ptr(), -1, 0, buf.data_ptr(), 64, s) == jpeg.EP24_E_ARG
    assert L.fn["ep24_jpeg_sample"](None, 1, 8, buf.data_ptr(), 64, s) == jpeg.EP24_E_ARG       # null with work to do
    assert L.fn["ep24_jpeg_sample"](buf.data_ptr(), 1, 8, buf.data_ptr() + 4, 64, s) == jpeg.EP24_E_ARG
    assert L.fn["ep24_jpeg_fdct"](buf.data_ptr(), 64, buf.data_ptr(), 1, buf.data_ptr(), 1, -1, buf.data_ptr(), s) == jpeg.EP24_E_ARG
    assert L.fn["ep24_jpeg_fdct"](buf.data_ptr(), 64, buf.data_ptr() + 8, 1, buf.data_ptr(), 1, 1, buf.data_ptr(), s) == jpeg.EP24_E_ARG
    torch.cuda.synchronize()
    assert int(buf.sum()) == 0


def test_refusals():
    ok = torch.zeros(8, 8, 3, dtype=torch.uint8, device="cuda")
    for bad, word in ((ok.float(), "uint8"), (ok.cpu(), "not on the GPU"), (torch.zeros(1, 8193, 3, dtype=torch.uint8, device="cuda"), "8192"),
                      (torch.zeros(8193, 1, dtype=torch.uint8, device="cuda"), "8192"), (ok[:, :, :2], "[h, w, 3]")):
        with pytest.raises(jpeg.JpegError) as e:
            jpeg.encode([ok, bad])
        assert word in e.value.message and "image 1" in e.value.message


def test_show_24p_without_pil_writes_jpeg(tmp_path, monkeypatch):
    """Two small .jpg files in, PIL "missing", --jpeg-encoder auto: two baseline .jpg files out that ep24.jpeg reads back."""
    sys.path.insert(0, Y24)
    try:
        mod = importlib.import_module("show_24p")
        (tmp_path / "tiny_show_exp.py").write_text(
            "from exp import Exp as MyExp\n\n\nclass Exp(MyExp):\n    def __init__(self):\n        super().__init__()\n"
            "        self.depth, self.width, self.input_size, self.test_size = 0.33, 0.25, (128, 128), (128, 128)\n"
            "        self.exp_name = 'tiny_show'\n")
        monkeypatch.setattr(mod, "_pil", lambda: None)
        in_dir = tmp_path / "in"
        in_dir.mkdir()
        shapes = {}
        for n in ("enc_420_q95_33x50", "enc_444_q75_17x23"):
            (in_dir / (n + ".jpg")).write_bytes(ef.data(n))
            shapes[n + ".jpg"] = (ef.case(n)["height"], ef.case(n)["width"], 3)
        exp = mod.get_exp(str(tmp_path / "tiny_show_exp.py"))
        args = mod.make_parser().parse_args(["-p", str(in_dir), "-b", "2", "--jpeg-encoder", "auto", "--output-dir", str(tmp_path / "out")])
        torch.manual_seed(0)
        ev = mod.main(exp, args)
    finally:
        sys.path.remove(Y24)
        if str(tmp_path) in sys.path:                       # get_exp put the folder of the Exp file there
            sys.path.remove(str(tmp_path))
    written = sorted(glob.glob(os.path.join(ev.save_folder, "*.jpg")))
    assert [os.path.basename(p) for p in written] == sorted(shapes)
    for p in written:
        data = open(p, "rb").read()
        hd = jpeg.parse(data)
        assert (hd.h[0], hd.v[0]) == (2, 2) and np.array_equal(hd.qt[:2], jpeg.quality_tables(95))      # cv2.imwrite's defaults
        assert tuple(jpeg.decode([data])[0].shape) == shapes[os.path.basename(p)]
