"""The writer's Huffman stage on the GPU (csrc/jpeg_huffenc.hip: ep24_jpeg_huffenc_count + ep24_jpeg_huffenc_emit) against the committed
Pillow files and against the serial host writer, byte for byte: ``encode(entropy="device")`` on every fixture alone and in batches,
``entropy_encode_device`` on seeded arrays at baseline's limits and on the crafted shapes of tests/jpeg_encode_device_cases.py (emit
tile and stuff chunk boundaries, shared words, FF bytes at every boundary, restart markers), the refusals, determinism, the round
trip through the device decoder and show_24p.py's flag."""
import importlib
import os
import sys

import numpy as np
import pytest
import torch

import jpeg_encode_device_cases as dc
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


def _where(got, want):
    return "lengths %d / %d, first difference at byte %d" % (len(got), len(want), next((i for i in range(min(len(got), len(want))) if got[i] != want[i]), -1))


@pytest.mark.parametrize("name", ef.names())
def test_every_fixture_alone(name):
    got = jpeg.encode([_dev(ef.pixels(name))], bgr=False, entropy="device", **_kw(name))
    assert len(got) == 1 and isinstance(got[0], bytes)
    assert got[0] == ef.data(name), _where(got[0], ef.data(name))


def test_all_fixtures_in_one_call_in_two_orders():
    """The compact offsets across images: all 100 fixtures - six sizes, one- and three-component images mixed - in ONE call per
    (quality, sampling, restart interval), in two orders; an image of another sampling is then written at the call's, so the expected
    bytes are the host path's on the same batch, which the first test pins to the files."""
    names = ef.names()
    order_b = list(np.random.RandomState(3).permutation(names))
    assert names != order_b
    dev = {n: _dev(ef.pixels(n)) for n in names}
    for kw in (dict(quality=75, subsampling="4:2:0"), dict(quality=95, subsampling="4:4:4", restart_interval=5), dict(quality=10, subsampling="4:2:2")):
        for order in (names, order_b):
            batch = [dev[n] for n in order]
            want = jpeg.encode(batch, bgr=False, **kw)
            got = jpeg.encode(batch, bgr=False, entropy="device", **kw)
            assert len(got) == len(order)
            for n, g, w in zip(order, got, want):
                assert g == w, (n, _where(g, w))
                c = ef.case(n)
                if (c["quality"], c["restart_interval"]) == (kw["quality"], kw.get("restart_interval", 0)) and c["sampling"] in (kw["subsampling"], "grey"):
                    assert g == ef.data(n), n


def test_a_batch_of_one_and_of_none():
    name = "enc_420_q95_33x50"
    assert jpeg.encode([_dev(ef.pixels(name))], bgr=False, entropy="device", **_kw(name)) == [ef.data(name)]
    assert jpeg.encode([], entropy="device") == [] and jpeg.entropy_encode_device([]) == []
    L, s = _lib.lib(), _lib.stream_ptr()
    assert L.fn["ep24_jpeg_huffenc_count"](None, 0, None, 0, 0, 0, None, None, None, None, None, s) == 0
    assert L.fn["ep24_jpeg_huffenc_emit"](None, 0, None, 0, 0, 0, None, None, None, None, 0, None, None, None, 0, None, s) == 0
    buf = torch.zeros(1024, dtype=torch.uint8, device="cuda")
    p, rcs = buf.data_ptr(), []

    def refused():                                          # on a thread of its own: the library's last-error text is per thread
        count, emit = L.fn["ep24_jpeg_huffenc_count"], L.fn["ep24_jpeg_huffenc_emit"]
        rcs.append(count(p, 64, p, -1, 1, 1, p, p, p, p, p, s))
        rcs.append(count(p, 64, None, 1, 1, 1, p, p, p, p, p, s))             # null with work to do
        rcs.append(count(p + 2, 64, p, 1, 1, 1, p, p, p, p, p, s))            # misaligned coefficients
        rcs.append(emit(p, 64, p, 1, 1, 1, p, p, p, None, 1, p, p, p, 16, p, s))
        rcs.append(emit(p, 64, p, 1, 1, 1, p, p, p, p, -1, p, p, p, 16, p, s))
    import threading
    th = threading.Thread(target=refused)
    th.start()
    th.join()
    assert rcs == [jpeg.EP24_E_ARG] * 5
    torch.cuda.synchronize()
    assert int(buf.sum()) == 0


@pytest.mark.parametrize("mode", sorted(dc.MODES))
def test_seeded_arrays_at_the_limits(mode):
    """DC differences of +-2047, AC of +-1023, zero runs of 15, 16, 31 and 62, a run to the end, empty blocks, FF-rich streams and all
    zero at restart interval 0, 1, 5 and beyond the MCU count: the 16 arrays of a sampling in ONE call."""
    items = [it for ri in dc.INTERVALS for it in dc.seeded(mode, ri)]
    got = jpeg.entropy_encode_device(items)
    assert len(got) == len(items)
    for i, (g, it) in enumerate(zip(got, items)):
        want = jpeg.entropy_encode(it)
        assert g == want, (i, _where(g, want))


@pytest.mark.parametrize("name", sorted(dc.crafted()))
def test_crafted_shapes(name):
    it = dc.crafted()[name]
    want = jpeg.entropy_encode(it)
    got = jpeg.entropy_encode_device([it])
    assert got == [want], _where(got[0], want)


def test_crafted_shapes_in_one_batch():
    """Every crafted image behind the other: an image's first block in the middle of an emit tile, its words behind another's."""
    items = [dc.crafted()[n] for n in sorted(dc.crafted())]
    got = jpeg.entropy_encode_device(items)
    for n, g, it in zip(sorted(dc.crafted()), got, items):
        want = jpeg.entropy_encode(it)
        assert g == want, (n, _where(g, want))


def test_restart_markers_wrap_and_stay_away():
    data = jpeg.entropy_encode_device([dc.crafted()["rst_wraps_420_33x50"], dc.crafted()["rst_beyond_420_33x50"]])
    scan = data[0][data[0].index(b"\xff\xda"):]
    marks = [scan[i + 1] for i in range(len(scan) - 1) if scan[i] == 0xFF and 0xD0 <= scan[i + 1] <= 0xD7]
    assert marks == [0xD0 + (j & 7) for j in range(11)]      # 12 segments: the RSTn number wraps
    assert b"\xff\xdd\x00\x04\x03\xe8" in data[1]
    scan = data[1][data[1].index(b"\xff\xda"):]
    assert not any(b"\xff" + bytes([0xD0 + k]) in scan for k in range(8))


@pytest.mark.parametrize("kind", ["DC", "AC"])
def test_out_of_range_names_the_item_and_the_kind(kind):
    items = dc.out_of_range(kind)
    with pytest.raises(jpeg.JpegError) as e:
        jpeg.entropy_encode_device(items)
    assert e.value.code == jpeg.EP24_E_ARG and "item 1" in e.value.message and kind in e.value.message
    assert ("AC" if kind == "DC" else "DC") not in e.value.message
    with pytest.raises(jpeg.JpegError):
        jpeg.entropy_encode(items[1])                       # the host writer refuses it too
    rest = [items[0], items[2]]
    assert jpeg.entropy_encode_device(rest) == [jpeg.entropy_encode(it) for it in rest]


def test_the_same_batch_twice_gives_the_same_bytes():
    names = ["enc_420_q95_33x50", "enc_grey_q75_5x3", "enc_rst5_420_q75_33x50", "enc_444_q10_40x7"]
    batch = [_dev(ef.pixels(n)) for n in names]
    a = jpeg.encode(batch, bgr=False, restart_interval=1, entropy="device")
    b = jpeg.encode(batch, bgr=False, restart_interval=1, entropy="device")
    assert a == b and a == jpeg.encode(batch, bgr=False, restart_interval=1)
    items = [dc.crafted()["empty_luma_run"], dc.crafted()["ff_three"], dc.seeded(3, 1)[0]]
    assert jpeg.entropy_encode_device(items) == jpeg.entropy_encode_device(items)


@pytest.mark.parametrize("name", ["enc_420_q95_33x50", "enc_422_q75_17x23", "enc_444_q10_40x7", "enc_grey_q75_5x3", "enc_rst5_420_q75_33x50"])
def test_round_trip_through_the_device_decoder(name):
    px = _dev(ef.pixels(name))
    mine = jpeg.decode(jpeg.encode([px], bgr=False, entropy="device", **_kw(name)), bgr=False, entropy="device")[0]
    theirs = jpeg.decode(jpeg.encode([px], bgr=False, **_kw(name)), bgr=False)[0]
    assert torch.equal(mine, theirs)


def test_show_24p_writes_the_same_file_either_way(tmp_path):
    sys.path.insert(0, Y24)
    try:
        mod = importlib.import_module("show_24p")
    finally:
        sys.path.remove(Y24)
    imgs = [ef.pixels("enc_420_q95_33x50"), _dev(ef.pixels("enc_444_q75_17x23"))]
    for where in ("host", "device"):
        mod.write_images([str(tmp_path / ("%s_%d.jpg" % (where, i))) for i in range(2)], imgs, jpeg_encoder="native", jpeg_entropy=where)
    for i in range(2):
        assert (tmp_path / ("device_%d.jpg" % i)).read_bytes() == (tmp_path / ("host_%d.jpg" % i)).read_bytes()
    assert (tmp_path / "device_0.jpg").read_bytes() == ef.data("enc_420_q95_33x50")
