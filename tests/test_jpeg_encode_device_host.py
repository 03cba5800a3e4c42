"""The device entropy ENCODER's algorithm without a GPU: its phases run on the host through the shared text (csrc/jpeg_huffenc_core.h ->
ep24jpeg_encode_emulate of ep24/libep24jpeg.so -> ep24.jpeg.encode_emulate) against the committed Pillow files and against the serial
host writer, byte for byte; the factored header; the refusals; the exports; the flags; the sanitizer build of the stand-alone check."""
import importlib
import os
import subprocess
import sys

import pytest
import torch

import jpeg_encode_device_cases as dc
import jpeg_encode_fixtures as ef
import jpeg_fixtures as fx
from ep24 import jpeg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "exploration-of-potential_amd", "csrc")
Y24 = os.path.join(ROOT, "exploration-of-potential_amd", "yolox_24p")
TILES = (64, 1024)


@pytest.mark.parametrize("name", ef.names())
def test_every_fixture_byte_for_byte(name):
    data = ef.data(name)
    it = jpeg.entropy_decode(data)
    for tile in TILES:
        got = jpeg.encode_emulate(it, tile=tile)
        assert isinstance(got, bytes) and got == data, (tile, len(got), len(data))


@pytest.mark.parametrize("name", fx.decodable())
def test_older_fixtures_by_their_coefficients(name):
    """Files written with other Huffman tables (optimised ones among them): their coefficients and header, written with the Annex K
    tables by the emulation and by the serial writer, are the same bytes."""
    it = jpeg.entropy_decode(fx.data(name))
    want = jpeg.entropy_encode(it)
    for tile in TILES:
        assert jpeg.encode_emulate(it, tile=tile) == want, tile


@pytest.mark.parametrize("mode", sorted(dc.MODES))
@pytest.mark.parametrize("ri", dc.INTERVALS)
def test_seeded_arrays_at_the_limits(mode, ri):
    for i, it in enumerate(dc.seeded(mode, ri)):
        want = jpeg.entropy_encode(it)
        for tile in (1, 7) + TILES:
            assert jpeg.encode_emulate(it, tile=tile) == want, (i, tile)
    if ri == 1:
        assert want.count(b"\xff\xd0") >= 1
    if ri == 1000:
        assert b"\xff\xdd\x00\x04\x03\xe8" in want and b"\xff\xd0" not in want[want.index(b"\xff\xda"):]


@pytest.mark.parametrize("name", sorted(dc.crafted()))
def test_crafted_shapes(name):
    it = dc.crafted()[name]
    want = jpeg.entropy_encode(it)
    for tile in TILES + (dc.T,):
        assert jpeg.encode_emulate(it, tile=tile) == want, tile


def test_the_crafted_shapes_are_what_they_claim():
    c = dc.crafted()
    for n in (63, 64, 65, 65535, 65536, 65537):
        name = ("stuff_chunk_%d_bytes" if n < 100 else "stuff_round_%d_bytes") % n
        seg = dc.segments(jpeg.entropy_encode(c[name]))
        assert len(seg) == 1 and len(seg[0]) == n, name
    assert dc.CHUNK == 64 and dc.ROUND * dc.CHUNK == 65536 and dc.T == 256
    for n in (dc.T - 1, dc.T, dc.T + 1):
        assert c["emit_tile_grey_%d" % n].header.nblocks == [n]
    assert sum(c["emit_tile_420_%d_mcus" % (dc.T // 4)].header.nblocks) == 6 * dc.T // 4
    assert len(dc.segments(jpeg.entropy_encode(c["rst_wraps_420_33x50"]))) == 12
    assert len(dc.segments(jpeg.entropy_encode(c["rst_beyond_420_33x50"]))) == 1
    # 37 empty luma blocks of 6 bits: 222 bits in 7 words, so every word is shared by five or six blocks
    assert len(dc.segments(jpeg.entropy_encode(c["empty_luma_run"]))[0]) == 28
    # a block of maximum length: 9 + 11 bits of DC and 63 x (16 + 10) of AC
    grey = dc.segments(jpeg.entropy_encode(c["max_block_grey"]))[0]
    assert 8 * len(grey) >= 20 + 63 * 26


def test_the_ff_seeds_hold_what_they_promise():
    for kind in dc.FF_SEEDS:
        assert dc.ff_property(kind, dc.ff_case(kind)), kind
    assert dc.padded_bits(dc.ff_case("padded")) > 0
    # with restart interval 1 the stuffed file holds the padded FF 00 right in front of a marker
    data = jpeg.entropy_encode(dc.ff_case("padded", 1))
    assert b"\xff\x00\xff\xd0" in data or b"\xff\x00\xff\xd1" in data or b"\xff\x00\xff\xd2" in data or data.endswith(b"\xff\x00\xff\xd9")


@pytest.mark.parametrize("kind", ["DC", "AC"])
def test_out_of_range_is_refused_as_by_the_writer(kind):
    items = dc.out_of_range(kind)
    for call in (jpeg.entropy_encode, jpeg.encode_emulate):
        with pytest.raises(jpeg.JpegError) as e:
            call(items[1])
        assert e.value.code == jpeg.EP24_E_ARG and kind in e.value.message, call
    for idx, val in ((0, 2048), (0, -2048), (5, 1024), (64 + 63, -1024)):
        it = jpeg.entropy_decode(ef.data("enc_420_q95_17x23"))
        it.coef[idx] = val
        with pytest.raises(jpeg.JpegError) as e:
            jpeg.encode_emulate(it)
        assert e.value.code == jpeg.EP24_E_ARG
    with pytest.raises(jpeg.JpegError):
        jpeg.encode_emulate(items[0], tile=0)
    assert jpeg.encode_emulate(items[0]) == jpeg.entropy_encode(items[0])


@pytest.mark.parametrize("name", ["enc_420_q95_33x50", "enc_grey_q75_5x3", "enc_rst5_420_q75_33x50", "enc_444_q10_40x7"])
def test_header_then_scan_then_eoi(name):
    data = ef.data(name)
    it = jpeg.entropy_decode(data)
    head = jpeg.encode_header(it.header)
    at = data.index(b"\xff\xda")
    assert head == data[:at + 2 + (data[at + 2] << 8 | data[at + 3])]
    assert head[:2] == b"\xff\xd8" and (b"\xff\xdd" in head) == (it.header.restart_interval > 0)
    # the emulation's scan is what lies between: header + scan + FF D9 is the writer's file
    scan = jpeg.encode_emulate(it)[len(head):-2]
    assert head + scan + b"\xff\xd9" == jpeg.entropy_encode(it) == data
    hd = jpeg.parse(data)
    hd.width = 8193
    with pytest.raises(jpeg.JpegError) as e:
        jpeg.encode_header(hd)
    assert e.value.code == jpeg.EP24_E_ARG


def test_host_library_exports_the_new_calls():
    out = subprocess.run(["nm", "-D", "--defined-only", jpeg.HOST_LIB_PATH], capture_output=True, text=True).stdout
    names = {l.split()[-1] for l in out.splitlines() if " T " in l}
    assert {"ep24jpeg_encode_header", "ep24jpeg_encode_emulate", "ep24jpeg_entropy_encode"} <= names
    assert not any(n.startswith("ep24_") for n in names)   # no device entry point in the host library
    assert jpeg.host_lib().ep24jpeg_abi_version() == 1      # additions only


def test_the_device_library_declares_and_exports_the_encoder():
    from ep24 import _lib
    protos = _lib.parse_header()
    assert {"ep24_jpeg_huffenc_count", "ep24_jpeg_huffenc_emit"} <= set(protos)
    L = _lib.lib()
    assert L.fn["ep24_abi_version"]() == 3                  # additions only
    for name in ("ep24_jpeg_huffenc_count", "ep24_jpeg_huffenc_emit"):
        assert protos[name][1][-1] == ("void*", "stream")


def test_entropy_keyword_is_checked_before_anything_touches_the_gpu(monkeypatch):
    from ep24 import _lib
    monkeypatch.setattr(_lib, "require_gpu", lambda: pytest.fail("the GPU was asked for"))
    cpu = torch.zeros(8, 8, 3, dtype=torch.uint8)
    for bad in ("bogus", "", None, "Device"):
        with pytest.raises(jpeg.JpegError) as e:
            jpeg.encode([cpu], entropy=bad)
        assert e.value.code == jpeg.EP24_E_ARG and "entropy" in e.value.message
    assert jpeg.encode([], entropy="device") == [] and jpeg.encode([], entropy="host") == []


def test_device_entropy_raises_without_a_gpu(monkeypatch):
    from ep24 import _lib
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    with pytest.raises(_lib.Ep24Error, match="no GPU"):
        jpeg.encode([torch.zeros(8, 8, 3, dtype=torch.uint8)], entropy="device")
    with pytest.raises(_lib.Ep24Error, match="no GPU"):
        jpeg.entropy_encode_device([dc.crafted()["grey_1x1"]])


def test_show_24p_accepts_jpeg_entropy():
    sys.path.insert(0, Y24)
    try:
        mod = importlib.import_module("show_24p")
    finally:
        sys.path.remove(Y24)
    assert mod.make_parser().parse_args([]).jpeg_entropy == "host"
    a = mod.make_parser().parse_args(["--jpeg-encoder", "native", "--jpeg-entropy", "device"])
    assert (a.jpeg_encoder, a.jpeg_entropy) == ("native", "device")
    with pytest.raises(SystemExit):
        mod.make_parser().parse_args(["--jpeg-entropy", "gpu"])
    import inspect
    assert inspect.signature(mod.write_images).parameters["jpeg_entropy"].default == "host"


def test_sanitizer_build_of_the_device_encoder_check_program(tmp_path):
    """csrc/jpeg_huffenc_check.cpp + jpeg_host.cpp under AddressSanitizer and UBSan (make jpeg_huffenc_check), run as a child process:
    the shared text driven through count, scan, emit in three orders and the stuff passes, into buffers of exactly the counted sizes, on
    seeded and crafted blocks and on every fixture, against ep24jpeg_entropy_encode.  Host code only; nothing is loaded into Python."""
    if torch.cuda.is_available():
        pytest.skip("sanitizer runs belong on a machine without a GPU")
    # the only other skip: a probe, made before anything of the project is built - an empty program under the same sanitizers must
    # compile, link and run (g++ and make themselves are what build() needs: without them this test fails)
    (tmp_path / "probe.cpp").write_text("int main() { return 0; }\n")
    probe = subprocess.run(["g++", "-fsanitize=address,undefined", str(tmp_path / "probe.cpp"), "-o", str(tmp_path / "probe")],
                           capture_output=True, text=True, timeout=300)
    if probe.returncode != 0 or subprocess.run([str(tmp_path / "probe")], capture_output=True, timeout=60).returncode != 0:
        pytest.skip("this g++ cannot build or run an empty program under -fsanitize=address,undefined: " + probe.stderr[-300:])
    b = subprocess.run(["make", "-C", CSRC, "jpeg_huffenc_check", "CHECK_DIR=" + str(tmp_path)], capture_output=True, text=True, timeout=600)
    assert b.returncode == 0, b.stderr[-3000:]
    cmd = [str(tmp_path / "jpeg_huffenc_check")] + [ef.path(n) for n in ef.names()] + [fx.path(n) for n in fx.decodable()]
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, (p.stdout[-1000:], p.stderr[-3000:])
    assert "no crash" in p.stdout and "ERROR" not in p.stderr and "runtime error" not in p.stderr, p.stderr[-3000:]
    assert "(%d files)" % (len(ef.names()) + len(fx.decodable())) in p.stdout
