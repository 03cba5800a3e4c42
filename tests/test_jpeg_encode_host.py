"""The host half of the JPEG writer (csrc/jpeg_host.cpp -> ep24/libep24jpeg.so: ep24.jpeg.entropy_encode / quality_tables) against the
committed Pillow files, byte for byte; seeded coefficient arrays at baseline's limits; the refusals; the sanitizer build of the
stand-alone check; show_24p.py's new flags.  No GPU."""
import ctypes
import importlib
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest
import torch

import jpeg_encode_fixtures as ef
import jpeg_fixtures as fx
from ep24 import jpeg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "exploration-of-potential_amd", "csrc")
Y24 = os.path.join(ROOT, "exploration-of-potential_amd", "yolox_24p")
ZIGZAG = [0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28, 35, 42, 49,
          56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63]


def _same_header(a, b):
    return all(np.array_equal(np.asarray(getattr(a, k)), np.asarray(getattr(b, k))) for k in jpeg.JpegHeader.__slots__)


@pytest.mark.parametrize("name", ef.names())
def test_bytes_round_trip(name):
    """entropy_encode(entropy_decode(file)) == file: markers, tables, scan, stuffing, padding and restart markers as Pillow writes them."""
    data = ef.data(name)
    got = jpeg.entropy_encode(jpeg.entropy_decode(data))
    assert isinstance(got, bytes) and len(got) == len(data)
    assert got == data, "first difference at byte %d" % next(i for i in range(len(data)) if got[i] != data[i])


@pytest.mark.parametrize("name", fx.decodable())
def test_coefficient_round_trip(name):
    """Files written with other Huffman tables (optimised ones among them) come back as the same coefficients and header."""
    c = jpeg.entropy_decode(fx.data(name))
    back = jpeg.entropy_decode(jpeg.entropy_encode(c))
    assert np.array_equal(back.coef, c.coef) and _same_header(back.header, c.header)


def _blank(h, w, mode, ri=0, q=75):
    hd = jpeg.make_header(h, w, mode, jpeg.quality_tables(q), ri)
    return jpeg.JpegCoefficients(hd, np.zeros(hd.ncoef, dtype=np.int16))


def _back(it):
    data = jpeg.entropy_encode(it)
    back = jpeg.entropy_decode(data)
    assert np.array_equal(back.coef, it.coef) and _same_header(back.header, it.header)
    return data


@pytest.mark.parametrize("mode", [0, 1, 2, 3])
@pytest.mark.parametrize("ri", [0, 1, 2, 1000])
def test_seeded_arrays_at_the_limits(mode, ri):
    """37 x 21: more than one MCU row, dummy blocks in 4:2:2 and 4:2:0.  Restart intervals 1, 2 and one beyond the MCU count."""
    rs = np.random.RandomState(7 + mode)
    # DC differences of +-2047 between consecutive blocks of a component (whatever the scan order: the values alternate by component
    # block parity in MCU order only for mode 0 / 1, so every block is simply set to one of the two extremes), AC at +-1023
    it = _blank(21, 37, mode, ri)
    blocks = it.coef.reshape(-1, 64)
    blocks[:, 0] = np.where(rs.randint(0, 2, len(blocks)) == 1, 1023, -1024)
    blocks[:, 1:] = np.where(rs.randint(0, 2, (len(blocks), 63)) == 1, 1023, -1023)        # no EOB: every block ends on coefficient 63
    data = _back(it)
    if ri == 1:
        assert data.count(b"\xff\xd0") >= 1                # RST0 is there
    # zero runs of 15, 16, 31 and 62 in front of one coefficient (62: only coefficient 63 is set), and 63 = an empty block
    it = _blank(21, 37, mode, ri)
    blocks = it.coef.reshape(-1, 64)
    for b, run in zip(range(len(blocks)), [15, 16, 31, 62, None, 47] * len(blocks)):
        blocks[b, 0] = rs.randint(-1024, 1024)
        if run is not None:
            blocks[b, ZIGZAG[1 + run]] = rs.choice([1, -1, 1023, -700])
    _back(it)
    # streams rich in 0xFF: values whose bits are all ones
    it = _blank(21, 37, mode, ri)
    blocks = it.coef.reshape(-1, 64)
    blocks[:, 1:] = (1 << rs.randint(1, 11, (len(blocks), 63))) - 1
    blocks[:, 0] = np.where(np.arange(len(blocks)) % 2 == 1, 1023, 0)
    data = _back(it)
    assert data.count(b"\xff\x00") > 10                     # the stuffing was exercised
    _back(_blank(21, 37, mode, ri))                          # all zero


def test_restart_interval_beyond_the_mcu_count_writes_dri_and_no_rst():
    it = _blank(21, 37, 3, 1000)
    it.coef[:] = np.random.RandomState(0).randint(-5, 6, it.coef.size)
    data = _back(it)
    assert b"\xff\xdd\x00\x04\x03\xe8" in data
    scan = data[data.index(b"\xff\xda"):]
    assert not any(b"\xff" + bytes([0xD0 + k]) in scan for k in range(8))


@pytest.mark.parametrize("q", [10, 75, 95, 100])
def test_quality_tables(q):
    qt = jpeg.quality_tables(q)
    assert qt.dtype == np.uint16 and qt.shape == (2, 64) and 1 <= int(qt.min()) and int(qt.max()) <= 255
    hd = jpeg.parse(ef.data("enc_420_q%d_17x23" % q))
    assert np.array_equal(qt[0], hd.qt[0]) and np.array_equal(qt[1], hd.qt[1]) and np.array_equal(qt[1], hd.qt[2])
    assert np.array_equal(qt[0], jpeg.parse(ef.data("enc_grey_q%d_17x23" % q)).qt[0])
    if q == 100:
        assert int(qt.max()) == 1


def test_quality_outside_1_100_is_refused():
    for q in (0, 101, -3):
        with pytest.raises(jpeg.JpegError) as e:
            jpeg.quality_tables(q)
        assert e.value.code == jpeg.EP24_E_ARG


def _raw_encode(hd, coef, capacity, guard=64):
    """The library call itself with ``capacity`` bytes of output followed by a guard region -> (rc, bytes written, guard intact)."""
    L = jpeg.host_lib()
    c = jpeg._c_header(hd)
    buf = np.full(capacity + guard, 0xA5, dtype=np.uint8)
    n = ctypes.c_int64(-1)
    rc = L.ep24jpeg_entropy_encode(ctypes.byref(c), coef.ctypes.data, coef.size, buf.ctypes.data, capacity, ctypes.byref(n))
    return rc, n.value, bool((buf[capacity:] == 0xA5).all())


def test_refusals_return_e_arg_and_leave_the_guard_intact():
    L = jpeg.host_lib()
    it = jpeg.entropy_decode(ef.data("enc_420_q95_17x23"))
    bound = L.ep24jpeg_encode_bound(ctypes.byref(jpeg._c_header(it.header)))
    assert bound > len(ef.data("enc_420_q95_17x23"))
    rc, n, ok = _raw_encode(it.header, it.coef, bound)
    assert rc == 0 and n == len(ef.data("enc_420_q95_17x23")) and ok
    rc, n, ok = _raw_encode(it.header, it.coef, bound - 1)                      # one byte short
    assert rc == jpeg.EP24_E_ARG and ok and b"capacity" in L.ep24jpeg_last_error()
    for idx, val in ((0, 2048), (0, -2048), (5, 1024), (5, -1024)):              # first DC difference, an AC coefficient
        coef = it.coef.copy()
        coef[idx] = val
        rc, n, ok = _raw_encode(it.header, coef, bound)
        assert rc == jpeg.EP24_E_ARG and ok, (idx, val)
        with pytest.raises(jpeg.JpegError) as e:
            jpeg.entropy_encode(jpeg.JpegCoefficients(it.header, coef))
        assert e.value.code == jpeg.EP24_E_ARG and ("DC" in e.value.message or "AC" in e.value.message)

    def broken(**kw):
        hd = jpeg.parse(ef.data("enc_420_q95_17x23"))
        for k, v in kw.items():
            setattr(hd, k, v)
        return hd
    qt0 = it.header.qt.copy()
    qt0[2, 63] = 0
    qt256 = it.header.qt.copy()
    qt256[0, 0] = 256
    for hd in (broken(blocks_w=[5, 2, 2]), broken(ncoef=it.header.ncoef - 64), broken(width=8193), broken(h=[2, 2, 1]), broken(height=0),
               broken(qt=qt0), broken(qt=qt256), broken(restart_interval=65536), broken(nblocks=[8, 2, 3])):
        rc, n, ok = _raw_encode(hd, it.coef, bound)
        assert rc == jpeg.EP24_E_ARG and ok
        assert L.ep24jpeg_encode_bound(ctypes.byref(jpeg._c_header(hd))) == jpeg.EP24_E_ARG
    with pytest.raises(jpeg.JpegError):
        jpeg.entropy_encode(jpeg.JpegCoefficients(it.header, it.coef[:-64]))
    with pytest.raises(jpeg.JpegError):
        jpeg.entropy_encode(jpeg.JpegCoefficients(it.header, it.coef.astype(np.int32)))


def test_host_library_exports_the_writer():
    out = subprocess.run(["nm", "-D", "--defined-only", jpeg.HOST_LIB_PATH], capture_output=True, text=True).stdout
    names = {l.split()[-1] for l in out.splitlines() if " T " in l}
    assert {"ep24jpeg_quality_tables", "ep24jpeg_encode_bound", "ep24jpeg_entropy_encode"} <= names
    assert jpeg.host_lib().ep24jpeg_abi_version() == 1      # additions only


def test_forward_argument_checks_need_no_gpu():
    assert jpeg.forward([]) == [] and jpeg.encode([]) == []
    cpu = torch.zeros(8, 8, 3, dtype=torch.uint8)
    with pytest.raises(jpeg.JpegError, match="not on the GPU"):
        jpeg.forward([cpu])
    with pytest.raises(jpeg.JpegError, match="uint8"):
        jpeg.forward([cpu.float()])
    with pytest.raises(jpeg.JpegError, match="subsampling"):
        jpeg.forward([cpu], subsampling="4:1:1")
    with pytest.raises(jpeg.JpegError):
        jpeg.forward([cpu], quality=0)
    with pytest.raises(jpeg.JpegError, match="tables"):
        jpeg.forward([cpu], quality=np.zeros((2, 64), dtype=np.int64))


def test_sanitizer_build_of_the_encoder(tmp_path):
    """csrc/jpeg_encode_check.cpp + jpeg_host.cpp under AddressSanitizer and UBSan, run as a child process: every new fixture written
    again byte for byte, every decodable older fixture by its coefficients, 80 seeded arrays, every refusal, and the kernel's
    quantisation reciprocal (csrc/jpeg_quant.h) against the integer division for every |t| <= 32 768 and qt in 1 .. 255.  Host code only."""
    if torch.cuda.is_available():
        pytest.skip("sanitizer runs belong on a machine without a GPU")
    cxx = shutil.which("g++")
    if cxx is None:
        pytest.skip("no g++")
    exe = str(tmp_path / "jpeg_encode_check")
    b = subprocess.run([cxx, "-std=c++17", "-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                        os.path.join(CSRC, "jpeg_encode_check.cpp"), os.path.join(CSRC, "jpeg_host.cpp"), "-o", exe],
                       capture_output=True, text=True, timeout=600)
    if b.returncode != 0 and ("asan" in b.stderr or "ubsan" in b.stderr or "sanitize" in b.stderr):
        pytest.skip("sanitizer runtime missing: " + b.stderr[-300:])
    assert b.returncode == 0, b.stderr[-3000:]
    cmd = [exe, "--exact"] + [ef.path(n) for n in ef.names()] + ["--coefficients"] + [fx.path(n) for n in fx.decodable()]
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, (p.stdout[-1000:], p.stderr[-3000:])
    assert "no crash" in p.stdout and "ERROR" not in p.stderr and "runtime error" not in p.stderr, p.stderr[-3000:]
    assert "%d files" % (len(ef.names()) + len(fx.decodable())) in p.stdout
    assert "%d quantisation cases" % (255 * 9 * 32769) in p.stdout          # the kernel's reciprocal against the division, exhaustively


def _show24p():
    sys.path.insert(0, Y24)
    try:
        return importlib.import_module("show_24p")
    finally:
        sys.path.remove(Y24)


def test_show_24p_jpeg_flags(monkeypatch, tmp_path):
    mod = _show24p()
    a = mod.make_parser().parse_args([])
    assert (a.jpeg_encoder, a.jpeg_quality) == ("auto", None)
    a = mod.make_parser().parse_args(["--jpeg-encoder", "native", "--jpeg-quality", "80"])
    assert (a.jpeg_encoder, a.jpeg_quality) == ("native", 80)
    assert mod.make_parser().parse_args(["--jpeg-encoder", "pil"]).jpeg_encoder == "pil"
    with pytest.raises(SystemExit):
        mod.make_parser().parse_args(["--jpeg-encoder", "cv2"])
    try:
        import PIL.Image  # noqa: F401
        have = True
    except Exception:
        have = False
    assert mod.resolve_jpeg_encoder("auto") == ("pil" if have else "native")
    assert mod.resolve_jpeg_encoder("native") == "native"
    monkeypatch.setattr(mod, "_pil", lambda: None)
    assert mod.resolve_jpeg_encoder("auto") == "native"
    with pytest.raises(SystemExit, match="PIL"):
        mod.resolve_jpeg_encoder("pil")
    img = np.zeros((4, 4, 3), dtype=np.uint8)
    for name in ("x.png", "x.bmp"):
        with pytest.raises(SystemExit, match="needs PIL"):
            mod.write_image(str(tmp_path / name), img)
    mod.write_image(str(tmp_path / "x.ppm"), img)           # the native formats do not ask for it
    assert np.array_equal(mod.read_image(str(tmp_path / "x.ppm")), img)
