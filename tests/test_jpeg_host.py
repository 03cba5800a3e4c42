"""The host entropy stage (csrc/jpeg_host.cpp -> ep24/libep24jpeg.so, ep24.jpeg.parse / entropy_decode) on the committed fixtures."""
import os
import pickle
import shutil
import subprocess

import numpy as np
import pytest
import torch

import jpeg_fixtures as fx
from ep24 import jpeg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "exploration-of-potential_amd", "csrc")
SUB = {"444": (1, 1), "422": (2, 1), "420": (2, 2)}


@pytest.mark.parametrize("c", fx.cases(), ids=lambda c: c["name"])
def test_header_fields(c):
    if not c["decodable"]:
        with pytest.raises(jpeg.JpegError) as e:
            jpeg.parse(fx.data(c["name"]))
        assert e.value.code == jpeg.EP24_E_UNSUPPORTED
        return
    hd = jpeg.parse(fx.data(c["name"]))
    ohd, _ = fx.oracle_coefficients(c["name"])
    assert (hd.height, hd.width) == (c["height"], c["width"]) and hd.shape == (c["height"], c["width"], 3)
    assert hd.ncomp == (1 if c["mode"] == "L" else 3)
    save = c["save"] or {}
    if hd.ncomp == 1:
        assert hd.h == [1] and hd.v == [1]
    elif "subsampling" in save:
        assert (hd.h[0], hd.v[0]) == SUB[{0: "444", 1: "422", 2: "420"}[save["subsampling"]]] and hd.h[1:] == [1, 1] and hd.v[1:] == [1, 1]
    assert hd.h == ohd.h and hd.v == ohd.v and hd.blocks_w == ohd.blocks_w and hd.blocks_h == ohd.blocks_h
    assert hd.restart_interval == ohd.restart_interval
    if "restart_marker_blocks" in save:
        assert hd.restart_interval == save["restart_marker_blocks"]
    if "restart_marker_rows" in save:
        assert hd.restart_interval == save["restart_marker_rows"] * ohd.mcus_x
    hmax, vmax = max(hd.h), max(hd.v)
    for i in range(hd.ncomp):
        assert hd.blocks_w[i] == -(-hd.width // (8 * hmax)) * hd.h[i] and hd.blocks_h[i] == -(-hd.height // (8 * vmax)) * hd.v[i]
        assert hd.nblocks[i] == hd.blocks_w[i] * hd.blocks_h[i]
    assert hd.ncoef == 64 * sum(hd.nblocks)
    assert hd.qt.dtype == np.uint16 and hd.qt.shape == (hd.ncomp, 64) and np.array_equal(hd.qt, ohd.qt)
    if c["name"].startswith("flat_q100"):
        assert int(hd.qt.max()) == 1


@pytest.mark.parametrize("name", fx.decodable())
def test_coefficients_equal_the_oracle(name):
    it = jpeg.entropy_decode(fx.data(name))
    _, want = fx.oracle_coefficients(name)
    assert it.coef.dtype == np.int16 and it.coef.shape == want.shape
    assert np.array_equal(it.coef, want)


@pytest.mark.parametrize("name", fx.refused())
def test_refused_files_raise_unsupported(name):
    with pytest.raises(jpeg.JpegError) as e:
        jpeg.entropy_decode(fx.data(name))
    assert e.value.code == jpeg.EP24_E_UNSUPPORTED and isinstance(e.value, jpeg.Ep24Error)
    word = {"refused_progressive": "progressive", "refused_cmyk": "4 components", "refused_12bit": "12-bit"}[name]
    assert word in e.value.message and word in str(e.value)


def test_other_refusals_name_their_reason():
    """Patched frame headers: 1x2 sampling, a side above 8192; a scan that holds one of three components."""
    d = bytearray(fx.data("q90_444_16x16"))
    p = d.index(b"\xff\xc0")
    for patch, word in (((p + 11, 0x12), "sampling"), ((p + 5, 0x40), "8192"), ((p + 7, 0x40), "8192")):
        e = bytearray(d)
        e[patch[0]] = patch[1]
        with pytest.raises(jpeg.JpegError) as err:
            jpeg.parse(bytes(e))
        assert err.value.code == jpeg.EP24_E_UNSUPPORTED and word in err.value.message, err.value.message
    s = d.index(b"\xff\xda")
    e = bytearray(d)
    e[s + 4] = 1
    with pytest.raises(jpeg.JpegError) as err:
        jpeg.parse(bytes(e))
    assert err.value.code == jpeg.EP24_E_UNSUPPORTED and "scan" in err.value.message


@pytest.mark.parametrize("name", fx.PREFIX_CASES)
def test_every_prefix_is_an_error_or_a_success(name):
    data = fx.data(name)
    _, want = fx.oracle_coefficients(name)
    ok = 0
    for n in range(len(data) + 1):
        try:
            it = jpeg.entropy_decode(data[:n])
        except jpeg.JpegError as e:
            assert e.code in (jpeg.EP24_E_UNSUPPORTED, jpeg.EP24JPEG_E_DATA) and e.message
            continue
        ok += 1
        assert np.array_equal(it.coef, want)              # a prefix that decodes holds the whole scan (only EOI is missing)
    assert 1 <= ok <= 3


def test_restart_marker_out_of_sequence_is_an_error():
    d = bytearray(fx.data("q75rst_444_33x50"))
    p = d.index(b"\xff\xd1")
    d[p + 1] = 0xD2
    with pytest.raises(jpeg.JpegError) as e:
        jpeg.entropy_decode(bytes(d))
    assert e.value.code == jpeg.EP24JPEG_E_DATA and "RST1" in e.value.message


def test_not_a_jpeg_and_empty_input():
    for data in (b"", b"\xff", b"not a jpeg at all", b"\xff\xd8", b"\xff\xd8\xff\xd9"):
        with pytest.raises(jpeg.JpegError) as e:
            jpeg.entropy_decode(data)
        assert e.value.code == jpeg.EP24JPEG_E_DATA


def test_coefficients_pickle():
    it = jpeg.entropy_decode(fx.data("scene_420_rst"), tag=False)
    back = pickle.loads(pickle.dumps(it))
    assert isinstance(back, jpeg.JpegCoefficients) and back.shape == it.shape == (240, 320, 3) and back.tag is False
    assert np.array_equal(back.coef, it.coef) and np.array_equal(back.header.qt, it.header.qt)
    assert back.header.blocks_w == it.header.blocks_w and back.header.h == it.header.h
    err = pickle.loads(pickle.dumps(jpeg.JpegError(-3, "x")))
    assert isinstance(err, jpeg.JpegError) and err.code == -3 and err.message == "x"


def test_host_half_touches_neither_the_gpu_library_nor_cuda():
    """A fresh interpreter: entropy_decode loads libep24jpeg.so only."""
    import sys
    code = ("import sys; sys.path.insert(0, %r)\n"
            "from ep24 import jpeg, _lib\n"
            "it = jpeg.entropy_decode(open(%r, 'rb').read())\n"
            "import torch\n"
            "maps = open('/proc/self/maps').read()\n"
            "assert 'libep24jpeg.so' in maps and 'libep24.so' not in maps and _lib._lib is None\n"
            "assert not torch.cuda.is_initialized()\n"
            "print(it.shape)\n") % (os.path.join(ROOT, "exploration-of-potential_amd"), fx.path("q90_420_17x23"))
    p = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and "(17, 23, 3)" in p.stdout, p.stderr[-2000:]


def test_host_library_exports_only_its_prefix():
    out = subprocess.run(["nm", "-D", "--defined-only", jpeg.HOST_LIB_PATH], capture_output=True, text=True).stdout
    names = {l.split()[-1] for l in out.splitlines() if " T " in l}
    assert {"ep24jpeg_parse", "ep24jpeg_entropy_decode", "ep24jpeg_last_error", "ep24jpeg_abi_version"} <= names
    assert not [n for n in names if n.startswith("ep24_")]
    deps = subprocess.run(["ldd", jpeg.HOST_LIB_PATH], capture_output=True, text=True).stdout
    assert "amdhip" not in deps and "hsa" not in deps


def test_finish_without_a_gpu_raises():
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    with pytest.raises(jpeg.Ep24Error, match="no GPU"):
        jpeg.finish([jpeg.entropy_decode(fx.data("q90_444_8x8"))])


def test_sanitizer_build_of_the_entropy_stage(tmp_path):
    """csrc/jpeg_host_check.cpp + jpeg_host.cpp under AddressSanitizer and UBSan, run as a child process: every fixture, every prefix
    of three of them, 2 000 seeded single-byte corruptions of the scene.  Host code on a CPU machine only."""
    if torch.cuda.is_available():
        pytest.skip("sanitizer runs belong on a machine without a GPU")
    cxx = shutil.which("g++")
    if cxx is None:
        pytest.skip("no g++")
    exe = str(tmp_path / "jpeg_host_check")
    b = subprocess.run([cxx, "-std=c++17", "-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                        os.path.join(CSRC, "jpeg_host_check.cpp"), os.path.join(CSRC, "jpeg_host.cpp"), "-o", exe],
                       capture_output=True, text=True, timeout=600)
    if b.returncode != 0 and ("asan" in b.stderr or "ubsan" in b.stderr or "sanitize" in b.stderr):
        pytest.skip("sanitizer runtime missing: " + b.stderr[-300:])
    assert b.returncode == 0, b.stderr[-3000:]
    cmd = [exe, "--all"] + [fx.path(c["name"]) for c in fx.cases()] + ["--prefix"] + [fx.path(n) for n in fx.PREFIX_CASES] + \
          ["--corrupt", fx.path(fx.SCENE)]
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, (p.stdout[-1000:], p.stderr[-3000:])
    assert "no crash" in p.stdout and "ERROR" not in p.stderr and "runtime error" not in p.stderr, p.stderr[-3000:]
