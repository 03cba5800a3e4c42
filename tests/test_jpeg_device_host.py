"""The host side of the device entropy decoder (no GPU): ``ep24.jpeg.scan`` (ep24jpeg_scan_layout) against ``parse`` and a Python walk
of the bytes, the kernel's phases on the host (ep24jpeg_selfsync_emulate: csrc/jpeg_huff_core.h with threads as loops) against
``entropy_decode``, the sanitizer build of csrc/jpeg_device_check.cpp, and the crafted streams of tests/jpeg_device_streams.py, whose
properties are asserted here from the files' bytes."""
import os
import pickle
import shutil
import subprocess
import sys

import numpy as np
import pytest
import torch

import jpeg_device_streams as ds
import jpeg_fixtures as fx
from ep24 import jpeg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "exploration-of-potential_amd", "csrc")


def _segments(data):
    """[(offset in the scan, length)] by the Python walk."""
    start, segs = ds.python_segments(data)
    return start, [(p - start, n) for p, n in segs]


@pytest.mark.parametrize("c", fx.cases(), ids=lambda c: c["name"])
def test_scan_header_fields_equal_parse(c):
    data = fx.data(c["name"])
    if not c["decodable"]:
        with pytest.raises(jpeg.JpegError) as e:
            jpeg.scan(data)
        assert e.value.code == jpeg.EP24_E_UNSUPPORTED
        return
    it, hd = jpeg.scan(data), jpeg.parse(data)
    for k in ("width", "height", "ncomp", "restart_interval", "h", "v", "blocks_w", "blocks_h", "nblocks", "ncoef"):
        assert getattr(it.header, k) == getattr(hd, k), k
    assert np.array_equal(it.header.qt, hd.qt) and it.shape == hd.shape
    hmax, vmax = max(hd.h), max(hd.v)
    assert (it.mcus_x, it.mcus_y) == (-(-hd.width // (8 * hmax)), -(-hd.height // (8 * vmax)))
    assert it.data.dtype == np.uint8 and it.tables.shape == (6, jpeg.SPEC_BYTES) and it.segments.dtype == np.int32


@pytest.mark.parametrize("name", fx.decodable())
def test_segment_table_equals_a_python_walk_of_the_bytes(name):
    data = fx.data(name)
    it = jpeg.scan(data)
    start, segs = _segments(data)
    mcus, ri = it.mcus_x * it.mcus_y, it.header.restart_interval
    nseg = -(-mcus // ri) if ri else 1
    assert len(it.segments) == nseg == len(segs)
    assert [(int(o), int(n)) for o, n, _ in it.segments] == segs
    assert [int(m) for m in it.segments[:, 2]] == ([ri] * (nseg - 1) + [mcus - ri * (nseg - 1)] if ri else [mcus])
    assert bytes(it.data) == data[start:start + segs[-1][0] + segs[-1][1]]
    assert data[start + it.data.size:start + it.data.size + 2] == b"\xff\xd9"


def test_table_specifications_are_the_files_dht_segments():
    data = ds.all_symbols()                               # the Annex K tables, written by entropy_encode
    it = jpeg.scan(data)
    found = {}
    p = 2
    while data[p + 1] != 0xDA:
        ln = (data[p + 2] << 8) | data[p + 3]
        if data[p + 1] == 0xC4:
            found[data[p + 4]] = data[p + 5:p + 2 + ln]
        p += 2 + ln
    for c, (tc, th) in enumerate([(0, 0), (0, 1), (0, 1), (1, 0), (1, 1), (1, 1)]):
        seg = found[(tc << 4) | th]
        row = it.tables[c]
        n = int(row[272:276].view(np.int32)[0])
        assert bytes(row[:16]) == seg[:16] and n == len(seg) - 16 == sum(seg[:16]) and bytes(row[16:16 + n]) == seg[16:]
    assert int(it.tables[3][272:276].view(np.int32)[0]) == 162


def test_refused_files_raise_what_parse_raises():
    for name in fx.refused():
        with pytest.raises(jpeg.JpegError) as a:
            jpeg.scan(fx.data(name))
        with pytest.raises(jpeg.JpegError) as b:
            jpeg.parse(fx.data(name))
        assert a.value.code == b.value.code == jpeg.EP24_E_UNSUPPORTED and a.value.message == b.value.message
    for data in (b"", b"\xff", b"not a jpeg at all", b"\xff\xd8", b"\xff\xd8\xff\xd9"):
        with pytest.raises(jpeg.JpegError) as e:
            jpeg.scan(data)
        assert e.value.code == jpeg.EP24JPEG_E_DATA


def test_restart_marker_out_of_sequence_and_wrong_segment_count_are_refused_by_name():
    d = bytearray(fx.data("q75rst_444_33x50"))
    p = d.index(b"\xff\xd1")
    e = bytearray(d)
    e[p + 1] = 0xD2
    for fn in (jpeg.scan, jpeg.entropy_decode, jpeg.selfsync_emulate):
        with pytest.raises(jpeg.JpegError) as err:
            fn(bytes(e))
        assert err.value.code == jpeg.EP24JPEG_E_DATA and "RST1" in err.value.message
    # one segment too few: the file ends (EOI) where RST1 should be
    short = bytes(d[:p]) + b"\xff\xd9"
    for fn in (jpeg.scan, jpeg.entropy_decode, jpeg.selfsync_emulate):
        with pytest.raises(jpeg.JpegError) as err:
            fn(short)
        assert err.value.code == jpeg.EP24JPEG_E_DATA and "RST1" in err.value.message


def test_a_missing_eoi_is_judged_as_entropy_decode_judges_it():
    """ep24jpeg_entropy_decode does not look behind the last coded bit, so a file cut in front of its EOI decodes; the marker walk
    reaches the same verdict on every cut (the check program compares every prefix of three files)."""
    data = fx.data("q90_420_17x23")
    assert data[-2:] == b"\xff\xd9"
    want = jpeg.entropy_decode(data).coef
    for cut in (data[:-2], data[:-1]):
        assert np.array_equal(jpeg.entropy_decode(cut).coef, want)
        assert bytes(jpeg.scan(cut).data) == bytes(jpeg.scan(data).data)
        assert np.array_equal(jpeg.selfsync_emulate(cut)[0].coef, want)
    with pytest.raises(jpeg.JpegError) as a:
        jpeg.entropy_decode(data[:-3])
    with pytest.raises(jpeg.JpegError) as b:
        jpeg.selfsync_emulate(data[:-3])
    assert a.value.code == b.value.code == jpeg.EP24JPEG_E_DATA


def test_scan_pickles():
    it = jpeg.scan(fx.data("scene_420_rst"), tag=False)
    it.source = "a.jpg"
    back = pickle.loads(pickle.dumps(it))
    assert isinstance(back, jpeg.JpegScan) and back.shape == it.shape == (240, 320, 3) and back.tag is False and back.source == "a.jpg"
    assert isinstance(back.data, np.ndarray) and back.data.dtype == np.uint8 and np.array_equal(back.data, it.data)
    assert np.array_equal(back.tables, it.tables) and np.array_equal(back.segments, it.segments) and back.segments.dtype == np.int32
    assert np.array_equal(back.header.qt, it.header.qt) and (back.mcus_x, back.mcus_y) == (it.mcus_x, it.mcus_y)
    import torch.multiprocessing  # noqa: F401  (registers the tensor reductions a DataLoader's queue uses: shared memory)
    from multiprocessing.reduction import ForkingPickler
    assert len(bytes(ForkingPickler.dumps(it))) < it.data.size              # the scan bytes did not go through the pipe


def test_scan_touches_neither_the_gpu_library_nor_cuda():
    code = ("import sys; sys.path.insert(0, %r)\n"
            "from ep24 import jpeg, _lib\n"
            "it = jpeg.scan(open(%r, 'rb').read())\n"
            "co, rounds = jpeg.selfsync_emulate(open(%r, 'rb').read())\n"
            "import torch\n"
            "maps = open('/proc/self/maps').read()\n"
            "assert 'libep24jpeg.so' in maps and 'libep24.so' not in maps and _lib._lib is None\n"
            "assert not torch.cuda.is_initialized()\n"
            "print(it.shape, rounds >= 1)\n") % (os.path.join(ROOT, "exploration-of-potential_amd"), fx.path("q90_420_17x23"), fx.path("q90_420_17x23"))
    p = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and "(17, 23, 3) True" in p.stdout, p.stderr[-2000:]


def test_host_library_exports_the_two_new_calls_and_keeps_its_abi_version():
    out = subprocess.run(["nm", "-D", "--defined-only", jpeg.HOST_LIB_PATH], capture_output=True, text=True).stdout
    names = {l.split()[-1] for l in out.splitlines() if " T " in l}
    assert {"ep24jpeg_scan_layout", "ep24jpeg_selfsync_emulate"} <= names and not [n for n in names if n.startswith("ep24_")]
    assert jpeg.host_lib().ep24jpeg_abi_version() == 1


@pytest.mark.parametrize("tile", [64, 1024])
@pytest.mark.parametrize("S", [16, 128])
def test_emulation_equals_entropy_decode_on_every_decodable_fixture(S, tile):
    names = fx.decodable()
    assert len(names) == 67
    for name in names:
        want = jpeg.entropy_decode(fx.data(name)).coef
        got, rounds = jpeg.selfsync_emulate(fx.data(name), S, tile)
        assert got.coef.dtype == np.int16 and np.array_equal(got.coef, want), name
        assert 1 <= rounds <= tile


def test_emulation_refuses_other_sizes():
    for S, tile in ((0, 64), (24, 64), (512, 64), (128, 0), (128, 1025)):
        with pytest.raises(jpeg.JpegError) as e:
            jpeg.selfsync_emulate(fx.data("q90_444_8x8"), S, tile)
        assert e.value.code == jpeg.EP24_E_ARG


def test_pack_lays_out_a_mixed_batch_without_a_gpu():
    """The planes of the JpegCoefficients items first, the device-decoded ones behind them; segment rows with cumulative MCUs and
    subsequences; every part inside the buffer."""
    a, b = jpeg.entropy_decode(fx.data("q90_420_33x50")), jpeg.scan(fx.data("q75rst_422_40x7"))
    c, d = jpeg.scan(fx.data("grey_q80_16x16")), jpeg.entropy_decode(fx.data("q90_444_17x23"))
    P = jpeg.pack([b, a, c, d], subseq_bytes=16, tile=64)
    nb = lambda it: sum(it.header.nblocks)
    assert P.n_scan == 2 and P.scan_items == [0, 2] and P.host_split == 128 * (nb(a) + nb(d)) and P.gap == 128 * (nb(b) + nb(c))
    assert P.dev_size == P.host.size + P.gap and P.o_qt == 128 * P.blocks and P.o_by + P.n_bytes == P.dev_size
    assert np.array_equal(P.host[:a.coef.nbytes].view(np.int16), a.coef)
    g = P.gap
    hd = P.host[P.o_hd - g:P.o_sg - g].view(np.int64)[:32].reshape(2, 16)
    assert list(hd[:, 5]) == [0, 64 * nb(b)] and list(hd[:, 6]) == [b.header.ncoef, c.header.ncoef] and list(hd[:, 2]) == [0, len(b.segments)]
    rows = P.host[P.o_sg - g:P.o_sg - g + 24 * P.n_seg].view(np.int32).reshape(-1, 6)
    rb = rows[:len(b.segments)]
    assert np.array_equal(rb[:, [0, 1, 3]], b.segments) and list(rb[:, 2]) == list(np.cumsum(b.segments[:, 2]) - b.segments[:, 2])
    nsub = np.maximum(-(-b.segments[:, 1] // 16), 1)
    assert list(rb[:, 4]) == list(np.cumsum(nsub) - nsub) and hd[0, 4] == nsub.sum()
    by = P.host[P.o_by - g:]
    assert bytes(by[hd[1, 0]:hd[1, 0] + hd[1, 1]]) == bytes(c.data)
    with pytest.raises(jpeg.JpegError):
        jpeg.pack([b], subseq_bytes=48)
    bad = jpeg.JpegScan(b.header, b.data[:-5], b.tables, b.segments, b.mcus_x, b.mcus_y)
    with pytest.raises(jpeg.JpegError):
        jpeg.pack([bad])
    # a batch without JpegScan items is laid out as it always was: one buffer, no gap
    Q = jpeg.pack([a, d])
    assert Q.n_scan == 0 and Q.gap == 0 and Q.dev_size == Q.host.size


def test_decode_refuses_another_entropy_mode_and_the_device_mode_needs_a_gpu():
    with pytest.raises(jpeg.JpegError):
        jpeg.decode([fx.data("q90_444_8x8")], entropy="gpu")
    if not torch.cuda.is_available():
        with pytest.raises(jpeg.Ep24Error, match="no GPU"):
            jpeg.decode([fx.data("q90_444_8x8")], entropy="device")


# ---- the crafted streams: what each must be, from its bytes; and the emulation on each ----

def _exact(data, S=(16, 128), tiles=(64, 1024)):
    want = jpeg.entropy_decode(data).coef
    rounds = {}
    for s in S:
        for t in tiles:
            got, r = jpeg.selfsync_emulate(data, s, t)
            assert np.array_equal(got.coef, want), (s, t)
            rounds[(s, t)] = r
    return rounds


def test_crafted_tiny_grey():
    data = ds.tiny_grey()
    it = jpeg.scan(data)
    assert it.header.ncomp == 1 and it.shape == (8, 8, 3) and 0 < it.data.size < min(jpeg.SUBSEQ_SIZES)
    _exact(data)


@pytest.mark.parametrize("S", [16, 128])
@pytest.mark.parametrize("delta", [-1, 0, 1])
def test_crafted_exact_lengths(S, delta):
    data = ds.exact_length(2 * S + delta)
    assert jpeg.scan(data).data.size == 2 * S + delta
    _exact(data)


@pytest.mark.parametrize("S", [16, 128])
@pytest.mark.parametrize("where", ["straddle", "inside", "first"])
def test_crafted_stuffed_bytes_at_a_boundary(S, where):
    data, k = ds.stuffed_at(S, where)
    d = jpeg.scan(data).data
    p = k * S + {"straddle": -1, "inside": -2, "first": 0}[where]
    assert k >= 1 and d[p] == 0xFF and d[p + 1] == 0 and d.size > (k + 1) * S
    if where == "straddle":
        assert d[k * S] == 0                              # the 00 is the boundary byte: the subsequence starts one byte later
    _exact(data)


def _symbols(coef):
    """The DC sizes and AC (run << 4 | size) symbols a baseline encoder codes for these blocks (n x 64, natural order; DC = difference)."""
    dc, ac, no_eob = set(), set(), 0
    for blk in coef:
        dc.add(int(abs(int(blk[0]))).bit_length())
        run, last = 0, 0
        for k in range(1, 64):
            v = int(blk[ds.ZIGZAG[k]])
            if v == 0:
                run += 1
                continue
            while run > 15:
                ac.add(0xF0)
                run -= 16
            ac.add((run << 4) | abs(v).bit_length())
            run, last = 0, k
        if last < 63:
            ac.add(0)
        else:
            no_eob += 1
    return dc, ac, no_eob


def test_crafted_all_symbols():
    data = ds.all_symbols()
    it = jpeg.entropy_decode(data)
    hd = it.header
    assert hd.ncomp == 3 and hd.h == [1, 1, 1] and b"\xff\xdd" not in data[:data.index(b"\xff\xda")]
    blocks = it.coef.reshape(-1, 64).astype(np.int64)
    n = hd.nblocks[0]
    want_ac = {(r << 4) | s for r in range(16) for s in range(1, 11)} | {0x00, 0xF0}
    assert len(want_ac) == 162
    for c in range(3):                                    # 4:4:4 without restarts: scan order is block order, the first difference is the DC
        comp = blocks[c * n:(c + 1) * n].copy()
        comp[1:, 0] = np.diff(comp[:, 0])
        dc, ac, no_eob = _symbols(comp)
        assert dc == set(range(12)) and ac == want_ac and no_eob >= 2, c
    # both Annex K AC tables end in 16-bit codes, and the file uses them: symbol 0xFA is the last of either table
    rounds = _exact(data)
    assert all(r >= 1 for r in rounds.values())


@pytest.mark.parametrize("interval", [1, 2, 7])
def test_crafted_restarts(interval):
    data = ds.restarts(interval)
    it = jpeg.scan(data)
    start, segs = _segments(data)
    assert it.header.restart_interval == interval and len(segs) == len(it.segments) == -(-64 // interval) > 8
    markers = [data[start + o + n + 1] for o, n in segs[:-1]]
    assert markers == [0xD0 + (i & 7) for i in range(len(segs) - 1)] and 0xD0 in markers[8:]           # RST7 -> RST0
    lens = it.segments[:, 1]
    assert lens.min() < 128 < lens.max() and lens.max() > 256
    _exact(data)


def test_crafted_flat_420_locks_to_the_wrong_phase():
    data = ds.flat_420()
    it = jpeg.entropy_decode(data)
    hd = it.header
    assert hd.shape == (64, 64, 3) and (hd.h[0], hd.v[0]) == (2, 2) and hd.restart_interval == 0
    blocks = it.coef.reshape(-1, 64)
    assert not blocks[:, 1:].any()                        # every block: EOB at once
    off = 0
    for c in range(3):                                    # every block but a component's first: DC difference 0, the size-0 code
        assert len(set(blocks[off:off + hd.nblocks[c], 0].tolist())) == 1
        off += hd.nblocks[c]
    d = jpeg.scan(data).data
    period = "001010" * 4 + "0000" * 2                    # an MCU: 4 x (DC size 0, luma EOB), 2 x (DC size 0, chroma EOB) = 32 bits
    tail = "".join("{:08b}".format(int(b)) for b in d[8:8 + 48])
    assert any(tail == (period[r:] + period[:r]) * 12 for r in range(32)), tail
    rounds = _exact(data)
    assert rounds[(16, 64)] > 2 and rounds[(16, 1024)] > 2, rounds


def test_truncated_scene_is_data_in_both_decoders():
    data = ds.truncated_scene()
    assert data[-2:] == b"\xff\xd9" and len(data) == len(fx.data(fx.SCENE)) - 100
    assert bytes(jpeg.scan(data).data) == bytes(jpeg.scan(fx.data(fx.SCENE)).data[:-100])
    for fn in (jpeg.entropy_decode, jpeg.selfsync_emulate, lambda d: jpeg.selfsync_emulate(d, 16, 64)):
        with pytest.raises(jpeg.JpegError) as e:
            fn(data)
        assert e.value.code == jpeg.EP24JPEG_E_DATA


def test_sanitizer_build_of_the_device_check_program(tmp_path):
    """csrc/jpeg_device_check.cpp + jpeg_host.cpp under AddressSanitizer and UBSan (the Makefile's jpeg_device_check target), run as
    a child process: every fixture and every crafted file, every prefix of three fixtures, 2 000 seeded single-byte corruptions of the
    scene, at S = 16 and S = 128.  Host code on a CPU machine only."""
    if torch.cuda.is_available():
        pytest.skip("sanitizer runs belong on a machine without a GPU")
    # the only other skip: a probe, made before anything of the project is built - an empty program under the same sanitizers must
    # compile, link and run (g++ and make themselves are what build() needs: without them this test fails)
    (tmp_path / "probe.cpp").write_text("int main() { return 0; }\n")
    probe = subprocess.run(["g++", "-fsanitize=address,undefined", str(tmp_path / "probe.cpp"), "-o", str(tmp_path / "probe")],
                           capture_output=True, text=True, timeout=300)
    if probe.returncode != 0 or subprocess.run([str(tmp_path / "probe")], capture_output=True, timeout=60).returncode != 0:
        pytest.skip("this g++ cannot build or run an empty program under -fsanitize=address,undefined: " + probe.stderr[-300:])
    b = subprocess.run(["make", "-C", CSRC, "jpeg_device_check", "CHECK_DIR=" + str(tmp_path)], capture_output=True, text=True, timeout=600)
    assert b.returncode == 0, b.stderr[-3000:]
    crafted = {"tiny": ds.tiny_grey(), "flat": ds.flat_420(), "symbols": ds.all_symbols(), "truncated": ds.truncated_scene(),
               "stuffed": ds.stuffed_at(16, "straddle")[0], "rst1": ds.restarts(1), "rst7": ds.restarts(7)}
    paths = []
    for k, v in crafted.items():
        paths.append(str(tmp_path / (k + ".jpg")))
        with open(paths[-1], "wb") as fh:
            fh.write(v)
    cmd = [str(tmp_path / "jpeg_device_check"), "--all"] + [fx.path(c["name"]) for c in fx.cases()] + paths + \
          ["--prefix"] + [fx.path(n) for n in fx.PREFIX_CASES] + ["--corrupt", fx.path(fx.SCENE), "--corrupt-rst", fx.path("scene_420_rst")]
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
    assert p.returncode == 0, (p.stdout[-1000:], p.stderr[-3000:])
    # the one documented difference, which only a file with restart markers can show: bytes left over in a restart segment are refused
    # by the host decoder ("RSTn expected") and ignored by the device decoder; every other input of the 2 000 gets one verdict
    surplus = [l for l in p.stdout.splitlines() if l.startswith("surplus bytes in a restart segment")]
    assert len(surplus) <= 1, p.stdout[-1000:]            # printed once, with their number (47 of the 2 000 when this was written)
    assert "no disagreement, no crash" in p.stdout and "ERROR" not in p.stderr and "runtime error" not in p.stderr, p.stderr[-3000:]
    lines = [l for l in p.stdout.splitlines() if l.startswith("rounds ")]
    assert len(lines) == len(fx.cases()) + len(paths) and any(l.startswith("rounds photo_") for l in lines)
