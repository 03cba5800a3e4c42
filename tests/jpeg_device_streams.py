"""Crafted JPEG files for the device entropy decoder's tests (tests/test_jpeg_device_host.py, tests/test_gpu_jpeg_device.py): every one
comes from ``jpeg.entropy_encode`` on seeded coefficients - a host-only, deterministic call - and is searched or built so that its scan
has the property its name says.  The properties are asserted from the files' bytes in test_jpeg_device_host.py."""
import functools

import numpy as np

import jpeg_fixtures as fx
from ep24 import jpeg

ZIGZAG = np.array([0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28, 35,
                   42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63])


def encode(height, width, mode, coef, restart_interval=0, quality=75):
    hd = jpeg.make_header(height, width, mode, jpeg.quality_tables(quality), restart_interval)
    coef = np.ascontiguousarray(coef, dtype=np.int16).reshape(-1)
    assert coef.size == hd.ncoef
    return jpeg.entropy_encode(jpeg.JpegCoefficients(hd, coef))


def scan_bytes(data):
    return jpeg.scan(data).data


def _sparse(rng, nblocks, density, amp):
    """nblocks x 64 coefficients: each AC nonzero with probability ``density`` (falling with the frequency), DC steps within +-amp."""
    c = np.zeros((nblocks, 64), dtype=np.int64)
    keep = rng.random_sample((nblocks, 63)) < density * np.linspace(1.0, 0.15, 63)
    vals = rng.randint(-amp, amp + 1, size=(nblocks, 63))
    c[:, ZIGZAG[1:]] = np.where(keep, vals, 0)
    c[:, 0] = np.clip(np.cumsum(rng.randint(-amp, amp + 1, size=nblocks)), -1000, 1000)
    return c


@functools.lru_cache(maxsize=None)
def tiny_grey():
    """A grey 8 x 8 file whose scan is shorter than the smallest subsequence."""
    c = np.zeros(64, dtype=np.int64)
    c[0], c[1], c[8] = 5, -3, 2
    return encode(8, 8, 0, c)


@functools.lru_cache(maxsize=None)
def exact_length(target, seed0=0):
    """A grey 16 x 24 file (6 blocks) whose scan is exactly ``target`` bytes: the first seed at which a density that aims there hits."""
    for seed in range(seed0, seed0 + 20000):
        rng = np.random.RandomState(seed)
        c = _sparse(rng, 6, min(0.9, target / 420.0), 60)
        data = encode(16, 24, 0, c)
        if scan_bytes(data).size == target:
            return data
    raise AssertionError("no seed gives a scan of %d bytes" % target)


@functools.lru_cache(maxsize=None)
def stuffed_at(S, where):
    """A grey 32 x 32 file with an FF 00 pair at a subsequence boundary k * S (k >= 1) of its scan.  where = "straddle": FF is the
    last byte of a subsequence and 00 the first of the next (the boundary byte); "inside": FF 00 are the last two bytes of a
    subsequence; "first": FF 00 are the first two bytes of one.  -> (file, k)."""
    shift = {"straddle": -1, "inside": -2, "first": 0}[where]
    for seed in range(20000):
        rng = np.random.RandomState(1000 + seed)
        data = encode(32, 32, 0, _sparse(rng, 16, 0.8, 900), quality=95)
        d = scan_bytes(data)
        for k in range(1, d.size // S):
            p = k * S + shift
            if p + 1 < d.size and d[p] == 0xFF and d[p + 1] == 0:
                return data, k
    raise AssertionError("no seed puts FF 00 at a boundary of %d bytes" % S)


def _symbol_blocks(size_cap=10):
    """Blocks (64 coefficients, natural order) that use every AC (run, size) symbol with run 0 .. 15 and size 1 .. size_cap, ZRL, EOB,
    and one block whose last coefficient is set (no EOB)."""
    blocks, cur, k = [], np.zeros(64, dtype=np.int64), 1
    sign = 1
    for s in range(1, size_cap + 1):
        for r in range(16):
            if k + r > 63:
                blocks.append(cur)
                cur, k = np.zeros(64, dtype=np.int64), 1
            k += r
            cur[ZIGZAG[k]] = sign * ((1 << (s - 1)) + (r % (1 << (s - 1)) if s > 1 else 0))
            sign = -sign
            k += 1
    blocks.append(cur)
    zrl = np.zeros(64, dtype=np.int64)
    zrl[ZIGZAG[20]] = 3                                   # 16 zeros (ZRL), then run 3
    zrl[ZIGZAG[63]] = -1                                  # 42 zeros: two more ZRL, run 10; the block ends without EOB
    blocks.append(zrl)
    full = np.zeros(64, dtype=np.int64)
    full[ZIGZAG[1:]] = np.where(np.arange(63) % 2, 1, -1)  # 63 symbols (0, 1): no EOB either
    blocks.append(full)
    return blocks


@functools.lru_cache(maxsize=None)
def all_symbols():
    """A 4:4:4 file in which every component's blocks walk through every DC size 0 .. 11 and every one of the 162 AC symbols, so both
    Annex K tables are used in full: the 16-bit codes, ZRL, and blocks with no EOB."""
    blocks = _symbol_blocks()
    diffs = [0] + [(1 << (s - 1)) * (1 if s % 2 else -1) for s in range(1, 12)]       # sizes 0 .. 11, then the extremes of size 11
    diffs += [-2047, 2047, -1024, 1023]
    n = max(len(blocks), len(diffs))
    side = 8 * int(np.ceil(np.sqrt(n)))
    nb = (side // 8) ** 2
    comp = np.zeros((nb, 64), dtype=np.int64)
    dc = 0
    for i in range(nb):
        comp[i] = blocks[i % len(blocks)]
        dc += diffs[i] if i < len(diffs) else 0
        comp[i, 0] = dc
    coef = np.concatenate([comp, comp, comp])
    return encode(side, side, 1, coef)


@functools.lru_cache(maxsize=None)
def restarts(interval):
    """A 4:2:0 128 x 128 file (64 MCUs) with a restart marker every ``interval`` MCUs: MCUs 0, 9, 18, .. are dense, the others almost
    empty, so some segments are far longer than a subsequence and some far shorter."""
    rng = np.random.RandomState(70 + interval)
    hd = jpeg.make_header(128, 128, 3, jpeg.quality_tables(75), interval)
    comps = []
    for c in range(3):
        bw, bh = hd.blocks_w[c], hd.blocks_h[c]
        dense = _sparse(rng, bw * bh, 0.9, 400).reshape(bh, bw, 64)
        thin = _sparse(rng, bw * bh, 0.02, 3).reshape(bh, bw, 64)
        f = hd.h[c]
        my, mx = np.meshgrid(np.arange(bh) // f, np.arange(bw) // f, indexing="ij")
        is_dense = ((my * 8 + mx) % 9 == 0)[:, :, None]
        comps.append(np.where(is_dense, dense, thin).reshape(-1, 64))
    return encode(128, 128, 3, np.concatenate(comps), interval)


@functools.lru_cache(maxsize=None)
def flat_420():
    """A flat 4:2:0 image of 64 x 64: behind the first block of each component, whose DC holds the level, every block is a DC size-0
    code plus EOB - a stream of period 32 bits (4 x 6 luma bits, 2 x 4 chroma bits) on which a speculative decoder, which starts at
    block 0 of an MCU wherever it is put down, locks to the wrong component phase."""
    hd = jpeg.make_header(64, 64, 3, jpeg.quality_tables(75))
    coef = np.zeros(hd.ncoef, dtype=np.int64)
    off = 0
    for c, level in enumerate((-57, 5, 0)):
        coef[off::64][:hd.nblocks[c]] = level
        off += 64 * hd.nblocks[c]
    return encode(64, 64, 3, coef)


@functools.lru_cache(maxsize=None)
def truncated_scene(cut=100):
    """scene_420 with the last ``cut`` bytes of its scan removed and EOI appended again."""
    data = fx.data(fx.SCENE)
    assert data[-2:] == b"\xff\xd9"
    return data[:-2 - cut] + b"\xff\xd9"


def python_segments(data):
    """The restart segments of a file by a plain walk of its bytes: [(offset in the file, length)], and where the scan starts."""
    p = 2
    while True:
        assert data[p] == 0xFF
        m, ln = data[p + 1], (data[p + 2] << 8) | data[p + 3]
        p += 2 + ln
        if m == 0xDA:
            break
    start, segs, q = p, [], p
    while True:
        if data[q] == 0xFF and data[q + 1] != 0:
            segs.append((p, q - p))
            if 0xD0 <= data[q + 1] <= 0xD7:
                q += 2
                p = q
                continue
            return start, segs
        q += 2 if data[q] == 0xFF else 1
