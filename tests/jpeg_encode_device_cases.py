"""Coefficient arrays for the device entropy encoder's tests (test_jpeg_encode_device_host.py, test_gpu_jpeg_encode_device.py): seeded
arrays at baseline's limits and crafted arrays at the smallest shapes at which the count / emit / stuff passes can still go wrong.
Built once per process and read-only; the expected bytes always come from ``ep24.jpeg.entropy_encode`` (the serial host writer)."""
import functools

import numpy as np

from ep24 import jpeg

ZIGZAG = [0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28, 35, 42, 49,
          56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63]
MODES = {0: "grey", 1: "4:4:4", 2: "4:2:2", 3: "4:2:0"}
INTERVALS = (0, 1, 5, 1000)                               # none, every MCU, a few, beyond the MCU count of a 37 x 21 image
T, CHUNK, ROUND = jpeg.EMIT_TILE, jpeg.STUFF_CHUNK, jpeg.STUFF_TILE


def blank(h, w, mode, ri=0, q=75):
    hd = jpeg.make_header(h, w, mode, jpeg.quality_tables(q), ri)
    return jpeg.JpegCoefficients(hd, np.zeros(hd.ncoef, dtype=np.int16))


def _done(it):
    it.coef.setflags(write=False)
    return it


@functools.lru_cache(maxsize=None)
def seeded(mode, ri):
    """Four arrays on 37 x 21 (more than one MCU row, dummy blocks at 4:2:2 and 4:2:0): DC differences up to +-2047 with every AC at
    +-1023; zero runs of 15, 16, 31 and 62 in front of one coefficient, a run to the end and an empty block; values whose bits are all
    ones (streams rich in FF); all zero."""
    rs = np.random.RandomState(100 + 10 * mode + INTERVALS.index(ri))
    out = []
    it = blank(21, 37, mode, ri)
    b = it.coef.reshape(-1, 64)
    b[:, 0] = np.where(rs.randint(0, 2, len(b)) == 1, 1023, -1024)
    b[:, 1:] = np.where(rs.randint(0, 2, (len(b), 63)) == 1, 1023, -1023)
    out.append(_done(it))
    it = blank(21, 37, mode, ri)
    b = it.coef.reshape(-1, 64)
    for i, run in zip(range(len(b)), [15, 16, 31, 62, None, 47, 0] * len(b)):
        b[i, 0] = rs.randint(-1024, 1024)
        if run is not None:                               # None: an empty block; 47: a run in front of coefficient 48, then a run to the end
            b[i, ZIGZAG[1 + run]] = rs.choice([1, -1, 1023, -700])
    out.append(_done(it))
    it = blank(21, 37, mode, ri)
    b = it.coef.reshape(-1, 64)
    b[:, 1:] = (1 << rs.randint(1, 11, (len(b), 63))) - 1
    b[:, 0] = np.where(np.arange(len(b)) % 2 == 1, 1023, 0)
    out.append(_done(it))
    out.append(_done(blank(21, 37, mode, ri)))
    return tuple(out)


def segments(data):
    """The UNSTUFFED bytes of every restart segment of a file this project wrote: what the emit pass leaves in its words."""
    at = data.index(b"\xff\xda")
    body = data[at + 2 + (data[at + 2] << 8 | data[at + 3]):-2]
    out, cur, i = [], bytearray(), 0
    while i < len(body):
        if body[i] == 0xFF and body[i + 1] != 0:
            assert 0xD0 <= body[i + 1] <= 0xD7
            out.append(bytes(cur))
            cur = bytearray()
        else:
            cur.append(body[i])
        i += 2 if body[i] == 0xFF else 1
    out.append(bytes(cur))
    return out


def ff_blocks(seed, nblocks=4, ri=0):
    """A one-component image of ``nblocks`` blocks in a row whose AC values have all their bits set and whose last coefficient is 1023."""
    rs = np.random.RandomState(seed)
    it = blank(8, 8 * nblocks, 0, ri)
    b = it.coef.reshape(-1, 64)
    b[:, 1:] = (1 << rs.randint(1, 11, (nblocks, 63))) - 1
    b[:, 0] = rs.randint(-3, 4, nblocks)
    b[-1, 63] = 1023
    return _done(it)


def ff_runs(dc, nblocks=4):
    """Blocks that code (run 15, size 10) = 1111111111111110 and the value 1023 three times over: 25 ones in a row between the zeros of
    two codes, which hold three FF bytes where they start on (or one bit in front of) a byte.  ``dc``, the first block's DC value, shifts
    the alignment."""
    it = blank(8, 8 * nblocks, 0)
    b = it.coef.reshape(-1, 64)
    for k in (16, 32, 48):
        b[:, ZIGZAG[k]] = 1023
    b[:, 0] = dc
    b[-1, 63] = 1023
    return _done(it)


# where the unstuffed stream of ff_blocks(seed) - for "three": of ff_runs(seed) - holds FF bytes; the first hits of a search over seeds
# 0 .. 999 against entropy_encode, checked again by test_the_ff_seeds_hold_what_they_promise
FF_SEEDS = {"word": 0, "chunk": 1, "three": 0, "padded": 1}


def ff_case(kind, ri=0):
    return ff_runs(FF_SEEDS[kind]) if kind == "three" else ff_blocks(FF_SEEDS[kind], 4, ri)


def ff_property(kind, it):
    seg = segments(jpeg.entropy_encode(it))[0]
    ff = [i for i, v in enumerate(seg) if v == 0xFF]
    pair = {i for i in ff if i + 1 in set(ff)}
    if kind == "word":                                    # the last byte of a word and the first of the next
        return any(i % 4 == 3 for i in pair)
    if kind == "chunk":                                   # the last byte of a stuff chunk and the first of the next
        return any(i % CHUNK == CHUNK - 1 for i in pair)
    if kind == "three":
        return any(i + 1 in pair for i in pair)
    if kind == "padded":                                  # the segment's last byte is FF only once its free bits are filled with ones
        return seg[-1] == 0xFF and padded_bits(it) > 0
    raise KeyError(kind)


def padded_bits(it):
    """Bits of 1-padding in the last byte of ff_blocks' one segment.  With -1023 as the last coefficient its ten value bits are zeros, so
    the last byte of the stream is then nothing but the padding: 2^pad - 1."""
    twin = jpeg.JpegCoefficients(it.header, it.coef.copy())
    assert twin.coef[-1] == 1023
    twin.coef[-1] = -1023
    last = segments(jpeg.entropy_encode(twin))[-1][-1]
    assert last in (0, 1, 3, 7, 15, 31, 63, 127), last
    return (last + 1).bit_length() - 1


def empty_luma(nblocks_w, nblocks_h=1, extra=0, ri=0):
    """A one-component image of empty blocks - 6 bits each: DC size 0, EOB, so five or more blocks share a 32-bit word - of which the
    first ``extra`` carry AC coefficient 1 = 1 (3 bits more each)."""
    it = blank(8 * nblocks_h, 8 * nblocks_w, 0, ri)
    it.coef.reshape(-1, 64)[:extra, 1] = 1
    return _done(it)


def max_block(mode):
    """One block of maximum length per component - DC difference +-2047, all 63 AC at +-1023 - between empty blocks, 40 x 24."""
    it = blank(24, 40, mode, 0, 50)
    hd = it.header
    b = it.coef.reshape(-1, 64)
    mid = hd.nblocks[0] // 2
    b[mid, 0] = 2047
    b[mid, 1:] = np.where(np.arange(63) % 2 == 0, 1023, -1023)
    if hd.ncomp == 3:
        for c, first in ((1, hd.nblocks[0]), (2, hd.nblocks[0] + hd.nblocks[1])):
            b[first + 1, 0] = -2047
            b[first + 1, 1:] = np.where(np.arange(63) % 2 == 0, -1023, 1023)
    return _done(it)


@functools.lru_cache(maxsize=None)
def crafted():
    """name -> JpegCoefficients.  Every one is compared with ``entropy_encode``."""
    rs = np.random.RandomState(5)
    out = {"grey_1x1": _done(blank(1, 1, 0))}
    one = blank(1, 1, 0)
    one.coef[0] = -3
    out["grey_1x1_dc"] = _done(one)                        # one block, a scan shorter than one word
    for n in (T - 1, T, T + 1, 2 * T + 1):                 # blocks against the emit tile, in one and in three components
        out["emit_tile_grey_%d" % n] = _done(_noise(blank(8, 8 * n, 0), rs))
    for n in (T // 4 - 1, T // 4, T // 4 + 1):              # 4:2:0 has 6 blocks per MCU, 4:4:4 three: tiles end inside an MCU
        out["emit_tile_420_%d_mcus" % n] = _done(_noise(blank(16, 16 * n, 3), rs))
        out["emit_tile_444_%d_mcus" % n] = _done(_noise(blank(8, 8 * n, 1, ri=7), rs))
    # 84 / 85 / 86 empty blocks are 504 / 510 / 516 bits: 63, 64 and 65 unstuffed bytes against the 64-byte stuff chunk
    for n in (84, 85, 86):
        out["stuff_chunk_%d_bytes" % -(-6 * n // 8)] = empty_luma(n)
    # 340 x 257 empty blocks are 524 280 bits = 65 535 bytes; 2 and 4 blocks with 3 bits more make 65 536 and 65 537: the stuff
    # kernels' round of 1 024 chunks
    for extra in (0, 2, 4):
        out["stuff_round_%d_bytes" % -(-(6 * 340 * 257 + 3 * extra) // 8)] = empty_luma(340, 257, extra)
    for mode in MODES:
        out["max_block_%s" % MODES[mode]] = max_block(mode)
    out["empty_luma_run"] = empty_luma(37)
    out["empty_luma_run_restart_3"] = empty_luma(37, 1, 0, 3)
    out["rst_wraps_420_33x50"] = _done(_noise(blank(33, 50, 3, ri=1), rs))       # 12 segments: RST0 .. RST7, RST0 .. RST2
    out["rst_beyond_420_33x50"] = _done(_noise(blank(33, 50, 3, ri=1000), rs))   # DRI is written and no RST
    for kind in FF_SEEDS:
        out["ff_%s" % kind] = ff_case(kind)
    out["ff_padded_restart_1"] = ff_case("padded", 1)        # a segment per block, each ends on a value whose bits are all ones
    return out


def _noise(it, rs):
    """What a photograph gives: DC within +-100 of its neighbour, a few small AC values in front."""
    b = it.coef.reshape(-1, 64)
    b[:, 0] = rs.randint(-100, 101, len(b))
    for k in range(1, 10):
        b[:, ZIGZAG[k]] = np.where(rs.randint(0, 3, len(b)) == 0, rs.randint(-9, 10, len(b)), 0)
    b[::7, 63] = -1                                        # some blocks end on coefficient 63: no EOB
    return it


def out_of_range(kind):
    """Three items of which item 1 has a DC difference of 2048 (kind "DC") or an AC coefficient of 1024 ("AC")."""
    items = [seeded(3, 0)[1], None, seeded(1, 5)[2]]
    bad = blank(21, 37, 3)
    bad.coef[:] = seeded(3, 0)[1].coef
    if kind == "DC":
        b = bad.coef.reshape(-1, 64)
        b[0, 0], b[1, 0] = -1024, 1024                     # the second luma block of the first MCU: 1024 - (-1024)
    else:
        bad.coef[64 * 5 + 9] = 1024
    items[1] = _done(bad)
    return items
