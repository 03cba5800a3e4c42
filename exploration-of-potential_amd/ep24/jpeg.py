"""Baseline JPEG decode and encode, split between host and GPU ("JPEG decode" and "JPEG encode").

    coefs = entropy_decode(bytes)          # host: libep24jpeg.so (marker parser + Huffman), no GPU, no torch.cuda - loader processes
    images = finish([coefs, ...])          # GPU: one upload, ep24_jpeg_idct + ep24_jpeg_color on the current stream, no host sync
    images = decode([bytes, ...])          # both

The result is what libjpeg's default path (Pillow, ``cv2.imread``) gives, bit for bit: uint8 ``[h, w, 3]`` device tensors, BGR by
default (``cv2.imread``'s order, what ``ep24.input.preproc_batch`` is fed), RGB with ``bgr=False``.  Progressive, arithmetic-coded,
12-bit and four-component files, other samplings than 4:4:4 / 4:2:2 / 4:2:0, several scans and sides above 8192 raise ``JpegError``
with ``code == EP24_E_UNSUPPORTED``; corrupt files raise it with ``EP24JPEG_E_DATA``.

The Huffman stage can run on the GPU as well ("JPEG decode: Huffman stage on the GPU"); a file then travels as its scan bytes:

    item = scan(bytes)                     # host: the marker walk only (ep24jpeg_scan_layout) -> JpegScan, no GPU - loader processes
    images = finish([item, ...])           # GPU: upload, memset, ep24_jpeg_huffman + ep24_jpeg_dc, then the two launches; .status
    images = decode([bytes, ...], entropy="device")       # both, and one read of the status words: corrupt data raises JpegError

The writer mirrors the reader:

    coefs = forward([image, ...])          # GPU: one descriptor upload, ep24_jpeg_sample + ep24_jpeg_fdct, one copy to the host
    data = entropy_encode(coefs[i])        # host: libep24jpeg.so (markers, Annex K Huffman tables, the scan), no GPU
    datas = encode([image, ...])           # both

The writer's Huffman stage can run on the GPU as well ("JPEG encode: Huffman stage on the GPU"); the coefficients then
never leave the device and only the finished scans cross the bus:

    datas = encode([image, ...], entropy="device")        # sample, FDCT, ep24_jpeg_huffenc_count + _emit; header and FF D9 on the host
    datas = entropy_encode_device([coefs, ...])           # the kernels on uploaded coefficients (tests and tools)
    data = encode_emulate(coefs)           # host: the kernels' phases with threads as loops (libep24jpeg.so), no GPU

The files are what libjpeg-turbo's default compress path (Pillow, ``cv2.imwrite``) writes from the same pixels at the same quality
and sampling, byte for byte: baseline, 4:4:4 / 4:2:2 / 4:2:0 or one component, quality 1 .. 100 or explicit tables, optional restart
markers.  Input that is not uint8, not on the GPU or above 8192 a side raises ``JpegError``.  Optimised Huffman tables, progressive
and arithmetic coding and 12-bit samples are out of scope.
"""
import ctypes
import os

import numpy as np

from ._lib import Ep24Error

_HERE = os.path.dirname(os.path.abspath(__file__))
HOST_LIB_PATH = os.environ.get("EP24_JPEG_LIB") or os.path.join(_HERE, "libep24jpeg.so")
EP24_E_ARG, EP24_E_UNSUPPORTED, EP24JPEG_E_DATA = -1, -3, -4
ABI_VERSION = 1


class JpegError(Ep24Error):
    """``code``: the library's return code, ``message``: its text."""

    def __init__(self, code, message):
        super().__init__("ep24.jpeg: %s (%d)" % (message, code))
        self.code, self.message = code, message

    def __reduce__(self):                                 # crosses the loader's process boundary
        return (JpegError, (self.code, self.message))


class _Header(ctypes.Structure):
    _fields_ = [("width", ctypes.c_int32), ("height", ctypes.c_int32), ("ncomp", ctypes.c_int32), ("restart_interval", ctypes.c_int32),
                ("h", ctypes.c_int32 * 3), ("v", ctypes.c_int32 * 3), ("blocks_w", ctypes.c_int32 * 3), ("blocks_h", ctypes.c_int32 * 3),
                ("nblocks", ctypes.c_int64 * 3), ("ncoef", ctypes.c_int64), ("qt", (ctypes.c_uint16 * 64) * 3)]


class JpegHeader:
    """width, height, ncomp (1 or 3), h / v (sampling factors per component), qt (uint16 [ncomp, 64], natural order),
    restart_interval, blocks_w / blocks_h (the MCU-padded block grid per component), nblocks, ncoef.  Ints and numpy arrays only."""
    __slots__ = ("width", "height", "ncomp", "h", "v", "qt", "restart_interval", "blocks_w", "blocks_h", "nblocks", "ncoef")

    def __init__(self, c):
        n = int(c.ncomp)
        self.width, self.height, self.ncomp, self.restart_interval = int(c.width), int(c.height), n, int(c.restart_interval)
        self.h, self.v = [int(x) for x in c.h[:n]], [int(x) for x in c.v[:n]]
        self.blocks_w, self.blocks_h = [int(x) for x in c.blocks_w[:n]], [int(x) for x in c.blocks_h[:n]]
        self.nblocks, self.ncoef = [int(x) for x in c.nblocks[:n]], int(c.ncoef)
        self.qt = np.array([list(c.qt[i]) for i in range(n)], dtype=np.uint16)

    def __getstate__(self):
        return {k: getattr(self, k) for k in self.__slots__}

    def __setstate__(self, st):
        for k, v in st.items():
            setattr(self, k, v)

    @property
    def shape(self):
        return (self.height, self.width, 3)


class JpegCoefficients:
    """One entropy-decoded image: ``header`` and ``coef`` (int16 [ncoef]: component-major, block row-major within a component over
    the MCU-padded grid, 64 per block in natural order, not dequantised).  Pickles; ``shape`` is the decoded image's (h, w, 3)."""
    __slots__ = ("header", "coef", "tag")

    def __init__(self, header, coef, tag=None):
        self.header, self.coef, self.tag = header, coef, tag

    def __getstate__(self):
        # the coefficients (1.6 MB for a 640 x 427 4:4:4 file) travel as a torch tensor where torch is loaded: the DataLoader's
        # queues move tensors through shared memory, a numpy array would be copied through the worker's pipe by the trainer's
        # main thread (measured: 9 - 18 ms per batch of 20 there); any other pickler stores the tensor by value
        import sys
        coef = self.coef
        if "torch" in sys.modules:
            coef = sys.modules["torch"].from_numpy(np.ascontiguousarray(coef))
        return (self.header, coef, self.tag)

    def __setstate__(self, st):
        self.header, coef, self.tag = st
        self.coef = coef if isinstance(coef, np.ndarray) else coef.numpy()

    @property
    def shape(self):
        return self.header.shape


class _HuffSpec(ctypes.Structure):
    _fields_ = [("counts", ctypes.c_uint8 * 16), ("symbols", ctypes.c_uint8 * 256), ("nsymbols", ctypes.c_int32)]


class _ScanInfo(ctypes.Structure):
    _fields_ = [("header", _Header), ("mcus_x", ctypes.c_int32), ("mcus_y", ctypes.c_int32), ("blocks_per_mcu", ctypes.c_int32),
                ("nseg", ctypes.c_int32), ("scan_pos", ctypes.c_int64), ("scan_len", ctypes.c_int64), ("dc", _HuffSpec * 3), ("ac", _HuffSpec * 3)]


SPEC_BYTES = ctypes.sizeof(_HuffSpec)                      # 276: what ep24_jpeg_huffman reads per table
SUBSEQ_SIZES = (16, 32, 64, 128, 256)
SUBSEQ_BYTES, TILE = 128, 1024                            # the device decoder's defaults: bytes per subsequence, subsequences per tile
MAX_SCAN = 1 << 28


class JpegScan:
    """One file whose Huffman coding is still to be undone - on the device (``finish`` / ``decode(entropy="device")``): ``header``,
    ``data`` (uint8: the entropy-coded bytes of the one scan, restart markers included), ``tables`` (uint8 [6, 276]: the DC tables of
    component 0 .. 2, then the AC tables, as the file specifies them: 16 counts, 256 symbols, int32 count) and ``segments`` (int32
    [nseg, 3]: byte offset in ``data``, length, MCUs of every restart segment).  Made by ``scan`` with the host library only.  Pickles
    like JpegCoefficients; ``shape`` is the decoded image's (h, w, 3).  ``source``: a name for error messages (the dataset sets it)."""
    __slots__ = ("header", "data", "tables", "segments", "mcus_x", "mcus_y", "tag", "source")

    def __init__(self, header, data, tables, segments, mcus_x, mcus_y, tag=None, source=None):
        self.header, self.data, self.tables, self.segments = header, data, tables, segments
        self.mcus_x, self.mcus_y, self.tag, self.source = mcus_x, mcus_y, tag, source

    def __getstate__(self):
        import sys
        data = self.data
        if "torch" in sys.modules:                        # through shared memory between processes, as JpegCoefficients.coef
            data = sys.modules["torch"].from_numpy(np.array(data, dtype=np.uint8))
        return (self.header, data, self.tables, self.segments, self.mcus_x, self.mcus_y, self.tag, self.source)

    def __setstate__(self, st):
        self.header, data, self.tables, self.segments, self.mcus_x, self.mcus_y, self.tag, self.source = st
        self.data = data if isinstance(data, np.ndarray) else data.numpy()

    @property
    def shape(self):
        return self.header.shape


class Finished(list):
    """What ``finish`` / ``finish_mixed`` return when the batch held JpegScan items: the list of images, plus ``status`` (int32 device
    tensor, one word per JpegScan item in batch order: 0 or EP24JPEG_E_DATA, valid once the stream has run) and ``status_items``
    ((index in the batch, name) per word)."""
    status = None
    status_items = ()


_host = None


def host_lib():
    """libep24jpeg.so: host code only - loading it does not touch the GPU (and never loads libep24.so)."""
    global _host
    if _host is None:
        if not os.path.exists(HOST_LIB_PATH):
            raise Ep24Error("ep24: %s is missing - build it with `python -c 'import __graft_entry__ as g; g.build()'` (or make -C "
                            "exploration-of-potential_amd/csrc).  There is no Python fallback for the Huffman stage." % HOST_LIB_PATH)
        L = ctypes.CDLL(HOST_LIB_PATH)
        L.ep24jpeg_abi_version.restype = ctypes.c_int
        L.ep24jpeg_last_error.restype = ctypes.c_char_p
        L.ep24jpeg_parse.restype = ctypes.c_int
        L.ep24jpeg_parse.argtypes = [ctypes.c_char_p, ctypes.c_int64, ctypes.POINTER(_Header)]
        L.ep24jpeg_entropy_decode.restype = ctypes.c_int
        L.ep24jpeg_entropy_decode.argtypes = [ctypes.c_char_p, ctypes.c_int64, ctypes.c_void_p, ctypes.c_int64]
        L.ep24jpeg_quality_tables.restype = ctypes.c_int
        L.ep24jpeg_quality_tables.argtypes = [ctypes.c_int, ctypes.c_void_p]
        L.ep24jpeg_encode_bound.restype = ctypes.c_int64
        L.ep24jpeg_encode_bound.argtypes = [ctypes.POINTER(_Header)]
        L.ep24jpeg_entropy_encode.restype = ctypes.c_int
        L.ep24jpeg_entropy_encode.argtypes = [ctypes.POINTER(_Header), ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p, ctypes.c_int64,
                                              ctypes.POINTER(ctypes.c_int64)]
        L.ep24jpeg_scan_layout.restype = ctypes.c_int
        L.ep24jpeg_scan_layout.argtypes = [ctypes.c_char_p, ctypes.c_int64, ctypes.POINTER(_ScanInfo), ctypes.c_void_p, ctypes.c_int64]
        L.ep24jpeg_selfsync_emulate.restype = ctypes.c_int
        L.ep24jpeg_selfsync_emulate.argtypes = [ctypes.c_char_p, ctypes.c_int64, ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_int64,
                                                ctypes.POINTER(ctypes.c_int32)]
        L.ep24jpeg_encode_header.restype = ctypes.c_int
        L.ep24jpeg_encode_header.argtypes = [ctypes.POINTER(_Header), ctypes.c_void_p, ctypes.c_int64, ctypes.POINTER(ctypes.c_int64)]
        L.ep24jpeg_encode_emulate.restype = ctypes.c_int
        L.ep24jpeg_encode_emulate.argtypes = [ctypes.POINTER(_Header), ctypes.c_void_p, ctypes.c_int64, ctypes.c_int, ctypes.c_void_p,
                                              ctypes.c_int64, ctypes.POINTER(ctypes.c_int64)]
        if L.ep24jpeg_abi_version() != ABI_VERSION:
            raise Ep24Error("ep24: %s reports ABI version %d, ep24.jpeg expects %d - rebuild the library" %
                            (HOST_LIB_PATH, L.ep24jpeg_abi_version(), ABI_VERSION))
        _host = L
    return _host


def _raise(L, rc):
    raise JpegError(rc, L.ep24jpeg_last_error().decode("utf-8", "replace"))


def _bytes(data):
    return data if isinstance(data, bytes) else bytes(data)


def parse(data):
    """-> JpegHeader of a JPEG file given as bytes (markers up to the scan)."""
    L, data, c = host_lib(), _bytes(data), _Header()
    rc = L.ep24jpeg_parse(data, len(data), ctypes.byref(c))
    if rc:
        _raise(L, rc)
    return JpegHeader(c)


def entropy_decode(data, tag=None):
    """-> JpegCoefficients: the host half (parser + Huffman decoder).  Uses the host library only."""
    L, data = host_lib(), _bytes(data)
    hd = parse(data)
    coef = np.empty(hd.ncoef, dtype=np.int16)
    rc = L.ep24jpeg_entropy_decode(data, len(data), coef.ctypes.data, coef.size)
    if rc:
        _raise(L, rc)
    return JpegCoefficients(hd, coef, tag)


def scan(data, tag=None):
    """-> JpegScan: the markers walked, no Huffman work (``ep24jpeg_scan_layout``).  Refuses what ``entropy_decode`` refuses in front of
    the first coded bit, and a restart marker that is missing or out of sequence.  Uses the host library only."""
    L, data, info = host_lib(), _bytes(data), _ScanInfo()
    rc = L.ep24jpeg_scan_layout(data, len(data), ctypes.byref(info), None, 0)
    if rc:
        _raise(L, rc)
    segs = np.empty((int(info.nseg), 3), dtype=np.int64)
    rc = L.ep24jpeg_scan_layout(data, len(data), ctypes.byref(info), segs.ctypes.data, segs.shape[0])
    if rc:
        _raise(L, rc)
    if info.scan_len >= MAX_SCAN:
        raise JpegError(EP24_E_UNSUPPORTED, "scan: a scan of %d bytes is above the device decoder's %d" % (info.scan_len, MAX_SCAN))
    tables = np.frombuffer(bytes(info.dc) + bytes(info.ac), dtype=np.uint8).reshape(6, SPEC_BYTES)
    body = np.frombuffer(data, dtype=np.uint8, count=int(info.scan_len), offset=int(info.scan_pos))
    return JpegScan(JpegHeader(info.header), body, tables, segs.astype(np.int32), int(info.mcus_x), int(info.mcus_y), tag)


def selfsync_emulate(data, subseq_bytes=SUBSEQ_BYTES, tile=TILE):
    """The device decoder's phases on the host (``ep24jpeg_selfsync_emulate``) -> (JpegCoefficients, the largest number of rounds a
    tile needed).  For tests and tools; uses the host library only."""
    L, data = host_lib(), _bytes(data)
    hd = parse(data)
    coef = np.empty(hd.ncoef, dtype=np.int16)
    rounds = ctypes.c_int32(0)
    rc = L.ep24jpeg_selfsync_emulate(data, len(data), int(subseq_bytes), int(tile), coef.ctypes.data, coef.size, ctypes.byref(rounds))
    if rc:
        _raise(L, rc)
    return JpegCoefficients(hd, coef), int(rounds.value)


def _mode(hd):
    if hd.ncomp == 1:
        return 0
    return {(1, 1): 1, (2, 1): 2, (2, 2): 3}[(hd.h[0], hd.v[0])]


def _check(it):
    """The descriptors are built from these fields: what the kernels index with must agree with what the arrays hold."""
    hd = it.header
    if hd.ncomp not in (1, 3) or len(hd.h) != hd.ncomp or not 1 <= hd.width <= 8192 or not 1 <= hd.height <= 8192:
        raise JpegError(EP24_E_ARG, "finish: inconsistent header (%d components, %d x %d)" % (hd.ncomp, hd.width, hd.height))
    hmax, vmax = max(hd.h), max(hd.v)
    if hd.ncomp == 3 and ((hd.h[0], hd.v[0]) not in ((1, 1), (2, 1), (2, 2)) or list(hd.h[1:]) != [1, 1] or list(hd.v[1:]) != [1, 1]):
        raise JpegError(EP24_E_UNSUPPORTED, "finish: sampling %s x %s" % (hd.h, hd.v))
    mx, my = -(-hd.width // (8 * hmax)), -(-hd.height // (8 * vmax))
    for c in range(hd.ncomp):
        if hd.blocks_w[c] != mx * hd.h[c] or hd.blocks_h[c] != my * hd.v[c] or hd.nblocks[c] != hd.blocks_w[c] * hd.blocks_h[c]:
            raise JpegError(EP24_E_ARG, "finish: the block grid of component %d does not fit a %d x %d image" % (c, hd.width, hd.height))
    if np.asarray(hd.qt).shape != (hd.ncomp, 64) or np.asarray(hd.qt).dtype != np.uint16:
        raise JpegError(EP24_E_ARG, "finish: the quantisation tables must be uint16 [%d, 64]" % hd.ncomp)
    if isinstance(it, JpegScan):
        _check_scan(it, mx, my)
        return
    coef = it.coef
    if not isinstance(coef, np.ndarray) or coef.dtype != np.int16 or coef.ndim != 1 or coef.size != 64 * sum(hd.nblocks) or coef.size != hd.ncoef:
        raise JpegError(EP24_E_ARG, "finish: the coefficient array does not hold the %d blocks of the header" % sum(hd.nblocks))


def _check_scan(it, mx, my):
    """What ep24_jpeg_huffman indexes with: the segment rows lie inside the bytes and hold the image's MCUs between them."""
    hd, d, sg, tb = it.header, it.data, it.segments, it.tables
    if hd.ncoef != 64 * sum(hd.nblocks) or (it.mcus_x, it.mcus_y) != (mx, my):
        raise JpegError(EP24_E_ARG, "finish: the scan's MCU grid does not fit a %d x %d image" % (hd.width, hd.height))
    if not isinstance(d, np.ndarray) or d.dtype != np.uint8 or d.ndim != 1 or d.size >= MAX_SCAN:
        raise JpegError(EP24_E_ARG, "finish: the scan bytes must be a one-dimensional uint8 array below %d bytes" % MAX_SCAN)
    if not isinstance(tb, np.ndarray) or tb.dtype != np.uint8 or tb.shape != (6, SPEC_BYTES):
        raise JpegError(EP24_E_ARG, "finish: the table specifications must be uint8 [6, %d]" % SPEC_BYTES)
    ok = isinstance(sg, np.ndarray) and sg.dtype == np.int32 and sg.ndim == 2 and sg.shape[1] == 3 and sg.shape[0] >= 1
    if ok:
        off, ln, mc = sg[:, 0].astype(np.int64), sg[:, 1].astype(np.int64), sg[:, 2].astype(np.int64)
        ri = hd.restart_interval
        ok = bool((off >= 0).all() and (ln >= 0).all() and (off + ln <= d.size).all() and (mc >= 1).all() and int(mc.sum()) == mx * my)
        ok = ok and (len(sg) == (-(-mx * my // ri) if ri else 1)) and (not ri or bool((mc[:-1] == ri).all()))
    if not ok:
        raise JpegError(EP24_E_ARG, "finish: the segment table does not fit the scan's %d bytes and %d MCUs" % (d.size, mx * my))


def _al(x, a):
    return -(-x // a) * a


class Packed:
    """A batch ready for upload: ``host`` (uint8: [coefficients | tables | plane descriptors | image descriptors], every part 16-byte
    aligned) and where the parts start; ``blocks`` / ``groups`` (IDCT blocks, 4-pixel groups of the colour kernel), ``out_bytes`` and
    ``shapes`` ((byte offset, h, w) of every image in the output buffer)."""
    __slots__ = ("host", "o_qt", "o_pd", "o_id", "n_qt", "n_planes", "n_images", "blocks", "groups", "out_bytes", "shapes",
                 "n_scan", "scan_items", "host_split", "gap", "dev_size", "o_hd", "o_sg", "n_seg", "o_tb", "o_by", "n_bytes",
                 "subseq_bytes", "tile")

    # With JpegScan items in the batch the DEVICE buffer has a part the host buffer lacks: the coefficients of those items, which the
    # device decodes itself.  The planes of the JpegCoefficients items come first (``host_split`` bytes, uploaded), then the planes of
    # the JpegScan items (``gap`` bytes, zeroed on the stream and filled by ep24_jpeg_huffman + ep24_jpeg_dc), then everything else:
    # device offset = host offset + gap for all that lies behind the coefficients.  The o_* are DEVICE offsets.  Behind the image
    # descriptors: o_hd (int64 [n_scan, 16]), o_sg (int32 [n_seg, 6]), o_tb (uint8 [n_scan, 6, 276]), o_by (the scans, each 16-byte
    # aligned, n_bytes in all), as include/ep24.h describes them.  Without JpegScan items gap is 0 and the two buffers are one.


_staging = {}        # finish()'s host buffer, kept and grown: a fresh 33 MB array per batch costs its page faults again (7.6 against 3.4 ms)


def pack(items, staging=None, subseq_bytes=None, tile=None):
    """The host half of ``finish``: checks every item (JpegCoefficients or JpegScan) and builds the one buffer that is uploaded.
    ``staging``: a dict that keeps the host buffer between calls - ``host`` is then a view of it, valid until the next call with the
    same dict.  ``subseq_bytes`` / ``tile``: the device decoder's subsequence size and threads per workgroup (SUBSEQ_BYTES, TILE)."""
    S, tile = int(subseq_bytes or SUBSEQ_BYTES), int(tile or TILE)
    if S not in SUBSEQ_SIZES or not 64 <= tile <= 1024 or tile % 64:
        raise JpegError(EP24_E_ARG, "pack: subsequences of %d bytes (one of %s) in tiles of %d (a multiple of 64 up to 1024)" % (S, SUBSEQ_SIZES, tile))
    pdesc, idesc, qts, shapes = [], [], [], []
    blocks = groups = out_off = 0
    for it in items:
        _check(it)
    # the planes of the JpegCoefficients items first, then those of the JpegScan items: one upload in front of the part the device fills
    firsts, scan_items = {}, [i for i, it in enumerate(items) if isinstance(it, JpegScan)]
    order = [i for i, it in enumerate(items) if not isinstance(it, JpegScan)] + scan_items
    blocks_c = 0
    for i in order:
        hd = items[i].header
        firsts[i] = []
        for c in range(hd.ncomp):
            firsts[i].append(blocks)
            pdesc.append([blocks, hd.blocks_w[c], len(qts), 0])
            qts.append(hd.qt[c])
            blocks += hd.nblocks[c]
        if not isinstance(items[i], JpegScan):
            blocks_c = blocks
    for i, it in enumerate(items):
        hd, first = it.header, firsts[i]
        H, W, mode = hd.height, hd.width, _mode(hd)
        dw = -(-W // 2) if mode >= 2 else W
        dh = -(-H // 2) if mode == 3 else H
        cb, cr = (first[1], first[2]) if hd.ncomp == 3 else (first[0], first[0])
        idesc.append([groups, out_off, H, W, mode, 64 * first[0], 8 * hd.blocks_w[0], 64 * cb, 64 * cr, 8 * hd.blocks_w[-1], dw, dh])
        # what the colour kernel reads lies inside the planes the IDCT kernel writes
        assert W <= 8 * hd.blocks_w[0] and H <= 8 * hd.blocks_h[0] and dw <= 8 * hd.blocks_w[-1] and dh <= 8 * hd.blocks_h[-1]
        shapes.append((out_off, H, W))
        groups += -(-H * W // 4)
        out_off += _al(H * W * 3, 4)
    pdesc.append([blocks, 0, 0, 0])
    idesc.append([groups] + [0] * 11)
    pd = np.asarray(pdesc, dtype=np.int64).reshape(-1)
    idn = np.asarray(idesc, dtype=np.int64).reshape(-1)
    qt = np.concatenate([np.asarray(q, dtype=np.uint16).reshape(64) for q in qts])
    P = Packed()
    P.o_qt = _al(blocks * 128, 16)
    P.o_pd = _al(P.o_qt + qt.nbytes, 16)
    P.o_id = _al(P.o_pd + pd.nbytes, 16)
    size = P.o_id + idn.nbytes
    P.n_scan, P.scan_items, P.subseq_bytes, P.tile = len(scan_items), scan_items, S, tile
    P.host_split, P.gap = blocks_c * 128, (blocks - blocks_c) * 128
    P.o_hd = P.o_sg = P.o_tb = P.o_by = P.n_seg = P.n_bytes = 0
    if scan_items:
        hdesc, srows, by_off, nseg = [], [], 0, 0
        for i in scan_items:
            it = items[i]
            hd, sg = it.header, it.segments.astype(np.int64)
            nsub = np.maximum(-(-sg[:, 1] // S), 1)
            rows = np.zeros((len(sg), 6), dtype=np.int64)
            rows[:, 0], rows[:, 1], rows[:, 3] = sg[:, 0], sg[:, 1], sg[:, 2]
            rows[1:, 2] = np.cumsum(sg[:-1, 2])
            rows[1:, 4] = np.cumsum(nsub[:-1])
            srows.append(rows.astype(np.int32))
            hdesc.append([by_off, it.data.size, nseg, len(sg), int(nsub.sum()), 64 * (firsts[i][0] - blocks_c), hd.ncoef, hd.ncomp,
                          hd.h[0], hd.v[0], it.mcus_x, it.mcus_y, hd.restart_interval, 0, 0, 0])
            nseg += len(sg)
            by_off += _al(it.data.size, 16)
        hdn = np.asarray(hdesc, dtype=np.int64).reshape(-1)
        sgn = np.concatenate(srows).reshape(-1)
        P.n_seg, P.n_bytes = nseg, max(by_off, 16)
        P.o_hd = _al(size, 16)
        P.o_sg = _al(P.o_hd + hdn.nbytes, 16)
        P.o_tb = _al(P.o_sg + sgn.nbytes, 16)
        P.o_by = _al(P.o_tb + len(scan_items) * 6 * SPEC_BYTES, 16)
        size = P.o_by + P.n_bytes
    P.dev_size = size
    size -= P.gap                                         # the host buffer lacks the coefficients the device decodes itself
    if staging is None:
        host = np.empty(size, dtype=np.uint8)
    else:
        if staging.get("buf") is None or staging["buf"].size < size:
            staging["buf"] = np.empty(size + size // 4, dtype=np.uint8)
        host = staging["buf"][:size]
    p, g = 0, P.gap
    for it in items:
        if not isinstance(it, JpegScan):
            host[p:p + it.coef.nbytes] = it.coef.view(np.uint8)
            p += it.coef.nbytes
    host[P.o_qt - g:P.o_qt - g + qt.nbytes] = qt.view(np.uint8)
    host[P.o_pd - g:P.o_pd - g + pd.nbytes] = pd.view(np.uint8)
    host[P.o_id - g:P.o_id - g + idn.nbytes] = idn.view(np.uint8)
    if scan_items:
        host[P.o_hd - g:P.o_hd - g + hdn.nbytes] = hdn.view(np.uint8)
        host[P.o_sg - g:P.o_sg - g + sgn.nbytes] = sgn.view(np.uint8)
        p = P.o_tb - g
        for i in scan_items:
            host[p:p + 6 * SPEC_BYTES] = items[i].tables.reshape(-1)
            p += 6 * SPEC_BYTES
        p = P.o_by - g
        for i in scan_items:
            d = items[i].data
            host[p:p + d.size] = d
            p += _al(d.size, 16)
    P.host, P.n_qt, P.n_planes, P.n_images = host, len(qts), len(pdesc) - 1, len(items)
    P.blocks, P.groups, P.out_bytes, P.shapes = blocks, groups, out_off, shapes
    return P


def upload(P, dev):
    """``P.host`` -> the device buffer the launches read (uint8 [P.dev_size]) on the current stream: one copy, or - with both kinds of
    items in the batch - one in front of the coefficients the device decodes itself and one behind them."""
    import torch
    # a copy from pageable memory has left the host buffer when the call returns (the runtime stages it), as ep24.input relies on
    # for the temporaries it uploads: the buffer is free for the next batch
    host = torch.from_numpy(P.host)
    if not P.gap:
        return host.to(dev, non_blocking=True)
    buf = torch.empty(P.dev_size, dtype=torch.uint8, device=dev)
    if P.host_split:
        buf[:P.host_split].copy_(host[:P.host_split], non_blocking=True)
    buf[P.host_split + P.gap:].copy_(host[P.host_split:], non_blocking=True)
    return buf


def launch_entropy(P, buf, status):
    """The device Huffman stage of the batch's JpegScan items on the current stream: the memset of their coefficients, ep24_jpeg_huffman,
    ep24_jpeg_dc.  buf: what ``upload`` returned; status: int32 [P.n_scan] on the device."""
    from . import _lib
    if buf.numel() != P.dev_size or status.numel() < P.n_scan:
        raise JpegError(EP24_E_ARG, "launch: buffers smaller than the packed batch needs")
    base, s = buf.data_ptr(), _lib.stream_ptr()
    coef = base + P.host_split
    buf[P.host_split:P.host_split + P.gap].zero_()
    _lib.call("jpeg_huffman", base + P.o_by, P.n_bytes, base + P.o_hd, P.n_scan, base + P.o_sg, P.n_seg, base + P.o_tb, P.subseq_bytes, P.tile,
              coef, P.gap // 2, _lib.ptr(status), s)
    _lib.call("jpeg_dc", base + P.o_hd, P.n_scan, coef, P.gap // 2, _lib.ptr(status), s)


def launch(P, buf, planes, out, bgr=True, status=None):
    """The launches on the current stream.  buf: ``P.host`` on the device (``upload``); planes: uint8 [64 * P.blocks]; out: uint8
    [P.out_bytes]; status: int32 [P.n_scan], needed when the batch holds JpegScan items (three more launches in front)."""
    from . import _lib
    if buf.numel() != P.dev_size or planes.numel() < 64 * P.blocks or out.numel() < P.out_bytes:
        raise JpegError(EP24_E_ARG, "launch: buffers smaller than the packed batch needs")
    if P.n_scan:
        if status is None:
            raise JpegError(EP24_E_ARG, "launch: a batch with JpegScan items needs its status words")
        launch_entropy(P, buf, status)
    base, s = buf.data_ptr(), _lib.stream_ptr()
    _lib.call("jpeg_idct", base, base + P.o_qt, P.n_qt, base + P.o_pd, P.n_planes, P.blocks, _lib.ptr(planes), s)
    _lib.call("jpeg_color", _lib.ptr(planes), base + P.o_id, P.n_images, P.groups, _lib.ptr(out), P.out_bytes, 1 if bgr else 0, s)


def _name(it, i):
    src = getattr(it, "source", None)
    if src is not None:
        return str(src)
    return "item %d" % i if it.tag is None else "item %d (%r)" % (i, it.tag)


def finish(items, device="cuda:0", bgr=True, subseq_bytes=None, tile=None):
    """items: list of JpegCoefficients and / or JpegScan -> list of uint8 [h, w, 3] device tensors (views of one buffer).  One
    concatenated upload (coefficients, tables, descriptors; for JpegScan items their scan bytes instead of coefficients), two launches
    on the current stream - with JpegScan items the memset of their coefficients, ep24_jpeg_huffman and ep24_jpeg_dc in front, and the
    result is a ``Finished`` list that carries their status words.  No host synchronisation."""
    from . import _lib
    _lib.require_gpu()
    items = list(items)
    if not items:
        return []
    import torch
    dev = torch.device(device)
    P = pack(items, _staging, subseq_bytes, tile)
    buf = upload(P, dev)
    planes = torch.empty(P.blocks * 64, dtype=torch.uint8, device=dev)
    out = torch.empty(P.out_bytes, dtype=torch.uint8, device=dev)
    status = torch.empty(P.n_scan, dtype=torch.int32, device=dev) if P.n_scan else None
    launch(P, buf, planes, out, bgr, status)
    # buf and planes go back to the caching allocator on return: it hands a block out again to work of this stream only
    images = [out[o:o + h * w * 3].view(h, w, 3) for o, h, w in P.shapes]
    if not P.n_scan:
        return images
    images = Finished(images)
    images.status, images.status_items = status, [(i, _name(items[i], i)) for i in P.scan_items]
    return images


def check_status(status, status_items):
    """Raises JpegError(EP24JPEG_E_DATA) for the first item whose status word is set.  status: the words on the host (any sequence)."""
    for code, (i, name) in zip([int(c) for c in status], status_items):
        if code:
            raise JpegError(EP24JPEG_E_DATA if code == EP24JPEG_E_DATA else code,
                            "%s: the device decoder found corrupt or truncated entropy-coded data (status %d)" % (name, code))


def entropy_decode_device(datas, device="cuda:0", subseq_bytes=None, tile=None):
    """list of JPEG files as bytes -> list of int16 numpy arrays in ``entropy_decode``'s layout, decoded by ep24_jpeg_huffman +
    ep24_jpeg_dc; the list carries ``status`` (numpy int32, one word per file) and raises nothing for a set word.  For tests and
    tools: it copies the coefficients back, which the product never does."""
    from . import _lib
    _lib.require_gpu()
    items = [d if isinstance(d, JpegScan) else scan(d) for d in datas]
    out = Finished()
    if not items:
        return out
    import torch
    dev = torch.device(device)
    P = pack(items, None, subseq_bytes, tile)
    buf = upload(P, dev)
    status = torch.empty(P.n_scan, dtype=torch.int32, device=dev)
    launch_entropy(P, buf, status)
    flat = buf[:P.gap].cpu().numpy().view(np.int16)
    p = 0
    for it in items:
        out.append(flat[p:p + it.header.ncoef])
        p += it.header.ncoef
    out.status, out.status_items = status.cpu().numpy(), [(i, _name(it, i)) for i, it in enumerate(items)]
    return out


def decode(datas, device="cuda:0", bgr=True, entropy="host"):
    """list of JPEG files as bytes -> list of uint8 [h, w, 3] device tensors.  ``entropy="host"``: ``entropy_decode`` of each, then one
    ``finish``.  ``entropy="device"``: ``scan`` of each, one ``finish`` that undoes the Huffman coding on the GPU too, then ONE read
    of the status words: JpegError(EP24JPEG_E_DATA) names the first corrupt item."""
    if entropy not in ("host", "device"):
        raise JpegError(EP24_E_ARG, "decode: entropy must be 'host' or 'device', got %r" % (entropy,))
    if entropy == "host":
        return finish([entropy_decode(d) for d in datas], device=device, bgr=bgr)
    out = finish([scan(d) for d in datas], device=device, bgr=bgr)
    if out:
        check_status(out.status.cpu().numpy(), out.status_items)
    return list(out)


# ---- the writer ----

SAMPLINGS = {"4:4:4": 1, "4:2:2": 2, "4:2:0": 3}
_LUMA_FACTORS = {0: (1, 1), 1: (1, 1), 2: (2, 1), 3: (2, 2)}
MAX_SIDE = 8192


def quality_tables(q):
    """``jpeg_set_quality``'s scaling of the Annex K tables for quality 1 .. 100 -> uint16 [2, 64] (luminance, chrominance), natural
    order.  Host library only."""
    L = host_lib()
    qt = ((ctypes.c_uint16 * 64) * 2)()
    rc = L.ep24jpeg_quality_tables(int(q), qt)
    if rc:
        _raise(L, rc)
    return np.array([list(qt[0]), list(qt[1])], dtype=np.uint16)


def _tables(quality):
    """``quality`` as an int, or explicit tables [1 .. 3, 64] (natural order; the last row serves the components beyond it)."""
    if isinstance(quality, (int, np.integer)):
        return quality_tables(quality)
    qt = np.asarray(quality)
    if qt.ndim != 2 or qt.shape[1] != 64 or not 1 <= qt.shape[0] <= 3 or qt.dtype.kind not in "iu" or int(qt.min()) < 1 or int(qt.max()) > 255:
        raise JpegError(EP24_E_ARG, "encode: quantisation tables must be integers 1 .. 255 of shape [1 .. 3, 64]")
    return qt.astype(np.uint16)


def _grids(height, width, mode):
    """Per component (h, v, wb, hb, blocks_w, blocks_h): sampling factors, the real block grid and the MCU-padded one."""
    hmax, vmax = _LUMA_FACTORS[mode]
    mx, my = -(-width // (8 * hmax)), -(-height // (8 * vmax))
    out = []
    for c in range(1 if mode == 0 else 3):
        hc, vc = (hmax, vmax) if c == 0 else (1, 1)
        cw, ch = -(-width * hc // hmax), -(-height * vc // vmax)
        out.append((hc, vc, -(-cw // 8), -(-ch // 8), mx * hc, my * vc))
    return out


def make_header(height, width, mode, qt, restart_interval=0):
    """-> JpegHeader of an image to be written: mode 0 one component, 1 4:4:4, 2 4:2:2, 3 4:2:0; qt [1 .. 3, 64] natural order."""
    c = _Header()
    gr = _grids(height, width, mode)
    c.width, c.height, c.ncomp, c.restart_interval, c.ncoef = width, height, len(gr), restart_interval, 0
    for i, (hc, vc, _, _, bw, bh) in enumerate(gr):
        c.h[i], c.v[i], c.blocks_w[i], c.blocks_h[i], c.nblocks[i] = hc, vc, bw, bh, bw * bh
        c.ncoef += 64 * bw * bh
        for k, v in enumerate(qt[min(i, len(qt) - 1)]):
            c.qt[i][k] = int(v)
    return JpegHeader(c)


def _c_header(hd):
    c = _Header()
    n = int(hd.ncomp)
    if n not in (1, 3) or any(len(x) != n for x in (hd.h, hd.v, hd.blocks_w, hd.blocks_h, hd.nblocks)) or np.asarray(hd.qt).shape != (n, 64):
        raise JpegError(EP24_E_ARG, "entropy_encode: inconsistent header (%d components)" % n)
    c.width, c.height, c.ncomp, c.restart_interval, c.ncoef = int(hd.width), int(hd.height), n, int(hd.restart_interval), int(hd.ncoef)
    for i in range(n):
        c.h[i], c.v[i], c.blocks_w[i], c.blocks_h[i], c.nblocks[i] = hd.h[i], hd.v[i], hd.blocks_w[i], hd.blocks_h[i], hd.nblocks[i]
        for k in range(64):
            c.qt[i][k] = int(hd.qt[i][k])
    return c


def _host_encode(coefficients, tile=None):
    L, hd = host_lib(), coefficients.header
    coef = coefficients.coef
    if not isinstance(coef, np.ndarray) or coef.dtype != np.int16 or coef.ndim != 1:
        raise JpegError(EP24_E_ARG, "entropy_encode: the coefficients must be a one-dimensional int16 array")
    coef = np.ascontiguousarray(coef)
    c = _c_header(hd)
    bound = L.ep24jpeg_encode_bound(ctypes.byref(c))
    if bound < 0:
        _raise(L, bound)
    out = np.empty(bound, dtype=np.uint8)                  # untouched pages of it cost nothing
    n = ctypes.c_int64(0)
    if tile is None:
        rc = L.ep24jpeg_entropy_encode(ctypes.byref(c), coef.ctypes.data, coef.size, out.ctypes.data, out.size, ctypes.byref(n))
    else:
        rc = L.ep24jpeg_encode_emulate(ctypes.byref(c), coef.ctypes.data, coef.size, int(tile), out.ctypes.data, out.size, ctypes.byref(n))
    if rc:
        _raise(L, rc)
    return out[:n.value].tobytes()


def entropy_encode(coefficients):
    """JpegCoefficients -> the bytes of a baseline JFIF file: the host half of the writer (markers, the Annex K Huffman tables, the
    interleaved scan with restart markers every ``header.restart_interval`` MCUs).  Uses the host library only."""
    return _host_encode(coefficients)


EMIT_TILE = 256                                           # blocks per workgroup of the device encoder's count and emit kernels
STUFF_CHUNK, STUFF_TILE = 64, 1024                        # unstuffed bytes per item of its stuff passes, items per workgroup round
STATUS_BAD_DC, STATUS_BAD_AC, STATUS_BAD_STORE = 1, 2, 4  # bits of the device encoder's status words (csrc/jpeg_huffenc_core.h)
stats = {"d2h_bytes": 0}                                  # bytes the writer copied from the device so far (tools/jpeg_encode_device_timing.py)


def encode_emulate(coefficients, tile=EMIT_TILE):
    """``entropy_encode`` by the device encoder's phases run on the host (``ep24jpeg_encode_emulate``): count, scan, emit by ORing into
    zeroed words - tiles of ``tile`` blocks last first - and the stuff passes.  For tests and tools; uses the host library only."""
    return _host_encode(coefficients, int(tile))


def encode_header(header):
    """-> the bytes in front of the entropy-coded data: SOI up to and including the SOS header.  Host library only."""
    L, c = host_lib(), _c_header(header)
    out = np.empty(1024, dtype=np.uint8)
    n = ctypes.c_int64(0)
    rc = L.ep24jpeg_encode_header(ctypes.byref(c), out.ctypes.data, out.size, ctypes.byref(n))
    if rc:
        _raise(L, rc)
    return out[:n.value].tobytes()


def _huffenc_desc(headers):
    """image_desc[n + 1][16] of ep24_jpeg_huffenc_count / _emit for images whose planes lie back to back in header order."""
    rows, blocks, segs = [], 0, 0
    for hd in headers:
        mx, my = hd.blocks_w[0] // hd.h[0], hd.blocks_h[0] // hd.v[0]
        first, b = [], blocks
        for c in range(3):
            first.append(b if c < hd.ncomp else 0)
            b += hd.nblocks[c] if c < hd.ncomp else 0
        ri = hd.restart_interval
        rows.append([blocks, segs, hd.ncomp, hd.h[0], hd.v[0], mx, my, ri] + first + [0] * 5)
        blocks, segs = b, segs + (-(-mx * my // ri) if ri else 1)
    rows.append([blocks, segs] + [0] * 14)
    return np.asarray(rows, dtype=np.int64), blocks, segs


def _entropy_device(headers, coef, dev):
    """The device Huffman stage: coef (int16 device tensor: the planes of ``headers`` back to back) -> (the entropy-coded bytes of every
    image, restart markers included, as a list of bytes; the status words as numpy int32).  Two small reads wait for the stream: the
    word totals, from which the word and the output buffer are sized, then the offsets, the status words and the bytes themselves."""
    import torch
    from . import _lib
    desc, blocks, segs = _huffenc_desc(headers)
    n = len(headers)
    if coef.numel() != 64 * blocks:
        raise JpegError(EP24_E_ARG, "encode: the coefficient buffer does not hold the %d blocks of the headers" % blocks)
    with torch.cuda.device(dev):
        d = torch.from_numpy(desc.reshape(-1)).to(dev, non_blocking=True)
        pos = torch.empty(blocks, dtype=torch.int64, device=dev)
        seg = torch.empty(2 * segs, dtype=torch.int64, device=dev)
        sums = torch.empty(4 * n + 2, dtype=torch.int64, device=dev)      # words per image, bytes per image, word_base[n + 1], offsets[n + 1]
        status = torch.zeros(n, dtype=torch.int32, device=dev)
        s, p = _lib.stream_ptr(), sums.data_ptr()
        p_words, p_bytes, p_base, p_off = p, p + 8 * n, p + 16 * n, p + 8 * (3 * n + 1)
        _lib.call("jpeg_huffenc_count", _lib.ptr(coef), coef.numel(), _lib.ptr(d), n, blocks, segs, _lib.ptr(pos), _lib.ptr(seg), p_words,
                  p_base, _lib.ptr(status), s)
        base = sums[2 * n:3 * n + 1].cpu().numpy()          # first read-back: the unstuffed words in front of every image
        nwords = int(base[n])
        words = torch.zeros(max(nwords, 1), dtype=torch.int32, device=dev)
        cap = 8 * nwords + 2 * segs + 16                   # every byte stuffed, a marker per segment
        out = torch.empty(cap, dtype=torch.uint8, device=dev)
        _lib.call("jpeg_huffenc_emit", _lib.ptr(coef), coef.numel(), _lib.ptr(d), n, blocks, segs, _lib.ptr(pos), _lib.ptr(seg), p_base,
                  _lib.ptr(words), nwords, p_bytes, p_off, _lib.ptr(out), cap, _lib.ptr(status), s)
        off = sums[3 * n + 1:].cpu().numpy()                # second read-back: where every image's bytes lie
        st = status.cpu().numpy()
        total = int(off[n])
        flat = out[:min(max(total, 0), cap)].cpu().numpy()
    stats["d2h_bytes"] += base.nbytes + off.nbytes + st.nbytes + flat.nbytes
    if total > cap or (np.diff(off) < 0).any():
        raise JpegError(EP24_E_ARG, "encode: the device encoder's offsets do not fit its output buffer")
    return [flat[int(off[i]):int(off[i + 1])].tobytes() for i in range(n)], st


def _check_encode_status(st):
    for i, code in enumerate(int(c) for c in st):
        if code < 0:
            raise JpegError(EP24_E_ARG, "item %d: the device encoder refused its descriptor (status %d)" % (i, code))
        if code & STATUS_BAD_DC:
            raise JpegError(EP24_E_ARG, "item %d: a DC difference is outside baseline's +-2047 (status %d)" % (i, code))
        if code & STATUS_BAD_AC:
            raise JpegError(EP24_E_ARG, "item %d: an AC coefficient is outside baseline's +-1023 (status %d)" % (i, code))
        if code:
            raise JpegError(EP24_E_ARG, "item %d: the device encoder dropped a store outside its buffers (status %d)" % (i, code))


def _assemble(headers, scans):
    return [encode_header(hd) + sc + b"\xff\xd9" for hd, sc in zip(headers, scans)]


def entropy_encode_device(coefficients, device="cuda:0"):
    """list of JpegCoefficients -> list of files as bytes, equal to ``entropy_encode`` of each: the coefficients are uploaded and coded
    by ep24_jpeg_huffenc_count + ep24_jpeg_huffenc_emit; header and FF D9 are added on the host.  The status words are read once: a DC
    difference outside +-2047 or an AC coefficient outside +-1023 raises JpegError(EP24_E_ARG) that names the item and the kind.  For
    tests and tools: the product's coefficients are on the device already (``encode(entropy="device")``)."""
    from . import _lib
    _lib.require_gpu()
    items = list(coefficients)
    L = host_lib()
    for i, it in enumerate(items):
        coef = it.coef
        if not isinstance(coef, np.ndarray) or coef.dtype != np.int16 or coef.ndim != 1 or coef.size != it.header.ncoef:
            raise JpegError(EP24_E_ARG, "entropy_encode_device: item %d: the coefficients must be the header's %d int16 values" % (i, it.header.ncoef))
        bound = L.ep24jpeg_encode_bound(ctypes.byref(_c_header(it.header)))
        if bound < 0:
            _raise(L, bound)
    if not items:
        return []
    import torch
    dev = torch.device(device)
    coef = torch.from_numpy(np.concatenate([it.coef for it in items])).to(dev)
    headers = [it.header for it in items]
    scans, st = _entropy_device(headers, coef, dev)
    _check_encode_status(st)
    return _assemble(headers, scans)


def forward(images, quality=95, subsampling="4:2:0", bgr=True, restart_interval=0):
    """The GPU half of the writer.  images: uint8 device tensors ``[h, w, 3]`` (BGR by default, as ``decode`` gives them; RGB with
    ``bgr=False``), or ``[h, w]`` / ``[h, w, 1]`` for a one-component file; any sizes up to 8192 a side.  -> list of JpegCoefficients
    whose coefficients equal libjpeg's at these tables.  ``quality``: 1 .. 100, or explicit tables (``_tables``).  One descriptor
    upload, ep24_jpeg_sample + ep24_jpeg_fdct on the current stream, one device-to-host copy.  The pixels are read where they lie:
    a view with a row stride (a crop of a wider tensor) is not copied first (only a tensor whose pixels are not packed is)."""
    headers, coef, _ = _forward_device(images, quality, subsampling, bgr, restart_interval)
    if not headers:
        return []
    flat = coef.cpu().numpy()                              # waits for the stream
    stats["d2h_bytes"] += flat.nbytes
    out, p = [], 0
    for hd in headers:
        out.append(JpegCoefficients(hd, flat[p:p + hd.ncoef]))
        p += hd.ncoef
    return out


def _forward_device(images, quality, subsampling, bgr, restart_interval):
    """``forward`` without its copy -> (headers, the int16 coefficients of all images on the device, the device); ([], None, None)
    for no images."""
    from . import _lib
    images = list(images)
    qt = _tables(quality)
    if subsampling not in SAMPLINGS:
        raise JpegError(EP24_E_ARG, "encode: subsampling %r (one of %s)" % (subsampling, ", ".join(sorted(SAMPLINGS))))
    if not 0 <= int(restart_interval) <= 65535:
        raise JpegError(EP24_E_ARG, "encode: restart interval %r outside 0 .. 65535" % (restart_interval,))
    if not images:
        return [], None, None
    import torch
    srcs = []
    for i, im in enumerate(images):
        if not isinstance(im, torch.Tensor) or im.dtype != torch.uint8:
            raise JpegError(EP24_E_ARG, "encode: image %d is not a uint8 tensor (got %s)" % (i, getattr(im, "dtype", type(im).__name__)))
        if not im.is_cuda:
            raise JpegError(EP24_E_ARG, "encode: image %d is not on the GPU (the arithmetic runs only as HIP kernels)" % i)
        if im.ndim not in (2, 3) or (im.ndim == 3 and im.shape[2] not in (1, 3)) or im.device != images[0].device:
            raise JpegError(EP24_E_ARG, "encode: image %d must be [h, w, 3], [h, w, 1] or [h, w] on one device (got %s)" % (i, tuple(im.shape)))
        h, w = int(im.shape[0]), int(im.shape[1])
        if not (1 <= h <= MAX_SIDE and 1 <= w <= MAX_SIDE):
            raise JpegError(EP24_E_UNSUPPORTED, "encode: image %d is %d x %d: a side must be 1 .. %d" % (i, h, w, MAX_SIDE))
        ch = 1 if im.ndim == 2 else int(im.shape[2])
        packed = (w == 1 or im.stride(1) == ch) and (ch == 1 or im.stride(2) == 1)
        srcs.append((im if packed else im.contiguous(), h, w, 0 if ch == 1 else SAMPLINGS[subsampling]))
    _lib.require_gpu()
    dev = images[0].device
    idesc, pdesc, headers = [], [], []
    groups = blocks = plane_off = 0
    for im, h, w, mode in srcs:
        gr = _grids(h, w, mode)
        idesc.append([groups, im.data_ptr(), im.stride(0) if h > 1 else 0, h, w, mode + (256 if bgr and mode else 0), plane_off, 0])
        for c, (hc, _, wb, hb, bw, bh) in enumerate(gr):
            pdesc.append([blocks, bw, min(c, len(qt) - 1), plane_off, wb, hb, hc, 0])
            blocks += bw * bh
            plane_off += 64 * wb * hb
        groups += 8 * gr[0][2] * gr[0][3] + (8 * gr[1][2] * gr[1][3] if mode else 0)
        headers.append(make_header(h, w, mode, qt, int(restart_interval)))
    idesc.append([groups] + [0] * 7)
    pdesc.append([blocks] + [0] * 7)
    idn, pdn = np.asarray(idesc, dtype=np.int64).reshape(-1), np.asarray(pdesc, dtype=np.int64).reshape(-1)
    o_id = _al(qt.nbytes, 16)
    o_pd = o_id + idn.nbytes
    host = np.zeros(o_pd + pdn.nbytes, dtype=np.uint8)
    host[:qt.nbytes] = np.ascontiguousarray(qt).view(np.uint8).reshape(-1)
    host[o_id:o_pd] = idn.view(np.uint8)
    host[o_pd:] = pdn.view(np.uint8)
    with torch.cuda.device(dev):
        buf = torch.from_numpy(host).to(dev, non_blocking=True)
        planes = torch.empty(plane_off, dtype=torch.uint8, device=dev)
        coef = torch.empty(blocks * 64, dtype=torch.int16, device=dev)
        base, s = buf.data_ptr(), _lib.stream_ptr()
        _lib.call("jpeg_sample", base + o_id, len(srcs), groups, _lib.ptr(planes), plane_off, s)
        _lib.call("jpeg_fdct", _lib.ptr(planes), plane_off, base, len(qt), base + o_pd, len(pdesc) - 1, blocks, _lib.ptr(coef), s)
    # the caching allocator hands the blocks of srcs' packed copies, buf and planes out again to work of this stream only
    return headers, coef, dev


def encode(images, quality=95, subsampling="4:2:0", bgr=True, restart_interval=0, entropy="host"):
    """list of uint8 device images -> list of JPEG files as bytes.  The default is what ``cv2.imwrite`` writes: quality 95 at 4:2:0, BGR
    input.  ``entropy="host"``: one ``forward``, then ``entropy_encode`` of each.  ``entropy="device"``: the coefficients stay on the
    device, ep24_jpeg_huffenc_count + ep24_jpeg_huffenc_emit code them there, and only the finished scans are copied; header and FF D9
    are added on the host.  The same bytes either way."""
    if entropy not in ("host", "device"):
        raise JpegError(EP24_E_ARG, "encode: entropy must be 'host' or 'device', got %r" % (entropy,))
    if entropy == "host":
        return [entropy_encode(c) for c in forward(images, quality, subsampling, bgr, restart_interval)]
    images = list(images)
    if images:
        from . import _lib
        _lib.require_gpu()
    headers, coef, dev = _forward_device(images, quality, subsampling, bgr, restart_interval)
    if not headers:
        return []
    scans, st = _entropy_device(headers, coef, dev)
    _check_encode_status(st)
    return _assemble(headers, scans)


def finish_checked(images, device="cuda:0", bgr=True):
    """``finish_mixed`` for a caller that uses the pixels at once and keeps no status words (the transforms' ``batch``): with JpegScan
    items in the batch it reads their status words - one host synchronisation - and raises JpegError(EP24JPEG_E_DATA) with the item's
    name and the pointer to ``--jpeg-decoder pil``, so that no corrupt file is ever used as pixels.  Only a batch that THIS call
    finishes is checked: a ``Finished`` list that comes in belongs to whoever finished it (``DataPrefetcher`` hands the transform a
    plain list and reads the words itself a step later) and passes without a synchronisation; without JpegScan items this is
    ``finish_mixed``."""
    own = any(isinstance(im, JpegScan) for im in images)
    out = finish_mixed(images, device=device, bgr=bgr)
    if own and isinstance(out, Finished):
        try:
            check_status(out.status.cpu().numpy(), out.status_items)
        except JpegError as e:
            raise JpegError(e.code, "%s - such files can be read with --jpeg-decoder pil (Pillow)" % e.message) from None
        out = list(out)
    return out


def is_coefficients(x):
    return isinstance(x, JpegCoefficients)


def finish_mixed(images, device="cuda:0", bgr=True):
    """A batch in which some (or all, or none) of the images are JpegCoefficients or JpegScan: those are finished in ONE call, the
    others pass.  With JpegScan items the result is a ``Finished`` list: ``status`` and ``status_items`` (indices in THIS batch)."""
    idx = [i for i, im in enumerate(images) if isinstance(im, (JpegCoefficients, JpegScan))]
    if not idx:
        return images
    done = finish([images[i] for i in idx], device=device, bgr=bgr)
    items, images = images, list(images)
    for i, t in zip(idx, done):
        images[i] = t
    if isinstance(done, Finished):
        images = Finished(images)
        images.status, images.status_items = done.status, [(idx[j], _name(items[idx[j]], idx[j])) for j, _ in done.status_items]
    return images
