"""Baseline JPEG decode and encode, split between host and GPU ("JPEG decode" and "JPEG encode").

    coefs = entropy_decode(bytes)          # host: libep24jpeg.so (marker parser + Huffman), no GPU, no torch.cuda - loader processes
    images = finish([coefs, ...])          # GPU: one upload, ep24_jpeg_idct + ep24_jpeg_color on the current stream, no host sync
    images = decode([bytes, ...])          # both

The result is what libjpeg's default path (Pillow, ``cv2.imread``) gives, bit for bit: uint8 ``[h, w, 3]`` device tensors, BGR by
default (``cv2.imread``'s order, what ``ep24.input.preproc_batch`` is fed), RGB with ``bgr=False``.  Progressive, arithmetic-coded,
12-bit and four-component files, other samplings than 4:4:4 / 4:2:2 / 4:2:0, several scans and sides above 8192 raise ``JpegError``
with ``code == EP24_E_UNSUPPORTED``; corrupt files raise it with ``EP24JPEG_E_DATA``.

The writer mirrors the reader:

    coefs = forward([image, ...])          # GPU: one descriptor upload, ep24_jpeg_sample + ep24_jpeg_fdct, one copy to the host
    data = entropy_encode(coefs[i])        # host: libep24jpeg.so (markers, Annex K Huffman tables, the scan), no GPU
    datas = encode([image, ...])           # both

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
    coef = it.coef
    if not isinstance(coef, np.ndarray) or coef.dtype != np.int16 or coef.ndim != 1 or coef.size != 64 * sum(hd.nblocks) or coef.size != hd.ncoef:
        raise JpegError(EP24_E_ARG, "finish: the coefficient array does not hold the %d blocks of the header" % sum(hd.nblocks))
    if np.asarray(hd.qt).shape != (hd.ncomp, 64) or np.asarray(hd.qt).dtype != np.uint16:
        raise JpegError(EP24_E_ARG, "finish: the quantisation tables must be uint16 [%d, 64]" % hd.ncomp)


def _al(x, a):
    return -(-x // a) * a


class Packed:
    """A batch ready for upload: ``host`` (uint8: [coefficients | tables | plane descriptors | image descriptors], every part 16-byte
    aligned) and where the parts start; ``blocks`` / ``groups`` (IDCT blocks, 4-pixel groups of the colour kernel), ``out_bytes`` and
    ``shapes`` ((byte offset, h, w) of every image in the output buffer)."""
    __slots__ = ("host", "o_qt", "o_pd", "o_id", "n_qt", "n_planes", "n_images", "blocks", "groups", "out_bytes", "shapes")


_staging = {}        # finish()'s host buffer, kept and grown: a fresh 33 MB array per batch costs its page faults again (7.6 against 3.4 ms)


def pack(items, staging=None):
    """The host half of ``finish``: checks every item and builds the one buffer that is uploaded.  ``staging``: a dict that keeps the
    host buffer between calls - ``host`` is then a view of it, valid until the next call with the same dict."""
    pdesc, idesc, qts, shapes = [], [], [], []
    blocks = groups = out_off = 0
    for it in items:
        _check(it)
        hd = it.header
        first = []
        for c in range(hd.ncomp):
            first.append(blocks)
            pdesc.append([blocks, hd.blocks_w[c], len(qts), 0])
            qts.append(hd.qt[c])
            blocks += hd.nblocks[c]
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
    if staging is None:
        host = np.empty(size, dtype=np.uint8)
    else:
        if staging.get("buf") is None or staging["buf"].size < size:
            staging["buf"] = np.empty(size + size // 4, dtype=np.uint8)
        host = staging["buf"][:size]
    p = 0
    for it in items:
        host[p:p + it.coef.nbytes] = it.coef.view(np.uint8)
        p += it.coef.nbytes
    host[P.o_qt:P.o_qt + qt.nbytes] = qt.view(np.uint8)
    host[P.o_pd:P.o_pd + pd.nbytes] = pd.view(np.uint8)
    host[P.o_id:P.o_id + idn.nbytes] = idn.view(np.uint8)
    P.host, P.n_qt, P.n_planes, P.n_images = host, len(qts), len(pdesc) - 1, len(items)
    P.blocks, P.groups, P.out_bytes, P.shapes = blocks, groups, out_off, shapes
    return P


def launch(P, buf, planes, out, bgr=True):
    """The two launches on the current stream.  buf: ``P.host`` on the device; planes: uint8 [64 * P.blocks]; out: uint8 [P.out_bytes]."""
    from . import _lib
    if buf.numel() != P.host.size or planes.numel() < 64 * P.blocks or out.numel() < P.out_bytes:
        raise JpegError(EP24_E_ARG, "launch: buffers smaller than the packed batch needs")
    base, s = buf.data_ptr(), _lib.stream_ptr()
    _lib.call("jpeg_idct", base, base + P.o_qt, P.n_qt, base + P.o_pd, P.n_planes, P.blocks, _lib.ptr(planes), s)
    _lib.call("jpeg_color", _lib.ptr(planes), base + P.o_id, P.n_images, P.groups, _lib.ptr(out), P.out_bytes, 1 if bgr else 0, s)


def finish(items, device="cuda:0", bgr=True):
    """items: list of JpegCoefficients -> list of uint8 [h, w, 3] device tensors (views of one buffer).  One concatenated upload
    (coefficients, tables, descriptors), two launches on the current stream, no host synchronisation."""
    from . import _lib
    _lib.require_gpu()
    items = list(items)
    if not items:
        return []
    import torch
    dev = torch.device(device)
    P = pack(items, _staging)
    # a copy from pageable memory has left the host buffer when the call returns (the runtime stages it), as ep24.input relies on
    # for the temporaries it uploads: the buffer is free for the next batch
    buf = torch.from_numpy(P.host).to(dev, non_blocking=True)
    planes = torch.empty(P.blocks * 64, dtype=torch.uint8, device=dev)
    out = torch.empty(P.out_bytes, dtype=torch.uint8, device=dev)
    launch(P, buf, planes, out, bgr)
    # buf and planes go back to the caching allocator on return: it hands a block out again to work of this stream only
    return [out[o:o + h * w * 3].view(h, w, 3) for o, h, w in P.shapes]


def decode(datas, device="cuda:0", bgr=True):
    """list of JPEG files as bytes -> list of uint8 [h, w, 3] device tensors: ``entropy_decode`` of each, then one ``finish``."""
    return finish([entropy_decode(d) for d in datas], device=device, bgr=bgr)


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


def entropy_encode(coefficients):
    """JpegCoefficients -> the bytes of a baseline JFIF file: the host half of the writer (markers, the Annex K Huffman tables, the
    interleaved scan with restart markers every ``header.restart_interval`` MCUs).  Uses the host library only."""
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
    rc = L.ep24jpeg_entropy_encode(ctypes.byref(c), coef.ctypes.data, coef.size, out.ctypes.data, out.size, ctypes.byref(n))
    if rc:
        _raise(L, rc)
    return out[:n.value].tobytes()


def forward(images, quality=95, subsampling="4:2:0", bgr=True, restart_interval=0):
    """The GPU half of the writer.  images: uint8 device tensors ``[h, w, 3]`` (BGR by default, as ``decode`` gives them; RGB with
    ``bgr=False``), or ``[h, w]`` / ``[h, w, 1]`` for a one-component file; any sizes up to 8192 a side.  -> list of JpegCoefficients
    whose coefficients equal libjpeg's at these tables.  ``quality``: 1 .. 100, or explicit tables (``_tables``).  One descriptor
    upload, ep24_jpeg_sample + ep24_jpeg_fdct on the current stream, one device-to-host copy.  The pixels are read where they lie:
    a view with a row stride (a crop of a wider tensor) is not copied first (only a tensor whose pixels are not packed is)."""
    from . import _lib
    images = list(images)
    qt = _tables(quality)
    if subsampling not in SAMPLINGS:
        raise JpegError(EP24_E_ARG, "encode: subsampling %r (one of %s)" % (subsampling, ", ".join(sorted(SAMPLINGS))))
    if not 0 <= int(restart_interval) <= 65535:
        raise JpegError(EP24_E_ARG, "encode: restart interval %r outside 0 .. 65535" % (restart_interval,))
    if not images:
        return []
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
        flat = coef.cpu().numpy()                          # waits for the stream: srcs (and any packed copies) outlive the kernels
    out, p = [], 0
    for hd in headers:
        out.append(JpegCoefficients(hd, flat[p:p + hd.ncoef]))
        p += hd.ncoef
    return out


def encode(images, quality=95, subsampling="4:2:0", bgr=True, restart_interval=0):
    """list of uint8 device images -> list of JPEG files as bytes: one ``forward``, then ``entropy_encode`` of each.  The default is
    what ``cv2.imwrite`` writes: quality 95 at 4:2:0, BGR input."""
    return [entropy_encode(c) for c in forward(images, quality, subsampling, bgr, restart_interval)]


def is_coefficients(x):
    return isinstance(x, JpegCoefficients)


def finish_mixed(images, device="cuda:0", bgr=True):
    """A batch in which some (or all, or none) of the images are JpegCoefficients: those are finished in ONE call, the others pass."""
    idx = [i for i, im in enumerate(images) if isinstance(im, JpegCoefficients)]
    if not idx:
        return images
    done = finish([images[i] for i in idx], device=device, bgr=bgr)
    images = list(images)
    for i, t in zip(idx, done):
        images[i] = t
    return images
