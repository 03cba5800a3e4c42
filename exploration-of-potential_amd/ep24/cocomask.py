"""COCO segmentations -> instance masks on the GPU: pycocotools' ``annToMask`` (polygons: rleFrPoly, their union, rleDecode;
RLE dicts: rleFrString, rleDecode) without pycocotools and without a host mask.

``decode_batch(segmentations, sizes)`` decodes any number of annotations into one device buffer and returns it with the
``desc`` table ``ep24_ray24`` reads, so ``labels24.rays_from_buffer(buf, desc, centres)`` takes it as it is.
``ann_to_mask(segmentation, h, w)`` is the single-annotation drop-in (numpy out).

The host does O(vertices) numpy work: the integer vertices ``(int)(5 * x + .5)``, every edge's number of dense points
``max(|dx|, |dy|) + 1`` and their prefix sums.  The dense points, the boundary points among them and the pixels are the
kernels' (csrc/cocomask.hip).  An annotation's polygons go in rounds of 7 (one mask bit each, bit 7 carries the union of
the earlier rounds).  Compressed RLE strings are parsed into run lengths here; the runs are decoded on the GPU.

The other direction, masks -> COCO run lengths (pycocotools' ``rleEncode`` and ``rleToString``; csrc/rle.hip): ``encode(packed)``
for a ``masks.PackedMasks``, ``encode_buffer(buf, desc)`` for the byte buffer ``decode_batch`` returns - together the GPU form of
``frPyObjects`` + ``merge`` - both giving ``RunLengths`` on the device; ``RunLengths.to_coco()`` copies the runs (not the pixels)
to the host and writes the compressed strings there with numpy (``rle_string_from_counts``).
"""
from itertools import chain

import numpy as np
import torch

from . import _lib
from ._lib import Ep24Error, call, ptr, stream_ptr

ROUND = 7                                   # polygons of one annotation per xor / scan round
COORD_LIMIT = float(1 << 20)                # |x|, |y| of a vertex, in pixels


def rle_counts_from_string(s):
    """rleFrString: 5 bits per char of ``ord - 48``, 0x20 = more chars follow, the last char's 0x10 = negative; from the
    fourth count on a count is stored as its difference to the count two before."""
    if isinstance(s, str):
        s = s.encode("ascii")
    cnts, x, k = [], 0, 0
    for ch in s:
        c = ch - 48
        if not 0 <= c < 64:
            raise ValueError("compressed RLE counts hold a character outside '0'..'o'")
        x |= (c & 0x1f) << (5 * k)
        k += 1
        if c & 0x20:
            continue
        if c & 0x10:
            x |= -1 << (5 * k)
        if len(cnts) > 2:
            x += cnts[-2]
        cnts.append(x)
        x, k = 0, 0
    if k:
        raise ValueError("compressed RLE counts end inside a number")
    return cnts


def _descriptors(sizes):
    hw = np.asarray(sizes, dtype=np.int64).reshape(-1, 2)
    if hw.size and hw.min() < 1:
        raise ValueError("image sizes are (h, w) with h, w >= 1")
    H, W = hw[:, 0], hw[:, 1]
    L = np.sqrt(np.power(H, 2) + np.power(W, 2)).astype(np.int64)            # labels24.rays_batch, reference :68
    if (H + W + L >= 32768).any():
        raise ValueError("image too large for the reference's int16 ray coordinates")
    ns = np.ceil((L - 0) / 0.2).astype(np.int64)                             # len(np.arange(0, L, 0.2)), :74
    off = np.concatenate([[0], np.cumsum(H * W)])
    return np.stack([off[:-1], H, W, L, ns, W], 1), int(off[-1])


def _polygon_tables(polys, owner, index):
    """polys: coordinate lists; owner / index: each one's annotation and its position among that annotation's polygons.
    -> edges int32 [ne, 8] sorted by round, start int64 [ne + 1], first edge of every round [rounds + 1]."""
    nv = np.array([len(p) for p in polys], dtype=np.int64)
    if (nv % 2).any():
        raise ValueError("a polygon is a flat list of x, y pairs: odd number of coordinates")
    if (nv == 0).any():
        raise ValueError("a polygon without vertices")
    nv //= 2
    xy = np.array(list(chain.from_iterable(polys)), dtype=np.float64).reshape(-1, 2)
    if not (np.abs(xy) < COORD_LIMIT).all():                                 # also NaN
        raise ValueError("polygon vertices must be finite and below 2^20 in magnitude")
    P = np.trunc(5 * xy + .5).astype(np.int64)                               # (int)(5 * x + .5): toward zero
    first = np.concatenate([[0], np.cumsum(nv)[:-1]])
    poly = np.repeat(np.arange(len(polys)), nv)
    nxt = np.arange(len(P)) + 1
    last = first + nv - 1
    nxt[last] = first                                                        # X[k] = X[0]
    Q = P[nxt]
    length = np.abs(Q - P).max(1) + 1
    e = np.zeros((len(P), 8), dtype=np.int32)
    e[:, 0:2], e[:, 2:4] = P, Q
    e[:, 4] = np.asarray(owner)[poly]
    idx = np.asarray(index)[poly]
    e[:, 5] = idx % ROUND
    e[first, 6] = 1
    rnd = idx // ROUND
    order = np.argsort(rnd, kind="stable")                                   # whole polygons, their edges still in order
    start = np.concatenate([[0], np.cumsum(length[order])]).astype(np.int64)
    bounds = np.searchsorted(rnd[order], np.arange(int(rnd.max()) + 2))
    return np.ascontiguousarray(e[order]), start, bounds


def _plan(segmentations, sizes):
    """Everything the launches need, as numpy arrays; raises on a bad argument and touches no GPU."""
    segmentations = list(segmentations)
    desc, nbytes = _descriptors(sizes)
    if len(desc) != len(segmentations):
        raise ValueError("one (h, w) per segmentation")
    polys, owner, index, npoly = [], [], [], np.zeros(len(desc), dtype=np.int64)
    runs, ends, n_ends = [], [], 0
    for i, seg in enumerate(segmentations):
        h, w = int(desc[i, 1]), int(desc[i, 2])
        if isinstance(seg, dict):
            if "size" in seg and tuple(int(v) for v in seg["size"]) != (h, w):
                raise ValueError("the RLE's size is not the image's")
            counts = seg["counts"]
            if isinstance(counts, (str, bytes)):
                counts = rle_counts_from_string(counts)
            counts = np.asarray(counts, dtype=np.int64).reshape(-1)
            if counts.size == 0 or counts.min() < 0 or int(counts.sum()) != h * w:
                raise ValueError("RLE counts must be non-negative and sum to h * w")
            runs.append([i, n_ends, counts.size])
            ends.append(np.cumsum(counts))
            n_ends += counts.size
        else:
            seg = list(seg)
            if not seg:
                raise ValueError("an annotation without polygons")
            polys.extend(seg)
            owner.extend([i] * len(seg))
            index.extend(range(len(seg)))
            npoly[i] = len(seg)
    plan = {"desc": desc, "nbytes": nbytes, "total": (nbytes + 3) // 4 * 4, "rounds": [], "runs": None}
    if polys:
        edges, start, bounds = _polygon_tables(polys, owner, index)
        plan["edges"], plan["start"] = edges, start
        for r in range(len(bounds) - 1):
            ann = np.nonzero(npoly > ROUND * r)[0]
            items = (ann * 2 + (npoly[ann] <= ROUND * (r + 1))).astype(np.int32)
            plan["rounds"].append((int(bounds[r]), int(bounds[r + 1]), items, int(desc[ann, 2].max())))
    if runs:
        runs = np.asarray(runs, dtype=np.int64)
        plan["runs"], plan["ends"] = runs, np.concatenate(ends).astype(np.int64)
        plan["max_w"] = int(desc[runs[:, 0], 2].max())
    return plan


def decode_batch(segmentations, sizes, device="cuda:0", out=None):
    """segmentations: per annotation a list of polygons ``[x0, y0, x1, y1, ...]`` or an RLE dict ``{"size": [h, w],
    "counts": list or compressed string}``; sizes: (h, w) per annotation.  Returns (buf uint8 [bytes], desc int64 [n, 6])
    on the device: mask i is ``buf[desc[i, 0] : desc[i, 0] + h * w].view(h, w)``, values 0 / 1.  The masks follow each
    other without gaps and the buffer is rounded up to 4 bytes.  ``out``: a contiguous uint8 device tensor, 4-byte aligned
    and at least that long, to decode into (its first bytes become ``buf``; nothing beyond them is written)."""
    plan = _plan(segmentations, sizes)
    total = plan["total"]
    if out is not None:
        if out.dtype != torch.uint8 or out.dim() != 1 or not out.is_contiguous() or out.numel() < total or out.data_ptr() % 4:
            raise ValueError("out is a contiguous 4-byte aligned uint8 tensor of at least %d bytes" % total)
    _lib.require_gpu()
    dev = torch.device(device) if out is None else out.device
    buf = torch.zeros(total, dtype=torch.uint8, device=dev) if out is None else out[:total].zero_()
    desc = torch.from_numpy(plan["desc"]).to(dev)
    if total == 0:
        return buf, desc
    if plan["rounds"]:
        edges, start = torch.from_numpy(plan["edges"]).to(dev), torch.from_numpy(plan["start"]).to(dev)
        for e0, e1, items, max_w in plan["rounds"]:
            npts = int(plan["start"][e1] - plan["start"][e0])
            call("cocomask_poly_xor", ptr(buf), total, ptr(desc), ptr(edges, e0 * 8), ptr(start, e0), e1 - e0, npts, stream_ptr())
            items_t = torch.from_numpy(items).to(dev)
            for lo in range(0, len(items), 65535):
                call("cocomask_poly_scan", ptr(buf), total, ptr(desc), ptr(items_t, lo), min(len(items) - lo, 65535), max_w,
                     stream_ptr())
    if plan["runs"] is not None:
        runs, ends = torch.from_numpy(plan["runs"]).to(dev), torch.from_numpy(plan["ends"]).to(dev)
        for lo in range(0, len(runs), 65535):
            call("cocomask_rle", ptr(buf), total, ptr(desc), ptr(runs, lo * 3), ptr(ends), min(len(runs) - lo, 65535),
                 plan["max_w"], stream_ptr())
    return buf, desc


def ann_to_mask(segmentation, h, w, device="cuda:0"):
    """``COCO.annToMask`` for one annotation's ``segmentation``: uint8 [h, w] of 0 / 1 as a numpy array."""
    buf, _ = decode_batch([segmentation], [(h, w)], device)
    return buf[: h * w].view(h, w).cpu().numpy()


def rle_string_from_counts(counts, offsets=None):
    """rleToString, the inverse of ``rle_counts_from_string``: from the fourth count on the value stored is the difference to
    the count two before; a value goes out 5 bits at a time, lowest first, as ``chr(48 + bits)`` with 0x20 set while more
    follow (for a value whose bit 0x10 is set "more" means the rest is not -1, otherwise not 0).  ``counts``: one mask's run
    lengths -> str.  With ``offsets [n + 1]`` the runs of n masks behind each other (mask i owns ``counts[offsets[i] :
    offsets[i + 1]]``) -> list of n str.  Numpy over all runs of all masks at once: one pass per character position."""
    c = np.asarray(counts, dtype=np.int64).reshape(-1)
    single = offsets is None
    off = np.array([0, c.size], dtype=np.int64) if single else np.asarray(offsets, dtype=np.int64).reshape(-1)
    if off.size < 1 or off[0] != 0 or off[-1] != c.size or (np.diff(off) < 0).any():
        raise ValueError("offsets start at 0, do not decrease and end at len(counts)")
    n = off.size - 1
    first = np.repeat(off[:-1], np.diff(off))
    late = np.flatnonzero(np.arange(c.size) - first > 2)
    x = c.copy()
    x[late] -= c[late - 2]
    chars, lives, alive = [], [], np.ones(c.size, dtype=bool)
    while alive.any():                                                       # at most 13 rounds for an int64, 7 for an int32
        ch = x & 0x1f
        x >>= 5
        more = np.where(ch & 0x10, x != -1, x != 0) & alive
        chars.append(ch + 32 * more + 48)
        lives.append(alive)
        alive = more
    if not chars:
        return "" if single else [""] * n
    live = np.stack(lives, 1)
    text = np.stack(chars, 1)[live].astype(np.uint8).tobytes().decode("ascii")     # row-major: run by run, low bits first
    at = np.concatenate([[0], np.cumsum(live.sum(1))])[off]
    return text if single else [text[at[i]:at[i + 1]] for i in range(n)]


class RunLengths:
    """COCO run lengths of n masks on the device: ``offsets`` int64 ``[n + 1]``, ``counts`` int32 ``[offsets[n]]`` - mask i owns
    ``counts[offsets[i] : offsets[i + 1]]``, column-major runs starting with a run of zeros (rleEncode).  ``size``: ``(H, W)``
    of all masks (``encode``), or a list of ``(h, w)`` per mask (``encode_buffer``); ``sizes`` is always the list."""

    def __init__(self, offsets, counts, size):
        self.offsets, self.counts, self.size = offsets, counts, size

    def __len__(self):
        return int(self.offsets.shape[0]) - 1

    @property
    def sizes(self):
        if isinstance(self.size, tuple):
            return [self.size] * len(self)
        return list(self.size)

    def to_coco(self, compress=True):
        """-> a list of ``{"size": [h, w], "counts": str}`` (pycocotools' compressed form), or lists of ints with
        ``compress=False``.  One device-to-host copy each of ``offsets`` and ``counts`` - runs, not pixels; the strings are
        written on the host by ``rle_string_from_counts``."""
        off, cnt = self.offsets.cpu().numpy(), self.counts.cpu().numpy()
        if compress:
            each = rle_string_from_counts(cnt, off)
        else:
            each = [cnt[off[i]:off[i + 1]].tolist() for i in range(len(off) - 1)]
        return [{"size": [int(h), int(w)], "counts": c} for (h, w), c in zip(self.sizes, each)]


def _check_out(out, n):
    if out is None:
        return
    ok = isinstance(out, (tuple, list)) and len(out) == 2 and all(isinstance(t, torch.Tensor) for t in out)
    if ok:
        o, c = out
        ok = (o.dtype == torch.int64 and c.dtype == torch.int32 and o.dim() == c.dim() == 1 and o.is_contiguous()
              and c.is_contiguous() and o.numel() >= n + 1 and o.device == c.device)
    if not ok:
        raise ValueError("out is (offsets, counts): contiguous int64 [>= %d] and int32 tensors on one device" % (n + 1))


def _encode_packed(bits, tab, n, H, W, ncols, size, out):
    """count, scan, the 8-byte read of offsets[n], emit, counts.  tab None: n masks of H x W; else H, W = the largest."""
    dev, s = bits.device, stream_ptr()
    colcnt = torch.empty(max(ncols, 1), dtype=torch.int32, device=dev)
    offsets = torch.empty(n + 1, dtype=torch.int64, device=dev) if out is None else out[0][:n + 1]
    call("rle_count", ptr(bits), ptr(tab), n, H, W, ptr(colcnt), s)
    call("rle_scan", ptr(colcnt), ptr(tab), n, H, W, ptr(offsets), s)
    total = int(offsets[n:].cpu()[0])                                        # the one read that sizes counts
    if out is None:
        counts = torch.empty(total, dtype=torch.int32, device=dev)
    elif out[1].numel() < total:
        raise Ep24Error("ep24: encode: out's counts hold %d runs, the masks have %d" % (out[1].numel(), total))
    else:
        counts = out[1][:total]
    ends = torch.empty(max(total, 1), dtype=torch.int32, device=dev)
    call("rle_emit", ptr(bits), ptr(tab), n, H, W, ptr(colcnt), ptr(offsets), ptr(ends), total, s)
    call("rle_counts", ptr(ends), ptr(offsets), ptr(tab), n, H, W, total, ptr(counts), s)
    return RunLengths(offsets, counts, size)


def encode(packed, out=None):
    """``masks.PackedMasks`` -> ``RunLengths`` (pycocotools' ``encode`` of the same masks), both tensors on the device.  All
    compute runs as HIP kernels (csrc/rle.hip): transitions counted per column, an ordered scan, positions emitted, differences
    taken.  Between the scan and the emit there is one 8-byte device-to-host read of ``offsets[N]`` to size ``counts``; nothing
    else leaves the device.  ``out = (offsets, counts)``: contiguous int64 ``[>= N + 1]`` and int32 device tensors to write
    into (their first entries become the result; nothing beyond them is written; too few ``counts`` raise ``Ep24Error``)."""
    from .masks import PackedMasks, _size
    if not isinstance(packed, PackedMasks):
        raise IndexError("encode takes PackedMasks, got %s" % type(packed).__name__)
    H, W = _size(packed.size)
    n, b = len(packed), packed.bits
    if tuple(b.shape) != (n, H, (W + 31) // 32) or b.dtype != torch.int32 or not b.is_contiguous():
        raise IndexError("PackedMasks of size %s with bits %s %s" % (packed.size, tuple(b.shape), b.dtype))
    if n * W >= 1 << 40:
        raise Ep24Error("ep24: encode: %d masks of width %d (EP24_E_UNSUPPORTED)" % (n, W))
    _check_out(out, n)
    _lib.require_gpu()
    if not b.is_cuda or (out is not None and out[0].device != b.device):
        raise Ep24Error("ep24: encode takes GPU tensors on one device (no CPU fallback on the product path)")
    return _encode_packed(b, None, n, H, W, n * W, (H, W), out)


def encode_buffer(buf, desc, out=None):
    """The byte masks of ``decode_batch`` (``buf`` uint8 device buffer, ``desc [n, 6]`` = byte offset, h, w, ., ., row
    stride) -> ``RunLengths`` whose ``size`` is the list of (h, w) per mask; ``encode_buffer(*decode_batch(segs, sizes))`` is
    pycocotools' ``frPyObjects`` + ``merge``.  The masks are first packed per descriptor into ragged bit rows by a kernel, so
    the run kernels have one input form; ``desc`` is read on the host (n rows) for the sizes.  ``out`` as for ``encode``."""
    d = desc.cpu().numpy() if isinstance(desc, torch.Tensor) else np.asarray(desc)
    if d.ndim != 2 or d.shape[1] != 6:
        raise ValueError("desc is [n, 6]: byte offset, h, w, L, ray samples, row stride")
    d = d.astype(np.int64)
    if not isinstance(buf, torch.Tensor) or buf.dtype != torch.uint8 or buf.dim() != 1 or not buf.is_contiguous():
        raise ValueError("buf is a contiguous 1-d uint8 tensor")
    n = len(d)
    off, H, W, ld = d[:, 0], d[:, 1], d[:, 2], d[:, 5]
    if n and (H.min() < 1 or W.min() < 1 or (H * W).max() >= 1 << 31 or (ld < W).any() or off.min() < 0
              or (off + (H - 1) * ld + W).max() > buf.numel()):
        raise ValueError("desc names a mask outside the buffer, or h, w < 1, h * w >= 2^31, a row stride below w")
    _check_out(out, n)
    _lib.require_gpu()
    if not buf.is_cuda or (out is not None and out[0].device != buf.device):
        raise Ep24Error("ep24: encode_buffer takes GPU tensors on one device (no CPU fallback on the product path)")
    dev = buf.device
    sizes = [(int(h), int(w)) for h, w in zip(H, W)]
    if n == 0:
        return _encode_packed(buf, None, 0, 1, 1, 0, sizes, out)
    words = np.concatenate([[0], np.cumsum(H * ((W + 31) // 32))])
    cols = np.concatenate([[0], np.cumsum(W)])
    tab = torch.from_numpy(np.ascontiguousarray(np.stack([words[:-1], H, W, cols[:-1]], 1))).to(dev)
    desc_t = desc.to(dev).contiguous() if isinstance(desc, torch.Tensor) and desc.dtype == torch.int64 else torch.from_numpy(d).to(dev)
    bits = torch.empty(int(words[-1]), dtype=torch.int32, device=dev)
    call("rle_pack_bytes", ptr(buf), buf.numel(), ptr(desc_t), ptr(tab), n, int(H.max()), ptr(bits), stream_ptr())
    return _encode_packed(bits, tab, n, int(H.max()), int(W.max()), int(cols[-1]), sizes, out)
