"""COCO segmentations -> instance masks on the GPU: pycocotools' ``annToMask`` (polygons: rleFrPoly, their union, rleDecode;
RLE dicts: rleFrString, rleDecode) without pycocotools and without a host mask.

``decode_batch(segmentations, sizes)`` decodes any number of annotations into one device buffer and returns it with the
``desc`` table ``ep24_ray24`` reads, so ``labels24.rays_from_buffer(buf, desc, centres)`` takes it as it is.
``ann_to_mask(segmentation, h, w)`` is the single-annotation drop-in (numpy out).

The host does O(vertices) numpy work: the integer vertices ``(int)(5 * x + .5)``, every edge's number of dense points
``max(|dx|, |dy|) + 1`` and their prefix sums.  The dense points, the boundary points among them and the pixels are the
kernels' (csrc/cocomask.hip).  An annotation's polygons go in rounds of 7 (one mask bit each, bit 7 carries the union of
the earlier rounds).  Compressed RLE strings are parsed into run lengths here; the runs are decoded on the GPU.
"""
from itertools import chain

import numpy as np
import torch

from . import _lib
from ._lib import call, ptr, stream_ptr

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
