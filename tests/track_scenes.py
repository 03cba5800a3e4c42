"""Seeded sequences for the tracking tests, built in numpy so that the CPU file (decision margins, what the scenes show) and the
GPU file (tables bit for bit) share them.  ``scene(name)`` -> ``Scene(kw, frames)``: the tracker's keyword arguments and a list of
``(det [S, N, 29] float32, count [S] int32)``, at most 30 frames.  Rows at and beyond ``count`` hold a large, confident object in
the middle of everything: a kernel that read them would not reproduce the oracle."""
import collections
import functools

import numpy as np

import track_oracle as TO

Scene = collections.namedtuple("Scene", ["kw", "frames"])
NAMES = ("edges", "crossing", "occlusion", "byte", "classes", "classes_agnostic", "duplicates", "nan", "tentative", "chain")


def row(cx, cy, r, obj=0.95, conf=0.95, cls=0):
    out = np.zeros(29, dtype=np.float32)
    out[0], out[1] = cx, cy
    out[2:26] = r
    out[26], out[27], out[28] = obj, conf, cls
    return out


def star(rng, cx, cy, r, noise=0.03, **kw):
    """A 24-gon of mean radius r with ``noise`` relative radial noise."""
    return row(cx, cy, r * (1.0 + noise * rng.uniform(-1.0, 1.0, 24)), **kw)


def pack(streams, N):
    """A list (streams) of lists of rows -> (det [S, N, 29], count [S]) with the filler after the rows."""
    S = len(streams)
    det = np.tile(row(50.0, 50.0, 30.0, 0.99, 0.99, 0)[None, None], (S, N, 1))
    count = np.zeros(S, dtype=np.int32)
    for s, rows in enumerate(streams):
        count[s] = len(rows)
        if len(rows):
            det[s, :len(rows)] = np.stack(rows)
    return det, count


def _kw(**over):
    kw = dict(streams=1, max_tracks=64, max_dets=16)
    kw.update(over)
    return kw


def _edges():
    """Counts 0, 1, 2, 63, 64, 65, 129 against T = 128 on a grid of disjoint stars; the 129 rows overflow the table by one.  Stream 1
    runs the counts backwards, stream 2 alternates between nothing and five."""
    rng = np.random.default_rng(11)
    counts = (0, 1, 2, 63, 64, 65, 129)
    base = [star(rng, 40.0 + 60.0 * (i % 12), 40.0 + 60.0 * (i // 12), 20.0) for i in range(129)]
    frames = []
    for f, c in enumerate(counts):
        def jit(i):
            r = base[i].copy()
            r[:2] += rng.uniform(-1.0, 1.0, 2).astype(np.float32)
            r[2:26] *= (1.0 + 0.03 * rng.uniform(-1.0, 1.0, 24)).astype(np.float32)
            return r
        frames.append(pack([[jit(i) for i in range(c)], [jit(i) for i in range(counts[len(counts) - 1 - f])],
                            [jit(i) for i in range(5 if f % 2 else 0)]], 129))
    return Scene(_kw(streams=3, max_tracks=128, max_dets=129), frames)


def _crossing():
    """Two objects of one class pass each other on neighbouring lanes; the rows swap their order half way."""
    rng = np.random.default_rng(12)
    frames = []
    for f in range(24):
        a = star(rng, 60.0 + 8.0 * f, 100.0, 20.0)
        b = star(rng, 244.0 - 8.0 * f, 122.0, 20.0)
        frames.append(pack([[a, b] if f < 12 else [b, a]], 16))
    return Scene(_kw(), frames)


def _occlusion():
    """max_age = 6.  Object a is gone for 5 frames and comes back to its id; object b is gone for 7 and comes back as a new one."""
    rng = np.random.default_rng(13)
    frames = []
    for f in range(22):
        rows = []
        if not 6 <= f < 11:
            rows.append(star(rng, 60.0 + 1.5 * f, 60.0, 18.0))
        if not 6 <= f < 13:
            rows.append(star(rng, 200.0, 60.0 + 1.0 * f, 22.0, cls=3))
        frames.append(pack([rows], 16))
    return Scene(_kw(max_age=6), frames)


def _byte():
    """The score of a confirmed object dips between low and high for three frames (stage 2 keeps it); a low row on its own and a
    row between high and new never spawn; a row below low_thre is not eligible at all."""
    rng = np.random.default_rng(14)
    frames = []
    for f in range(14):
        dip = 6 <= f < 9
        rows = [star(rng, 80.0 + 2.0 * f, 80.0, 20.0, obj=0.6 if dip else 0.95, conf=0.5 if dip else 0.95),
                star(rng, 200.0, 200.0, 15.0, obj=0.6, conf=0.5),              # 0.3: low alone
                star(rng, 300.0, 80.0, 15.0, obj=0.75, conf=0.75),            # 0.5625: above high, below new
                star(rng, 82.0 + 2.0 * f, 82.0, 20.0, obj=0.25, conf=0.25)]   # 0.0625: below low, on top of the object
        frames.append(pack([rows], 16))
    return Scene(_kw(), frames)


def _classes(agnostic):
    """Two objects of different classes, one largely over the other, the rows swapping their order every frame."""
    rng = np.random.default_rng(15)
    frames = []
    for f in range(10):
        a = star(rng, 100.0 + 1.0 * f, 100.0, 20.0, cls=1)
        b = star(rng, 106.0 + 1.0 * f, 103.0, 24.0, cls=2)
        frames.append(pack([[a, b] if f % 2 == 0 else [b, a]], 16))
    return Scene(_kw(class_agnostic=agnostic), frames)


def _duplicates():
    """Every object comes as two bit-identical rows, and stands still: the rows tie exactly, and so do the tracks they spawn."""
    rng = np.random.default_rng(16)
    a, b = star(rng, 70.0, 70.0, 20.0), star(rng, 200.0, 90.0, 25.0, cls=1)
    return Scene(_kw(), [pack([[a, b, a.copy(), b.copy()]], 16) for _ in range(6)])


def _nan():
    """A row with a NaN radius (it spawns a track nothing ever matches), a row with a NaN score (not eligible) and two sane objects,
    one of them under the NaN row."""
    rng = np.random.default_rng(17)
    frames = []
    for f in range(8):
        bad_r = star(rng, 100.0, 100.0, 20.0)
        bad_r[7] = np.nan
        bad_s = star(rng, 102.0, 98.0, 20.0, conf=np.nan)
        rows = [star(rng, 100.0 + 1.0 * f, 100.0, 20.0), bad_s, star(rng, 250.0, 100.0, 18.0, cls=2)]
        if f in (2, 3, 5):
            rows.insert(1, bad_r)
        frames.append(pack([rows], 16))
    return Scene(_kw(), frames)


def _tentative():
    """A detection seen once: its id is spent and not given out again."""
    rng = np.random.default_rng(18)
    frames = []
    for f in range(8):
        rows = [star(rng, 80.0, 80.0, 20.0)]
        if f == 2:
            rows.append(star(rng, 250.0, 80.0, 20.0))
        if f >= 5:
            rows.append(star(rng, 250.0, 200.0, 20.0))
        frames.append(pack([rows], 16))
    return Scene(_kw(), frames)


CHAIN = 20


def chain_positions():
    """40 centres on a line, tracks and detections in turn, the gaps shrinking from 20 to 8.3 px: with circles of radius 20 the IoU
    of neighbours grows strictly along the line."""
    gaps = 20.0 - 0.3 * np.arange(2 * CHAIN - 1)
    return 40.0 + np.concatenate([[0.0], np.cumsum(gaps)])


def _chain():
    """20 overlapping circles stand still for three frames (confirmed), then every detection lands between its track and the next:
    a slot's best row is the one to its right, a row's best slot the one to its right, so mutual best resolves one pair per round,
    from the far end."""
    x = chain_positions()
    still = [row(x[2 * j], 100.0, 20.0) for j in range(CHAIN)]
    moved = [row(x[2 * j + 1], 100.0, 20.0) for j in range(CHAIN)]
    return Scene(_kw(max_dets=32), [pack([still], 32)] * 3 + [pack([moved], 32)])


@functools.lru_cache(maxsize=None)
def scene(name):
    return {"edges": _edges, "crossing": _crossing, "occlusion": _occlusion, "byte": _byte, "classes": lambda: _classes(False),
            "classes_agnostic": lambda: _classes(True), "duplicates": _duplicates, "nan": _nan, "tentative": _tentative,
            "chain": _chain}[name]()


@functools.lru_cache(maxsize=None)
def replay(name):
    """The oracle's run of a scene, computed once and shared: (oracle after the last frame, per frame a dict of the outputs plus
    copies of the tables ``trk_f``, ``trk_i``, ``hdr`` after that frame).  Nobody changes it."""
    sc = scene(name)
    o = TO.TrackOracle(**sc.kw)
    out = []
    for det, count in sc.frames:
        r = o.step(det, count)
        r.update(trk_f=o.trk_f.copy(), trk_i=o.trk_i.copy(), hdr=o.hdr.copy())
        out.append(r)
    return o, out
