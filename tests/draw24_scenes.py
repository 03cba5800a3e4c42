"""Detection rows for the drawing tests: seeded random objects kept away from float decisions, and the hand-made edge cases."""
import numpy as np

from draw24_oracle import row_geometry, vertex_margin

MARGIN = 1e-3
NAMES3 = ["cat", "traffic light on a pole, far away", "Zq_9%"]      # the second is longer than 21 bytes


def make_row(cx, cy, radii, obj=0.9, cc=0.9, cls=0, ratio=1.0):
    """A ``postprocess`` row whose object sits at (cx, cy) with ``radii`` in IMAGE pixels: stored times the letterbox ratio."""
    row = np.zeros(29, dtype=np.float32)
    row[0], row[1] = np.float32(cx) * np.float32(ratio), np.float32(cy) * np.float32(ratio)
    row[2:26] = np.asarray(radii, dtype=np.float32) * np.float32(ratio)
    row[26], row[27], row[28] = obj, cc, cls
    return row


def random_rows(n, H, W, seed, num_classes=80, rmin=2.0, rmax=9.0, ratio=1.0, conf=0.0, spill=4.0):
    """-> (rows [n, 29] float32, dropped): objects of radius rmin..rmax with centres up to ``spill`` pixels outside the canvas,
    mixed classes and scores.  A drawn row whose float32 vertex values come within MARGIN of an integer is drawn again from the
    same generator and counted in ``dropped``."""
    rng = np.random.default_rng(seed)
    rows, dropped = [], 0
    while len(rows) < n:
        base = rng.uniform(rmin, rmax)
        radii = base * (1.0 + 0.35 * rng.uniform(-1.0, 1.0, 24))
        row = make_row(rng.uniform(-spill, W + spill), rng.uniform(-spill, H + spill), radii, obj=rng.uniform(0.3, 1.0),
                       cc=rng.uniform(0.3, 1.0), cls=int(rng.integers(0, num_classes)), ratio=ratio)
        geo = row_geometry(row, ratio, conf, H, W, num_classes)
        if geo is not None and vertex_margin(geo) < MARGIN:
            dropped += 1
            continue
        rows.append(row)
    return (np.stack(rows) if rows else np.zeros((0, 29), dtype=np.float32)), dropped


def wobble(base):
    return [base + 0.3 * (k % 3) + 0.45 * (k % 5) for k in range(24)]


def edge_rows(H, W, ratio):
    """The edge cases of the contract for ``num_classes = 3`` and ``conf = 0.25``, as (name, row)."""
    r = ratio
    big = wobble(11.0)
    return [
        ("centre outside, partly inside", make_row(-6, 10, big, cls=0, ratio=r)),
        ("centre outside, wholly outside", make_row(-40, -40, wobble(9.0), cls=1, ratio=r)),
        ("all radii zero", make_row(40, 12, [0.0] * 24, cls=2, ratio=r)),
        ("clamped to x = W and y = H", make_row(W - 3, H - 3, wobble(10.0), cls=1, ratio=r)),
        ("score below conf", make_row(60, 16, wobble(7.0), obj=0.5, cc=0.25, cls=0, ratio=r)),
        ("score equal to conf", make_row(70, 18, wobble(6.0), obj=0.5, cc=0.5, cls=1, ratio=r)),
        ("score above conf", make_row(84, 14, wobble(8.0), obj=0.9, cc=0.9, cls=2, ratio=r)),
        ("NaN radius", make_row(50, 20, [np.nan if k == 5 else 6.0 for k in range(24)], cls=0, ratio=r)),
        ("infinite centre", make_row(np.inf, 20, wobble(6.0), cls=0, ratio=r)),
        ("radius at least 2^20", make_row(30, 20, [3.0e6 if k == 7 else 6.0 for k in range(24)], cls=0, ratio=r)),
        ("centre at least 2^20", make_row(20, -2.5e6, wobble(6.0), cls=0, ratio=r)),
        ("class -1", make_row(100, 20, wobble(6.0), cls=-1, ratio=r)),
        ("class 3", make_row(110, 20, wobble(6.0), cls=3, ratio=r)),
        ("overlaps the clamped one", make_row(W - 12, H - 10, wobble(9.0), cls=0, ratio=r)),
    ]


def text_rows(H, W):
    """Labels cut by each side of the canvas: left, right, top, bottom (class 1 of NAMES3 is 21 bytes after the cut)."""
    return np.stack([make_row(-20, H // 2, wobble(3.0), cls=1), make_row(W - 9, H // 2 + 6, wobble(3.0), cls=1),
                     make_row(W // 2, 5, wobble(3.0), cls=2), make_row(W // 3, H + 8, wobble(3.0), cls=0)])
