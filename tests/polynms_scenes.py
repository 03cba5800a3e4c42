"""Seeded prediction tables for the polygon NMS tests, built in numpy so that the CPU file (decision margins) and the GPU file
(keep lists against tests/polynms_oracle.py) see the same scenes.

``ORACLE_SCENES`` lists every (scene, thresholds, options) combination the GPU file compares against the float64 oracle;
tests/test_polynms_oracle.py asserts that each of them stays at least ``MARGIN`` away from every decision.
"""
import functools

import numpy as np

import polynms_oracle as N

A = 512
C = 3
CONF_THRE = 0.3
NMS_THRE = 0.5
MARGIN = 1e-6                       # 1 000 x the established GPU-vs-oracle IoU difference of 1e-9 (tests/test_gpu_poly24.py)


def cluster_image(n, rng, A=A, C=C, nan_row=False):
    """[A, 27 + C] fp32 with exactly n candidates at CONF_THRE on random rows: clusters of jittered copies (and a few exact
    duplicates) of base polygons in a 220 px field, so that neighbours overlap; scores quantised (ties), classes mostly the
    base's.  The other rows score at most 0.1."""
    p = np.zeros((A, 27 + C), np.float32)
    p[:, 0:2] = rng.uniform(20.0, 600.0, (A, 2))
    p[:, 2:26] = rng.uniform(5.0, 30.0, (A, 24))
    p[:, 26] = 0.1
    p[:, 27:] = rng.uniform(0.0, 1.0, (A, C))
    rows = rng.permutation(A)[:n]
    nb = max(1, n // 6)
    bc = rng.uniform(40.0, 260.0, (nb, 2))
    br = rng.uniform(12.0, 30.0, (nb, 1)) * rng.uniform(0.8, 1.2, (nb, 24))
    bcls = rng.integers(0, C, nb)
    prev = None
    for q, a in enumerate(rows):
        k = int(rng.integers(0, nb))
        if prev is not None and q % 11 == 10:
            p[a, :26] = p[prev, :26]                                              # an exact duplicate of the previous candidate
        else:
            p[a, 0:2] = bc[k] + rng.normal(0.0, 4.0, 2)
            p[a, 2:26] = br[k] * (1.0 + rng.normal(0.0, 0.08, 24))
        cls = int(bcls[k]) if rng.uniform() < 0.85 else int(rng.integers(0, C))
        p[a, 26] = rng.integers(8, 21) / 20.0                                    # obj in {0.40, 0.45 .. 1.00}
        p[a, 27:] = 0.05
        p[a, 27 + cls] = 1.0 if rng.uniform() < 0.5 else 0.9
        prev = a
    if nan_row and n:
        p[rows[n // 2], 9] = np.nan                                               # a NaN radius on a row above the threshold
    return p


@functools.lru_cache(maxsize=None)
def scene(name):
    """pred [B, A, 27 + C] fp32 (treat as read-only)."""
    counts, seed, nan_row = SCENES[name]
    rng = np.random.default_rng(seed)
    pred = np.stack([cluster_image(n, rng, nan_row=nan_row) for n in counts])
    pred.setflags(write=False)
    return pred


# name -> (candidates per image, seed, a NaN row in every image).  The counts are the word and wave boundaries of the bit matrix
# and of the scan.
SCENES = {
    "edges_a": ((0, 1, 2, 63, 200), 101, False),
    "edges_b": ((64, 65, 128, 129), 102, False),
    "dense200": ((200,), 103, False),
    "three": ((3,), 104, False),
    "nan": ((40, 70), 105, True),
}

# (scene, class_agnostic, max_candidates) at CONF_THRE / NMS_THRE
ORACLE_SCENES = [
    ("edges_a", False, None), ("edges_a", True, None), ("edges_b", False, None), ("edges_b", True, None),
    ("three", False, None), ("edges_b", False, 64), ("nan", False, None),
]


def counts(name):
    return SCENES[name][0]


@functools.lru_cache(maxsize=None)
def oracle_keep(name, agnostic=False, max_candidates=None):
    """Per image the kept rows in NMS order (tuples), by the float64 oracle."""
    return tuple(tuple(int(a) for a in N.nms_rows(img, C, CONF_THRE, NMS_THRE, agnostic, max_candidates)) for img in scene(name))


def circles(d, r=10.0, n_cols=28):
    """[1, 2, 27 + 1]: two same-class circles of radius r, centres d apart; the first scores 0.9, the second 0.8."""
    p = np.zeros((1, 2, n_cols), np.float32)
    p[0, :, 0] = (100.0, 100.0 + d)
    p[0, :, 1] = 100.0
    p[0, :, 2:26] = r
    p[0, :, 26] = (0.9, 0.8)
    p[0, :, 27] = 1.0
    return p
