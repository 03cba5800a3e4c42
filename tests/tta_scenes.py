"""Seeded prediction tables for the polygon voting tests, built in numpy so that the CPU file (margins, scene conditions, the
consensus claim) and the GPU file (``ep24_post_vote_poly24`` against tests/tta_oracle.py) see the same scenes.

``ORACLE_SCENES`` lists every (scene, class_agnostic, max_candidates) combination the GPU file compares against the float64
oracle; tests/test_tta_oracle.py asserts that each of them stays ``MARGIN`` away from every NMS and every voter decision.
"""
import functools

import numpy as np

import polynms_scenes as S
import tta_oracle as T

A = S.A
C = S.C
CONF_THRE = S.CONF_THRE
NMS_THRE = S.NMS_THRE
VOTE_THRE = 0.45                    # below NMS_THRE: a kept row may also hear other kept rows, ranked before it or after
MARGIN = S.MARGIN

# name -> (candidates per image, seed).  The counts are the word and wave boundaries of the voter mask.
CLUSTER_SCENES = {
    "edges": ((0, 1, 2, 63, 64, 65, 129), 211),
    "dense200": ((200,), 212),
    "three": ((3,), 321),
}
SIX_SEED = 214
SIX_OBJECTS, SIX_VIEWS = 12, 6


def _theta():
    return np.arange(24, dtype=np.float64) * (15.0 * np.pi / 180.0)


@functools.lru_cache(maxsize=None)
def six_views_truth():
    """(centres [12, 2], radii [12, 24], classes [12]) float64: star polygons on a 4 x 3 grid that do not touch.  The scene shows
    each of them six times with independent radial, centre and score noise."""
    rng = np.random.default_rng(SIX_SEED)
    gx, gy = np.meshgrid(np.arange(4), np.arange(3))
    c = np.stack([70.0 + 120.0 * gx.ravel(), 70.0 + 120.0 * gy.ravel()], 1) + rng.uniform(-8.0, 8.0, (SIX_OBJECTS, 2))
    base = rng.uniform(28.0, 40.0, (SIX_OBJECTS, 1))
    lobes = rng.integers(3, 6, (SIX_OBJECTS, 1))
    phase = rng.uniform(0.0, 2.0 * np.pi, (SIX_OBJECTS, 1))
    r = base * (1.0 + 0.25 * np.sin(lobes * _theta()[None] + phase))
    return c, r, np.arange(SIX_OBJECTS) % C


def _six_views():
    c, r, cls = six_views_truth()
    rng = np.random.default_rng(SIX_SEED + 1)
    p = np.zeros((A, 27 + C), np.float32)
    p[:, 0:2] = rng.uniform(20.0, 480.0, (A, 2))
    p[:, 2:26] = rng.uniform(5.0, 30.0, (A, 24))
    p[:, 26] = 0.1
    p[:, 27:] = rng.uniform(0.0, 1.0, (A, C))
    rows = rng.permutation(A)[:SIX_OBJECTS * SIX_VIEWS]
    for q, a in enumerate(rows):
        o = q % SIX_OBJECTS
        p[a, 0:2] = c[o] + rng.normal(0.0, 1.0, 2)
        p[a, 2:26] = r[o] * (1.0 + rng.normal(0.0, 0.10, 24))
        p[a, 26] = rng.uniform(0.5, 1.0)
        p[a, 27:] = 0.05
        p[a, 27 + cls[o]] = rng.uniform(0.8, 1.0)
    # below the grid, a chain of three circles of radius 20, 8 px apart: the best removes the second (IoU 0.60) and does not reach
    # the third (IoU 0.34), which is kept and hears the second - a voter ranked before its kept row
    for q, a in enumerate(rng.permutation(np.setdiff1d(np.arange(A), rows))[:3]):
        p[a, 0:2] = (200.0 + 8.0 * q, 440.0)
        p[a, 2:26] = 20.0
        p[a, 26] = 0.9 - 0.1 * q
        p[a, 27:] = 0.05
        p[a, 27] = 1.0
    return p[None]


@functools.lru_cache(maxsize=None)
def scene(name):
    """pred [B, A, 27 + C] fp32 (treat as read-only)."""
    if name == "six_views":
        pred = _six_views()
    else:
        counts, seed = CLUSTER_SCENES[name]
        rng = np.random.default_rng(seed)
        pred = np.stack([S.cluster_image(n, rng) for n in counts])
    pred.setflags(write=False)
    return pred


def counts(name):
    return (SIX_OBJECTS * SIX_VIEWS + 3,) if name == "six_views" else CLUSTER_SCENES[name][0]


# (scene, class_agnostic, max_candidates) at CONF_THRE / NMS_THRE / VOTE_THRE
ORACLE_SCENES = [
    ("edges", False, None), ("edges", True, None), ("dense200", False, None), ("dense200", True, None), ("three", False, None),
    ("edges", False, 64), ("six_views", False, None),
]


@functools.lru_cache(maxsize=None)
def oracle_vote(name, agnostic=False, max_candidates=None):
    """Per image (keep rows, voted [n, 26], n_voters [n], kept sorted positions, voters' sorted positions, abstentions per ray) by
    the float64 oracle."""
    return tuple(T.vote(img, C, CONF_THRE, NMS_THRE, VOTE_THRE, agnostic, max_candidates, detail=True) for img in scene(name))
