"""Numpy restatement of the tracking contract (include/ep24.h section T1: ``ep24_track_cost`` / ``ep24_track_step``), written
from the header and independently of the kernels.

* the IoU matrix: ``poly24_oracle.poly24_iou`` in float64 on the live slots against the eligible rows - it is exactly 0 for pairs
  whose vertex boxes do not overlap, and only the sub-matrix of slots and rows that have such a partner at all is evaluated, which
  keeps the oracle quick;
* the filter: numpy float32, one operation at a time;
* the association: a sorted sequential greedy over the admissible pairs, deliberately not the round form the kernel uses
  (``rounds_match`` restates that one for the equivalence test).
"""
import numpy as np

import poly24_oracle as P

F = np.float32
TENTATIVE, CONFIRMED, LOST = 1, 2, 3


def polygons(q26):
    return P.det_polygons(np.asarray(q26, dtype=np.float32).reshape(-1, 26))


def _boxes(V):
    with np.errstate(all="ignore"):
        nan = np.isnan(V).any((1, 2))
        lo, hi = np.nanmin(np.where(np.isnan(V), np.inf, V), 1), np.nanmax(np.where(np.isnan(V), -np.inf, V), 1)
    return lo.astype(np.float64), hi.astype(np.float64), nan


def iou_matrix(A, B):
    """[G, 24, 2] x [D, 24, 2] fp32 vertices -> [G, D] float64: poly24_iou where the vertex boxes overlap with positive width and
    height or a side has a NaN vertex (then NaN), exactly 0 elsewhere."""
    G, D = len(A), len(B)
    out = np.zeros((G, D))
    if G == 0 or D == 0:
        return out
    alo, ahi, an = _boxes(A)
    blo, bhi, bn = _boxes(B)
    w = np.minimum(ahi[:, None, 0], bhi[None, :, 0]) - np.maximum(alo[:, None, 0], blo[None, :, 0])
    h = np.minimum(ahi[:, None, 1], bhi[None, :, 1]) - np.maximum(alo[:, None, 1], blo[None, :, 1])
    need = ((w > 0) & (h > 0)) | an[:, None] | bn[None, :]
    gi, di = np.nonzero(need.any(1))[0], np.nonzero(need.any(0))[0]
    if len(gi) and len(di):
        sub = P.poly24_iou(A[gi], B[di])
        out[np.ix_(gi, di)] = np.where(need[np.ix_(gi, di)], sub, 0.0)
    return out


def greedy_match(M, thr, slot_ok, row_ok):
    """The sorted sequential greedy: admissible pairs (M > thr, slot and row allowed) in the order (IoU descending, slot
    ascending, row ascending); take the first, remove its slot and row, repeat.  -> {slot: row}"""
    ts, ds = np.nonzero((M > thr) & slot_ok[:, None] & row_ok[None, :])
    order = sorted(zip((-M[ts, ds]).tolist(), ts.tolist(), ds.tolist()))
    got, used = {}, set()
    for _, t, d in order:
        if t in got or d in used:
            continue
        got[t] = d
        used.add(d)
    return got


def rounds_match(M, thr, slot_ok, row_ok):
    """The round form: every unmatched slot takes its best admissible unmatched row (ties: the lower row), every row its best
    slot (ties: the lower slot), mutual choices are matched; until a round matches nothing.  -> ({slot: row}, matching rounds)"""
    T, N = M.shape
    got, used, rounds = {}, set(), 0
    while True:
        adm = (M > thr) & slot_ok[:, None] & row_ok[None, :]
        for t in got:
            adm[t, :] = False
        for d in used:
            adm[:, d] = False
        X = np.where(adm, M, -1.0)
        new = []
        for t in range(T):
            if adm[t].any():
                d = int(np.argmax(X[t]))                                   # the first maximum: the lower row
                if int(np.argmax(X[:, d])) == t:
                    new.append((t, d))
        if not new:
            return got, rounds
        rounds += 1
        for t, d in new:
            got[t] = d
            used.add(d)


class TrackOracle:
    def __init__(self, streams=1, max_tracks=256, max_dets=256, high_thre=0.5, low_thre=0.1, new_thre=0.6, match_thre=0.2,
                 match_low_thre=0.5, max_age=30, min_hits=3, alpha=0.5, beta=0.25, gamma=0.5, class_agnostic=False):
        self.S, self.T, self.N = streams, max_tracks, max_dets
        self.high, self.low, self.new = F(high_thre), F(low_thre), F(new_thre)
        self.match, self.match_low = float(F(match_thre)), float(F(match_low_thre))
        self.max_age, self.min_hits = max_age, min_hits
        self.alpha, self.beta, self.gamma = F(alpha), F(beta), F(gamma)
        self.agnostic = class_agnostic
        self.reset()
        self.margin = np.inf          # the smallest |iou - threshold| over every admissibility decision taken so far
        self.tie_gap = np.inf         # the smallest difference of two admissible IoUs sharing a slot or a row (bit-identical rows apart)
        self.ties = 0                 # exact ties between admissible IoUs sharing a slot or a row

    def reset(self):
        S, T = self.S, self.T
        self.trk_f = np.zeros((S, T, 32), dtype=np.float32)
        self.trk_i = np.zeros((S, T, 8), dtype=np.int32)
        self.hdr = np.zeros((S, 4), dtype=np.int32)
        self.hdr[:, 0] = 1

    # ---- ep24_track_cost -----------------------------------------------------------------------------------
    def cost(self, det, count):
        S, T, N = self.S, self.T, self.N
        det = np.asarray(det, dtype=np.float32)
        iou = np.zeros((S, T, N))
        dscore = np.full((S, N), np.nan, dtype=np.float32)
        for s in range(S):
            n = max(0, min(int(count[s]), N))
            with np.errstate(all="ignore"):
                score = (det[s, :n, 26] * det[s, :n, 27]).astype(np.float32)
                elig = np.nonzero(score >= self.low)[0]
            dscore[s, elig] = score[elig]
            live = np.nonzero(self.trk_i[s, :, 0])[0]
            if not len(live) or not len(elig):
                continue
            f = self.trk_f[s, live]
            q = f[:, :26].copy()
            q[:, 0] = (f[:, 0] + f[:, 26]).astype(np.float32)
            q[:, 1] = (f[:, 1] + f[:, 27]).astype(np.float32)
            M = iou_matrix(polygons(q), polygons(det[s, elig, :26]))
            if not self.agnostic:
                dcls = np.array([int(c) for c in det[s, elig, 28]], dtype=np.int64)
                M = np.where(self.trk_i[s, live, 1][:, None] == dcls[None, :], M, 0.0)
            iou[s][np.ix_(live, elig)] = M
        return iou, dscore

    def _watch(self, M, thr, slot_ok, row_ok, rows26, slots28):
        """Margins of a stage's decisions, for tests/test_track_oracle.py.  Bit-identical rows may tie along a slot; they spawn
        bit-identical tracks, which may tie along a row."""
        sub = np.where(slot_ok[:, None] & row_ok[None, :], M, np.nan)
        with np.errstate(all="ignore"):
            if np.isfinite(sub).any():
                self.margin = min(self.margin, float(np.nanmin(np.abs(sub - thr))))
            adm = sub > thr
        for axis in (0, 1):
            X = adm if axis == 1 else adm.T
            V = sub if axis == 1 else sub.T
            for i in np.nonzero(X.sum(1) > 1)[0]:
                j = np.nonzero(X[i])[0]
                v = V[i, j]
                o = np.argsort(v)
                for a, b in zip(o[:-1], o[1:]):
                    gap = float(v[b] - v[a])
                    if gap == 0.0:
                        self.ties += 1
                    key = rows26 if axis == 1 else slots28                 # along a slot the partners are rows, and the reverse
                    if key[j[a]].tobytes() == key[j[b]].tobytes():
                        continue
                    self.tie_gap = min(self.tie_gap, gap)

    # ---- ep24_track_step -----------------------------------------------------------------------------------
    def step(self, det, count):
        """One frame.  -> dict(iou, dscore, det_track, out_f, out_i, out_count); the tables are updated in place."""
        S, T, N = self.S, self.T, self.N
        det = np.asarray(det, dtype=np.float32)
        iou, dscore = self.cost(det, count)
        det_track = np.zeros((S, N), dtype=np.int32)
        out_f = np.zeros((S, T, 29), dtype=np.float32)
        out_i = np.zeros((S, T, 4), dtype=np.int32)
        out_count = np.zeros(S, dtype=np.int32)
        a, b, g = self.alpha, self.beta, self.gamma
        for s in range(S):
            tf, ti, h, M, sc = self.trk_f[s], self.trk_i[s], self.hdr[s], iou[s], dscore[s]
            with np.errstate(all="ignore"):
                row1 = sc >= self.high
                row2 = ~np.isnan(sc) & ~row1
            live = ti[:, 0] != 0
            self._watch(M, self.match, live, row1, det[s, :, :26], tf[:, :28])
            m1 = greedy_match(M, self.match, live, row1)
            slot2 = live & (ti[:, 2] == CONFIRMED) & (ti[:, 4] == 0)
            for t in m1:
                slot2[t] = False
            self._watch(M, self.match_low, slot2, row2, det[s, :, :26], tf[:, :28])
            m2 = greedy_match(M, self.match_low, slot2, row2)
            match = dict(m1)
            match.update(m2)
            frame = int(h[1]) + 1
            tail = np.zeros((T, 3), dtype=np.float32)
            for t in np.nonzero(live)[0]:
                px, py = F(tf[t, 0] + tf[t, 26]), F(tf[t, 1] + tf[t, 27])
                if t in match:
                    d = match[t]
                    z = det[s, d]
                    with np.errstate(all="ignore"):
                        ex, ey = F(z[0] - px), F(z[1] - py)
                        tf[t, 0] = F(px + F(a * ex))
                        tf[t, 1] = F(py + F(a * ey))
                        tf[t, 26] = F(tf[t, 26] + F(b * ex))
                        tf[t, 27] = F(tf[t, 27] + F(b * ey))
                        r = tf[t, 2:26].copy()
                        tf[t, 2:26] = (r + (g * (z[2:26] - r).astype(np.float32)).astype(np.float32)).astype(np.float32)
                    tf[t, 28] = sc[d]
                    tail[t] = z[26:29]
                    ti[t, 3] += 1
                    ti[t, 4] = 0
                    if ti[t, 2] == LOST or (ti[t, 2] == TENTATIVE and ti[t, 3] >= self.min_hits):
                        ti[t, 2] = CONFIRMED
                    ti[t, 6] = d
                    det_track[s, d] = ti[t, 0]
                else:
                    ti[t, 4] += 1
                    if ti[t, 2] == TENTATIVE or ti[t, 4] > self.max_age:
                        tf[t] = 0
                        ti[t] = 0
                    else:
                        ti[t, 2] = LOST
                        tf[t, 0], tf[t, 1] = px, py
                        ti[t, 6] = -1
            matched_rows = set(match.values())
            with np.errstate(all="ignore"):
                spawn = [d for d in range(N) if row1[d] and d not in matched_rows and sc[d] >= self.new]
            free = [t for t in range(T) if ti[t, 0] == 0]
            born = min(len(spawn), len(free))
            for k in range(born):
                t, d = free[k], spawn[k]
                z = det[s, d]
                tf[t] = 0
                tf[t, :26] = z[:26]
                tf[t, 28] = sc[d]
                tail[t] = z[26:29]
                ti[t] = (int(h[0]) + k, int(z[28]), TENTATIVE if self.min_hits > 1 else CONFIRMED, 1, 0, frame, d, 0)
                det_track[s, d] = ti[t, 0]
            h[0] += born
            h[1] = frame
            h[2] += len(spawn) - born
            h[3] = int((ti[:, 0] != 0).sum())
            m = 0
            for t in range(T):
                if ti[t, 0] != 0 and ti[t, 2] == CONFIRMED and ti[t, 4] == 0:
                    out_f[s, m, :26] = tf[t, :26]
                    out_f[s, m, 26:] = tail[t]
                    out_i[s, m] = (ti[t, 0], ti[t, 6], ti[t, 3], t)
                    m += 1
            out_count[s] = m
        return dict(iou=iou, dscore=dscore, det_track=det_track, out_f=out_f, out_i=out_i, out_count=out_count)
