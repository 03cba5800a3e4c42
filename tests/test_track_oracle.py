"""Tracking without a GPU: the seeded scenes of tests/track_scenes.py through the numpy oracle (tests/track_oracle.py).  Every
admissibility decision stays 1e-6 away from its threshold and from its competitors, so the GPU file may ask for equal tables; the
round form of the association equals the sorted greedy; and the scenes show what their names claim."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import track_oracle as TO  # noqa: E402
import track_scenes as S  # noqa: E402


def test_the_module_under_test_exists():
    from ep24 import track
    assert track.MAX_TRACKS == 1024 and track.MAX_DETS == 4096


@pytest.mark.parametrize("name", S.NAMES)
def test_decisions_keep_their_distance(name):
    sc = S.scene(name)
    assert 1 <= len(sc.frames) <= 30
    o, frames = S.replay(name)
    assert o.margin >= 1e-6, o.margin                       # |iou - threshold| over every pair a stage looked at
    assert o.tie_gap >= 1e-6, o.tie_gap                     # admissible IoUs sharing a slot or a row, bit-identical partners apart
    assert (o.ties > 0) == (name == "duplicates")
    assert sum(int((f["iou"] > 0).sum()) for f in frames) > 0


def test_round_form_equals_the_sorted_greedy():
    rng = np.random.default_rng(5)
    most = 0
    for trial in range(1500):
        T, N = int(rng.integers(1, 9)), int(rng.integers(1, 9))
        M = rng.uniform(0.0, 1.0, (T, N))
        if trial % 2:                                        # exact ties: a few levels only
            M = np.round(M * 4.0) / 4.0
        if trial % 5 == 0:
            M[rng.integers(0, T), rng.integers(0, N)] = np.nan
        slot_ok, row_ok = rng.uniform(size=T) < 0.85, rng.uniform(size=N) < 0.85
        with np.errstate(invalid="ignore"):
            a = TO.greedy_match(M, 0.3, slot_ok, row_ok)
            b, rounds = TO.rounds_match(M, 0.3, slot_ok, row_ok)
        assert a == b, (trial, M)
        assert rounds <= min(T, N)
        most = max(most, rounds)
    assert most >= 3


def _ids(frames, s=0):
    return [f["det_track"][s] for f in frames]


def test_crossing_keeps_both_ids():
    _, frames = S.replay("crossing")
    dt = _ids(frames)
    assert all((d[0], d[1]) == ((1, 2) if f < 12 else (2, 1)) for f, d in enumerate(dt))
    closest = min(float(np.hypot(*(det[0, 0, :2] - det[0, 1, :2]))) for det, _ in S.scene("crossing").frames)
    assert closest < 40.0                                    # they do overlap on the way
    assert frames[-1]["hdr"].tolist() == [[3, 24, 0, 2]]


def test_occlusion_short_gap_keeps_the_id_long_gap_gives_a_new_one():
    _, frames = S.replay("occlusion")
    for f, fr in enumerate(frames):
        live = {int(r[0]): (int(r[2]), int(r[4])) for r in fr["trk_i"][0] if r[0]}
        if 6 <= f < 11:
            assert live[1] == (TO.LOST, f - 5) and fr["out_count"][0] == 0
    assert frames[11]["det_track"][0, 0] == 1                # back after 5 frames: the same id
    assert frames[12]["trk_i"][0, :, 0].tolist().count(2) == 0          # age 7 > max_age 6: freed
    assert frames[13]["det_track"][0, 1] == 3 and frames[-1]["hdr"][0, 0] == 4
    assert frames[-1]["out_i"][0, :2, 0].tolist() == [1, 3]


def test_byte_low_scores_keep_a_track_and_never_start_one():
    _, frames = S.replay("byte")
    for f, fr in enumerate(frames):
        assert fr["det_track"][0, :4].tolist() == [1, 0, 0, 0], f
        assert np.isnan(fr["dscore"][0, 3]) and fr["dscore"][0, 1] == np.float32(0.6) * np.float32(0.5)
    assert frames[7]["trk_i"][0, 0].tolist()[:5] == [1, 0, TO.CONFIRMED, 8, 0]
    assert frames[-1]["hdr"][0, 0] == 2


def test_classes_separate_unless_agnostic():
    _, plain = S.replay("classes")
    _, agn = S.replay("classes_agnostic")
    assert int((plain[3]["iou"][0] > 0).sum()) == 2 and int((agn[3]["iou"][0] > 0).sum()) == 4
    for frames in (plain, agn):
        for f, fr in enumerate(frames):
            assert fr["det_track"][0, :2].tolist() == ([1, 2] if f % 2 == 0 else [2, 1])
        assert frames[-1]["trk_i"][0, :2, 1].tolist() == [1, 2]


def test_duplicates_resolve_by_index():
    _, frames = S.replay("duplicates")
    for fr in frames:
        assert fr["det_track"][0, :4].tolist() == [1, 2, 3, 4]
    assert frames[-1]["out_i"][0, :4].tolist() == [[1, 0, 6, 0], [2, 1, 6, 1], [3, 2, 6, 2], [4, 3, 6, 3]]


def test_nan_rows():
    _, frames = S.replay("nan")
    assert np.isnan(frames[3]["iou"]).any() and np.isnan(frames[2]["trk_f"][0, :, 7]).sum() == 1
    assert [int(fr["det_track"][0, 1]) for fr in frames] == [0, 0, 3, 4, 0, 5, 0, 0]          # spawned, never matched, never kept
    assert all(np.isnan(fr["dscore"][0, 2 if f in (2, 3, 5) else 1]) for f, fr in enumerate(frames))
    assert frames[-1]["out_i"][0, :2, 0].tolist() == [1, 2] and frames[-1]["hdr"].tolist() == [[6, 8, 0, 2]]


def test_tentative_id_is_spent():
    _, frames = S.replay("tentative")
    assert frames[2]["det_track"][0, 1] == 2 and frames[3]["hdr"].tolist() == [[3, 4, 0, 1]]
    assert frames[5]["det_track"][0, 1] == 3 and frames[7]["out_i"][0, :2, 0].tolist() == [1, 3]


def test_chain_needs_a_round_per_pair():
    o, frames = S.replay("chain")
    last = frames[-1]
    M = last["iou"][0]
    live = frames[-2]["trk_i"][0, :, 0] != 0
    rows = ~np.isnan(last["dscore"][0])
    got, rounds = TO.rounds_match(M, o.match, live, rows)
    assert rounds == S.CHAIN and got == {j: j for j in range(S.CHAIN)} == TO.greedy_match(M, o.match, live, rows)
    right = np.array([M[j + 1, j] for j in range(S.CHAIN - 1)])
    own = np.array([M[j, j] for j in range(S.CHAIN)])
    assert (right > own[:-1]).all() and (own[1:] > right).all()              # strictly increasing along the line
    assert last["det_track"][0, :S.CHAIN].tolist() == list(range(1, S.CHAIN + 1))


def test_edges_counts_and_the_overflow():
    sc = S.scene("edges")
    _, frames = S.replay("edges")
    assert [int(c[0]) for _, c in sc.frames] == [0, 1, 2, 63, 64, 65, 129]
    assert any(int(c[2]) == 0 and int(c[0]) > 0 for _, c in sc.frames)                 # an empty stream beside full ones
    assert frames[-1]["hdr"][0].tolist() == [129, 7, 1, 128] and frames[0]["hdr"][1].tolist() == [129, 1, 1, 128]
    assert frames[-1]["det_track"][0, 128] == 0 and frames[-1]["det_track"][0, 127] == 128
