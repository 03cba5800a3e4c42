"""Closed forms of the drawing oracle (tests/draw24_oracle.py), the font and the palette: no GPU needed."""
import numpy as np

import draw24_oracle as O
from draw24_scenes import make_row
from ep24 import draw
from ep24.font5x7 import FONT


def grid(x0, x1, y0, y1):
    Y, X = np.meshgrid(np.arange(y0, y1 + 1, dtype=np.int64), np.arange(x0, x1 + 1, dtype=np.int64), indexing="ij")
    return X, Y


def test_disc_areas():
    X, Y = grid(-8, 8, -8, 8)
    assert int(O.cover_disc(X, Y, 0, 0, 4).sum()) == 13           # a vertex dot, radius 2
    assert int(O.cover_disc(X, Y, 0, 0, 16).sum()) == 49          # the centre dot, radius 4


def test_horizontal_edge_covers_3L_plus_5():
    X, Y = grid(-4, 14, -4, 4)
    for L, want in ((0, 5), (1, 8), (2, 11), (7, 26)):
        assert want == 3 * L + 5
        assert int(O.cover_edge(X, Y, (0, 0), (L, 0)).sum()) == want
        assert int(O.cover_edge(X, Y, (L, 0), (0, 0)).sum()) == want
        assert int(O.cover_edge(Y, X, (0, 0), (0, L)).sum()) == want          # the vertical one, by symmetry


def test_edge_rule_is_exact_squared_distance():
    """(d x w)^2 <= L2 between the ends and the end discs elsewhere == exact rational squared distance <= 1."""
    rng = np.random.default_rng(24)
    X, Y = grid(-3, 12, -3, 12)
    for _ in range(200):
        P, Q = rng.integers(0, 10, 2), rng.integers(0, 10, 2)
        got = O.cover_edge(X, Y, P, Q)
        want = np.array([[O.segment_dist2_exact(int(x), int(y), P, Q) <= 1 for x in X[0]] for y in Y[:, 0]])
        assert np.array_equal(got, want), (P, Q)


def test_blend_formula():
    """(pix * (256 - a) + colour * a + 128) >> 8 at its ends.  Alpha 0 never reaches the formula (no fill); alpha 255 leaves the
    old pixel a weight of 1 / 256, so it gives the colour exactly when -128 <= pix - colour < 128 and the colour one level towards
    the pixel otherwise - checked over all 65 536 pairs.  (An oracle that returned the colour for every pair would not be the
    contract's formula.)"""
    p, c = np.meshgrid(np.arange(256), np.arange(256), indexing="ij")
    got = O.blend(p.astype(np.uint8), c, 255).astype(np.int64)
    d = p - c
    want = np.where(d >= 128, c + 1, np.where(d < -128, c - 1, c))
    assert np.array_equal(got, want)
    assert np.array_equal(got[np.abs(d) < 128], c[np.abs(d) < 128])
    assert np.array_equal(O.blend(p.astype(np.uint8), c, 128), ((p + c + 1) >> 1).astype(np.uint8))
    # alpha 0 through the whole oracle: a polygon's inside keeps its bytes, only the outline changes
    rng = np.random.default_rng(1)
    img = rng.integers(0, 256, (40, 40, 3), dtype=np.uint8)
    row = make_row(20, 22, [10.0] * 24, cls=0)[None]
    out0 = O.draw(img, row, num_classes=1, fill_alpha=0)
    out255 = O.draw(img, row, num_classes=1, fill_alpha=255)
    assert np.array_equal(out0[26, 14], img[26, 14]) and not np.array_equal(out0, img)
    col = O.default_colors(1)[0].astype(np.int64)
    assert np.all(np.abs(out255[26, 14].astype(np.int64) - col) <= 1)


def test_text_reproduces_the_glyph():
    for ch in (ord("R"), ord("g"), ord("%"), 7):                  # 7: outside 32..126, drawn as '?'
        rows = FONT[(ch if 32 <= ch <= 126 else ord("?")) - 32]
        for s in (1, 3):
            xc, yc = 10, 40
            X, Y = grid(0, 60, 0, 60)
            cov = O.cover_text(X, Y, xc, yc, bytes([ch]), s)
            tx, ty = xc + 3, yc - 3 - 7 * s
            want = np.zeros_like(cov)
            for v in range(7):
                for u in range(5):
                    if (rows[v] >> (4 - u)) & 1:
                        want[ty + v * s:ty + (v + 1) * s, tx + u * s:tx + (u + 1) * s] = True
            assert np.array_equal(cov, want), (ch, s)
    # two glyphs: the second starts one 6 s cell further, the sixth column stays empty
    X, Y = grid(0, 60, 0, 60)
    cov = O.cover_text(X, Y, 10, 40, b"11", 2)
    one = O.cover_text(X, Y, 10, 40, b"1", 2)
    shifted = np.zeros_like(one)
    shifted[:, 12:] = one[:, :-12]
    assert np.array_equal(cov, one | shifted) and cov.sum() == 2 * one.sum()
    assert not cov[:, 13 + 10:13 + 12].any()                      # tx = 13: columns u = 10, 11 are the first cell's gap


def test_font_sanity():
    assert len(FONT) == 95 and all(len(g) == 7 for g in FONT)
    assert all(0 <= row < 32 for g in FONT for row in g)
    need = "0123456789ABCDEFGHIJKLMNOPQRSTUVWXYZabcdefghijklmnopqrstuvwxyz-_.:%?"
    glyphs = [FONT[ord(ch) - 32] for ch in need]
    assert all(any(g) for g in glyphs)
    assert len(set(glyphs)) == len(need)
    assert not any(FONT[0])                                       # the space
    assert len(set(FONT)) == 95                                   # in fact every glyph differs from every other


def test_palette_is_pairwise_distinct():
    for C in (1, 3, 80):
        p = draw.palette(C)
        assert tuple(p.shape) == (C, 3) and str(p.dtype) == "torch.uint8"
        assert len({tuple(r) for r in p.tolist()}) == C
    assert draw.palette(80)[:3].tolist() == draw.palette(3).tolist()      # a class keeps its colour whatever C is


def test_label_table():
    tab, lens = draw.label_table(3, ["cat", "x" * 30, ""])
    assert lens.tolist() == [3, 21, 0] and bytes(tab[0, :3]) == b"cat" and not tab[0, 3:].any()
    tab, lens = draw.label_table(12)
    assert bytes(tab[11, :2]) == b"11" and lens.tolist() == [1] * 10 + [2, 2]
    assert O.label_bytes(11) == b"11" and O.label_bytes(1, ["a", "y" * 30]) == b"y" * 21


def test_skip_rules_and_score_digits():
    H, W, C = 50, 60, 3
    ok = make_row(20, 20, [5.0] * 24, obj=0.5, cc=0.5, cls=2)
    assert O.row_geometry(ok, 1.0, 0.25, H, W, C) is not None                 # score == conf draws
    assert O.row_geometry(ok, 1.0, 0.2500001, H, W, C) is None
    for col, val in ((28, -1.0), (28, 3.0), (0, np.inf), (5, np.nan), (1, 1048576.0), (9, -2.0e6)):
        bad = ok.copy()
        bad[col] = val
        assert O.row_geometry(bad, 1.0, 0.0, H, W, C) is None, (col, val)
    assert O.score_digits(0.0) == b" 00" and O.score_digits(0.057) == b" 05"
    assert O.score_digits(np.float32(0.999)) == b" 99" and O.score_digits(1.0) == b" 99"
    geo = O.row_geometry(make_row(58, 48, [9.0] * 24), 1.0, 0.0, H, W, C)
    assert geo["vx"].max() == W and geo["vy"].max() == H and geo["vx"].min() >= 0      # clipped to [0, W] x [0, H]
