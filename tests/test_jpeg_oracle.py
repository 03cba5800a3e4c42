"""tests/jpeg_oracle.py (libjpeg's default decode path restated in numpy) against the committed fixtures: bit equality."""
import os
import sys
import zlib

import numpy as np
import pytest

import jpeg_fixtures as fx
import jpeg_oracle

REFERENCE = os.environ.get("EP24_REFERENCE", "/root/reference")


def test_fixture_table_is_complete():
    names = [c["name"] for c in fx.cases()]
    assert len(names) == len(set(names)) == 70
    assert len(fx.decodable()) == 67 and sorted(fx.refused()) == ["refused_12bit", "refused_cmyk", "refused_progressive"]
    for c in fx.cases():
        assert zlib.crc32(fx.data(c["name"])) == c["jpg_crc32"], c["name"]
        if c["decodable"]:
            a = fx.rgb(c["name"])
            assert a.dtype == np.uint8 and a.shape == (c["height"], c["width"], 3) and zlib.crc32(a.tobytes()) == c["rgb_crc32"], c["name"]
        assert os.path.getsize(fx.path(c["name"])) < (1 << 20)


@pytest.mark.parametrize("name", fx.decodable())
def test_oracle_equals_libjpeg_exactly(name):
    got = jpeg_oracle.decode(fx.data(name))
    want = fx.rgb(name)
    assert got.shape == want.shape and got.dtype == np.uint8
    assert np.array_equal(got, want), "max difference %d" % int(np.abs(got.astype(int) - want.astype(int)).max())
    if name in ("scene_420", "q90_422_17x23", "clamp_q5_444"):
        assert np.array_equal(jpeg_oracle.decode(fx.data(name), bgr=True), want[:, :, ::-1])


@pytest.mark.parametrize("name", fx.refused())
def test_oracle_refuses(name):
    with pytest.raises(jpeg_oracle.Unsupported):
        jpeg_oracle.decode(fx.data(name))


def test_the_two_idct_passes_are_not_interchangeable():
    """Columns first (descale 11), then rows (descale 18): the transposed order rounds differently on a real block."""
    hd, flat = fx.oracle_coefficients("scene_420")
    blocks = np.asarray(flat[:64 * hd.blocks_w[0] * hd.blocks_h[0]]).reshape(-1, 64)
    a = jpeg_oracle.idct(blocks, hd.qt[0])
    b = jpeg_oracle.idct(blocks.reshape(-1, 8, 8).transpose(0, 2, 1).reshape(-1, 64), hd.qt[0].reshape(8, 8).T.reshape(64)).transpose(0, 2, 1)
    assert not np.array_equal(a, b)


def test_generator_reproduces_the_committed_fixtures(tmp_path):
    pytest.importorskip("PIL")
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
    try:
        import make_jpeg_golden
    finally:
        sys.path.pop(0)
    table = make_jpeg_golden.generate(str(tmp_path), photo=fx.path("photo_000000130566"))
    assert [c["name"] for c in table] == [c["name"] for c in fx.cases()]
    for c in table:
        with open(os.path.join(str(tmp_path), c["name"] + ".jpg"), "rb") as fh:
            assert fh.read() == fx.data(c["name"]), c["name"]
        if c["decodable"]:
            assert np.array_equal(np.load(os.path.join(str(tmp_path), c["name"] + ".rgb.npy")), fx.rgb(c["name"])), c["name"]
    assert table == fx.cases()


def test_photo_of_the_reference_tree():
    src = os.path.join(REFERENCE, "yolox", "test_data", "000000130566.jpg")
    if not os.path.isfile(src):
        pytest.skip("no reference tree at %s" % REFERENCE)
    with open(src, "rb") as fh:
        data = fh.read()
    assert data == fx.data("photo_000000130566")
    assert np.array_equal(jpeg_oracle.decode(data), fx.rgb("photo_000000130566"))
