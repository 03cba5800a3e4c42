"""tests/jpeg_encode_oracle.py (libjpeg's forward path restated in numpy) against the coefficients of the committed Pillow files, read
by the numpy decoder oracle (tests/jpeg_oracle.py): equal in every coefficient, for every fixture of tests/golden/jpeg_encode."""
import json
import os

import numpy as np
import pytest

import jpeg_encode_fixtures as ef
import jpeg_encode_oracle as eo
import jpeg_oracle


def test_fixture_table_is_the_grid_of_the_generator():
    t = ef.table()
    assert t["pillow"] and t["libjpeg_turbo"]
    names = set(ef.names())
    for hw in ((5, 3), (8, 8), (16, 16), (17, 23), (33, 50), (40, 7)):
        for s in ("444", "422", "420", "grey"):
            for q in (10, 75, 95, 100):
                assert "enc_%s_q%d_%dx%d" % (s, q, hw[0], hw[1]) in names
    rst = [c for c in ef.cases() if c["restart_interval"]]
    assert len(rst) == 2
    mcus = [-(-c["width"] // (16 if c["sampling"] != "4:4:4" else 8)) * -(-c["height"] // (16 if c["sampling"] == "4:2:0" else 8)) for c in rst]
    assert sorted(m % c["restart_interval"] == 0 for m, c in zip(mcus, rst)) == [False, True]
    assert {"enc_scene_420_q95", "enc_photo_420_q95"} <= names
    for c in ef.cases():
        assert os.path.getsize(ef.path(c["name"])) == c["jpg_bytes"] < (1 << 20)
    assert json.dumps(t)                                     # plain data


@pytest.mark.parametrize("name", ef.names())
def test_oracle_equals_libjpeg(name):
    c = ef.case(name)
    hd, coef = jpeg_oracle.entropy_decode(ef.data(name))
    want = jpeg_oracle.flat_coefficients(coef)
    qt = eo.quality_tables(c["quality"])
    assert np.array_equal(hd.qt[0], qt[0]) and all(np.array_equal(hd.qt[i], qt[1]) for i in range(1, hd.ncomp))
    assert hd.restart_interval == c["restart_interval"] and (hd.height, hd.width) == (c["height"], c["width"])
    got = ef.oracle_coefficients(name)
    assert got.dtype == np.int16 and got.shape == want.shape
    assert np.array_equal(got, want), "%d coefficients differ" % int((got != want).sum())


def test_bgr_input_is_rgb_reversed():
    px = ef.pixels("enc_420_q75_17x23")
    qt = eo.quality_tables(75)
    a = eo.flat(eo.forward(px, qt, "4:2:0"))
    b = eo.flat(eo.forward(np.ascontiguousarray(px[:, :, ::-1]), qt, "4:2:0", bgr=True))
    assert np.array_equal(a, b)


def test_generator_reproduces_the_fixtures():
    """Where the Pillow and libjpeg-turbo of cases.json are installed, the generator writes the committed bytes again."""
    try:
        import PIL
        from PIL import features
    except ImportError:
        pytest.skip("Pillow is not installed")
    t = ef.table()
    if (PIL.__version__, features.version_feature("libjpeg_turbo")) != (t["pillow"], t["libjpeg_turbo"]):
        pytest.skip("another Pillow / libjpeg-turbo than the one that wrote the fixtures")
    import importlib.util
    spec = importlib.util.spec_from_file_location("make_jpeg_encode_golden", os.path.join(os.path.dirname(ef.DIR), "make_jpeg_encode_golden.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    cases = gen.build_cases()
    assert [c["name"] for c in cases] == ef.names()
    for c in cases:
        assert gen.encode(c)[1] == ef.data(c["name"]), c["name"]
