"""The fixtures of tests/golden/jpeg_encode (written by tests/golden/make_jpeg_encode_golden.py): Pillow's encodes of arrays of
tests/golden/jpeg, shared by the test_jpeg_encode_* / test_gpu_jpeg_encode files."""
import functools
import json
import os

import numpy as np

import jpeg_fixtures as fx

DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "jpeg_encode")


@functools.lru_cache(maxsize=None)
def table():
    with open(os.path.join(DIR, "cases.json")) as fh:
        return json.load(fh)


def cases():
    return table()["cases"]


def names():
    return [c["name"] for c in cases()]


@functools.lru_cache(maxsize=None)
def case(name):
    return {c["name"]: c for c in cases()}[name]


def path(name):
    return os.path.join(DIR, name + ".jpg")


@functools.lru_cache(maxsize=None)
def data(name):
    with open(path(name), "rb") as fh:
        return fh.read()


@functools.lru_cache(maxsize=None)
def pixels(name):
    """The source array: uint8 [h, w, 3] RGB, or [h, w] for a grey case.  Read-only."""
    c = case(name)
    a = fx.rgb(c["source"])
    if c["sampling"] == "grey":
        a = np.ascontiguousarray(a[:, :, 0])
        a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def oracle_coefficients(name):
    """The numpy forward path (tests/jpeg_encode_oracle.py) on the source array at the case's tables: flat int16, computed once."""
    import jpeg_encode_oracle as eo
    c = case(name)
    flat = eo.flat(eo.forward(pixels(name), eo.quality_tables(c["quality"]), c["sampling"]))
    flat.setflags(write=False)
    return flat
