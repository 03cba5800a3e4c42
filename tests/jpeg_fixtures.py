"""The JPEG fixtures of tests/golden/jpeg (written by tests/golden/make_jpeg_golden.py), shared by the test_jpeg_* / test_gpu_jpeg files."""
import functools
import json
import os

import numpy as np

DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "jpeg")
PREFIX_CASES = ("q90_420_17x23", "q75rst_444_33x50", "grey_q80_8x8")          # every prefix of these is decoded
SCENE = "scene_420"


@functools.lru_cache(maxsize=None)
def cases():
    with open(os.path.join(DIR, "cases.json")) as fh:
        return json.load(fh)


def decodable():
    return [c["name"] for c in cases() if c["decodable"]]


def refused():
    return [c["name"] for c in cases() if not c["decodable"]]


def path(name):
    return os.path.join(DIR, name + ".jpg")


@functools.lru_cache(maxsize=None)
def data(name):
    with open(path(name), "rb") as fh:
        return fh.read()


@functools.lru_cache(maxsize=None)
def rgb(name):
    a = np.load(os.path.join(DIR, name + ".rgb.npy"), allow_pickle=False)
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def oracle_coefficients(name):
    """(header, flat int16 coefficients) of the numpy oracle, computed once per session."""
    import jpeg_oracle
    hd, coef = jpeg_oracle.entropy_decode(data(name))
    flat = jpeg_oracle.flat_coefficients(coef)
    flat.setflags(write=False)
    return hd, flat
