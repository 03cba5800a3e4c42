"""Writes the fixtures of tests/golden/jpeg_encode/: Pillow's (libjpeg-turbo's) encodes NAME.jpg of arrays that tests/golden/jpeg
already holds (NAME.rgb.npy there, read-only and used as pixels), and cases.json (source array, sampling, quality, restart interval,
size, CRC-32, and the versions of Pillow and libjpeg-turbo that wrote the files).  Needs Pillow; the fixtures are committed, so the
tests do not.

    python tests/golden/make_jpeg_encode_golden.py [OUT_DIR]
"""
import io
import json
import os
import sys
import zlib

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "jpeg")
SIZES = [(5, 3), (8, 8), (16, 16), (17, 23), (33, 50), (40, 7)]        # height x width
SAMPLINGS = ["4:4:4", "4:2:2", "4:2:0", "grey"]
QUALITIES = [10, 75, 95, 100]
PIL_SUB = {"4:4:4": 0, "4:2:2": 1, "4:2:0": 2}


def source(mode, hw):
    return ("grey_q80_%dx%d" if mode == "grey" else "q90_444_%dx%d") % hw


def build_cases():
    """-> list of dicts: name, source, sampling, quality, restart_interval"""
    out = []
    for hw in SIZES:
        for s in SAMPLINGS:
            for q in QUALITIES:
                out.append(dict(name="enc_%s_q%d_%dx%d" % (s.replace(":", ""), q, hw[0], hw[1]), source=source(s, hw), sampling=s, quality=q,
                                restart_interval=0))
    # 33 x 50 at 4:2:0 has 12 MCUs: 5 does not divide them; 17 x 23 at 4:4:4 has 9: 3 does
    out.append(dict(name="enc_rst5_420_q75_33x50", source=source("4:2:0", (33, 50)), sampling="4:2:0", quality=75, restart_interval=5))
    out.append(dict(name="enc_rst3_444_q75_17x23", source=source("4:4:4", (17, 23)), sampling="4:4:4", quality=75, restart_interval=3))
    out.append(dict(name="enc_scene_420_q95", source="scene_420", sampling="4:2:0", quality=95, restart_interval=0))
    out.append(dict(name="enc_photo_420_q95", source="photo_000000130566", sampling="4:2:0", quality=95, restart_interval=0))
    return out


def pixels(case):
    a = np.load(os.path.join(SRC, case["source"] + ".rgb.npy"), allow_pickle=False)
    return np.ascontiguousarray(a[:, :, 0]) if case["sampling"] == "grey" else a


def encode(case):
    from PIL import Image
    arr = pixels(case)
    kw = dict(quality=case["quality"])
    if case["sampling"] != "grey":
        kw["subsampling"] = PIL_SUB[case["sampling"]]
    if case["restart_interval"]:
        kw["restart_marker_blocks"] = case["restart_interval"]
    buf = io.BytesIO()
    Image.fromarray(arr, "L" if case["sampling"] == "grey" else "RGB").save(buf, "JPEG", **kw)
    return arr, buf.getvalue()


def generate(out_dir):
    import PIL
    from PIL import features
    os.makedirs(out_dir, exist_ok=True)
    table = []
    for case in build_cases():
        arr, data = encode(case)
        with open(os.path.join(out_dir, case["name"] + ".jpg"), "wb") as fh:
            fh.write(data)
        table.append(dict(case, height=int(arr.shape[0]), width=int(arr.shape[1]), jpg_bytes=len(data), jpg_crc32=zlib.crc32(data)))
    with open(os.path.join(out_dir, "cases.json"), "w") as fh:
        json.dump({"pillow": PIL.__version__, "libjpeg": features.version("jpg"),
                   "libjpeg_turbo": features.version_feature("libjpeg_turbo"), "cases": table}, fh, indent=1, sort_keys=True)
        fh.write("\n")
    return table


if __name__ == "__main__":
    t = generate(sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "jpeg_encode"))
    print("%d cases, %d bytes of JPEG" % (len(t), sum(r["jpg_bytes"] for r in t)))
