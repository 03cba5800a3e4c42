"""Writes the JPEG fixtures of tests/golden/jpeg/: NAME.jpg, NAME.rgb.npy (Pillow's decode, ``convert("RGB")``, uint8) and cases.json
(encoder arguments, sizes, CRC-32s).  Needs Pillow (libjpeg-turbo); the fixtures are committed, so the tests do not.

    python tests/golden/make_jpeg_golden.py [OUT_DIR] [--photo PATH/000000130566.jpg]

Sources are seeded synthetic images (smooth ramps plus noise, RandomState(0)); ``--photo`` adds the 640 x 427 baseline 4:4:4 test
photo (data, copied as it is) with its decode.  Without it an existing photo fixture in OUT_DIR is kept.
"""
import io
import json
import os
import sys
import zlib

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
SIZES = [(8, 8), (16, 16), (17, 23), (33, 50), (5, 3), (40, 7)]        # height x width
SUB = {0: "444", 1: "422", 2: "420"}


def ramp_noise(rs, h, w, ch):
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    img = np.stack([255.0 * xx / max(w - 1, 1), 255.0 * yy / max(h - 1, 1), 255.0 * (xx + yy) / max(h + w - 2, 1)], -1)[:, :, :ch]
    img = img + rs.normal(0.0, 12.0, img.shape)
    return np.clip(np.rint(img), 0, 255).astype(np.uint8)


def scene(rs, h=240, w=320):
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    img = np.stack([60 + 120.0 * xx / w, 40 + 160.0 * yy / h, 200 - 100.0 * (xx + yy) / (h + w)], -1)
    for _ in range(7):
        cy, cx = rs.uniform(0, h), rs.uniform(0, w)
        ay, ax = rs.uniform(12, 60), rs.uniform(12, 80)
        col = rs.uniform(0, 255, 3)
        img[((yy - cy) / ay) ** 2 + ((xx - cx) / ax) ** 2 <= 1.0] = col
    img = img + rs.normal(0.0, 6.0, img.shape)
    return np.clip(np.rint(img), 0, 255).astype(np.uint8)


def build_cases():
    """-> list of (name, array, mode, save kwargs, decodable)"""
    rs = np.random.RandomState(0)
    src = {hw: ramp_noise(rs, hw[0], hw[1], 3) for hw in SIZES}
    grey = {hw: ramp_noise(rs, hw[0], hw[1], 1)[:, :, 0] for hw in SIZES}
    cases = []
    for tag, kw in (("q90", dict(quality=90)), ("q30opt", dict(quality=30, optimize=True)), ("q75rst", dict(quality=75, restart_marker_blocks=2))):
        for sub in (0, 1, 2):
            for hw in SIZES:
                cases.append(("%s_%s_%dx%d" % (tag, SUB[sub], hw[0], hw[1]), src[hw], "RGB", dict(kw, subsampling=sub), True))
    for hw in SIZES:
        cases.append(("grey_q80_%dx%d" % hw, grey[hw], "L", dict(quality=80), True))
    yy, xx = np.mgrid[0:16, 0:16]
    chk = ((((yy // 2) + (xx // 2)) & 1) * 255).astype(np.uint8)
    chk3 = np.repeat(chk[:, :, None], 3, 2)
    cases.append(("clamp_q10_420", chk3, "RGB", dict(quality=10, subsampling=2), True))
    cases.append(("clamp_q5_444", chk3, "RGB", dict(quality=5, subsampling=0), True))
    cases.append(("clamp_grey_q10", chk, "L", dict(quality=10), True))
    cases.append(("flat_q100_420_24x40", rs.randint(0, 256, (24, 40, 3)).astype(np.uint8), "RGB", dict(quality=100, subsampling=2), True))
    sc = scene(rs)
    cases.append(("scene_420", sc, "RGB", dict(quality=75, subsampling=2), True))
    cases.append(("scene_420_rst", sc, "RGB", dict(quality=75, subsampling=2, restart_marker_rows=1), True))
    cases.append(("refused_progressive", src[(16, 16)], "RGB", dict(quality=90, progressive=True), False))
    cases.append(("refused_cmyk", np.concatenate([src[(16, 16)], src[(16, 16)][:, :, :1]], 2), "CMYK", dict(quality=90), False))
    cases.append(("refused_12bit", src[(8, 8)], "RGB", dict(quality=90, subsampling=0), False))
    return cases


def encode(name, arr, mode, kw):
    from PIL import Image
    buf = io.BytesIO()
    Image.fromarray(arr, mode).save(buf, "JPEG", **kw)
    data = buf.getvalue()
    if name == "refused_12bit":                           # the SOF0 precision byte: FF C0, length (2), precision
        p = data.index(b"\xff\xc0")
        data = data[:p + 4] + b"\x0c" + data[p + 5:]
    return data


def pil_rgb(data):
    from PIL import Image
    return np.asarray(Image.open(io.BytesIO(data)).convert("RGB"), dtype=np.uint8)


def save_npy(path, arr):
    with open(path, "wb") as fh:
        np.lib.format.write_array(fh, np.ascontiguousarray(arr), version=(1, 0))


def generate(out_dir, photo=None):
    os.makedirs(out_dir, exist_ok=True)
    table = []
    for name, arr, mode, kw, ok in build_cases():
        data = encode(name, arr, mode, kw)
        with open(os.path.join(out_dir, name + ".jpg"), "wb") as fh:
            fh.write(data)
        rec = {"name": name, "height": int(arr.shape[0]), "width": int(arr.shape[1]), "mode": mode, "save": kw, "decodable": ok,
               "jpg_crc32": zlib.crc32(data), "jpg_bytes": len(data)}
        if ok:
            rgb = pil_rgb(data)
            save_npy(os.path.join(out_dir, name + ".rgb.npy"), rgb)
            rec["rgb_crc32"] = zlib.crc32(rgb.tobytes())
        table.append(rec)
    pname = "photo_000000130566"
    ppath = os.path.join(out_dir, pname + ".jpg")
    if photo:
        with open(photo, "rb") as fh:
            data = fh.read()
        with open(ppath, "wb") as fh:
            fh.write(data)
    if os.path.exists(ppath):
        with open(ppath, "rb") as fh:
            data = fh.read()
        rgb = pil_rgb(data)
        save_npy(os.path.join(out_dir, pname + ".rgb.npy"), rgb)
        table.append({"name": pname, "height": int(rgb.shape[0]), "width": int(rgb.shape[1]), "mode": "RGB", "save": None, "decodable": True,
                      "external": True, "jpg_crc32": zlib.crc32(data), "jpg_bytes": len(data), "rgb_crc32": zlib.crc32(rgb.tobytes())})
    with open(os.path.join(out_dir, "cases.json"), "w") as fh:
        json.dump(table, fh, indent=1, sort_keys=True)
        fh.write("\n")
    return table


if __name__ == "__main__":
    args = sys.argv[1:]
    photo = None
    if "--photo" in args:
        i = args.index("--photo")
        photo = args[i + 1]
        del args[i:i + 2]
    t = generate(args[0] if args else os.path.join(HERE, "jpeg"), photo)
    print("%d cases, %d bytes of JPEG" % (len(t), sum(r["jpg_bytes"] for r in t)))
