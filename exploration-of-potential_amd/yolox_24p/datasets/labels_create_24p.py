"""Offline 24-point label generation with the reference's ``Polygon_24`` surface (datasets/2+24_labels_create.py):

    cd exploration-of-potential_amd/yolox_24p
    python datasets/labels_create_24p.py --json instances_train2017.json --images train2017 --out COCO_24p_label --decoder gpu

``json_anno_process`` walks the COCO annotations exactly as the reference does (:122-199: crowds, areas below one pixel and
annotations whose image file is missing are skipped; class ids are re-indexed to 0..79; box centre = bbox corner + half
size), but the ray casting, the convex-hull area of the acceptance filter and nothing else run on the GPU for a whole
batch of annotations at a time (ep24.labels24 -> ep24_ray24 / ep24_hull_area24).  ``save_24r_to_txt`` writes the
reference's files (``%d`` + 50 x ``%0.4f`` in "Cord" mode, + 26 in "Radius" mode).  The masks come from one of two decoders:
``decoder="pycocotools"`` (the default, the reference's ``coco.annToMask`` on the host; the class raises ImportError with that
name when it is constructed without the package) or ``decoder="gpu"`` (ep24.cocomask: the same masks decoded into the device
buffer the rays read, no pycocotools, image sizes from the json's ``images``).  With the GPU decoder ``--save-rle FILE`` also writes
``{annotation id: {"size": [h, w], "counts": str}}`` for every annotation decoded: the masks of that same device buffer, run-length
encoded on the GPU (``cocomask.encode_buffer``) - a polygon annotation stored as the RLE pycocotools' ``frPyObjects`` + ``merge`` give.
"""
import argparse
import json
import os
import sys
from pathlib import Path

import numpy as np

_TOP = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if _TOP not in sys.path:                  # `python datasets/labels_create_24p.py` puts datasets/ first, not yolox_24p/
    sys.path.insert(0, _TOP)
import _path  # noqa: F401,E402
from ep24 import cocomask, labels24  # noqa: E402
from ep24.labels24 import COCO_IDS  # noqa: E402  (category ids in ascending order -> contiguous class index, :36-51)


class Polygon_24:
    def __init__(self, mode="Cord", json_label_pth=None, image_data_pth=None, new_label_pth="./COCO_24p_label", batch=1024,
                 decoder="pycocotools", *, save_rle=None):
        if decoder not in ("pycocotools", "gpu"):
            raise ValueError("decoder is 'pycocotools' or 'gpu'")
        if save_rle and decoder != "gpu":
            raise ValueError("--save-rle encodes the masks of the GPU decoder's device buffer: it needs --decoder gpu")
        if decoder == "pycocotools":
            try:
                from pycocotools.coco import COCO
            except ImportError as e:
                raise ImportError("labels_create_24p needs pycocotools to decode COCO masks (annToMask), or decoder='gpu'") from e
        self.mode, self.decoder = mode, decoder
        self.json_label_pth, self.image_data_pth, self.new_label_pth = json_label_pth, image_data_pth, new_label_pth
        self.batch = batch
        self.save_rle, self.rle = save_rle, {}
        self.coco = COCO(self.json_label_pth) if decoder == "pycocotools" else None
        self.json_dict = self.load_label_json()
        self.label_dict_cord24, self.label_dict_radius = {}, {}
        self.coco_id2idx = {str(cid): i for i, cid in enumerate(COCO_IDS)}

    def load_label_json(self):
        with open(self.json_label_pth, "r") as f:
            return json.load(f)

    def rotation_for_24p(self, center_x, center_y, mask):
        return labels24.rotation_for_24p(center_x, center_y, mask)

    def _flush(self, pending, area_t_low, area_t_high):
        if not pending:
            return
        names, cls, centres, masks, areas, shapes, ids = zip(*pending)
        if self.decoder == "gpu":                             # masks are segmentations: decoded where the rays read them
            buf, desc = cocomask.decode_batch(list(masks), list(shapes))
            pts, rad = labels24.rays_from_buffer(buf, desc, centres)
            if self.save_rle:
                self.rle.update(zip((str(i) for i in ids), cocomask.encode_buffer(buf, desc).to_coco()))
        else:
            pts, rad = labels24.rays_batch(list(masks), centres)
        hull = labels24.hull_areas(pts)
        keep, cord, radius = labels24.label_rows(cls, centres, list(shapes), pts, rad, hull, areas, area_t_low, area_t_high)
        for j, i in enumerate(np.nonzero(keep)[0]):
            self.label_dict_cord24[names[i]].append(cord[j])
            self.label_dict_radius[names[i]].append(radius[j])
        del pending[:]

    def json_anno_process(self, area_t_low=0.5, area_t_high=1.5):
        sizes = {im["id"]: (im["height"], im["width"]) for im in self.json_dict.get("images", [])}
        pending = []
        for anno in self.json_dict["annotations"]:
            name = str(anno["image_id"]).zfill(12)
            self.label_dict_cord24.setdefault(name, [])
            self.label_dict_radius.setdefault(name, [])
            if anno["iscrowd"] or anno["area"] < 1:
                continue
            if not os.path.exists(Path(self.image_data_pth) / Path(name + ".jpg")):
                continue
            if self.decoder == "gpu":
                mask, shape = anno["segmentation"], tuple(sizes[anno["image_id"]])
            else:
                mask = self.coco.annToMask(anno)              # uint8 [H,W]; the json's height / width = the image's
                shape = tuple(mask.shape)
                assert shape == tuple(sizes.get(anno["image_id"], shape))
            cx = anno["bbox"][0] + anno["bbox"][2] / 2
            cy = anno["bbox"][1] + anno["bbox"][3] / 2
            pending.append((name, self.coco_id2idx[str(anno["category_id"])], (cx, cy), mask, anno["area"], shape, anno.get("id")))
            if len(pending) >= self.batch:
                self._flush(pending, area_t_low, area_t_high)
        self._flush(pending, area_t_low, area_t_high)
        if self.save_rle:
            with open(self.save_rle, "w") as f:
                json.dump(self.rle, f)
        return self.label_dict_cord24, self.label_dict_radius

    def save_24r_to_txt(self):
        label_dict = self.label_dict_cord24 if self.mode == "Cord" else self.label_dict_radius
        os.makedirs(self.new_label_pth, exist_ok=True)
        width = 51 if self.mode == "Cord" else 27
        for name, rows in label_dict.items():
            labels24.save_rows(Path(self.new_label_pth) / Path(name + ".txt"), np.array(rows).reshape(-1, width))


if __name__ == "__main__":
    ap = argparse.ArgumentParser("24-point label generation")
    ap.add_argument("--json", required=True)
    ap.add_argument("--images", required=True)
    ap.add_argument("--out", default="./COCO_24p_label")
    ap.add_argument("--mode", default="Cord", choices=["Cord", "Radius"])
    ap.add_argument("--decoder", default="pycocotools", choices=["pycocotools", "gpu"],
                    help="where annToMask runs: pycocotools on the host, or the ep24.cocomask kernels (no pycocotools needed)")
    ap.add_argument("--save-rle", default=None, metavar="FILE",
                    help="with --decoder gpu: also write {annotation id: {size, counts}}, the decoded masks as COCO RLE")
    a = ap.parse_args()
    if a.save_rle and a.decoder != "gpu":
        ap.error("--save-rle encodes the masks of the GPU decoder's device buffer: it needs --decoder gpu")
    polygon = Polygon_24(a.mode, a.json, a.images, a.out, decoder=a.decoder, save_rle=a.save_rle)
    polygon.json_anno_process()
    polygon.save_24r_to_txt()
