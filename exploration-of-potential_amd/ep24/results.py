"""COCO "segm" results of 24-point detections: every detection's polygon as an RLE-encoded instance mask on the original image.

``SegmResults.add`` takes one image's ``postprocess`` rows, rasterises them (``masks.detections_to_masks``), encodes the packed
masks on the GPU (``cocomask.encode``) and keeps one record per detection; ``dump`` writes the list a COCO evaluation loads with
``loadRes``: ``{"image_id", "category_id", "segmentation": {"size", "counts"}, "score", "bbox": [x, y, w, h], "area"}``.  What
crosses to the host per image is the runs, the boxes, the areas and the rows - never a pixel.
"""
import json

import numpy as np

from . import cocomask, masks


class SegmResults:
    def __init__(self, category_ids=None):
        """category_ids: ``category_id = category_ids[class index]`` (``labels24.COCO_IDS`` for COCO's 80 classes);
        None writes the class index itself."""
        self.category_ids = None if category_ids is None else [int(c) for c in category_ids]
        self.records = []

    def __len__(self):
        return len(self.records)

    def add_records(self, image_id, segmentations, bbox, area, scores, classes):
        """The host half of ``add``: ``segmentations`` = ``RunLengths.to_coco()`` of n masks, ``bbox [n, 4]`` and ``area [n]``
        as ``PackedMasks`` holds them ((x0, y0, x1, y1) of the set pixels, (W, H, -1, -1) for none), ``scores [n]``, class
        indices ``[n]``.  A mask without a pixel keeps its record: bbox [0, 0, 0, 0], area 0, counts of the single run."""
        bbox, area = np.asarray(bbox).reshape(-1, 4), np.asarray(area).reshape(-1)
        scores, classes = np.asarray(scores).reshape(-1), np.asarray(classes).reshape(-1)
        if not len(segmentations) == len(bbox) == len(area) == len(scores) == len(classes):
            raise ValueError("one segmentation, box, area, score and class per detection")
        for seg, (x0, y0, x1, y1), a, s, c in zip(segmentations, bbox.tolist(), area.tolist(), scores.tolist(), classes.tolist()):
            c = int(c)
            if self.category_ids is not None and not 0 <= c < len(self.category_ids):
                raise IndexError("class %d has no entry in category_ids" % c)
            box = [x0, y0, x1 - x0 + 1, y1 - y0 + 1] if a > 0 else [0, 0, 0, 0]
            self.records.append({"image_id": image_id, "category_id": c if self.category_ids is None else self.category_ids[c],
                                 "segmentation": {"size": list(seg["size"]), "counts": seg["counts"]}, "score": float(s),
                                 "bbox": [int(v) for v in box], "area": int(a)})

    def add(self, image_id, dets, ratio, image_hw):
        """One image: ``dets`` = its ``postprocess`` rows ``[n, 29]`` on the GPU (or None), ``ratio`` its letterbox ratio,
        ``image_hw`` the original image's (h, w).  score = obj_conf * class_conf (columns 26 and 27, an fp32 product),
        class = column 28.  Returns the number of records added."""
        if dets is not None and (dets.dim() != 2 or dets.shape[1] != 29):
            raise IndexError("expected postprocess rows [n, 29], got %s" % (tuple(dets.shape),))
        pm = masks.detections_to_masks(dets, ratio, image_hw)
        if len(pm) == 0:
            return 0
        segs = cocomask.encode(pm).to_coco()
        rows = dets.detach().float().cpu().numpy()
        self.add_records(image_id, segs, pm.bbox.cpu().numpy(), pm.area.cpu().numpy(), rows[:, 26] * rows[:, 27],
                         rows[:, 28].astype(np.int64))
        return len(segs)

    def dump(self, path):
        with open(path, "w") as fh:
            json.dump(self.records, fh)
        return path
