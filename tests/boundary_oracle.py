"""Numpy restatement of Boundary IoU (Cheng et al., CVPR 2021) on boolean masks, the specification of ep24_mask_boundary and of
``SegmEvaluator(iou_type="boundary")``.  Written from the definitions in include/ep24.h section E7, one statement per step:

    erode(M, d)      d iterations of the 3 x 3 minimum on the mask framed by one ring of zeros (cv2.copyMakeBorder + cv2.erode);
                     pixel (x, y) survives iff every pixel within d of it in x and in y is set, pixels outside the image being unset
    boundary(M, d)   M & ~erode(M, d)
    dilation(h, w)   max(1, int(round(ratio * sqrt(h * h + w * w)))): from the IMAGE's size, Python's round on the float64 product
    boundary_iou     min(rleIou of the masks, rleIou of the bands); a crowd GT divides by the area of the detection's band

Groups built with that IoU go through the unchanged ``segmeval_oracle.evaluate``.
"""
import math

import numpy as np

import segmeval_oracle as ora


def erode(m, d):
    """bool [H, W] -> bool [H, W]: ``d`` literal iterations of the 3 x 3 minimum on a zero-framed copy."""
    m = np.asarray(m).astype(bool)
    H, W = m.shape
    f = np.zeros((H + 2, W + 2), dtype=bool)
    f[1:H + 1, 1:W + 1] = m
    for _ in range(int(d)):
        g = np.zeros_like(f)
        g[1:H + 1, 1:W + 1] = f[1:H + 1, 1:W + 1]
        for dy in (-1, 0, 1):
            for dx in (-1, 0, 1):
                g[1:H + 1, 1:W + 1] &= f[1 + dy:H + 1 + dy, 1 + dx:W + 1 + dx]
        f = g
    return f[1:H + 1, 1:W + 1]


def boundary(m, d):
    m = np.asarray(m).astype(bool)
    return m & ~erode(m, d)


def dilation(h, w, ratio=0.02):
    return max(1, int(round(ratio * math.sqrt(h * h + w * w))))


def boundary_iou(dt_masks, gt_masks, gt_crowd, d):
    """[D, G] float64: the elementwise minimum of ``segmeval_oracle.mask_iou`` on the masks and on their bands of radius ``d``."""
    _, iou_mask = ora.mask_iou(dt_masks, gt_masks, gt_crowd)
    _, iou_band = ora.mask_iou([boundary(m, d) for m in dt_masks], [boundary(m, d) for m in gt_masks], gt_crowd)
    return np.minimum(iou_mask, iou_band)
