"""Score a COCO "segm" result file against the ground-truth instances on the GPU: pycocotools' 12-line summary for
iouType = "segm" (mask IoU with the crowd rule, ignore flags, the four area ranges, maxDets 1 / 10 / 100) without pycocotools.

    python eval_segm.py --gt instances_val2017.json --dt segm.json [--max-dets 1 10 100] [--out stats.json]
    python eval_segm.py --gt instances_val2017.json --dt segm.json --iou-type boundary [--dilation-ratio 0.02]

``segm.json`` is what ``show_24p.py --save-segm`` writes (``ep24.results.SegmResults``); any COCO result list whose
segmentations are RLE dicts or polygon lists is taken.  Masks are decoded, intersected, matched and accumulated by HIP kernels
(``ep24.segmeval.SegmEvaluator``); ``--out`` receives the 12 numbers and the AP per category.  ``--iou-type boundary`` prints the
same 12 lines for Boundary AP (Cheng et al., CVPR 2021): each pair's IoU is the smaller of the mask IoU and the IoU of the two masks'
boundary bands, the pixels within ``--dilation-ratio`` x the image diagonal of the mask's outside.
"""
import argparse
import json

import _path  # noqa: F401

from ep24.segmeval import SegmEvaluator


def make_parser():
    p = argparse.ArgumentParser("eval_segm")
    p.add_argument("--gt", required=True, help="COCO instances file (images, annotations, categories)")
    p.add_argument("--dt", required=True, help="COCO segm result file")
    p.add_argument("--max-dets", type=int, nargs="+", default=[1, 10, 100], help="detections per image and category (at most 4 values, each <= 128)")
    p.add_argument("--out", default=None, help="write the stats and the per-category AP here as JSON")
    p.add_argument("--device", default="cuda:0")
    p.add_argument("--chunk-mb", type=int, default=256, help="decoded mask bytes per chunk of images")
    p.add_argument("--iou-type", choices=["segm", "boundary"], default="segm", help="mask IoU, or Boundary IoU = min(mask IoU, IoU of the boundary bands)")
    p.add_argument("--dilation-ratio", type=float, default=0.02, help="boundary band radius as a fraction of the image diagonal (--iou-type boundary)")
    return p


def main(args):
    ev = SegmEvaluator(args.gt, max_dets=args.max_dets, device=args.device, chunk_bytes=args.chunk_mb << 20, iou_type=args.iou_type,
                       dilation_ratio=args.dilation_ratio)
    ev.add_results(args.dt)
    st = ev.evaluate()
    print(ev.summary, end="")
    if args.out:
        doc = {"stats": st["stats"], "per_class_AP": dict(zip(map(str, st["category_ids"]), st["per_class_AP"].tolist())),
               "max_dets": ev.max_dets, "images": st["images"], "results": st["results"], "dropped": st["dropped"]}
        if args.iou_type == "boundary":
            doc.update(iou_type=st["iou_type"], dilation_ratio=st["dilation_ratio"])
        with open(args.out, "w") as f:
            json.dump(doc, f)
    return st


if __name__ == "__main__":
    main(make_parser().parse_args())
