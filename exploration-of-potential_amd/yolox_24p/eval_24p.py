"""Evaluate a saved checkpoint: COCO-style AP of its 24-point detections on the validation set, by object size and by distortion
zone if asked (ep24.evaluate; the single-process run that train_24p.py's --eval-interval message points to).

    python eval_24p.py -f load_train/yolox_24p_train.py -c YOLOX_outputs/yolox_24p/last_epoch_ckpt.pth --synthetic --eval-areas \
        --eval-zones radius --out stats.json

The checkpoint is loaded as show_24p.py loads it; the EMA weights are taken when the file holds them.  ``Exp.eval`` runs once, the
summary is printed, and ``--out`` receives every stratum's numbers and ``per_class_AP`` as JSON.
"""
import argparse
import json
import os

import _path  # noqa: F401
import torch

from exp import get_exp
from train_24p import add_eval_strata_flags, apply_eval_args


def make_parser():
    p = argparse.ArgumentParser("YOLOX-24p eval parser")
    p.add_argument("-f", "--exp_file", default=None, type=str, required=True, help="experiment description file")
    p.add_argument("-c", "--ckpt", default=None, type=str, required=True, help="checkpoint file (train_24p.py's *_ckpt.pth)")
    p.add_argument("-b", "--batch_size", type=int, default=8, help="images per evaluation batch")
    p.add_argument("--synthetic", action="store_true", help="the Exp's synthetic validation set (the source when no --val-data-dir is given)")
    p.add_argument("--val-data-dir", default=None, type=str, help="folder of validation images (with --val-label-dir)")
    p.add_argument("--val-label-dir", default=None, type=str, help="folder of validation label files")
    p.add_argument("--out", default=None, type=str, metavar="stats.json", help="write the numbers as JSON")
    p.add_argument("--device", default="cuda", type=str, help="cuda or cuda:N (the ep24 path has no CPU fallback: cpu is refused)")
    p.add_argument("--eval-iou", default=None, choices=["circle24", "rect", "poly24"], help="IoU type (overrides the Exp's eval_iou_type)")
    p.add_argument("--nms-iou", default=None, choices=["rect", "poly24"], help="NMS of the evaluation (overrides the Exp's nms_iou_type)")
    p.add_argument("--eval-tta", action="store_true", help="test-time augmentation (ep24.tta; implies --nms-iou poly24)")
    p.add_argument("--eval-tta-scales", default=None, type=float, nargs="+", metavar="S", help="with --eval-tta: the views' scales, 1.0 first")
    p.add_argument("--eval-vote", default=None, type=float, metavar="T", help="polygon voting (needs --nms-iou poly24 or --eval-tta)")
    add_eval_strata_flags(p)
    return p


def stats_json(stats):
    """What --out holds: the headline numbers, every stratum's, per_class_AP; -1 stays -1 (no GT to find)."""
    out = {k: stats[k] for k in ("AP", "AP50", "AP75", "AR100", "iou_type", "nms_iou", "images")}
    out["per_class_AP"] = [float(x) for x in stats["per_class_AP"]]
    if "strata" in stats:
        out["max_dets"] = list(stats["max_dets"])
        out["strata"] = stats["strata"]
    return out


def main(exp, args):
    if int(os.environ.get("WORLD_SIZE", 1)) > 1:
        raise SystemExit("eval_24p.py: WORLD_SIZE=%s: distributed evaluation (gathering records across ranks) is not implemented; "
                         "run one process" % os.environ["WORLD_SIZE"])
    if args.device == "cpu" or not torch.cuda.is_available():
        raise SystemExit("eval_24p.py: the ep24 path has no CPU fallback: a GPU is needed")
    if (args.val_data_dir is None) != (args.val_label_dir is None):
        raise SystemExit("eval_24p.py: --val-data-dir and --val-label-dir go together")
    if args.val_data_dir is not None and args.synthetic:
        raise SystemExit("eval_24p.py: --val-data-dir reads a real dataset; drop --synthetic")
    if not os.path.isfile(args.ckpt):
        raise SystemExit("eval_24p.py: -c %s: no such checkpoint" % args.ckpt)
    apply_eval_args(exp, args)                            # stops with a message on flags that do not go together
    for name in ("val_data_dir", "val_label_dir"):
        if getattr(args, name) is not None:
            setattr(exp, name, getattr(args, name))
    device = torch.device(args.device if ":" in args.device else "cuda:0")
    torch.cuda.set_device(device)
    from utils import load_ckpt
    model = exp.get_model()
    ck = torch.load(args.ckpt, map_location="cpu")
    which = "ema_model" if "ema_model" in ck else "model"
    load_ckpt(model, ck.get(which, ck))
    model.to(device)
    evaluator = exp.get_evaluator(args.batch_size)
    ap50_95, ap50, summary = exp.eval(model, evaluator, False)
    print("eval %s (%s weights)  AP50_95 %.4f  AP50 %.4f  (%d images)\n%s" % (args.ckpt, "EMA" if which == "ema_model" else "model",
                                                                            ap50_95, ap50, evaluator.seq, summary), end="")
    if args.out:
        with open(args.out, "w") as f:
            json.dump(stats_json(evaluator.stats), f, indent=1)
    return evaluator


if __name__ == "__main__":
    args = make_parser().parse_args()
    main(get_exp(args.exp_file), args)
