"""Feature-map response study with the reference's flags (yolox/demo_featuremap.py:46-61, :590-620) for the 24-point model: how
strongly the three FPN levels respond to one object shifted to several vertical offsets, undistorted and sector-warped at a list
of angles.

    cd exploration-of-potential_amd/yolox_24p
    python demo_featuremap.py -f load_train/yolox_24p_l_train.py --backbone resnet -c last_epoch_ckpt.pth -p object.npy --labels object.txt --vis
    python demo_featuremap.py -f load_train/yolox_24p_train.py --synthetic --tsize 320 --thetas 30 90 --offsets -50 0 50

``Exp.get_model()`` with ``--backbone``, the checkpoint's ``"model"`` entry (``-c``), ``eval()``, then ``ep24.featmap.study``: the
channel mean of each neck output, its mean inside every label's region (the reference's rectangle, and the 24-gon itself) and the AP
of the detections per distortion - all on the GPU.  One plain-text table per level is printed (rows: none, theta_30 ...; columns:
the offsets, :613-620) and ``<output-dir>/response.json`` written; ``--vis`` also saves every heat map there.
"""
import argparse
import os

import _path  # noqa: F401
import numpy as np
import torch

from exp import get_exp
from show_24p import read_image

REGIONS = ("rect", "poly24")


def make_parser():
    p = argparse.ArgumentParser("YOLOX feature-map response parser")
    # the reference's flags
    p.add_argument("--backbone", choices=["darknet", "vgg", "resnet", "densenet"], default=None, help="type of backbone (default: the Exp's)")
    p.add_argument("--vis", action="store_true", help="save the heat maps of every image and level")
    p.add_argument("-c", "--ckpt", default=None, type=str, help="weights file")
    p.add_argument("--device", default="cuda", type=str, help="cuda or cuda:N (the ep24 path has no CPU fallback: cpu is refused)")
    p.add_argument("--conf", default=0.25, type=float, help="test conf")
    p.add_argument("--nms", default=0.45, type=float, help="test nms threshold")
    p.add_argument("--tsize", default=640, type=int, help="test img size")
    p.add_argument("-f", "--exp_file", default=None, type=str, help="pls input your experiment description file")
    # additions of this build
    p.add_argument("-p", "--path", default=None, type=str, help="the object's image: .npy (uint8 HWC), binary .ppm, or what PIL reads")
    p.add_argument("--labels", default=None, type=str, help="its label file: the label creator's txt rows (class + 50 normalised coordinates)")
    p.add_argument("--synthetic", action="store_true", help="one synthetic object of ep24.synth instead of -p / --labels")
    p.add_argument("--offsets", default=[-100, -50, 0, 50, 100], type=int, nargs="+", help="vertical shifts in rows of the image")
    p.add_argument("--thetas", default=list(range(30, 95, 5)), type=int, nargs="*", help="sector angles in degrees")
    p.add_argument("--region", default="rect", choices=REGIONS, help="the region whose means the printed tables show (the json holds both)")
    p.add_argument("--output-dir", default=None, type=str, help="response.json and the heat maps go here (default: <exp.output_dir>/<exp_name>_<backbone>/featuremap)")
    p.add_argument("--seed", default=0, type=int, help="seed of the initial parameters and of the synthetic object")
    return p


def synthetic_object(size, seed):
    """One ep24.synth image with one label -> (uint8 [size, size, 3], rows [1, 51] normalised)."""
    from ep24 import synth
    img = synth.make_images(1, size, seed=seed + 1)[0].permute(1, 2, 0).to(torch.uint8).contiguous().numpy()
    rows = synth.make_labels(1, 1, size=size, seed=seed + 2)[0, :1].double().numpy()
    rows[:, 1::2] /= float(size)
    rows[:, 2::2] /= float(size)
    return img, rows


def load_inputs(args):
    if args.synthetic:
        return synthetic_object(args.tsize, args.seed)
    if args.path is None or args.labels is None:
        raise SystemExit("demo_featuremap.py: give -p IMAGE and --labels FILE, or --synthetic")
    from ep24.labels24 import load_rows
    rows = np.asarray(load_rows(args.labels), dtype=np.float64)
    if rows.size == 0 or rows.ndim != 2 or rows.shape[1] != 51:
        raise SystemExit("demo_featuremap.py: %s holds no [k, 51] label rows" % args.labels)
    return read_image(args.path), rows


def format_tables(result, region):
    """One table per level: rows none, theta_30 ...; columns the offsets; a cell is the mean response of the image's first label
    (``-`` when the label left the image or its region is empty)."""
    lines = []
    tags = ["none"] + ["theta_%d" % t for t in result["thetas"]]
    for k, (st, (h, w)) in enumerate(zip(result["strides"], result["map_sizes"])):
        lines.append("*" * 24 + " Feature Map Size:%dx%d (stride %d, region %s) " % (h, w, st, region) + "*" * 24)
        lines.append("%-10s" % "" + "".join("%12d" % o for o in result["offsets"]) + "%9s" % "AP")
        for tag in tags:
            cells = []
            for o in result["offsets"]:
                lev = result["table"]["offset_%s_%s" % (str(o).zfill(3), tag)]["levels"][k][region]
                cells.append("%12.5f" % lev["mean"][0] if lev["mean"] and lev["count"][0] > 0 else "%12s" % "-")
            lines.append("%-10s" % tag + "".join(cells) + "%9.3f" % result["AP"][tag]["AP"])
    return "\n".join(lines)


def main(exp, args):
    from ep24 import featmap
    from ep24._lib import Ep24Error
    dev = torch.device(args.device)
    if dev.type != "cuda":
        raise Ep24Error("demo_featuremap.py --device %s: the ep24 path runs on an MI355X only (no CPU fallback)" % args.device)
    dev = torch.device("cuda", dev.index if dev.index is not None else 0)
    if args.backbone is not None:
        exp.backbone_type = args.backbone
    exp.test_conf, exp.nmsthre, exp.test_size = args.conf, args.nms, (args.tsize, args.tsize)
    image, rows = load_inputs(args)
    torch.manual_seed(args.seed)
    torch.cuda.set_device(dev)
    model = exp.get_model()
    if args.ckpt:
        from utils import load_ckpt
        ck = torch.load(args.ckpt, map_location="cpu")
        load_ckpt(model, ck.get("model", ck))
    else:
        print("demo_featuremap.py: no -c / --ckpt: the model keeps its initial parameters")
    model.to(dev)
    model.eval()
    out_dir = args.output_dir or os.path.join(exp.output_dir, "%s_%s" % (exp.exp_name, exp.backbone_type), "featuremap")
    os.makedirs(out_dir, exist_ok=True)
    result = featmap.study(model, image, rows, exp.test_size, thetas=args.thetas, offsets=args.offsets, conf=args.conf, nms=args.nms,
                           save_dir=out_dir if args.vis else None)
    if not args.vis:
        import json
        with open(os.path.join(out_dir, "response.json"), "w") as fh:
            json.dump(result, fh, indent=1)
    print(format_tables(result, args.region))
    print("saved %s" % os.path.join(out_dir, "response.json"))
    return result


if __name__ == "__main__":
    args = make_parser().parse_args()
    exp = get_exp(args.exp_file)
    main(exp, args)
