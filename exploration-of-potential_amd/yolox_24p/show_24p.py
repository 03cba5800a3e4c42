"""Inference entry point with the reference's flags (yolox_24p/show_24p.py:370-385): run a trained model over a folder of images and
save every image with its 24-point detections drawn on it.

    cd exploration-of-potential_amd/yolox_24p
    python show_24p.py -f load_train/yolox_24p_l_train.py -p demo_images -w YOLOX_outputs/yolox_24p_l/last_epoch_ckpt.pth

``Exp.get_model()``, the checkpoint's ``"model"`` entry (``-w``), ``eval()``; then batches of ``-b`` files go through
``ep24.input.preproc_batch`` (letterbox on the GPU), ``model(images, train=False)``, ``ep24.infer.postprocess`` and
``ep24.draw.draw_detections`` on the ORIGINAL image with the letterbox ratio - the reference's ``Evaluator.eval`` /
``save_eval_results`` / ``vis`` (:266-367) without the host-side OpenCV.  Results go to ``<output_dir>/<timestamp>/``: the drawn
image under its own name, ``<name>.dets.npy`` with the ``[n, 29]`` float32 rows beside it, and one ``detections.json`` (file, size,
ratio, count).  ``--track`` reads the folder's files in sorted order as the frames of one sequence (``ep24.track.Tracker24``: one frame at a time
whatever ``-b`` is; the drawn label and colour are the track's id; ``--save-tracks FILE`` writes MOTChallenge ``.txt`` or ``.json``).  ``--save-segm FILE`` also writes every detection of the run as a COCO "segm" result (``ep24.results``: the polygon
rasterised on the original image and run-length encoded on the GPU).  ``.npy`` (uint8 HWC) and binary PPM are read and written natively; JPEG / PNG / BMP through PIL when it is installed.  Without it
baseline JPEG files are read AND written through ``ep24.jpeg`` (``--jpeg-encoder``, ``--jpeg-quality``; the drawn device tensors of a
batch are encoded in one call), and a ``.png`` / ``.bmp`` name ends in a clear message.
"""
import argparse
import json
import os
import time

import _path  # noqa: F401
import numpy as np
import torch

from exp import get_exp

NATIVE_EXT = (".npy", ".ppm")
PIL_EXT = (".jpg", ".jpeg", ".png", ".bmp")
JPEG_EXT = (".jpg", ".jpeg")                                # read through ep24.jpeg when PIL is not installed


def _pil():
    try:
        from PIL import Image
        return Image
    except Exception:                                       # PIL is optional
        return None


def read_ppm(path):
    """Binary PPM (P6, maxval 255) -> uint8 [h, w, 3]."""
    data = open(path, "rb").read()
    fields, pos = [], 0
    while len(fields) < 4:                                  # magic, width, height, maxval: whitespace-separated, '#' comments
        while data[pos:pos + 1].isspace():
            pos += 1
        if data[pos:pos + 1] == b"#":
            pos = data.index(b"\n", pos) + 1
            continue
        end = pos
        while not data[end:end + 1].isspace():
            end += 1
        fields.append(data[pos:end])
        pos = end
    if fields[0] != b"P6" or int(fields[3]) != 255:
        raise ValueError("%s: only binary PPM (P6) with maxval 255 is read" % path)
    w, h = int(fields[1]), int(fields[2])
    pix = np.frombuffer(data, dtype=np.uint8, count=h * w * 3, offset=pos + 1)
    return pix.reshape(h, w, 3).copy()


def write_ppm(path, img):
    with open(path, "wb") as fh:
        fh.write(b"P6\n%d %d\n255\n" % (img.shape[1], img.shape[0]))
        fh.write(np.ascontiguousarray(img, dtype=np.uint8).tobytes())


def read_image(path):
    ext = os.path.splitext(path)[1].lower()
    if ext == ".npy":
        img = np.load(path, allow_pickle=False)
    elif ext == ".ppm":
        img = read_ppm(path)
    else:
        Image = _pil()
        if Image is None and ext in JPEG_EXT:               # without PIL: the project's own baseline decoder (host Huffman stage + GPU)
            from ep24 import jpeg
            with open(path, "rb") as fh:
                img = jpeg.decode([fh.read()], bgr=False)[0].cpu().numpy()
        elif Image is None:
            raise SystemExit("show_24p.py: %s needs PIL, which is not installed (.npy, .ppm and baseline .jpg are read natively)" % path)
        else:
            img = np.asarray(Image.open(path).convert("RGB"))
    if img.ndim != 3 or img.shape[2] != 3 or img.dtype != np.uint8:
        raise SystemExit("show_24p.py: %s is not a uint8 [h, w, 3] image (got %s %s)" % (path, img.shape, img.dtype))
    return np.ascontiguousarray(img)


def resolve_jpeg_encoder(choice):
    """--jpeg-encoder: ``auto`` is PIL where it is installed and the project's own encoder (``ep24.jpeg``) otherwise."""
    if choice == "auto":
        return "pil" if _pil() is not None else "native"
    if choice == "pil" and _pil() is None:
        raise SystemExit("show_24p.py: --jpeg-encoder pil needs PIL, which is not installed (native writes baseline .jpg without it)")
    return choice


def write_images(paths, images, jpeg_encoder="auto", jpeg_quality=None, jpeg_entropy="host"):
    """Saves a batch: uint8 [h, w, 3] RGB numpy arrays or (device) tensors.  ``.jpg`` / ``.jpeg`` names go through ``ep24.jpeg.encode``
    with the native encoder - every one of the batch in one call, straight from the device tensors, at quality 95 and 4:2:0 (what
    ``cv2.imwrite`` writes) unless ``jpeg_quality`` says otherwise - and through PIL with the other (its own defaults unless
    ``jpeg_quality`` is given).  ``jpeg_entropy``: where the native encoder's Huffman stage runs, ``host`` or ``device`` (the same
    files either way; with ``device`` only the finished scans leave the GPU)."""
    native = []
    for path, img in zip(paths, images):
        ext = os.path.splitext(path)[1].lower()
        if ext in JPEG_EXT and resolve_jpeg_encoder(jpeg_encoder) == "native":
            native.append((path, img if torch.is_tensor(img) else torch.from_numpy(np.ascontiguousarray(img))))
            continue
        arr = img.cpu().numpy() if torch.is_tensor(img) else img
        if ext == ".npy":
            np.save(path, arr)
        elif ext == ".ppm":
            write_ppm(path, arr)
        else:
            Image = _pil()
            if Image is None:
                raise SystemExit("show_24p.py: writing %s needs PIL, which is not installed (.npy, .ppm and .jpg are written natively)" % path)
            kw = {"quality": int(jpeg_quality)} if ext in JPEG_EXT and jpeg_quality is not None else {}
            Image.fromarray(arr).save(path, **kw)
    if native:
        from ep24 import jpeg
        tensors = [t if t.is_cuda else t.cuda() for _, t in native]
        datas = jpeg.encode(tensors, quality=95 if jpeg_quality is None else int(jpeg_quality), subsampling="4:2:0", bgr=False,
                            entropy=jpeg_entropy)
        for (path, _), data in zip(native, datas):
            with open(path, "wb") as fh:
                fh.write(data)


def write_image(path, img, jpeg_encoder="auto", jpeg_quality=None, jpeg_entropy="host"):
    write_images([path], [img], jpeg_encoder, jpeg_quality, jpeg_entropy)


def list_images(load_path):
    """The image files of a folder (sorted), or the one file given."""
    exts = NATIVE_EXT + (PIL_EXT if _pil() is not None else JPEG_EXT)
    if os.path.isfile(load_path):
        return os.path.dirname(load_path) or ".", [os.path.basename(load_path)]
    if not os.path.isdir(load_path):
        raise SystemExit("show_24p.py: -p %s is neither a folder nor a file" % load_path)
    files = sorted(f for f in os.listdir(load_path) if f.lower().endswith(exts) and not f.endswith(".dets.npy"))
    return load_path, files


def read_class_names(path):
    with open(path) as fh:
        return [ln.rstrip("\n") for ln in fh if ln.strip()]


class Evaluator:
    def __init__(self, exp, args):
        self.exp, self.args = exp, args
        self.num_classes = exp.num_classes
        dev = torch.device(args.device)
        if dev.type != "cuda":
            from ep24._lib import Ep24Error
            raise Ep24Error("show_24p.py --device %s: the ep24 path runs on an MI355X only (no CPU fallback)" % args.device)
        self.device = torch.device("cuda", dev.index if dev.index is not None else args.start_device)
        self.input_size = tuple(exp.test_size)
        if args.load_path is None:
            raise SystemExit("show_24p.py: -p / --load_path is required")
        self.folder, self.file_list = list_images(args.load_path)
        self.class_names = read_class_names(args.class_names) if args.class_names else None
        if self.class_names is not None and len(self.class_names) < self.num_classes:
            raise SystemExit("show_24p.py: --class-names has %d lines for %d classes" % (len(self.class_names), self.num_classes))

    @torch.no_grad()
    def eval(self):
        from ep24.draw import draw_detections
        from ep24.infer import postprocess
        from ep24.input import preproc_batch
        args = self.args
        torch.cuda.set_device(self.device)
        model = self.exp.get_model()
        if args.weights:
            from utils import load_ckpt
            ck = torch.load(args.weights, map_location="cpu")
            load_ckpt(model, ck.get("model", ck))
        else:
            print("show_24p.py: no -w / --weights: the model keeps its initial parameters")
        model.to(self.device)
        model.eval()
        self.save_folder = os.path.join(args.output_dir or self.exp.output_dir, time.strftime("%Y_%m_%d_%H_%M_%S", time.localtime()))
        os.makedirs(self.save_folder, exist_ok=True)
        records = []
        segm = None
        if args.save_segm:
            from ep24.labels24 import COCO_IDS
            from ep24.results import SegmResults
            segm = SegmResults(COCO_IDS if args.segm_category_ids == "coco" else None)
        tracker, track_frames, frame_no = None, [], 0
        if getattr(args, "track", False):
            from ep24 import track
            # one stream; postprocess's rows are in score order, so a frame with more than the cap keeps its best rows
            tracker = track.Tracker24(streams=1, max_tracks=256, max_dets=track.MAX_DETS, high_thre=args.track_high, low_thre=args.track_low,
                                      new_thre=args.track_new, match_thre=args.track_match, max_age=args.track_max_age,
                                      min_hits=args.track_min_hits, device=self.device)
        step = max(int(args.batch_size), 1)
        for lo in range(0, len(self.file_list), step):
            names = self.file_list[lo:lo + step]
            originals = [torch.from_numpy(read_image(os.path.join(self.folder, f))).to(self.device) for f in names]
            images, ratios = preproc_batch(originals, self.input_size, device=self.device)
            if getattr(args, "tta", False):
                # every view of ep24.tta.views_for, merged; polygon NMS over the canonical view's anchor count of candidates
                from ep24 import tta
                outputs = tta.postprocess(tta.predict(model, images), self.num_classes, tta.anchors_for(self.input_size),
                                          conf_thre=args.conf, nms_thre=args.nms, vote_thre=getattr(args, "vote", None))
            else:
                outputs = postprocess(model(images, train=False), self.num_classes, conf_thre=args.conf, nms_thre=args.nms,
                                      nms_iou=args.nms_iou, vote_thre=getattr(args, "vote", None))
            drawn_batch = []
            for name, img, ratio, dets in zip(names, originals, ratios, outputs):
                if tracker is not None:
                    frame_no += 1
                    tracks = tracker.update([None if dets is None else dets[:tracker.N]])[0]
                    drawn = track.draw_tracks(img, tracks, ratio=ratio, conf=args.draw_conf, fill_alpha=args.fill_alpha,
                                              show_scores=args.show_scores)
                    np.save(os.path.join(self.save_folder, name + ".ids.npy"), tracks.ids.cpu().numpy())
                    track_frames.append((frame_no, track.Tracks(tracks.dets.cpu(), tracks.ids.cpu(), tracks.hits.cpu()), float(ratio)))
                    dets = tracks.dets if tracks.dets.shape[0] else None          # the rows saved and exported are the tracks'
                else:
                    drawn = draw_detections(img, dets, ratio=ratio, conf=args.draw_conf, num_classes=self.num_classes,
                                            class_names=self.class_names, fill_alpha=args.fill_alpha, show_scores=args.show_scores)
                rows = np.zeros((0, 29), dtype=np.float32) if dets is None else dets.float().cpu().numpy()
                drawn_batch.append(drawn)
                np.save(os.path.join(self.save_folder, name + ".dets.npy"), rows)
                records.append({"file": name, "height": int(img.shape[0]), "width": int(img.shape[1]), "ratio": float(ratio),
                                "count": int(rows.shape[0])})
                if segm is not None:
                    stem = os.path.splitext(name)[0]
                    segm.add(int(stem) if stem.isascii() and stem.isdigit() else stem, dets, ratio, (int(img.shape[0]), int(img.shape[1])))
                print("%s: %d detections" % (name, rows.shape[0]))
            write_images([os.path.join(self.save_folder, f) for f in names], drawn_batch, args.jpeg_encoder, args.jpeg_quality,
                         getattr(args, "jpeg_entropy", "host"))
        with open(os.path.join(self.save_folder, "detections.json"), "w") as fh:
            summary = {"input_size": list(self.input_size), "conf": args.conf, "nms": args.nms, "nms_iou": args.nms_iou,
                       "tta": bool(getattr(args, "tta", False)), "vote": getattr(args, "vote", None), "draw_conf": args.draw_conf, "images": records}
            if tracker is not None:                             # the rows of every image are then its shown tracks, ids in <name>.ids.npy
                summary["track"] = True
            json.dump(summary, fh, indent=1)
        if tracker is not None and args.save_tracks:
            n = track.write_tracks(args.save_tracks, track_frames)
            print("saved %d track rows of %d frames to %s" % (n, frame_no, args.save_tracks))
        if segm is not None:
            segm.dump(args.save_segm)
            print("saved %d segm results to %s" % (len(segm), args.save_segm))
        print("saved %d images to %s" % (len(records), self.save_folder))
        return self.save_folder


class _NmsIouAction(argparse.Action):
    """--nms-iou, remembering that it was given: --tta implies poly24 and refuses an explicit rect."""

    def __call__(self, parser, namespace, values, option_string=None):
        setattr(namespace, self.dest, values)
        namespace.nms_iou_given = True


def check_tta_args(args):
    """--tta implies --nms-iou poly24 (and refuses an explicit rect); --vote T >= 0 needs the polygon NMS.  Returns the message of
    the refusal, or None."""
    given = getattr(args, "nms_iou_given", False)
    if getattr(args, "tta", False):
        if given and args.nms_iou != "poly24":
            return "--tta merges the views by the polygon NMS: it implies --nms-iou poly24 (got --nms-iou %s)" % args.nms_iou
        args.nms_iou = "poly24"
    vote = getattr(args, "vote", None)
    if vote is not None:
        if args.nms_iou != "poly24":
            return "--vote finds its voters in the buffers of the polygon NMS: add --nms-iou poly24 or --tta"
        if not vote >= 0.0:
            return "--vote %r: the IoU threshold of the voters, at least 0" % vote
    return None


def check_track_args(args):
    """--save-tracks and the --track-* thresholds belong to --track; the tracker's own argument rules (ep24.track.check_args) are
    applied here, before a model is built.  Returns the message of the refusal, or None."""
    if not getattr(args, "track", False):
        if getattr(args, "save_tracks", None):
            return "--save-tracks writes the tracks of --track: add --track"
        return None
    if args.track_new is None:
        args.track_new = args.track_high + 0.1                  # ByteTrack: new = track + 0.1
    if args.save_tracks and os.path.splitext(args.save_tracks)[1].lower() not in (".txt", ".json"):
        return "--save-tracks %s: the name must end in .txt (MOTChallenge) or .json" % args.save_tracks
    from ep24.track import check_args
    try:
        check_args(high_thre=args.track_high, low_thre=args.track_low, new_thre=args.track_new, match_thre=args.track_match,
                   max_age=args.track_max_age, min_hits=args.track_min_hits)
    except ValueError as e:
        return "--track: %s" % e
    return None


class _Parser(argparse.ArgumentParser):
    def parse_args(self, args=None, namespace=None):
        a = super().parse_args(args, namespace)
        msg = check_tta_args(a) or check_track_args(a)
        if msg:
            self.error(msg)
        return a


def make_parser():
    p = _Parser("YOLOX show parser")
    p.add_argument("-b", "--batch_size", type=int, default=64, help="batch size")
    p.add_argument("-s", "--start_device", default=0, type=int, help="device for start count")
    p.add_argument("-d", "--devices", default=1, type=int, help="number of devices (one is used)")
    p.add_argument("-f", "--exp_file", default=None, type=str, help="plz input your experiment description file")
    p.add_argument("-p", "--load_path", type=str, default=None, help="plz input your file path (a folder of images, or one image)")
    p.add_argument("-w", "--weights", type=str, default=None, help="plz input your weights path")
    # additions of this build
    p.add_argument("--output-dir", default=None, type=str, help="results go to <output-dir>/<timestamp>/ (default: exp.output_dir)")
    p.add_argument("--conf", default=0.01, type=float, help="postprocess: obj * class_conf threshold (the reference's 0.01)")
    p.add_argument("--nms", default=0.3, type=float, help="postprocess: NMS IoU threshold (the reference's 0.3)")
    p.add_argument("--nms-iou", default="rect", choices=["rect", "poly24"], action=_NmsIouAction, help="NMS by the reference's "
                   "rectangles or by the exact area IoU of the 24-point polygons")
    p.add_argument("--tta", action="store_true", help="test-time augmentation (ep24.tta): every batch also at 0.85 and 0.7 of the input "
                   "size, each size plain and mirrored, the predictions brought back into one frame and merged by the polygon NMS "
                   "(implies --nms-iou poly24); one forward per view")
    p.add_argument("--vote", default=None, type=float, metavar="T", help="polygon voting: every kept detection becomes the score-weighted "
                   "consensus of the candidates whose area IoU with it is above T (needs --nms-iou poly24 or --tta)")
    p.add_argument("--track", action="store_true", help="the files in sorted order are the frames of one sequence: detections are "
                   "associated across them by the polygons' area IoU (ep24.track), one frame at a time whatever -b is, and drawn with "
                   "their track id as label and colour")
    p.add_argument("--track-high", default=0.5, type=float, help="--track: rows with score >= this are associated first (ByteTrack 0.5)")
    p.add_argument("--track-low", default=0.1, type=float, help="--track: rows below this score are ignored (ByteTrack 0.1)")
    p.add_argument("--track-new", default=None, type=float, help="--track: an unmatched row starts a track from this score "
                   "(default: --track-high + 0.1)")
    p.add_argument("--track-match", default=0.2, type=float, help="--track: first association needs area IoU above this (ByteTrack 1 - 0.8)")
    p.add_argument("--track-max-age", default=30, type=int, help="--track: frames a lost track is kept (ByteTrack 30)")
    p.add_argument("--track-min-hits", default=3, type=int, help="--track: matches before a track is confirmed and shown")
    p.add_argument("--save-tracks", default=None, type=str, metavar="FILE", help="--track: write every shown track of every frame, "
                   "MOTChallenge rows to a .txt name, the same plus the 26 shape numbers to a .json name")
    p.add_argument("--draw-conf", default=1e-4, type=float, help="detections below this score are not drawn (the reference's 0.0001)")
    p.add_argument("--fill-alpha", default=0, type=int, help="0..255: blend the class colour over the polygon's inside (0 = outline only)")
    p.add_argument("--show-scores", action="store_true", help="append the score's two decimals to the label")
    p.add_argument("--class-names", default=None, type=str, help="a file with one class name per line (default: the class index)")
    p.add_argument("--save-segm", default=None, type=str, metavar="FILE", help="write every detection as a COCO segm result (RLE mask of "
                   "its polygon on the original image, score, bbox, area) to this json file")
    p.add_argument("--segm-category-ids", default="index", choices=["coco", "index"], help="--save-segm: category_id is COCO's id of "
                   "the class (80 classes) or the class index")
    p.add_argument("--jpeg-encoder", default="auto", choices=["auto", "native", "pil"], help="who writes .jpg results: PIL, or the "
                   "project's own baseline encoder (ep24.jpeg: arithmetic on the GPU); auto = PIL where it is installed, native otherwise")
    p.add_argument("--jpeg-quality", default=None, type=int, metavar="Q", help="quality 1..100 of .jpg results (native default: 95 at "
                   "4:2:0, what cv2.imwrite writes; PIL keeps its own default when the flag is absent)")
    p.add_argument("--jpeg-entropy", default="host", choices=["host", "device"], help="the native encoder's Huffman stage: on the host "
                   "(the int16 coefficients are copied back) or on the GPU (only the finished scans are); the same files either way")
    p.add_argument("--device", default="cuda", type=str, help="cuda or cuda:N (the ep24 path has no CPU fallback: cpu is refused)")
    return p


def main(exp, args):
    ev = Evaluator(exp, args)
    ev.eval()
    return ev


if __name__ == "__main__":
    args = make_parser().parse_args()
    exp = get_exp(args.exp_file)
    main(exp, args)
