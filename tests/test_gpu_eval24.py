"""The GPU evaluator (csrc/evaluate.hip, ep24.evaluate) against the numpy oracle (tests/eval24_oracle.py), fed with the
kernels' own IoU matrices: TP masks, record order, precision / recall tables and the summary bit-equal."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import eval24_oracle as O  # noqa: E402
from ep24 import evaluate as E, infer, synth  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
Y24 = os.path.join(ROOT, "exploration-of-potential_amd", "yolox_24p")
pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _det26_from_gt(gt50):
    r = O._gt_radii(gt50)
    return np.concatenate([gt50[:, :2], r], 1).astype(np.float32)


def test_pairwise_iou_against_the_oracle():
    lab = synth.make_labels(2, 25, size=640, seed=11).reshape(-1, 51)[:, 1:].numpy()
    gt50 = lab[:50]
    det = synth.decode_head(synth.make_raw_head(1, 640, seed=12))[0, :, :26].numpy()
    det[:50] = _det26_from_gt(gt50) * np.float32(1.02)    # a few close pairs (every case of the lens code)
    det[:50, :2] = gt50[:, :2] + 3.0
    g, d = torch.from_numpy(gt50).to(DEV), torch.from_numpy(det).to(DEV)
    rect = E.pairwise_iou(g, d, "rect").cpu().numpy()
    assert rect.shape == (50, 8400)
    want = O.iou_rect(gt50, det)
    assert np.array_equal(rect, want, equal_nan=True)
    circ = E.pairwise_iou(g, d, "circle24").cpu().numpy()
    wc = O.iou_circle24(gt50, det).astype(np.float64)
    assert np.all(np.isfinite(circ)) and float(np.abs(circ - wc).max()) <= 2e-6
    assert float(circ.max()) > 0.5 and float(circ.min()) >= 0.0


def make_scenes(n_img, C, seed):
    """labels [n, 50, 51] and per image detections [k, 29] (None for some): jittered GTs, duplicates, false positives,
    quantised scores (ties), empty images and images with more than 100 detections of one class."""
    rng = np.random.RandomState(seed)
    counts = [0 if i % 9 == 4 else int(rng.randint(0, 51)) for i in range(n_img)]
    labels = synth.make_labels(n_img, counts, size=640, seed=seed, num_classes=C)
    dets = []
    for i in range(n_img):
        n = counts[i]
        gt50 = labels[i, :n, 1:].numpy()
        rows = []
        if n:
            base = _det26_from_gt(gt50)
            for rep in range(int(rng.randint(1, 3))):     # jittered copies and duplicates
                j = base.copy()
                j[:, :2] += rng.randn(n, 2).astype(np.float32) * (2.0 + 6.0 * rep)
                j[:, 2:] *= (1.0 + rng.randn(n, 24) * 0.08).astype(np.float32)
                cls = labels[i, :n, 0].numpy().copy()
                flip = rng.rand(n) < 0.1
                cls[flip] = rng.randint(0, C, flip.sum())
                rows.append(np.concatenate([j, np.zeros((n, 3), np.float32)], 1))
                rows[-1][:, 28] = cls
        nfp = int(rng.randint(0, 40)) if i % 9 != 4 else 0
        if i % 16 == 7:
            nfp = 150                                     # > 100 detections of one class
        if nfp:
            fp = synth.decode_head(synth.make_raw_head(1, 640, seed=seed * 1000 + i))[0, :nfp, :29].numpy().copy()
            fp[:, 28] = 3 if i % 16 == 7 else rng.randint(0, C, nfp)
            rows.append(fp)
        if not rows:
            dets.append(None)
            continue
        r = np.concatenate(rows, 0)
        r[:, 26] = (rng.randint(1, 11, len(r)) / 10.0).astype(np.float32)     # obj in {0.1 .. 1.0}
        r[:, 27] = np.where(rng.rand(len(r)) < 0.5, 1.0, 0.5).astype(np.float32)
        perm = rng.permutation(len(r))
        dets.append(torch.from_numpy(r[perm].copy()).to(DEV))
    return labels, dets


def oracle_images(labels, dets, iou_type):
    imgs = []
    for i, d in enumerate(dets):
        n = O.num_gt(labels[i].numpy())
        gt = labels[i, :n].numpy()
        if d is None:
            imgs.append({"gt_cls": gt[:, 0].astype(np.int64), "det_cls": np.zeros(0, np.int64), "det_score": np.zeros(0, np.float32),
                         "iou": np.zeros((n, 0))})
            continue
        dh = d.cpu().numpy()
        iou = E.pairwise_iou(torch.from_numpy(gt[:, 1:]).to(DEV), d[:, :26], iou_type).cpu().numpy() if n else np.zeros((0, len(dh)))
        imgs.append({"gt_cls": gt[:, 0].astype(np.int64), "det_cls": dh[:, 28].astype(np.int64), "det_score": dh[:, 26] * dh[:, 27],
                     "iou": iou})
    return imgs


def run_gpu(labels, dets, C, iou_type, splits):
    ev = E.Evaluator24(C, iou_type=iou_type)
    lo = 0
    for s in splits:
        ev.update_detections(dets[lo:lo + s], labels[lo:lo + s].to(DEV))
        lo += s
    assert lo == len(dets)
    st = ev.summarize()
    return ev, st


def check_against_oracle(ev, st, want, C):
    rec = ev.records()
    wr = want["records"]
    assert len(rec["cls"]) == len(wr)
    assert np.array_equal(rec["cls"], [r[0] for r in wr])
    assert np.array_equal(rec["score"].view(np.uint32), np.array([r[1] for r in wr], dtype=np.float32).view(np.uint32))
    assert np.array_equal(rec["seq"], [r[2] for r in wr])
    assert np.array_equal(rec["p"], [r[3] for r in wr])
    assert np.array_equal(rec["rank"], [r[4] for r in wr])
    assert np.array_equal(rec["tp"], [r[5] for r in wr])
    assert np.array_equal(st["precision"], want["precision"])
    assert np.array_equal(st["recall"], want["recall"])
    ws = O.summarize(want["precision"], want["recall"])
    for k in ("AP", "AP50", "AP75", "AR100"):
        assert st[k] == ws[k], k
    assert np.array_equal(st["per_class_AP"], ws["per_class_AP"])


@pytest.mark.parametrize("C,iou_type", [(80, "circle24"), (120, "rect"), (120, "circle24")])
def test_random_scenes_bit_equal_to_the_oracle(C, iou_type):
    labels, dets = make_scenes(64, C, seed=C + len(iou_type))
    ev, st = run_gpu(labels, dets, C, iou_type, [64])
    want = O.evaluate(oracle_images(labels, dets, iou_type), C)
    check_against_oracle(ev, st, want, C)
    assert 0.0 < st["AP"] < 1.0 and st["AP50"] > st["AP"]


def test_batch_split_and_repeat_invariance():
    labels, dets = make_scenes(64, 80, seed=5)
    ref = None
    splits13 = [5] * 12 + [4]
    for splits in ([64], [16] * 4, splits13, [64]):
        _, st = run_gpu(labels, dets, 80, "circle24", splits)
        if ref is None:
            ref = st
        assert np.array_equal(st["precision"], ref["precision"]) and np.array_equal(st["recall"], ref["recall"])


def test_update_equals_update_detections_of_postprocess():
    B, S, C = 4, 320, 80
    pred = synth.decode_head(synth.make_raw_head(B, S, seed=21, num_classes=C), S)
    pred[..., 26:] = torch.sigmoid(pred[..., 26:])
    pred = pred.to(DEV)
    labels = synth.make_labels(B, [6, 0, 12, 3], size=S, seed=22).to(DEV)
    for iou_type in ("circle24", "rect"):
        a = E.Evaluator24(C, iou_type=iou_type)
        a.update(pred, labels)
        b = E.Evaluator24(C, iou_type=iou_type)
        b.update_detections(infer.postprocess(pred, C, conf_thre=0.01, nms_thre=0.65), labels)
        sa, sb = a.summarize(), b.summarize()
        assert a.n_records == b.n_records > 0
        ra, rb = a.records(), b.records()
        for k in ra:
            assert np.array_equal(ra[k], rb[k]), k
        assert np.array_equal(sa["precision"], sb["precision"]) and np.array_equal(sa["recall"], sb["recall"])


def test_eval_accumulate_across_chunk_boundaries():
    """The synthetic records of tests/test_gpu_segmeval.py (classes of 2 500, 1 024 and 1 025 records: sums and maxima carried over
    the accumulate kernel's chunks of 1 024) in the 24-point shape - the TP bits of range 0, npig [K]: ep24_eval_accumulate bit-equal
    to the segm oracle at one maxDets that keeps every record and to ep24_segm_accumulate on the same buffers with NA = NM = 1."""
    import segmeval_oracle as ora
    from ep24._lib import call, ptr, stream_ptr
    from test_gpu_segmeval import CHUNK_K as K, chunk_records, dev, framed, frames_intact
    rec, _ = chunk_records()
    rec = dict(rec, m=rec["m"][:, :1] & 0x3FF, npig=rec["npig"][:, :1])
    want_p, want_r = (x[..., 0, 0] for x in ora.accumulate(rec, K, (128,)))
    n = len(rec["cls"])
    ranks = ora.score_ranks(rec["score"]).astype(np.uint64)
    key = dev(((ranks << np.uint64(32)) | (rec["seq"].astype(np.uint64) << np.uint64(7)) | rec["rank"].astype(np.uint64)).view(np.int64))
    cls, tp, npig = dev(rec["cls"].astype(np.int32)), dev(rec["m"].astype(np.int32).reshape(-1)), dev(rec["npig"].astype(np.int32).reshape(-1))
    order = E.sort_records(key, cls, 7 + int(rec["seq"].max()).bit_length(), max(K - 1, 1).bit_length())
    md, rthr = dev(np.array([128], dtype=np.int32)), dev(ora.REC_THRS.copy())
    npr, nrc = 10 * 101 * K, 10 * K
    got = []
    for segm in (False, True):
        p_big, prec, f64 = framed(npr, torch.float64)
        r_big, recl, _ = framed(nrc, torch.float64)
        ctp = torch.full((n,), -1, dtype=torch.int32, device=DEV)
        env = torch.full((n,), float("nan"), dtype=torch.float64, device=DEV)
        if segm:
            call("segm_accumulate", ptr(order), ptr(key), ptr(cls), ptr(tp), n, ptr(npig), K, 1, ptr(md), 1, ptr(rthr), None, ptr(ctp),
                 ptr(env), ptr(prec), ptr(recl), stream_ptr())
        else:
            call("eval_accumulate", ptr(order), ptr(cls), ptr(tp), n, ptr(npig), K, ptr(rthr), None, ptr(ctp), ptr(env), ptr(prec),
                 ptr(recl), stream_ptr())
        assert frames_intact(p_big, npr, f64) and frames_intact(r_big, nrc, f64)
        got.append((prec.cpu().numpy().reshape(10, 101, K), recl.cpu().numpy().reshape(10, K)))
    for got_p, got_r in got:
        assert np.array_equal(got_p.view(np.int64), want_p.view(np.int64))
        assert np.array_equal(got_r.view(np.int64), want_r.view(np.int64))
    assert ((want_p > 0) & (want_p < 0.99)).any() and np.all(want_p[:, :, 4] == -1) and np.all(want_p[:, :, 3] == 0)


def _small_exp():
    sys.path.insert(0, Y24)
    from exp import get_exp
    exp = get_exp(os.path.join(Y24, "load_train", "yolox_24p_train.py"))
    exp.depth, exp.width = 0.33, 0.25
    exp.test_size = (320, 320)
    exp.eval_len = 10
    return exp


def test_exp_eval_equals_the_decomposed_path():
    from ep24.input import TrainTransform
    exp = _small_exp()
    torch.manual_seed(0)
    model = exp.get_model().to(DEV)
    ev = exp.get_evaluator(4)
    ap, ap50, summary = exp.eval(model, ev, False)
    assert model.training and "Average Precision" in summary
    ref = E.Evaluator24(exp.num_classes, conf_thre=exp.test_conf, nms_thre=exp.nmsthre)
    model.eval()
    tt = TrainTransform(max_labels=50)
    with torch.no_grad():
        for images, targets, _, _ in exp.get_eval_loader(4):
            imgs, labs = tt.batch(images, targets, (320, 320))
            eng = model.engine(imgs.shape[0], 320)
            ref.update(eng.forward_eval(imgs), labs)
    st = ref.summarize()
    model.train()
    assert ref.seq == 10 and ev.seq == 10
    assert np.array_equal(st["precision"], ev.stats["precision"]) and np.array_equal(st["recall"], ev.stats["recall"])
    assert (ap, ap50) == (st["AP"], st["AP50"])


def _train(out, *extra):
    env = dict(os.environ)
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK"):
        env.pop(k, None)
    cmd = [sys.executable, os.path.join(Y24, "train_24p.py"), "-f", os.path.join(Y24, "load_train", "yolox_24p_train.py"), "-b", "4",
           "-l", "0.01", "--synthetic", "--synthetic-len", "8", "--steps", "4", "--log-interval", "1", "--loader-workers", "0",
           "--output-dir", out] + list(extra)
    p = subprocess.run(cmd, cwd=Y24, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=900)
    assert p.returncode == 0, p.stdout[-4000:]
    return p.stdout


def test_trainer_eval_interval(tmp_path):
    with_eval = _train(str(tmp_path / "a"), "--eval-interval", "1")
    evals = [ln for ln in with_eval.splitlines() if ln.startswith("eval epoch")]
    assert len(evals) == 2 and "AP50_95" in evals[0], with_eval[-3000:]
    assert os.path.exists(str(tmp_path / "a" / "yolox_24p" / "best_ckpt.pth"))
    plain = _train(str(tmp_path / "b"))
    assert "eval epoch" not in plain
    la = [ln.rsplit(None, 2)[0] for ln in with_eval.splitlines() if ln.startswith("step ")]
    lb = [ln.rsplit(None, 2)[0] for ln in plain.splitlines() if ln.startswith("step ")]
    assert len(la) == 4 and la == lb                      # steps 3 and 4 ran after an evaluation: same loss terms and num_fg
    ca = torch.load(str(tmp_path / "a" / "yolox_24p" / "last_epoch_ckpt.pth"), map_location="cpu")
    cb = torch.load(str(tmp_path / "b" / "yolox_24p" / "last_epoch_ckpt.pth"), map_location="cpu")
    for k, v in cb["model"].items():
        assert torch.equal(ca["model"][k], v), k          # the step after an evaluation is bitwise the step without one
