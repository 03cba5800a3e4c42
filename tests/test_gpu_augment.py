"""GPU half of the augmentation tests: ``ep24_augment_u8`` / ``ep24_augment_labels`` against the plain transform and the
numpy oracle (tests/augment_oracle.py), then ``MosaicTransform`` behind the prefetcher, in a captured training step and in
the trainer.  Label tolerance 1e-3 px: fp32 rounding of a coordinate <= 1280 is <= 8e-5, the double-precision order effects of
these well-conditioned intersections are many orders below, and a wrong edge, ray or convention is off by pixels."""
import os
import sys

import numpy as np
import pytest
import torch

import augment_oracle as ao
from test_augment_oracle import INPUT_SIZE, MAX_LABELS, SEEDS, make_source, seeded_case, simple_case

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
Y24 = os.path.join(ROOT, "exploration-of-potential_amd", "yolox_24p")


def test_identity_parameters_are_the_plain_transform():
    from ep24 import augment as aug, input as ein
    images, targets, size = simple_case()
    want_img, rs = ein.preproc_batch(images, size)
    want_lab = ein.labels_batch(targets, [im.shape[:2] for im in images], rs)
    img, lab, counts = aug.mosaic_batch(images, targets, aug.identity_params(len(images)), size)
    assert torch.equal(img, want_img)
    assert counts.tolist() == [len(t) for t in targets]
    diff = float((lab - want_lab).abs().max())
    print("identity: label max abs diff %.3g px" % diff)
    assert diff <= 1e-3
    assert torch.equal(lab[:, :, 0], want_lab[:, :, 0])


def test_mirror_only_is_the_flipped_plain_transform():
    from ep24 import augment as aug
    images, targets, size = simple_case()
    p = aug.identity_params(len(images))
    base, base_lab, _ = aug.mosaic_batch(images, targets, p, size)
    p.mirror[:] = True
    img, lab, counts = aug.mosaic_batch(images, targets, p, size)
    assert torch.equal(img, base.flip(-1))
    assert counts.tolist() == [len(t) for t in targets]
    want, _, _ = ao.augment_labels(targets, [im.shape[:2] for im in images], p, size)
    assert float((lab.cpu() - torch.from_numpy(want)).abs().max()) <= 1e-3
    k = len(targets[0])
    assert float((lab[0, :k, 1] - (size[1] - base_lab[0, :k, 1])).abs().max()) <= 1e-3


@pytest.mark.parametrize("seed", SEEDS)
def test_seeded_mosaics_match_the_oracle(seed):
    """Unequal source sizes, a rectangular input, star objects, an image without labels, images with more survivors than
    rows (tests/test_augment_oracle.py asserts the content and the decision margins of these seeds on the CPU)."""
    from ep24 import augment as aug
    images, targets, params = seeded_case(seed)
    sizes = [im.shape[:2] for im in images]
    img, lab, counts = aug.mosaic_batch(images, targets, params, INPUT_SIZE, MAX_LABELS)
    want_img, _, _ = ao.sample_u8(images, params, INPUT_SIZE)
    want_lab, want_counts, info = ao.augment_labels(targets, sizes, params, INPUT_SIZE, MAX_LABELS)
    got_img = img.cpu().numpy()
    print("seed %d: %d of %d pixels differ; survivors %s (oracle %s)" %
          (seed, int((got_img != want_img).sum()), got_img.size, counts.tolist(), want_counts.tolist()))
    assert np.array_equal(got_img, want_img)
    assert counts.tolist() == want_counts.tolist()
    got_lab = lab.cpu().numpy()
    assert np.array_equal(got_lab[:, :, 0], want_lab[:, :, 0])                       # the same objects in the same rows
    assert np.array_equal(got_lab.any(-1), want_lab.any(-1))
    diff = float(np.abs(got_lab - want_lab).max())
    print("seed %d: label max abs diff %.3g px" % (seed, diff))
    assert diff <= 1e-3


def test_hsv_stays_within_the_float32_bound():
    """HSV runs in fp32 on the GPU and in float64 in the oracle.  The bound is not tuned to the kernel: the oracle's own HSV
    formulas are evaluated in float32 and in float64 on this test's pixels on the CPU, and 4x their largest difference is
    allowed for instruction-order differences.  Measured on the CPU for the pixels of these two seeds: float32 vs float64
    max abs difference 1.22e-4 (seed 7) and 1.10e-4 (seed 11) on values up to 255, i.e. bounds of 4.9e-4 and 4.4e-4."""
    from ep24 import augment as aug
    for seed in SEEDS:
        images, targets, params = seeded_case(seed, hsv=True)
        params.hsv_on[:] = True
        params.hsv[0] = (5.0, -30.0, 30.0)                                           # the extremes too, whatever the seed drew
        params.hsv[1] = (-5.0, 30.0, -30.0)
        want64, owner, _ = ao.augment_images(images, params, INPUT_SIZE, np.float64)
        want32, _, _ = ao.augment_images(images, params, INPUT_SIZE, np.float32)
        measured = float(np.abs(want32.astype(np.float64) - want64).max())
        bound = 4.0 * measured
        img, _, _ = aug.mosaic_batch(images, targets, params, INPUT_SIZE, MAX_LABELS)
        got = img.cpu().numpy().astype(np.float64)
        diff = float(np.abs(got - want64).max())
        print("seed %d: float32 vs float64 oracle %.3g, bound %.3g, GPU vs float64 oracle %.3g" % (seed, measured, bound, diff))
        assert 0 < measured < 1e-2
        assert np.array_equal(got[:, 0][owner < 0], np.full(int((owner < 0).sum()), 114.0))      # padding stays 114
        base, _, _ = ao.sample_u8(images, params, INPUT_SIZE)
        assert np.abs(want64 - base).max() > 10                                        # the gains really move the pixels
        assert diff <= bound


def _raw_batches(n_batches, bs=4):
    out = []
    for b in range(n_batches):
        items = [make_source(150 + 20 * j + 5 * b, 200 + 10 * j, 2 + j, 300 + 10 * b + j, star=j == 1) for j in range(bs)]
        out.append(([it[0] for it in items], [it[1] for it in items], None, None))
    return out


def _positioned(batches, tr, epoch):
    for it, b in enumerate(batches):
        tr.set_position(epoch, it)
        yield b


def _drain(pf):
    got = []
    while True:
        inp, tgt = pf.next()
        if inp is None:
            return got
        got.append((inp.clone(), tgt.clone()))


def test_prefetcher_with_mosaic_transform_is_reproducible():
    from ep24 import augment as aug, input as ein
    size = (160, 192)
    batches = _raw_batches(3)
    tr = aug.MosaicTransform(seed=9)
    a = _drain(ein.DataPrefetcher(_positioned(batches, tr, 1), size, tr))
    b = _drain(ein.DataPrefetcher(_positioned(batches, tr, 1), size, tr))
    assert len(a) == len(b) == 3
    for (ia, la), (ib, lb) in zip(a, b):
        assert torch.equal(ia, ib) and torch.equal(la, lb)                            # same position, same batch
    # the same data at another iteration / epoch gives another batch
    c = _drain(ein.DataPrefetcher(_positioned([batches[0], batches[0]], tr, 1), size, tr))
    assert torch.equal(c[0][0], a[0][0]) and not torch.equal(c[1][0], c[0][0])
    d = _drain(ein.DataPrefetcher(_positioned(batches, tr, 2), size, tr))
    assert not torch.equal(d[0][0], a[0][0])
    # disabled: the plain transform's output
    tr.enabled = False
    e = _drain(ein.DataPrefetcher(_positioned(batches, tr, 1), size, tr))
    plain = _drain(ein.DataPrefetcher(batches, size, ein.TrainTransform(max_labels=50)))
    for (ie, le), (ip, lp) in zip(e, plain):
        assert torch.equal(ie, ip) and torch.equal(le, lp)
    assert not torch.equal(a[0][0], plain[0][0])


def _augmented_batch(S):
    """Four sources (one without labels, kept un-mosaicked: a zero-GT image for certain) through ``mosaic_batch``."""
    from ep24 import augment as aug
    items = [make_source(300, 400, 6, 41), make_source(260, 300, 5, 42, star=True), make_source(280, 280, 0, 43),
             make_source(240, 380, 7, 44)]
    images, targets = [it[0] for it in items], [it[1] for it in items]
    params = aug.sample_params(aug.position_rng(4, 0, 0), [im.shape[:2] for im in images], (S, S))
    plain = aug.identity_params(4)
    for k in ("mosaic", "centre", "partners", "M", "Minv"):
        getattr(params, k)[2] = getattr(plain, k)[2]
    img, lab, counts = aug.mosaic_batch(images, targets, params, (S, S))
    return img, lab, counts


def test_training_step_on_an_augmented_batch():
    """One captured step (bf16 plan) on an augmented batch with a zero-GT image: finite loss, ring guard 0; and in the engine's
    fp32 mode the SimOTA indices on the same images and labels equal the CPU oracle's, as tests/test_gpu_fp32.py compares them."""
    from ep24 import _lib, loss as eloss, nn as enn, train as etrain
    from oracle.loss import LossOracle
    from test_gpu_fp32 import _paired
    S = 320
    img, lab, counts = _augmented_batch(S)
    counts = counts.tolist()
    print("survivors per image", counts)
    assert counts[2] == 0 and sum(counts) > 0 and float(lab[2].abs().max()) == 0
    assert bool(torch.isfinite(lab).all()) and float(lab[..., 1:].min()) >= -1e-3 and float(lab[..., 1:].max()) <= S + 1e-3
    torch.manual_seed(0)
    model = enn.YOLOX(enn.YOLOPAFPN(0.33, 0.25), enn.YOLOXHead(80, 0.25))
    model.head.initialize_biases(1e-2)
    model.to(DEV)
    step = etrain.TrainStep(model, eloss.Loss_Function(80), lr=0.01, momentum=0.9, batch=4, size=S)
    res = step.step(img, lab)
    torch.cuda.synchronize()
    loss = float(res[0])
    assert loss == loss and 0 < loss < 1e4, loss
    assert _lib.lib().fn["ep24_conv_ring_timeouts"]() == 0
    # fp32 parity mode against the CPU oracle on the same batch
    ref, m = _paired(0.33, 0.25)
    images_cpu, labels_cpu = img.cpu(), lab.cpu()
    ref.train()
    ora = LossOracle(80)
    o_tup = ora(ref(images_cpu, train=True), labels_cpu)
    lf = eloss.Loss_Function(80)
    tup = lf(m(img, train=True), lab)
    torch.cuda.synchronize()
    for b in range(4):
        o = ora.trace[b]
        cls_m, fg, ious, gt_idx, nfg = lf.assignment_of(labels_cpu, b)
        if o is None:
            assert nfg == 0 and b == 2
            continue
        assert nfg == o[4], (b, nfg, o[4])
        assert torch.equal(fg.cpu(), o[1]) and torch.equal(gt_idx.cpu(), o[3]) and torch.equal(cls_m.cpu().long(), o[0].long())
    l32, lo = float(tup[0].detach()), float(o_tup[0].detach())
    print("fp32 loss %.7g, oracle %.7g" % (l32, lo))
    assert l32 == l32 and lo == lo


def test_trainer_augments_until_the_no_aug_epochs(tmp_path):
    """``train_24p.py --synthetic --augment --steps 6`` on a tiny Exp (3 epochs of 2 iterations, no_aug_epochs = 1): the batches
    of epochs 0 and 1 differ from the plain source (and from each other), those of epoch 2 equal it."""
    sys.path.insert(0, Y24)
    try:
        import importlib
        mod = importlib.import_module("train_24p")
        from exp import get_exp
        from ep24 import input as ein
        exp = get_exp(os.path.join(Y24, "load_train", "yolox_24p_train.py"))
        exp.width, exp.input_size, exp.synthetic_len, exp.synthetic_gts = 0.25, (320, 320), 8, 4
        exp.max_epoch, exp.no_aug_epochs = 3, 1
        seen = []
        plain_preprocess = exp.preprocess

        def recording(inputs, targets, tsize):
            seen.append((inputs.clone(), targets.clone()))
            return plain_preprocess(inputs, targets, tsize)

        exp.preprocess = recording
        args = mod.make_parser().parse_args(["-b", "4", "-l", "0.01", "--synthetic", "--augment", "--steps", "6", "--log-interval", "1",
                                             "--loader-workers", "0", "--output-dir", str(tmp_path)])
        trainer = mod.main(exp, args)
        torch.cuda.synchronize()
        assert trainer.run_steps == 6 and len(seen) == 6 and trainer.transform.enabled is False
        assert trainer.ring_timeouts() == 0
        tt = ein.TrainTransform(max_labels=50)
        plain = []
        for it in range(2):
            items = [exp.dataset[4 * it + j] for j in range(4)]
            plain.append(tt.batch([x[0] for x in items], [x[1] for x in items], (320, 320)))
        for step, (img, lab) in enumerate(seen):
            epoch, it = divmod(step, 2)
            same = torch.equal(img, plain[it][0]) and torch.equal(lab, plain[it][1])
            assert same == (epoch == 2), (epoch, it, same)
            assert bool(torch.isfinite(lab).all())
        assert not torch.equal(seen[0][0], seen[2][0])                                # epoch 0 and epoch 1: other parameters
    finally:
        sys.path.remove(Y24)
