"""GPU half of the mixup tests: ``ep24_augment_mix_u8`` / ``ep24_augment_mix_labels`` against the plain entry points and the
numpy oracle (tests/mixup_oracle.py), then ``MosaicTransform(mixup_prob=...)`` behind the prefetcher, in a captured training step
and in the trainer.  Label tolerance 1e-3 px, as in tests/test_gpu_augment.py and for its reason: fp32 rounding of a coordinate
<= 1280 is <= 8e-5, the double-precision order effects of these well-conditioned intersections are many orders below, and a
wrong edge, ray or convention is off by pixels."""
import os
import sys

import numpy as np
import pytest
import torch

import mixup_oracle as mo
from test_augment_oracle import INPUT_SIZE, MAX_LABELS, make_source, seeded_case
from test_gpu_augment import _drain, _positioned, _raw_batches
from test_mixup_oracle import MIX_SEEDS, seeded_mix_case

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
Y24 = os.path.join(ROOT, "exploration-of-potential_amd", "yolox_24p")


def test_images_without_the_flag_pass_through_bit_identical():
    """Mixup on image 0 only: every other image, its label rows and its count are what the plain entry points give."""
    from ep24 import augment as aug
    images, targets, params = seeded_case(11, hsv=True)
    assert params.mosaic[0] and not params.mixup.any()
    want_img, want_lab, want_counts = aug.mosaic_batch(images, targets, params, INPUT_SIZE, MAX_LABELS)
    params.mixup[0], params.mix_partner[0], params.mix_jit[0], params.mix_flip[0], params.mix_off[0] = True, 1, 1.2, True, (7, 9)
    img, lab, counts = aug.mosaic_batch(images, targets, params, INPUT_SIZE, MAX_LABELS)
    assert torch.equal(img[1:], want_img[1:]) and torch.equal(lab[1:], want_lab[1:]) and torch.equal(counts[1:], want_counts[1:])
    assert not torch.equal(img[0], want_img[0]) and int(counts[0]) > int(want_counts[0])
    params.mixup[:] = False                                                      # cleared again: the old entry points, the old result
    img, lab, counts = aug.mosaic_batch(images, targets, params, INPUT_SIZE, MAX_LABELS)
    assert torch.equal(img, want_img) and torch.equal(lab, want_lab) and torch.equal(counts, want_counts)


@pytest.mark.parametrize("seed", MIX_SEEDS)
def test_seeded_mixups_match_the_oracle(seed):
    """The seeded mosaics of tests/test_gpu_augment.py with ``sample_mixup``'s draws on top (tests/test_mixup_oracle.py asserts
    what these seeds cover and their decision margins on the CPU)."""
    from ep24 import augment as aug
    images, targets, params = seeded_mix_case(seed)
    sizes = [im.shape[:2] for im in images]
    img, lab, counts = aug.mosaic_batch(images, targets, params, INPUT_SIZE, MAX_LABELS)
    want_img, _, _, _, _ = mo.sample_u8(images, params, INPUT_SIZE)
    want_lab, want_counts, info = mo.augment_labels(targets, sizes, params, INPUT_SIZE, MAX_LABELS)
    got_img = img.cpu().numpy()
    print("seed %d: %d of %d pixels differ; survivors %s (oracle %s), of the partner %s" %
          (seed, int((got_img != want_img).sum()), got_img.size, counts.tolist(), want_counts.tolist(), info["partner_kept"]))
    assert np.array_equal(got_img, want_img)
    assert counts.tolist() == want_counts.tolist()
    got_lab = lab.cpu().numpy()
    assert np.array_equal(got_lab[:, :, 0], want_lab[:, :, 0])                       # the same objects in the same rows
    assert np.array_equal(got_lab.any(-1), want_lab.any(-1))
    diff = float(np.abs(got_lab - want_lab).max())
    print("seed %d: label max abs diff %.3g px" % (seed, diff))
    assert diff <= 1e-3


def test_hsv_after_the_blend_stays_within_the_float32_bound():
    """HSV runs in fp32 on the GPU and in float64 in the oracle, on the BLENDED pixel.  The bound is derived as
    tests/test_gpu_augment.py::test_hsv_stays_within_the_float32_bound derives it: the oracle's own HSV formulas in float32 and in
    float64 on this test's pixels on the CPU, 4x their largest difference allowed.  Measured on the CPU for these two seeds:
    float32 vs float64 max abs difference 1.22e-4 (seed 7) and 1.10e-4 (seed 11), i.e. bounds of 4.9e-4 and 4.4e-4.
    Pixels that neither a tile nor the partner image owns are not recoloured: exactly 114 on padding, 57 on black."""
    from ep24 import augment as aug
    for seed in MIX_SEEDS:
        images, targets, params = seeded_mix_case(seed, hsv=True)
        params.hsv_on[:] = True
        params.hsv[0] = (5.0, -30.0, 30.0)                                           # the extremes too, whatever the seed drew
        params.hsv[1] = (-5.0, 30.0, -30.0)
        want64, cls, _, _, _ = mo.augment_images(images, params, INPUT_SIZE, np.float64)
        want32, _, _, _, _ = mo.augment_images(images, params, INPUT_SIZE, np.float32)
        measured = float(np.abs(want32.astype(np.float64) - want64).max())
        bound = 4.0 * measured
        img, _, _ = aug.mosaic_batch(images, targets, params, INPUT_SIZE, MAX_LABELS)
        got = img.cpu().numpy().astype(np.float64)
        diff = float(np.abs(got - want64).max())
        print("seed %d: float32 vs float64 oracle %.3g, bound %.3g, GPU vs float64 oracle %.3g" % (seed, measured, bound, diff))
        assert 0 < measured < 1e-2
        base, _, _, _, _ = mo.sample_u8(images, params, INPUT_SIZE)
        for c in range(3):
            for kind, value in ((mo.PLAIN_PAD, 114.0), (mo.PARTNER_PAD, 114.0), (mo.BLACK, 57.0)):
                m = cls == kind
                assert m.any() and np.array_equal(got[:, c][m], np.full(int(m.sum()), value)), (c, kind)
            assert np.array_equal(base[:, c][cls >= mo.PARTNER_PAD], got[:, c][cls >= mo.PARTNER_PAD])   # (a + b) >> 1 of the unowned
        assert np.abs(want64 - base).max() > 10                                        # the gains really move the pixels
        assert diff <= bound


def test_prefetcher_with_mixup_is_reproducible():
    from ep24 import augment as aug, input as ein
    size = (160, 192)
    batches = _raw_batches(3)
    tr = aug.MosaicTransform(seed=9, mixup_prob=1.0)
    a = _drain(ein.DataPrefetcher(_positioned(batches, tr, 1), size, tr))
    assert tr.last_params.mixup.any()
    b = _drain(ein.DataPrefetcher(_positioned(batches, tr, 1), size, tr))
    assert len(a) == len(b) == 3
    for (ia, la), (ib, lb) in zip(a, b):
        assert torch.equal(ia, ib) and torch.equal(la, lb)                            # same position, same batch
    c = _drain(ein.DataPrefetcher(_positioned([batches[0], batches[0]], tr, 1), size, tr))
    assert torch.equal(c[0][0], a[0][0]) and not torch.equal(c[1][0], c[0][0])        # another iteration: another batch
    d = _drain(ein.DataPrefetcher(_positioned(batches, tr, 2), size, tr))
    assert not torch.equal(d[0][0], a[0][0])                                          # another epoch: another batch
    # mixup_prob = 0 at the same seed: the transform without mixup, and another batch than with it
    t0, t_old = aug.MosaicTransform(seed=9, mixup_prob=0.0), aug.MosaicTransform(seed=9)
    z = _drain(ein.DataPrefetcher(_positioned(batches, t0, 1), size, t0))
    o = _drain(ein.DataPrefetcher(_positioned(batches, t_old, 1), size, t_old))
    for (iz, lz), (io, lo) in zip(z, o):
        assert torch.equal(iz, io) and torch.equal(lz, lo)
    assert not torch.equal(z[0][0], a[0][0]) and not torch.equal(z[0][1], a[0][1])
    # disabled: the plain transform's output
    tr.enabled = False
    e = _drain(ein.DataPrefetcher(_positioned(batches, tr, 1), size, tr))
    plain = _drain(ein.DataPrefetcher(batches, size, ein.TrainTransform(max_labels=50)))
    for (ie, le), (ip, lp) in zip(e, plain):
        assert torch.equal(ie, ip) and torch.equal(le, lp)


def test_training_step_on_a_mixup_batch():
    """One captured step (bf16 plan) at S = 320, width 0.25, on a batch whose images all carry a partner: finite loss, ring guard 0,
    labels finite and inside the input."""
    from ep24 import _lib, augment as aug, loss as eloss, nn as enn, train as etrain
    S = 320
    items = [make_source(300, 400, 6, 41), make_source(260, 300, 5, 42, star=True), make_source(280, 280, 0, 43),
             make_source(240, 380, 7, 44)]
    images, targets = [it[0] for it in items], [it[1] for it in items]
    sizes = [im.shape[:2] for im in images]
    params = aug.sample_params(aug.position_rng(4, 0, 0), sizes, (S, S))
    aug.sample_mixup(aug.mixup_rng(4, 0, 0), params, sizes, [len(t) for t in targets], (S, S))
    assert params.mixup.all()
    img, lab, counts = aug.mosaic_batch(images, targets, params, (S, S))
    print("survivors per image", counts.tolist())
    assert int(counts.sum()) > 0
    assert bool(torch.isfinite(lab).all()) and float(lab[..., 1:].min()) >= -1e-3 and float(lab[..., 1:].max()) <= S + 1e-3
    assert bool(torch.isfinite(img).all()) and float(img.min()) >= 0 and float(img.max()) <= 255
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


def test_trainer_mixes_until_the_no_aug_epochs(tmp_path):
    """``train_24p.py --synthetic --augment --mixup --steps 6`` on the tiny Exp of
    tests/test_gpu_augment.py::test_trainer_augments_until_the_no_aug_epochs (3 epochs of 2 iterations, no_aug_epochs = 1): the
    batches of epochs 0 and 1 differ from what ``--augment`` alone feeds at the same seed and position (the Exp's
    ``MosaicTransform`` without mixup on the same items), those of epoch 2 equal the plain source."""
    sys.path.insert(0, Y24)
    try:
        import importlib
        mod = importlib.import_module("train_24p")
        from exp import get_exp
        from ep24 import augment as aug, input as ein
        exp = get_exp(os.path.join(Y24, "load_train", "yolox_24p_train.py"))
        exp.width, exp.input_size, exp.synthetic_len, exp.synthetic_gts = 0.25, (320, 320), 8, 4
        exp.max_epoch, exp.no_aug_epochs = 3, 1
        seen = []
        plain_preprocess = exp.preprocess

        def recording(inputs, targets, tsize):
            seen.append((inputs.clone(), targets.clone()))
            return plain_preprocess(inputs, targets, tsize)

        exp.preprocess = recording
        args = mod.make_parser().parse_args(["-b", "4", "-l", "0.01", "--synthetic", "--augment", "--mixup", "--steps", "6",
                                             "--log-interval", "1", "--loader-workers", "0", "--output-dir", str(tmp_path)])
        trainer = mod.main(exp, args)
        torch.cuda.synchronize()
        assert trainer.run_steps == 6 and len(seen) == 6 and trainer.transform.enabled is False
        assert trainer.transform.mixup_prob == 1.0 and trainer.ring_timeouts() == 0
        tt = ein.TrainTransform(max_labels=50)
        alone = aug.MosaicTransform.from_exp(exp, max_labels=50, seed=args.augment_seed)
        for step, (img, lab) in enumerate(seen):
            epoch, it = divmod(step, 2)
            items = [exp.dataset[4 * it + j] for j in range(4)]
            raw = ([x[0] for x in items], [x[1] for x in items])
            p_img, p_lab = tt.batch(raw[0], raw[1], (320, 320))
            same = torch.equal(img, p_img) and torch.equal(lab, p_lab)
            assert same == (epoch == 2), (epoch, it, same)
            assert bool(torch.isfinite(lab).all())
            if epoch < 2:
                alone.set_position(epoch, it)
                a_img, a_lab = alone.batch(raw[0], raw[1], (320, 320))
                assert not alone.last_params.mixup.any()
                assert not torch.equal(img, a_img) and not torch.equal(lab, a_lab), (epoch, it)
                assert not torch.equal(a_img, p_img)
    finally:
        sys.path.remove(Y24)
