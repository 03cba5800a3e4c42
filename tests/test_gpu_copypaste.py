"""GPU half of the copy-paste tests: ``ep24_paste_labels`` / ``ep24_paste_u8`` against the numpy oracle (tests/copypaste_oracle.py)
on the cases of tests/test_copypaste_oracle.py, then ``mosaic_batch`` with the paste fields, ``MosaicTransform(copy_paste_prob=...)``
behind the prefetcher and a captured training step on a pasted batch.

The stage-level comparisons are EQUALITIES.  The transformed coordinates are specified operation by operation (double, one rounding
to fp32) and pixels are copied, so nothing is left to a tolerance; the accept / reject decisions compare quantities that the oracle
forms in another order, and tests/test_copypaste_oracle.py asserts on the CPU that none of them is closer than 1e-6 (IoA) or
1e-3 px (margin, inside) to its threshold in these cases - many orders above the difference between two double evaluations."""
import numpy as np
import pytest
import torch

import copypaste_oracle as co
from test_augment_oracle import INPUT_SIZE, make_source, seeded_case
from test_copypaste_oracle import CASES, MIN_MARGIN, N, SIZES, THR, case
from test_gpu_augment import _drain, _positioned, _raw_batches

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _run(c, desc=None, check=True):
    from ep24 import augment as aug
    pre_i = torch.from_numpy(c["pre_images"].copy()).to(DEV)
    pre_l = torch.from_numpy(c["pre_labels"].copy()).to(DEV)
    pre_c = torch.from_numpy(c["pre_count"].copy()).to(DEV)
    snap = (pre_i.clone(), pre_l.clone(), pre_c.clone())
    out = aug.paste_batch(pre_i, pre_l, pre_c, c["paste"] if desc is None else desc, min_margin=MIN_MARGIN, ioa_thr=THR, check=check)
    torch.cuda.synchronize()
    assert torch.equal(pre_i, snap[0]) and torch.equal(pre_l, snap[1]) and torch.equal(pre_c, snap[2])      # inputs are a snapshot
    return [t.cpu().numpy() for t in out]


@pytest.mark.parametrize("name", CASES)
def test_stage_matches_the_oracle_exactly(name):
    c = case(name)
    img, lab, counts, ranges = _run(c)
    print(name, "counts", counts.tolist(), "oracle", c["counts"].tolist(), "ranges", ranges.tolist())
    assert np.array_equal(counts, c["counts"]) and counts.dtype == np.int32
    assert np.array_equal(ranges, c["ranges"])
    assert np.array_equal(lab.view(np.uint32), c["rows"].view(np.uint32))                      # bit for bit, the zero padding included
    # the image kernel, fed the GPU's own rows and ranges, against the oracle on the same rows
    want, pasted = co.paste_u8(c["pre_images"], lab, ranges, c["paste"])
    print(name, "pasted pixels per image", pasted.sum((1, 2)).tolist(), "differing words", int((img != want).sum()))
    assert np.array_equal(img.view(np.uint32), want.view(np.uint32))
    for i in range(N):
        assert (pasted[i].sum() > 0) == (ranges[i, 1] > ranges[i, 0]), i               # every accepted candidate leaves pixels
        if not c["paste"][i, 0]:
            assert np.array_equal(img[i], c["pre_images"][i]) and np.array_equal(lab[i], c["pre_labels"][i]) and \
                counts[i] == c["pre_count"][i]                                         # on == 0: out == pre
    assert pasted.any()


def test_a_partner_outside_the_batch_is_refused_and_the_kernels_treat_it_as_off():
    from ep24 import _lib
    c = case("hand")
    desc = c["paste"].copy()
    desc[0, 1], desc[2, 1] = N, -1
    with pytest.raises(_lib.Ep24Error, match="EP24_E_ARG"):
        _run(c, desc)
    img, lab, counts, ranges = _run(c, desc, check=False)                              # the kernels themselves: as on == 0
    for i in (0, 2):
        E = min(int(c["pre_count"][i]), c["max_labels"])
        assert np.array_equal(img[i], c["pre_images"][i]) and np.array_equal(lab[i], c["pre_labels"][i])
        assert counts[i] == c["pre_count"][i] and ranges[i].tolist() == [E, E]
    assert np.array_equal(lab[3], c["rows"][3]) and counts[3] == c["counts"][3]        # the other images are untouched by it


def test_empty_batch_and_refused_arguments():
    from ep24 import _lib, augment as aug
    S_h, S_w = SIZES[1]
    e_i, e_l = torch.empty(0, 3, S_h, S_w, device=DEV), torch.empty(0, 6, 51, device=DEV)
    e_c = torch.empty(0, dtype=torch.int32, device=DEV)
    img, lab, counts, ranges = aug.paste_batch(e_i, e_l, e_c, np.zeros((0, 8), dtype=np.int64))
    torch.cuda.synchronize()
    assert tuple(img.shape) == (0, 3, S_h, S_w) and tuple(lab.shape) == (0, 6, 51) and tuple(counts.shape) == (0,) and tuple(ranges.shape) == (0, 2)
    c = case("hand")
    pre_i, pre_l = torch.from_numpy(c["pre_images"].copy()).to(DEV), torch.from_numpy(c["pre_labels"].copy()).to(DEV)
    pre_c = torch.from_numpy(c["pre_count"].copy()).to(DEV)
    with pytest.raises(_lib.Ep24Error, match="another buffer"):
        aug.paste_batch(pre_i, pre_l, pre_c, c["paste"], out_labels=pre_l)
    with pytest.raises(_lib.Ep24Error, match="ioa_thr"):
        aug.paste_batch(pre_i, pre_l, pre_c, c["paste"], ioa_thr=0.0)
    big = torch.zeros(N, 257, 51, device=DEV)
    with pytest.raises(_lib.Ep24Error, match="max_labels"):
        aug.paste_batch(pre_i, big, pre_c, c["paste"])


def test_images_without_the_flag_pass_through_bit_identical():
    """``mosaic_batch`` on a seeded mosaic: the same call before setting, after setting and after clearing the paste fields.  Paste on
    image 0 only: every other image, its label rows and its count are what the batch without the fields gives; cleared again, the
    whole batch is."""
    from ep24 import augment as aug
    ML = 50                                                                      # room for pasted rows behind the mosaic's own
    images, targets, params = seeded_case(11, hsv=True)
    assert not params.paste.any()
    want_img, want_lab, want_counts = aug.mosaic_batch(images, targets, params, INPUT_SIZE, ML)
    staging = {}
    params.paste[0], params.paste_partner[0], params.paste_flip[0], params.paste_off[0] = True, 1, True, (-31, 17)
    params.paste_select[0] = np.uint64(2 ** 64 - 1)
    img, lab, counts = aug.mosaic_batch(images, targets, params, INPUT_SIZE, ML, paste_staging=staging)
    assert torch.equal(img[1:], want_img[1:]) and torch.equal(lab[1:], want_lab[1:]) and torch.equal(counts[1:], want_counts[1:])
    E = min(int(want_counts[0]), ML)
    assert torch.equal(lab[0, :E], want_lab[0, :E]) and int(counts[0]) > int(want_counts[0]) and len(staging) == 1
    assert not torch.equal(img[0], want_img[0])
    # the post-pass is the stage the oracle restates: from the staged batch (what the two launches wrote) to the output
    pre_i, pre_l, pre_c = (t.cpu().numpy() for t in next(iter(staging.values())))
    assert np.array_equal(pre_i, want_img.cpu().numpy()) and np.array_equal(pre_l, want_lab.cpu().numpy())
    desc = aug.paste_descriptors(params)
    o_lab, o_counts, o_ranges, dec = co.paste_labels(pre_l, pre_c, desc, INPUT_SIZE, 2.0, 0.30, ML)
    o_img, pasted = co.paste_u8(pre_i, o_lab, o_ranges, desc)
    print("image 0: %d rows before, %d after, %d pixels pasted" % (int(want_counts[0]), int(counts[0]), int(pasted.sum())))
    assert np.array_equal(lab.cpu().numpy(), o_lab) and np.array_equal(counts.cpu().numpy(), o_counts)
    assert np.array_equal(img.cpu().numpy(), o_img)
    again = aug.mosaic_batch(images, targets, params, INPUT_SIZE, ML, paste_staging=staging)
    assert len(staging) == 1 and all(torch.equal(a, b) for a, b in zip(again, (img, lab, counts)))   # the cached staging buffers
    params.paste[:] = False                                                      # cleared again: the old calls, the old result
    img, lab, counts = aug.mosaic_batch(images, targets, params, INPUT_SIZE, ML)
    assert torch.equal(img, want_img) and torch.equal(lab, want_lab) and torch.equal(counts, want_counts)
    params.paste[2], params.paste_partner[2] = True, len(images)
    with pytest.raises(Exception, match="EP24_E_ARG"):
        aug.mosaic_batch(images, targets, params, INPUT_SIZE, ML)


def test_prefetcher_with_copy_paste_is_reproducible():
    from ep24 import augment as aug, input as ein
    size = (160, 192)
    batches = _raw_batches(3)
    tr = aug.MosaicTransform(seed=9, copy_paste_prob=1.0)
    a = _drain(ein.DataPrefetcher(_positioned(batches, tr, 1), size, tr))
    assert tr.last_params.paste.all()
    b = _drain(ein.DataPrefetcher(_positioned(batches, tr, 1), size, tr))
    assert len(a) == len(b) == 3
    for (ia, la), (ib, lb) in zip(a, b):
        assert torch.equal(ia, ib) and torch.equal(la, lb)                            # same position, same batch
    c = _drain(ein.DataPrefetcher(_positioned([batches[0], batches[0]], tr, 1), size, tr))
    assert torch.equal(c[0][0], a[0][0]) and not torch.equal(c[1][0], c[0][0])        # another iteration: another batch
    d = _drain(ein.DataPrefetcher(_positioned(batches, tr, 2), size, tr))
    assert not torch.equal(d[0][0], a[0][0])                                          # another epoch: another batch
    # copy_paste_prob = 0 at the same seed: the transform built without the argument; with it, rows were pasted somewhere
    t0, t_old = aug.MosaicTransform(seed=9, copy_paste_prob=0.0), aug.MosaicTransform(seed=9)
    z = _drain(ein.DataPrefetcher(_positioned(batches, t0, 1), size, t0))
    o = _drain(ein.DataPrefetcher(_positioned(batches, t_old, 1), size, t_old))
    for (iz, lz), (io, lo) in zip(z, o):
        assert torch.equal(iz, io) and torch.equal(lz, lo)
    rows_with = sum(int(l.any(-1).sum()) for _, l in a)
    rows_without = sum(int(l.any(-1).sum()) for _, l in z)
    print("label rows over 3 batches: %d without, %d with copy-paste" % (rows_without, rows_with))
    assert rows_with > rows_without and any(not torch.equal(ia, iz) for (ia, _), (iz, _) in zip(a, z))


def test_training_step_on_a_pasted_batch():
    """One captured step (bf16 plan) at S = 320, width 0.25, on a batch whose images all paste: finite loss, ring guard 0, labels
    finite and inside the input."""
    from ep24 import _lib, augment as aug, loss as eloss, nn as enn, train as etrain
    S = 320
    items = [make_source(300, 400, 6, 41), make_source(260, 300, 5, 42, star=True), make_source(280, 280, 0, 43),
             make_source(240, 380, 7, 44)]
    images, targets = [it[0] for it in items], [it[1] for it in items]
    sizes = [im.shape[:2] for im in images]
    params = aug.sample_params(aug.position_rng(4, 0, 0), sizes, (S, S))
    plain = aug.mosaic_batch(images, targets, params, (S, S))
    plain = [t.clone() for t in plain]
    aug.sample_paste(aug.paste_rng(4, 0, 0), params, len(images), (S, S), 1.0, obj_prob=1.0)
    assert params.paste.all()
    img, lab, counts = aug.mosaic_batch(images, targets, params, (S, S))
    print("rows per image", plain[2].tolist(), "->", counts.tolist())
    assert int(counts.sum()) > int(plain[2].sum()) and not torch.equal(img, plain[0])
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
