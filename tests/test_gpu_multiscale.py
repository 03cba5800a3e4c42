"""Multiscale training on the GPU: the resize and label kernels (csrc/preproc.hip) bit for bit against tests/resize_oracle.py,
``ep24.multiscale.resize_batch`` / ``Exp.preprocess``, ``MultiScaleStep`` against the eager drop-in loop, its residency policy,
and ``train_24p.py --multiscale``."""
import json
import os
import sys

import numpy as np
import pytest
import torch

import resize_oracle as ro
from ep24 import synth

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
Y24 = os.path.join(ROOT, "exploration-of-potential_amd", "yolox_24p")
SENTINEL = -12345.5
MARGIN = 256                                                                    # floats on either side of the output
SEQUENCE = [128, 96, 128, 160, 96]


def cos(got, want):
    got, want = got.float().cpu().reshape(-1), want.float().cpu().reshape(-1)
    return float(torch.dot(got, want) / (got.norm() * want.norm() + 1e-20))


def launch_resize(x, oh, ow, shift=0):
    """The kernel on x [B,3,H,W] into a sentinel-framed buffer -> (output [B,3,oh,ow], the frame is untouched).  ``shift``: floats
    by which the output starts off a 16-byte boundary."""
    from ep24._lib import call, ptr, stream_ptr
    B, C, H, W = x.shape
    n = B * C * oh * ow
    buf = torch.full((MARGIN + n + MARGIN,), SENTINEL, dtype=torch.float32, device=DEV)
    lo = MARGIN // 2 + shift
    assert buf.data_ptr() % 16 == 0
    call("resize_bilinear_f32", ptr(x), B * C, H, W, ptr(buf, lo), oh, ow, stream_ptr())
    torch.cuda.synchronize()
    clean = bool((buf[:lo] == SENTINEL).all()) and bool((buf[lo + n:] == SENTINEL).all())
    return buf[lo:lo + n].reshape(B, C, oh, ow).cpu(), clean


def make_exp(input_size=(128, 128), multiscale_range=1):
    sys.path.insert(0, Y24)
    try:
        from exp import get_exp
        exp = get_exp(os.path.join(Y24, "load_train", "yolox_24p_train.py"))
    finally:
        sys.path.remove(Y24)
    exp.input_size, exp.multiscale_range = input_size, multiscale_range
    return exp


def small_model(seed=0):
    from ep24 import nn as enn
    torch.manual_seed(seed)
    m = enn.YOLOX(enn.YOLOPAFPN(0.33, 0.25), enn.YOLOXHead(80, 0.25))
    m.head.initialize_biases(1e-2)
    return m.to(DEV)


def params(model):
    return torch.cat([p.detach().reshape(-1) for p in model.parameters()]).clone()


def tracked(model):
    return int(model.backbone.backbone.stem.conv.bn.num_batches_tracked)


@pytest.mark.parametrize("B", [1, 2])
@pytest.mark.parametrize("src,dst", ro.SHAPES)
def test_resize_kernel_matches_the_oracle_bit_for_bit(src, dst, B):
    rng = np.random.default_rng(B * 100 + src[0] + dst[1])
    x = rng.uniform(0.0, 255.0, (B, 3) + tuple(src)).astype(np.float32)
    got, clean = launch_resize(torch.from_numpy(x).to(DEV), *dst)
    assert clean, "the kernel wrote outside its output"
    want = torch.from_numpy(ro.resize(x, *dst))
    assert torch.equal(got, want), float((got - want).abs().max())
    if src == dst:
        assert torch.equal(got, torch.from_numpy(x))


def test_resize_kernel_negative_and_fractional_values():
    rng = np.random.default_rng(11)
    x = (rng.standard_normal((2, 3, 96, 64)) * 100.0).astype(np.float32)
    x[0, 0, :4, :4] = [[-0.125, 0.3, -7.75, 1e-3]] * 4
    assert (x < 0).any()
    for dst, shift in (((33, 131), 0), ((128, 96), 0), ((96, 64), 0), ((128, 96), 1), ((33, 130), 2)):   # shifted: no row starts on 16 bytes
        got, clean = launch_resize(torch.from_numpy(x).to(DEV), *dst, shift=shift)
        assert clean, (dst, shift)
        assert torch.equal(got, torch.from_numpy(ro.resize(x, *dst))), (dst, shift)


@pytest.mark.parametrize("src,dst", [((8, 1), (16, 5)), ((1, 1), (3, 3)), ((3, 2), (7, 9)), ((1, 9), (1, 4))])
def test_resize_kernel_narrow_sources(src, dst):
    """One source column has no second tap to load beside the first (the kernel's other load path); two columns are the smallest pair."""
    x = (np.random.default_rng(5).standard_normal((2, 3) + src) * 10.0).astype(np.float32)
    got, clean = launch_resize(torch.from_numpy(x).to(DEV), *dst)
    assert clean
    assert torch.equal(got, torch.from_numpy(ro.resize(x, *dst)))


def test_scale_labels_kernel_is_exact_also_in_place():
    from ep24._lib import call, ptr, stream_ptr
    rng = np.random.default_rng(3)
    lab = rng.uniform(-20.0, 660.0, (3, 50, 51)).astype(np.float32)
    lab[:, :, 0] = rng.integers(0, 80, (3, 50))
    lab[0, 5:] = 0.0                                                            # zero padding rows stay zero
    lab[2] = 0.0                                                                # an image without labels
    rows = 3 * 50
    for sx, sy in ((96 / 128, 96 / 128), (160 / 128, 160 / 128), (128 / 160, 64 / 96), (0.7, 1.3)):
        want = torch.from_numpy(ro.scale_labels(lab, sx, sy))
        src = torch.from_numpy(lab).to(DEV)
        buf = torch.full((MARGIN + rows * 51 + MARGIN,), SENTINEL, dtype=torch.float32, device=DEV)
        call("scale_labels", ptr(src), ptr(buf, MARGIN), rows, sx, sy, stream_ptr())
        torch.cuda.synchronize()
        assert bool((buf[:MARGIN] == SENTINEL).all()) and bool((buf[MARGIN + rows * 51:] == SENTINEL).all())
        assert torch.equal(buf[MARGIN:MARGIN + rows * 51].reshape(3, 50, 51).cpu(), want), (sx, sy)
        assert torch.equal(src.cpu(), torch.from_numpy(lab))                    # the input is read only
        call("scale_labels", ptr(src), ptr(src), rows, sx, sy, stream_ptr())    # out == in
        torch.cuda.synchronize()
        assert torch.equal(src.cpu(), want), (sx, sy)
        assert float(want[2].abs().max()) == 0.0 and float(want[0, 5:].abs().max()) == 0.0


def test_resize_batch_and_preprocess_write_the_out_buffers():
    from ep24 import _lib, multiscale
    images = synth.make_images(2, 128, seed=1).to(DEV)
    labels = synth.make_labels(2, [4, 2], size=128, seed=2).to(DEV)
    want_i = torch.from_numpy(ro.resize(images.cpu().numpy(), 96, 160))
    want_l = torch.from_numpy(ro.scale_labels(labels.cpu().numpy(), 160 / 128, 96 / 128))
    got_i, got_l = multiscale.resize_batch(images, labels, (96, 160))
    assert torch.equal(got_i.cpu(), want_i) and torch.equal(got_l.cpu(), want_l)
    out_i = torch.full((2, 3, 96, 160), SENTINEL, device=DEV)
    out_l = torch.full((2, 50, 51), SENTINEL, device=DEV)
    ri, rl = multiscale.resize_batch(images, labels, (96, 160), out_images=out_i, out_labels=out_l)
    assert ri is out_i and rl is out_l
    assert torch.equal(out_i.cpu(), want_i) and torch.equal(out_l.cpu(), want_l)
    with pytest.raises(IndexError):
        multiscale.resize_batch(images, labels, (96, 160), out_images=torch.empty(2, 3, 96, 128, device=DEV))
    with pytest.raises(_lib.Ep24Error):
        multiscale.resize_batch(images.cpu(), labels.cpu(), (96, 160))
    # Exp.preprocess: the same two launches, out= forwarded; the identity call returns its arguments and launches nothing
    exp = make_exp()
    out_i.fill_(SENTINEL)
    out_l.fill_(SENTINEL)
    pi, pl = exp.preprocess(images, labels, (96, 160), out=(out_i, out_l))
    assert pi is out_i and pl is out_l and torch.equal(out_i.cpu(), want_i) and torch.equal(out_l.cpu(), want_l)
    qi, ql = exp.preprocess(images, labels, (96, 160))
    assert torch.equal(qi.cpu(), want_i) and torch.equal(ql.cpu(), want_l)
    assert torch.equal(labels.cpu(), synth.make_labels(2, [4, 2], size=128, seed=2))       # the caller's labels are not rewritten
    out_i.fill_(SENTINEL)
    launches = []
    plain_call = _lib.call
    _lib.call = multiscale.call = lambda name, *a: launches.append(name) or plain_call(name, *a)
    try:
        si, sl = exp.preprocess(images, labels, (128, 128), out=(out_i, out_l))
        assert launches == []
        exp.preprocess(images, labels, (96, 160), out=(out_i, out_l))
        assert launches == ["resize_bilinear_f32", "scale_labels"]
    finally:
        _lib.call = multiscale.call = plain_call
    assert si is images and sl is labels


@pytest.fixture(scope="module")
def batch():
    return synth.make_images(2, 128, seed=1).to(DEV), synth.make_labels(2, [4, 2], size=128, seed=2).to(DEV)


def run_multiscale(model, batch, max_plans, sequence=SEQUENCE):
    from ep24 import loss as eloss, multiscale
    lf = eloss.Loss_Function(80)
    lf.draw = False
    ms = multiscale.MultiScaleStep(model, lf, lr=0.01, momentum=0.9, batch=2, base_size=128, max_plans=max_plans)
    losses, most = [], 0
    for s in sequence:
        losses.append(float(ms.step(batch[0], batch[1], (s, s))[0]))
        most = max(most, len(ms.resident))
        assert {k[1] for k in model._engines} == {r[0] for r in ms.resident}, (model._engines.keys(), ms.resident)
    torch.cuda.synchronize()
    return ms, losses, most


@pytest.fixture(scope="module")
def unbounded(batch):
    """The sequence through a MultiScaleStep that keeps every plan: shared by the tests that compare against it."""
    model = small_model()
    ms, losses, most = run_multiscale(model, batch, 0)
    return model, ms, losses, most


def test_multiscale_step_matches_the_eager_loop(batch, unbounded):
    """Model A: the drop-in loop (resize, model(...), Loss_Function, backward, SGD.step) at every size of the sequence; model B:
    ``MultiScaleStep.step``.  Bounds of test_gpu_engine.test_eager_api_step_matches_captured_step."""
    from ep24 import _lib, loss as eloss, multiscale, train as etrain
    images, labels = batch
    ma = small_model()
    mb, ms, losses_b, _ = unbounded
    lf_a = eloss.Loss_Function(80)
    lf_a.draw = False
    opt = etrain.SGD(ma.parameters(), lr=0.01, momentum=0.9, nesterov=True, model=ma)
    losses_a = []
    for s in SEQUENCE:
        img, lab = (images, labels) if s == 128 else multiscale.resize_batch(images, labels, (s, s))
        opt.zero_grad()
        tup = lf_a(ma(img, train=True), lab)
        tup[0].backward()
        opt.step()
        losses_a.append(float(tup[0]))
    torch.cuda.synchronize()
    print("eager", losses_a, "multiscale", losses_b, "footprints", ms.footprints, "capture s", ms.capture_seconds)
    assert all(np.isfinite(losses_a)) and all(np.isfinite(losses_b))
    assert losses_a[0] == losses_b[0]
    np.testing.assert_allclose(losses_a, losses_b, rtol=5e-2)
    assert cos(params(ma), params(mb)) > 0.99
    assert tracked(ma) == 5 and tracked(mb) == 5          # a capture warm-up at a size first met in mid-run is not a step
    assert ms.captures == 3
    assert ms.sizes_seen == [(128, 128), (96, 96), (160, 160)] and sorted(ms.resident) == sorted(ms.sizes_seen)
    assert set(ms.footprints) == set(ms.sizes_seen) and all(b > 0 for b in ms.footprints.values())
    assert _lib.lib().fn["ep24_conv_ring_timeouts"]() == 0


def test_bounded_residency_recaptures_and_computes_the_same(batch, unbounded):
    from ep24 import _lib
    m0, ms0, losses0, most0 = unbounded
    m2 = small_model()
    ms2, losses2, most2 = run_multiscale(m2, batch, 2)
    print("unbounded", losses0, ms0.captures, "bounded", losses2, ms2.captures, ms2.evictions)
    assert most2 <= 2 and len(ms2.resident) == 2 and most0 == 3
    assert ms2.captures > ms0.captures and ms2.evictions == ms2.captures - 2
    assert torch.equal(params(m2), params(m0))
    assert tracked(m2) == 5
    assert _lib.lib().fn["ep24_conv_ring_timeouts"]() == 0


def test_setters_reach_plans_created_later(batch):
    from ep24 import loss as eloss, multiscale
    model = small_model()
    lf = eloss.Loss_Function(80)
    lf.draw = False
    ms = multiscale.MultiScaleStep(model, lf, lr=0.01, momentum=0.9, batch=2, base_size=128)
    p0 = params(model)
    ms.step(batch[0], batch[1], (128, 128))
    p1 = params(model)
    assert not torch.equal(p0, p1)
    ms.set_lr(0.0)
    ms.set_use_l1(True)
    res = ms.step(batch[0], batch[1], (96, 96))          # a plan created after the calls
    torch.cuda.synchronize()
    assert np.isfinite(float(res[0]))
    assert torch.equal(params(model), p1), "lr = 0 did not reach the new plan"
    ts = ms.plans[(96, 96)]
    assert ts.use_l1 is True and ts.lr == 0.0 and ms.plans[(128, 128)].use_l1 is True
    ms.set_lr(0.01)
    ms.step(batch[0], batch[1], (96, 96))
    torch.cuda.synchronize()
    assert not torch.equal(params(model), p1)


def run_trainer(tmp_path, extra):
    sys.path.insert(0, Y24)
    try:
        import importlib
        mod = importlib.import_module("train_24p")
        exp = make_exp()
        exp.width, exp.synthetic_len, exp.synthetic_gts = 0.25, 8, 4
        calls = []
        plain_preprocess = exp.preprocess

        def recording(inputs, targets, tsize, out=None):
            res = plain_preprocess(inputs, targets, tsize) if out is None else plain_preprocess(inputs, targets, tsize, out=out)
            calls.append((tuple(tsize), tuple(inputs.shape), tuple(res[0].shape), tuple(res[1].shape)))
            return res

        exp.preprocess = recording
        tp = os.path.join(str(tmp_path), "tp.json")
        args = mod.make_parser().parse_args(["-b", "2", "-l", "0.01", "--synthetic", "--steps", "6", "--log-interval", "1", "--loader-workers", "0",
                                             "--throughput-json", tp, "--output-dir", str(tmp_path)] + extra)
        trainer = mod.main(exp, args)
        torch.cuda.synchronize()
        return trainer, exp, calls, json.load(open(tp))
    finally:
        sys.path.remove(Y24)


def test_trainer_multiscale(tmp_path, capfd):
    from ep24.multiscale import size_for
    trainer, exp, calls, rec = run_trainer(tmp_path, ["--multiscale", "--multiscale-interval", "2", "--multiscale-seed", "6"])
    drawn = [tuple(size_for(exp, 6, 1)), tuple(size_for(exp, 6, 2))]
    assert drawn == [(160, 160), (96, 96)]                # seed 6 draws two sizes that are not the base size
    want = [(128, 128)] * 2 + [drawn[0]] * 2 + [drawn[1]] * 2
    assert [c[0] for c in calls] == want
    assert all(c[1] == (2, 3, 128, 128) for c in calls)   # loader, prefetcher and letterbox keep producing input_size canvases
    assert [c[2] for c in calls] == [(2, 3) + s for s in want] and all(c[3] == (2, 50, 51) for c in calls)
    assert trainer.run_steps == 6 and trainer.ring_timeouts() == 0
    out = capfd.readouterr().out
    losses = [float(l.split("loss")[1].split()[0]) for l in out.splitlines() if l.startswith("step ")]
    assert len(losses) == 6 and all(np.isfinite(losses)), out[-2000:]
    assert rec["multiscale"] == {"sizes": [[128, 128], [160, 160], [96, 96]], "captures": 3, "resident": 3}
    # without the flag: one size, the record as it was
    trainer, exp, calls, rec = run_trainer(tmp_path, [])
    assert [c[0] for c in calls] == [(128, 128)] * 6 and all(c[2] == (2, 3, 128, 128) for c in calls)
    assert trainer.run_steps == 6 and "multiscale" not in rec
