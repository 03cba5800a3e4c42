"""Flags of the kept entry point that need no GPU (reference parser: yolox_24p/train_24p.py:180-201)."""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
Y24 = os.path.join(ROOT, "exploration-of-potential_amd", "yolox_24p")


def test_cpu_device_is_refused(tmp_path):
    env = dict(os.environ)
    p = subprocess.run([sys.executable, os.path.join(Y24, "train_24p.py"), "-f", os.path.join(Y24, "load_train", "yolox_24p_train.py"),
                        "-b", "1", "--device", "cpu", "--steps", "1", "--output-dir", str(tmp_path)], cwd=Y24, env=env,
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    assert p.returncode != 0 and "no CPU fallback" in p.stdout, p.stdout[-2000:]


def test_parser_keeps_the_reference_flags():
    sys.path.insert(0, Y24)
    try:
        import importlib
        mod = importlib.import_module("train_24p")
        a = mod.make_parser().parse_args(["-f", "x.py", "-b", "20", "-l", "0.01", "-s", "1", "-d", "2", "--resume", "-c", "w.pth", "-e", "3",
                                          "--num_machines", "1"])
        assert (a.exp_file, a.batch_size, a.learn_rate, a.start_device, a.devices, a.resume, a.ckpt, a.start_epoch) == \
            ("x.py", 20, 0.01, 1, 2, True, "w.pth", 3)
        d = mod.make_parser().parse_args([])
        assert (d.batch_size, d.learn_rate, d.device, d.synthetic, d.steps) == (4, 0.001, "cuda", False, 0)
    finally:
        sys.path.remove(Y24)


def test_backbone_swap_exp_files():
    """BASELINE config 4 is reachable from the kept entry points: Exp.backbone_type -> YOLOPAFPN(backbone_type)."""
    sys.path.insert(0, Y24)
    try:
        from exp import get_exp
        for name, kind in (("yolox_24p_l_resnet_train.py", "ResNet"), ("yolox_24p_l_densenet_train.py", "DenseNet"), ("yolox_24p_l_train.py", "CSPDarknet")):
            exp = get_exp(os.path.join(Y24, "load_train", name))
            model = exp.get_model()
            assert type(model.backbone.backbone).__name__ == kind
            assert abs(float(model.head.cls_preds[0].bias[0]) + 4.59512) < 1e-4
    finally:
        sys.path.remove(Y24)


def test_resume_continues_the_lr_schedule():
    """A run resumed at epoch e follows the yoloxwarmcos schedule where an uninterrupted run would be (the reference derives
    progress from epoch * max_iter + iter, utils/lr_scheduler.py:20-27); --steps still counts the steps of the run itself."""
    sys.path.insert(0, Y24)
    try:
        import importlib
        mod = importlib.import_module("train_24p")
        from exp import get_exp
        exp = get_exp(os.path.join(Y24, "load_train", "yolox_24p_train.py"))
        max_iter = 16
        sched = exp.get_lr_scheduler(0.01, max_iter)
        uninterrupted = [sched.update_lr(i) for i in range(1, 4 * max_iter + 1)]
        for start_epoch in (0, 1, 3):
            step = mod.Trainer.resumed_step(start_epoch, max_iter)
            assert step == start_epoch * max_iter
            resumed = [sched.update_lr(step + i) for i in range(1, 6)]
            assert resumed == uninterrupted[step:step + 5]
        # warm-up really is over at epoch 3 of this schedule's 5 warm-up epochs?  no - so the resumed rate must differ from a restart
        assert sched.update_lr(mod.Trainer.resumed_step(3, max_iter) + 1) != sched.update_lr(1)
        a = mod.make_parser().parse_args(["--prefetch"])
        assert a.prefetch is True and mod.make_parser().parse_args([]).prefetch is False
    finally:
        sys.path.remove(Y24)


def test_raw_u8_synthetic_source_matches_the_ready_made_one():
    """--raw-u8: the synthetic items as a decoder would hand them over (uint8 HWC, label rows normalised by width / height).  Through the
    oracle's TrainTransform restatement (data_augment.py:138-174) they give the label table of the ready-made source to fp32 rounding and
    the same image up to the uint8 truncation; a long synthetic epoch repeats 64 distinct items instead of holding 5 MB per index."""
    sys.path.insert(0, Y24)
    try:
        import numpy as np
        import torch
        from datasets import SyntheticDataset, raw_collate
        from oracle import input as oin
        ready, raw = SyntheticDataset(200, 64, 3), SyntheticDataset(200, 64, 3, raw=True)
        for idx in (0, 5, 63, 64 + 5):
            img, lab, hw, ident = ready[idx]
            rimg, rows, rhw, rident = raw[idx]
            assert ident == rident == idx and tuple(hw) == tuple(rhw) == (64, 64)
            assert rimg.dtype == torch.uint8 and tuple(rimg.shape) == (64, 64, 3) and rows.shape == (3, 51)
            out_img, out_lab = oin.train_transform(rimg.numpy(), rows.copy(), (64, 64))
            assert np.array_equal(out_img, img.to(torch.uint8).float().numpy())
            np.testing.assert_allclose(out_lab, lab.numpy(), rtol=1e-6, atol=1e-4)
        assert torch.equal(raw[5][0], raw[64 + 5][0]) and len(raw._cache) <= 64
        ims, rws, _, ids = raw_collate([raw[0], raw[1]])
        assert len(ims) == 2 and ids == [0, 1] and rws[1].shape == (3, 51)
        mod = __import__("train_24p")
        a = mod.make_parser().parse_args(["--raw-u8", "--dp-wire", "bf16", "--no-prefetch", "--synthetic-len", "640"])
        assert a.raw_u8 and a.dp_wire == "bf16" and a.no_prefetch and a.synthetic_len == 640
        assert mod.make_parser().parse_args([]).dp_wire == "fp32"
    finally:
        sys.path.remove(Y24)


def test_plan_options_are_per_model_objects():
    """What changes kernels or plans is an immutable option object attached to a model (ep24.options), not a process global."""
    sys.path.insert(0, os.path.join(ROOT, "exploration-of-potential_amd"))
    from ep24.options import DEFAULT, PlanOptions, get_options, set_options
    import torch
    o = PlanOptions.parse("merge_csp=0,forward_lanes=3,bwd_cuts=u4,conv_kernel_opts=1")
    assert (o.merge_csp, o.merge_head, o.forward_lanes, o.bwd_cuts, o.conv_kernel_opts) == (False, True, 3, (0.25, 0.5, 0.75), 1)
    assert PlanOptions.parse("") == DEFAULT and PlanOptions.parse("bwd_cuts=0.5:0.9").bwd_cuts == (0.5, 0.9)
    try:
        PlanOptions.parse("no_such_option=1")
        raise AssertionError("unknown option accepted")
    except ValueError:
        pass
    for text in ("conv_kernel_opts=256", "conv_kernel_opts=16"):        # a kernel option the library would refuse at its first launch
        try:
            PlanOptions.parse(text)
            raise AssertionError(text + " accepted")
        except ValueError:
            pass
    assert PlanOptions.parse("conv_kernel_opts=1").conv_kernel_opts == 1 and PlanOptions.parse("conv_kernel_opts=137").conv_kernel_opts == 137
    a, b = torch.nn.Linear(2, 2), torch.nn.Linear(2, 2)
    set_options(a, o)
    assert get_options(a) is o and get_options(b) is DEFAULT          # another model in the same process is untouched
    src = open(os.path.join(ROOT, "exploration-of-potential_amd", "ep24", "engine.py")).read() + \
        open(os.path.join(ROOT, "exploration-of-potential_amd", "ep24", "train.py")).read() + \
        open(os.path.join(ROOT, "exploration-of-potential_amd", "ep24", "dp.py")).read()
    assert "os.environ" not in src                                     # no environment switches on the product path


def test_update_chunks_only_cover_completed_gradients():
    """ep24.train.TrainStep._update_chunks (pure host logic): a piece of the flat buffer may be updated after weight-gradient-lane
    segment k only if every element in it was written by an entry of a segment <= k or is written by nobody (alignment padding),
    and the pieces tile a suffix of the buffer without gaps or overlaps."""
    import random
    import types
    sys.path.insert(0, os.path.join(ROOT, "exploration-of-potential_amd"))
    from ep24.train import TrainStep
    rnd = random.Random(7)
    for trial in range(20):
        # parameters in execution order: backward writes them from the tail, a few entries late (the slab reduce of a later segment)
        sizes = [rnd.choice([16, 64, 256, 1000, 4096, 30000]) for _ in range(rnd.randint(12, 60))]
        offs, n = [], 0
        for sz in sizes:
            offs.append(n)
            n += (sz + 3) // 4 * 4 + rnd.choice([0, 0, 4])            # some padding nobody writes
        order = list(range(len(sizes)))[::-1]
        for _ in range(len(order) // 4):                              # a few gradients complete later than their neighbours
            i = rnd.randrange(len(order) - 1)
            order[i], order[i + 1] = order[i + 1], order[i]
        nseg = rnd.randint(4, 9)
        per = (len(order) + nseg - 1) // nseg
        bwd_writes, segs = [], []
        for s in range(nseg):
            lo = len(bwd_writes)
            for j in order[s * per:(s + 1) * per]:
                bwd_writes.append([(offs[j], sizes[j])])
                bwd_writes.append([])                                 # entries that write no parameter gradient
            segs.append((lo, len(bwd_writes)))
        segs = [sg for sg in segs if sg[1] > sg[0]]
        fake = types.SimpleNamespace(eng=types.SimpleNamespace(bwd_writes=bwd_writes), home=types.SimpleNamespace(numel=n))
        k_early = len(segs) - 1
        chunks, lo_all = TrainStep._update_chunks(fake, segs, k_early)
        written_by = {}
        for k, (lo, hi) in enumerate(segs):
            for i in range(lo, hi):
                for off, cnt in bwd_writes[i]:
                    for e in range(off, off + cnt):
                        written_by[e] = k
        prev = n
        for k in sorted(chunks):
            lo, hi = chunks[k]
            assert hi == prev and lo < hi and lo % 4 == 0, (trial, chunks)
            assert all(written_by.get(e, -1) <= k for e in range(lo, hi)), (trial, k, chunks[k])
            prev = lo
        assert prev == lo_all


def test_ring_guard_stops_the_run_before_a_checkpoint_is_written(tmp_path):
    """VERDICT r4 item 3 / ADVICE r4: a given-up wait of a ring kernel (ep24_conv_ring_timeouts != 0) means wrong convolutions since
    that launch; the trainer must raise BEFORE save_checkpoint touches the directory, not once at the end of the run."""
    sys.path.insert(0, Y24)
    try:
        import importlib
        import pytest
        import torch
        mod = importlib.import_module("train_24p")
        tr = mod.Trainer.__new__(mod.Trainer)                       # no GPU: only the pieces save_ckpt touches
        tr.file_name, tr.epoch, tr.epoch_complete, tr.current_step, tr.ema_model = str(tmp_path), 0, True, 7, None
        tr.model = torch.nn.Linear(2, 2)
        tr.optimizer = torch.optim.SGD(tr.model.parameters(), lr=0.1)
        counter = [0]
        tr.ring_timeouts = lambda: counter[0]
        tr.save_ckpt("last_epoch")                                   # a clean counter: the checkpoint is written
        good = os.path.join(str(tmp_path), "last_epoch_ckpt.pth")
        assert os.path.exists(good)
        stamp = (os.path.getmtime(good), os.path.getsize(good))
        counter[0] = 3
        with torch.no_grad():
            tr.model.weight.fill_(float("nan"))                      # what a broken hand-off would have trained
        with pytest.raises(RuntimeError, match="ep24_conv_ring_timeouts"):
            tr.save_ckpt("last_epoch")
        assert (os.path.getmtime(good), os.path.getsize(good)) == stamp and os.listdir(str(tmp_path)) == ["last_epoch_ckpt.pth"]
        assert torch.isfinite(torch.load(good)["model"]["weight"]).all()   # the last good one is still there
        with pytest.raises(RuntimeError):
            tr.check_ring_guard()                                    # the log-interval / end-of-run call site
        # the loop calls the guard at the log interval and save_ckpt calls it first: pinned on the source so a refactor cannot drop it
        import inspect
        src = inspect.getsource(mod.Trainer.train)
        assert src.count("self.check_ring_guard()") >= 2 and src.index("self.TB_data(res") < src.index("self.check_ring_guard()")
        assert inspect.getsource(mod.Trainer.save_ckpt).index("check_ring_guard") < inspect.getsource(mod.Trainer.save_ckpt).index("save_checkpoint(")
    finally:
        sys.path.remove(Y24)


def test_resumed_epoch_continues_at_the_data_position():
    """resuming inside an epoch skips the batches the checkpointed run had trained on (once), keeps len() = the whole epoch,
    and the following epochs start at index 0 again; also under a DistributedSampler shard."""
    sys.path.insert(0, Y24)
    try:
        import torch
        from datasets import ResumableSampler
        data = list(range(23))
        s = ResumableSampler(torch.utils.data.SequentialSampler(data))
        loader = torch.utils.data.DataLoader(data, batch_size=4, drop_last=True, sampler=s)
        assert len(loader) == 5 and [b.tolist() for b in loader][0] == [0, 1, 2, 3]
        s.start = 2 * 4                                               # two iterations of this epoch were done before the checkpoint
        got = [b.tolist() for b in loader]
        assert got == [[8, 9, 10, 11], [12, 13, 14, 15], [16, 17, 18, 19]] and len(loader) == 5
        assert [b.tolist() for b in loader][0] == [0, 1, 2, 3]        # the next epoch is whole again
        d = ResumableSampler(torch.utils.data.distributed.DistributedSampler(data, num_replicas=2, rank=1, shuffle=False))
        d.set_epoch(3)
        whole = list(d)
        d.start = 5
        assert list(d) == whole[5:] and list(d) == whole and len(d) == 12
        from exp import get_exp
        exp = get_exp(os.path.join(Y24, "load_train", "yolox_24p_train.py"))
        exp.synthetic_len = 8
        ld = exp.get_data_loader(2, raw_u8=True, workers=0)
        assert isinstance(ld.sampler, ResumableSampler) and len(ld) == 4
        ld.sampler.start = 3 * 2
        assert len(list(ld)) == 1 and len(list(ld)) == 4
    finally:
        sys.path.remove(Y24)
