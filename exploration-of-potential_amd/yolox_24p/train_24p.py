"""Training entry point with the reference's flags (yolox_24p/train_24p.py:180-211):

    cd exploration-of-potential_amd/yolox_24p
    python train_24p.py -f load_train/yolox_24p_l_train.py -b 20 -l 0.01
    python -m torch.distributed.run --nproc-per-node 8 --master-addr 127.0.0.1 train_24p.py -f ... -b 20 -l 0.01

The step body of the reference ``Trainer.train`` (:80-111: zero_grad, forward, Loss_Function, backward, SGD step) runs
as ONE captured hipGraph (``ep24.train.TrainStep``); ``--no-graph`` runs the same kernels through the reference-style
eager API (model(...), loss_func.forward(...), loss.backward(), optimizer.step()).  Scalars are logged from a single
packed device->host copy every ``--log-interval`` steps instead of ~54 per-step ``add_scalar`` syncs (:115-137).
Under torch.distributed.run every rank trains on its own shard (DistributedSampler in Exp.get_data_loader), rank 0's
parameters are broadcast once, and gradients are averaged over RCCL (ep24.dp).

The reference carries three more pieces that its 24p trainer never switches on; they are opt-in
here and all of them run inside the captured step: ``--sched`` follows ``exp.get_lr_scheduler`` (yoloxwarmcos,
exp/yolox_base.py:155-167) per iteration, ``--ema`` keeps a ``ModelEMA`` copy (utils/ema.py) that is saved with the
checkpoint, ``--l1`` turns ``use_l1`` on for head and loss from epoch ``exp.L1_epoch`` on (exp/yolox_base.py:38).
``--weight-decay [W]`` is the fourth piece of that recipe: stock YOLOX's three optimizer groups (yolox/exp/yolox_base.py:198-224),
``exp.weight_decay`` (or W) on every weight that is not a BatchNorm's, applied by the fused update itself.
``--multiscale`` is the fifth: every ``--multiscale-interval`` steps a new input size (``exp.random_resize``, core/trainer.py:250-254),
the batch and its labels resized on the GPU (``exp.preprocess``), one captured step per size (``ep24.multiscale.MultiScaleStep``).
"""
import argparse
import os
import time

import _path  # noqa: F401
import torch

from exp import get_exp
from models import Loss_Function
from utils import save_checkpoint

try:
    from torch.utils.tensorboard import SummaryWriter
except Exception:                                         # tensorboard is optional
    SummaryWriter = None


class Trainer:
    def __init__(self, exp, args):
        self.exp, self.args = exp, args
        self.max_epoch = exp.max_epoch
        self.L1_epoch = exp.L1_epoch
        self.start_device, self.numb_device = args.start_device, args.devices
        self.world = int(os.environ.get("WORLD_SIZE", 1))
        self.rank = int(os.environ.get("RANK", 0))
        if getattr(args, "eval_interval", 0) and self.world > 1:
            raise SystemExit("train_24p.py: --eval-interval under WORLD_SIZE=%d: distributed evaluation (gathering records across "
                             "ranks) is not implemented; evaluate the saved checkpoints in a single-process run" % self.world)
        local = int(os.environ.get("LOCAL_RANK", args.start_device))
        dev = torch.device(args.device)
        if dev.type != "cuda":
            # SURVEY 5 lists --device for the reference's plumbing run (BASELINE config 1).  This build is the GPU path only:
            # there is no CPU fallback behind the C ABI, and the trainer says so instead of silently running something else.
            from ep24._lib import Ep24Error
            raise Ep24Error("train_24p.py --device %s: the ep24 path runs on an MI355X only (no CPU fallback); the CPU "
                            "restatement lives in oracle/ and is test infrastructure" % args.device)
        self.device = torch.device("cuda", dev.index if dev.index is not None else local)
        self.input_size = exp.input_size
        self.file_name = os.path.join(exp.output_dir, exp.exp_name)
        self.current_step = 0                             # global step (epoch * max_iter + iter): schedule / TensorBoard axis
        self.run_steps = 0                                # steps of THIS run: what --steps limits
        os.makedirs(self.file_name, exist_ok=True)
        check_data_args(args)
        if not args.synthetic and not getattr(args, "data_dir", None):
            print("note: the COCO24P loader of the reference reads hard-coded paths (datasets/coco24p.py:19-20) and is out of "
                  "scope; the synthetic source with the same label layout is used (--synthetic)")
        # Round 5: the raw uint8 source is the DEFAULT (0.98 of bench.py against 0.91 for ready-made fp32 canvases from four loader
        # processes, profiles/r04_trainer.json; one host core per rank instead of five: profiles/r05_trainer_8sets.json).
        # --fp32-batches restores the reference's form of the source; --no-prefetch implies it (raw batches are letterboxed by the
        # prefetcher's side stream).
        if args.raw_u8 and (args.no_prefetch or args.fp32_batches):
            raise SystemExit("train_24p.py: --raw-u8 batches are letterboxed by the prefetcher (drop --no-prefetch / --fp32-batches)")
        args.raw_u8 = not (args.fp32_batches or args.no_prefetch)
        if args.augment and not args.raw_u8:
            raise SystemExit("train_24p.py: --augment works on the raw uint8 batches behind the prefetcher (drop --no-prefetch / --fp32-batches)")
        check_mixup_args(args)
        check_copy_paste_args(args)
        if check_eval_tta_args(args):
            raise SystemExit("train_24p.py: " + check_eval_tta_args(args))
        check_multiscale_args(args, exp, self.world)
        if args.fisheye_theta is not None:
            check_fisheye_args(args)
        check_fisheye_lens_args(args)
        self.train_loader = exp.get_data_loader(args.batch_size, raw_u8=bool(args.raw_u8), workers=args.loader_workers,
                                                 pin=None if args.loader_pin is None else bool(args.loader_pin))
        self.loss_func = Loss_Function(exp.num_classes)
        self.loss_func.draw = False

    def train(self):
        from ep24 import dp
        from ep24.train import TrainStep
        args, exp = self.args, self.exp
        torch.cuda.set_device(self.device)
        reducer = None
        if self.world > 1:
            torch.distributed.init_process_group("nccl", device_id=self.device)
            # fp32 buckets like the reference's DDP (core/trainer.py:163) unless asked: --dp-wire bf16 halves the xGMI bytes
            reducer = dp.GradReducer(comm_dtype=torch.bfloat16 if args.dp_wire == "bf16" else None)
        torch.manual_seed(0)                              # identical replicas on every rank (made explicit by the reducer's broadcast)
        model = exp.get_model()
        model.to(self.device)
        self.model = model
        self.optimizer = exp.get_optimizer(args.learn_rate, weight_decay_arg(args, exp))
        self.max_iter = len(self.train_loader)
        # -c / --resume / -e: the reference's parser accepts them and its trainer never reads them (train_24p.py:180-211); here
        # they load what save_ckpt wrote.  The checkpoint goes in AFTER get_model() (which re-applies the bias prior on every
        # call, exp/yolox_base.py:70-71) so the loaded predictor biases survive; --resume also restores momentum and epoch.
        self.start_epoch, ck, resumed_step = 0, None, None
        if args.ckpt:
            from utils import load_ckpt
            ck = torch.load(args.ckpt, map_location="cpu")
            load_ckpt(model, ck.get("model", ck))
            if args.resume:
                if "optimizer" in ck:
                    self.optimizer.load_state_dict(ck["optimizer"])
                self.start_epoch = int(ck.get("start_epoch", 0))
                if "global_step" in ck:                   # written by this trainer: exact also when --steps cut an epoch short
                    resumed_step = int(ck["global_step"])
        if args.start_epoch is not None:
            self.start_epoch, resumed_step = args.start_epoch, None
        # progress = epoch * max_iter + iter, as the reference's schedulers / loggers count it: a resumed run continues the
        # learning-rate schedule and the TensorBoard axis where the checkpoint stopped instead of restarting the warm-up
        self.current_step = self.resumed_step(self.start_epoch, self.max_iter) if resumed_step is None else resumed_step
        # iterations of the start epoch that the checkpointed run had already done (a run cut short by --steps inside an epoch)
        skip_iters = min(max(self.current_step - self.start_epoch * self.max_iter, 0), self.max_iter)
        # ... and the DATA position with it: the loader's first pass leaves those batches out (the epoch's first batches
        # were trained twice and its tail never ran)
        if skip_iters and hasattr(self.train_loader.sampler, "start"):
            self.train_loader.sampler.start = skip_iters * args.batch_size
        if args.throughput_json and args.steps and args.steps <= args.throughput_window:
            print("train_24p.py: --throughput-window %d clamped to --steps %d - 1" % (args.throughput_window, args.steps))
            args.throughput_window = max(args.steps - 1, 1)
        self.tblogger = SummaryWriter(self.file_name) if (SummaryWriter and self.rank == 0) else None
        self.lr_scheduler = exp.get_lr_scheduler(args.learn_rate, self.max_iter) if args.sched else None
        self.ema_model = None
        if args.ema:
            from utils import ModelEMA
            self.ema_model = ModelEMA(model, 0.9998)
            if ck is not None and args.resume and "ema_model" in ck:
                self.ema_model.ema.load_state_dict(ck["ema_model"])
                self.ema_model.updates = int(ck.get("ema_updates", 0))
        step_fn = None
        multiscale = bool(getattr(args, "multiscale", False))
        tsize = tuple(self.input_size)                    # --multiscale: the size of the step; redrawn every --multiscale-interval steps
        if multiscale:
            from ep24.multiscale import MultiScaleStep, size_for
            step_fn = MultiScaleStep(model, self.loss_func, lr=args.learn_rate, momentum=exp.momentum, batch=args.batch_size,
                                     base_size=tuple(self.input_size), ema=self.ema_model, weight_decay=self.optimizer.weight_decay,
                                     max_plans=args.multiscale_plans)
            if self.current_step >= args.multiscale_interval:     # a resumed run: the size its last draw had chosen
                tsize = tuple(size_for(exp, args.multiscale_seed, self.current_step // args.multiscale_interval))
        elif not args.no_graph:
            # the optimizer's decay, not the flag's: --resume has restored the checkpoint's value by now
            step_fn = TrainStep(model, self.loss_func, lr=args.learn_rate, momentum=exp.momentum, batch=args.batch_size,
                                size=tuple(self.input_size), reducer=reducer, ema=self.ema_model, weight_decay=self.optimizer.weight_decay)
        print("Training start... (rank %d/%d, %s)" % (self.rank, self.world, "captured step" if step_fn else "eager API"))
        done = False
        self.epoch = self.start_epoch
        self.epoch_complete = False
        tp_t0 = tp_seen = tp_dt = None                    # --throughput-json: a synchronised window over the run's last steps
        for epoch in range(self.start_epoch, self.max_epoch):
            self.epoch = epoch
            model.train()
            if hasattr(self.train_loader.sampler, "set_epoch"):
                self.train_loader.sampler.set_epoch(epoch)
            t0, seen = time.time(), 0
            if args.l1 and epoch >= self.L1_epoch and not self.loss_func.use_l1:
                model.head.use_l1 = self.loss_func.use_l1 = True
                if step_fn is not None:
                    step_fn.set_use_l1(True)
            self.epoch_complete = False
            for it, (images, labels) in enumerate(self.batches()):
                if epoch == self.start_epoch and it + skip_iters >= self.max_iter:
                    self.epoch_complete = True            # that was the rest of a resumed partial epoch
                    break
                if args.throughput_json and args.steps and self.run_steps == args.steps - args.throughput_window:
                    torch.cuda.synchronize()
                    tp_t0, tp_seen = time.perf_counter(), 0
                    host = {"loader_and_upload": 0.0, "step_enqueue": 0.0, "rest": 0.0}
                    pf0 = getattr(self, "prefetcher", None)
                    pf_mark = (pf0.t_loader, pf0.t_upload) if pf0 is not None else None
                    t_mark = tp_t0
                elif tp_t0 is not None:                   # host time of the window by phase: what the loop's own thread spends where
                    now = time.perf_counter()
                    host["loader_and_upload"] += now - t_mark
                    t_mark = now
                self.current_step += 1
                self.run_steps += 1
                if self.lr_scheduler is not None:
                    lr = self.lr_scheduler.update_lr(self.current_step)
                    for group in self.optimizer.param_groups:
                        group["lr"] = lr
                    if step_fn is not None:
                        step_fn.set_lr(lr)
                if multiscale:
                    images, labels = exp.preprocess(images, labels, tsize, out=step_fn.inputs(tsize))
                else:
                    images, labels = exp.preprocess(images, labels, self.input_size)
                if multiscale:
                    res = step_fn.step(images, labels, tsize)
                    if self.current_step % args.multiscale_interval == 0:     # the reference's (progress_in_iter + 1) % 10 == 0
                        tsize = tuple(size_for(exp, args.multiscale_seed, self.current_step // args.multiscale_interval))
                elif step_fn is not None:
                    res = step_fn.step(images, labels)
                else:
                    self.optimizer.zero_grad()
                    loss_all = self.loss_func.forward(model(images, train=True), labels)
                    loss_all[0].backward()
                    if reducer is not None:
                        if reducer.flat is None:
                            eng = model.engine(images.shape[0], (images.shape[2], images.shape[3]))
                            reducer.attach(eng.home, eng)
                        reducer.reduce_all()
                    self.optimizer.step(grad_scale=1.0 / self.world)
                    if self.ema_model is not None:
                        self.ema_model.update(model)
                    res = self.loss_func._ws.result
                seen += images.shape[0]
                if tp_t0 is not None:
                    tp_seen += images.shape[0]
                    now = time.perf_counter()
                    host["step_enqueue"] += now - t_mark
                    t_mark = now
                if self.current_step % args.log_interval == 0:
                    self.TB_data(res, seen * self.world / (time.time() - t0))
                    self.check_ring_guard()               # the log line has synchronised already
                if tp_t0 is not None:
                    now = time.perf_counter()
                    host["rest"] += now - t_mark
                    t_mark = now
                if args.steps and self.run_steps >= args.steps:
                    if tp_t0 is not None:                 # the window ends HERE: the checkpoint written below is not training time
                        torch.cuda.synchronize()          # (rounds 3-5 measured it inside the window: ~0.25 s, 1.2 ms per step of 200)
                        tp_dt = time.perf_counter() - tp_t0
                    done = True
                    break
            else:
                self.epoch_complete = True
            if self.current_step >= (epoch + 1) * self.max_iter:
                self.epoch_complete = True                # --steps ended the run exactly on the epoch's last iteration
            if self.rank == 0:
                self.save_ckpt("last_epoch")
            if args.eval_interval and self.epoch_complete and (epoch + 1) % args.eval_interval == 0:
                self.evaluate_and_save_model()
            if done:
                break
        if tp_t0 is not None:
            if tp_dt is None:                             # the epochs ran out before --steps did
                torch.cuda.synchronize()
                tp_dt = time.perf_counter() - tp_t0
            dt = tp_dt
            if self.rank == 0:
                import json
                rec = {"images_per_s": round(tp_seen * self.world / dt, 2), "ms_per_step": round(dt / max(args.throughput_window, 1) * 1e3, 3),
                       "window_steps": args.throughput_window, "run_steps": self.run_steps, "batch_per_gpu": args.batch_size, "world": self.world,
                       "input_size": list(self.input_size), "prefetch": not args.no_prefetch, "raw_u8": bool(args.raw_u8),
                       "captured_step": step_fn is not None, "log_interval": args.log_interval, "exp_file": args.exp_file,
                       "loader_workers": self.train_loader.num_workers, "loader_pin": bool(self.train_loader.pin_memory),
                       "host_ms_per_step": {k: round(v / max(args.throughput_window, 1) * 1e3, 3) for k, v in host.items()}}
                pf1 = getattr(self, "prefetcher", None)
                if pf1 is not None and pf_mark is not None:      # of loader_and_upload: the loader's own work / the (blocking) upload enqueue
                    rec["host_ms_per_step"]["loader_only"] = round((pf1.t_loader - pf_mark[0]) / max(args.throughput_window, 1) * 1e3, 3)
                    rec["host_ms_per_step"]["upload_enqueue_blocking"] = round((pf1.t_upload - pf_mark[1]) / max(args.throughput_window, 1) * 1e3, 3)
                if multiscale:
                    rec["multiscale"] = {"sizes": [list(s) for s in step_fn.sizes_seen], "captures": step_fn.captures,
                                         "resident": len(step_fn.resident)}
                with open(args.throughput_json, "w") as fh:
                    json.dump(rec, fh)
                print("throughput %s" % json.dumps(rec))
        self.check_ring_guard()
        if self.world > 1:
            torch.distributed.destroy_process_group()

    def evaluate_and_save_model(self):
        """COCO-style AP of the EMA model (--ema) or the model on the Exp's validation loader (exp.eval, ep24.evaluate), logged
        and written to TensorBoard as val/COCOAP50 / val/COCOAP50_95; the best AP50:95 so far is saved as best_ckpt.pth.  Runs
        between epochs: the eval-mode plans and folded weights are separate buffers, so the captured step replays unchanged."""
        if getattr(self, "evaluator", None) is None:
            self.evaluator = self.exp.get_evaluator(self.args.batch_size)
            self.best_ap = -1.0
        model = self.ema_model.ema if self.ema_model is not None else self.model
        ap50_95, ap50, summary = self.exp.eval(model, self.evaluator, False)
        self.model.train()
        if self.rank == 0:
            print("eval epoch %d  AP50_95 %.4f  AP50 %.4f  (%d images)\n%s" % (self.epoch + 1, ap50_95, ap50, self.evaluator.seq, summary))
            if self.tblogger is not None:
                self.tblogger.add_scalar("val/COCOAP50", ap50, self.epoch + 1)
                self.tblogger.add_scalar("val/COCOAP50_95", ap50_95, self.epoch + 1)
            is_best = ap50_95 > self.best_ap
            self.best_ap = max(self.best_ap, ap50_95)
            self.save_ckpt("last_epoch", update_best_ckpt=is_best)

    @staticmethod
    def ring_timeouts():
        from ep24 import _lib
        return _lib.lib().fn["ep24_conv_ring_timeouts"]()

    def check_ring_guard(self):
        """A bounded wait of a loader / consumer ring kernel that gives up carries on with whatever is in LDS (by design: a protocol
        error must never hang the GPU), so the convolutions of that launch are wrong.  Never seen outside development builds; read at
        every log interval, BEFORE every checkpoint and at the end of the run, so that a run with a broken hand-off stops without
        overwriting its last good checkpoint (the reference's cadence: train_24p.py:139-154)."""
        n = self.ring_timeouts()
        if n != 0:
            raise RuntimeError("train_24p.py: %d bounded wait(s) of the loader / consumer ring kernels gave up (ep24_conv_ring_timeouts) at "
                               "step %d: the run stops and no checkpoint is written over the last good one" % (n, self.current_step))

    @staticmethod
    def resumed_step(start_epoch, max_iter):
        """Global step a run that starts at ``start_epoch`` continues from (reference: epoch * max_iter + iter)."""
        return int(start_epoch) * int(max_iter)

    def batches(self):
        """One epoch of (images, labels) on the device.  Default (round 4): the reference's ``DataPrefetcher``
        (data/data_prefetcher.py:16-51) in its ep24 form - the next batch is uploaded (and, for ``--raw-u8`` batches, letterboxed by
        ``TrainTransform.batch``) on a side stream while the current step runs.  ``--no-prefetch``: the loader's
        tensors uploaded on the compute stream, what the reference's 24p loop does (train_24p.py:86-88) - measured at BASELINE
        config 2 it leaves the GPU idle for the 98 MB upload of every step (profiles/r04_trainer.json)."""
        if self.args.no_prefetch:
            for images, labels, _info, _ids in self.train_loader:
                yield images.to(self.device, non_blocking=True), labels.to(self.device, non_blocking=True)
            return
        from ep24.input import DataPrefetcher, TrainTransform
        if self.args.augment:
            pf = DataPrefetcher(self.positioned(self.train_loader), tuple(self.input_size), self.augment_transform())
        elif self.args.fisheye_theta is not None:
            pf = DataPrefetcher(self.positioned(self.train_loader), tuple(self.input_size), self.fisheye_transform())
        elif getattr(self.args, "fisheye_lens", None):
            pf = DataPrefetcher(self.positioned(self.train_loader), tuple(self.input_size), self.lens_transform())
        else:
            pf = DataPrefetcher(self.train_loader, tuple(self.input_size), TrainTransform(max_labels=50))
        self.prefetcher = pf                              # its t_loader / t_upload split the throughput record's host time
        if self.args.resident_batch:                      # diagnostic: what the input pipeline costs the GPU (tools/trainer_timing.sh)
            images, labels = pf.next()
            for _ in range(len(self.train_loader)):
                yield images, labels
            return
        while True:
            images, labels = pf.next()
            if images is None:
                return
            yield images, labels

    def augment_transform(self):
        """--augment: ONE ``MosaicTransform`` for the run (the Exp's mosaic_prob / degrees / translate / mosaic_scale / shear /
        flip_prob / hsv_prob), switched on for epochs < max_epoch - no_aug_epochs and off after - what ``no_aug_epochs`` means in
        YOLOX (core/trainer.py before_epoch: close_mosaic).  --mixup adds the Exp's mixup_prob / mixup_scale iff exp.enable_mixup;
        mixup goes off with the rest.  --copy-paste [P] sets the Exp's copy_paste_prob to P and adds copy-paste; it goes off with
        the rest too."""
        if getattr(self, "transform", None) is None:
            from datasets import MosaicTransform
            mixup = bool(getattr(self.args, "mixup", False) and self.exp.enable_mixup)
            paste = float(getattr(self.args, "copy_paste", 0.0) or 0.0)
            if paste > 0:
                self.exp.copy_paste_prob = paste
            self.transform = MosaicTransform.from_exp(self.exp, max_labels=50, seed=self.args.augment_seed, mixup=mixup,
                                                      copy_paste=paste > 0)
        self.transform.enabled = self.epoch < self.max_epoch - self.exp.no_aug_epochs
        return self.transform

    def fisheye_transform(self):
        """--fisheye-theta LO HI: ONE ``FisheyeTransform`` for the run - every image through the sector warp at an angle drawn per
        image, its 24-point labels through the same warp (ep24.fisheye)."""
        if getattr(self, "transform", None) is None:
            from ep24.fisheye import FisheyeTransform
            self.transform = FisheyeTransform(theta=tuple(self.args.fisheye_theta), max_labels=50, seed=self.args.augment_seed)
        return self.transform

    def lens_transform(self):
        """--fisheye-lens FILE [FILE ...]: ONE ``LensTransform`` for the run - every image and its 24-point labels as one of the
        calibrated lenses sees them (ep24.lens), a lens drawn per image.  A file's ``size`` says which frame its intrinsics are for;
        without one they are taken as given for the Exp's input_size."""
        if getattr(self, "transform", None) is None:
            from ep24.lens import LensModel, LensTransform
            models = []
            for path in self.args.fisheye_lens:
                m = LensModel.from_json(path)
                if m.size is None:
                    m.size = (int(self.exp.input_size[0]), int(self.exp.input_size[1]))
                models.append(m)
            self.transform = LensTransform(models, max_labels=50, seed=self.args.augment_seed)
        return self.transform

    def positioned(self, loader):
        """The loader's raw batches, each one behind ``set_position(epoch, iteration of the epoch)``: the prefetcher transforms a
        batch right after it has drawn it, so every batch gets the parameters of its own data position (also in a resumed epoch,
        whose first batches the sampler leaves out)."""
        first = getattr(loader.sampler, "start", 0) // max(self.args.batch_size, 1)
        for it, batch in enumerate(loader, first):
            self.transform.set_position(self.epoch, it)
            yield batch

    def TB_data(self, res, ips):
        """One D2H copy of the packed result vector: [0] loss, [1..24] weighted IOU losses, [25] conf, [26] cls,
        [29..52] iou weights, [53] obj_w, [54] cls_w (same scalars as the reference's TB_data)."""
        r = res.detach().float().cpu().tolist()
        if self.rank == 0:
            print("step %d  loss %.4f  conf %.4f  cls %.4f  num_fg %.0f  %.1f img/s" % (self.current_step, r[0], r[25], r[26], r[55], ips))
        if self.tblogger is None:
            return
        s = self.current_step
        for i in range(24):
            self.tblogger.add_scalar("Loss/IOU_Loss_{}".format(i), r[1 + i], s)
            self.tblogger.add_scalar("Weights/iou_w_{}".format(i), r[29 + i], s)
        self.tblogger.add_scalar("Loss/Total_Loss", r[0], s)
        self.tblogger.add_scalar("Loss/Confi_Loss", r[25], s)
        self.tblogger.add_scalar("Loss/Class_Loss", r[26], s)
        self.tblogger.add_scalar("Weights/obj_w", r[53], s)
        self.tblogger.add_scalar("Weights/cls_w", r[54], s)

    def save_ckpt(self, ckpt_name, update_best_ckpt=False):
        # the reference's three keys (train_24p.py:144-148) plus the global step: "start_epoch" is the first epoch that is NOT complete
        # (a run cut short by --steps inside an epoch resumes that epoch at the step it stopped, not at the next epoch's first step)
        self.check_ring_guard()                           # raises before anything is written
        state = {"start_epoch": self.epoch + (1 if self.epoch_complete else 0), "model": self.model.state_dict(),
                 "optimizer": self.optimizer.state_dict(), "global_step": self.current_step}
        if self.ema_model is not None:
            state["ema_model"], state["ema_updates"] = self.ema_model.ema.state_dict(), self.ema_model.updates
        save_checkpoint(state, update_best_ckpt, self.file_name, ckpt_name)


def weight_decay_arg(args, exp):
    """--weight-decay absent: None (one optimizer group, no decay - the 24-point trainer's optimizer); the bare flag: the Exp's
    ``weight_decay``; with a value: that value."""
    w = getattr(args, "weight_decay", None)
    if w is None:
        return None
    w = float(exp.weight_decay if w is EXP_VALUE else w)
    if w < 0:
        raise SystemExit("train_24p.py: --weight-decay %r is negative" % w)
    return w


def check_data_args(args):
    """--data-dir / --label-dir: a folder of JPEG files and one of txt labels (datasets.COCO24PFolderDataset).  Its batches are raw
    (images of any sizes, entropy-decoded in the loader processes, finished and letterboxed on the GPU behind the prefetcher)."""
    data, label = getattr(args, "data_dir", None), getattr(args, "label_dir", None)
    val_data, val_label = getattr(args, "val_data_dir", None), getattr(args, "val_label_dir", None)
    if (data is None) != (label is None):
        raise SystemExit("train_24p.py: --data-dir and --label-dir go together (images <stem>.jpg, labels <stem>.txt)")
    if (val_data is None) != (val_label is None):
        raise SystemExit("train_24p.py: --val-data-dir and --val-label-dir go together")
    if data is None and val_data is None:
        return
    if args.synthetic:
        raise SystemExit("train_24p.py: --data-dir / --val-data-dir read a real dataset; drop --synthetic")
    if args.fp32_batches or args.no_prefetch:
        raise SystemExit("train_24p.py: --data-dir / --val-data-dir batches are decoded and letterboxed on the GPU behind the prefetcher "
                         "(drop --no-prefetch / --fp32-batches)")


def check_mixup_args(args):
    """--mixup blends a second image into the mosaic images of --augment: it needs --augment."""
    if getattr(args, "mixup", False) and not args.augment:
        raise SystemExit("train_24p.py: --mixup blends a second image into the mosaic of --augment (add --augment)")


def check_copy_paste_args(args):
    """--copy-paste pastes objects between the images that --augment produced: it needs --augment, and a probability in (0, 1]."""
    p = getattr(args, "copy_paste", 0.0) or 0.0
    if not p:
        return
    if not 0.0 < p <= 1.0:
        raise SystemExit("train_24p.py: --copy-paste %r: the probability that an image pastes objects, in (0, 1]" % p)
    if not args.augment:
        raise SystemExit("train_24p.py: --copy-paste pastes objects of the batch into the images of --augment (add --augment)")


def check_multiscale_args(args, exp, world):
    """--multiscale keeps one captured step per input size: it needs the captured step, a single process and a range of sizes."""
    if not getattr(args, "multiscale", False):
        return
    if args.no_graph:
        raise SystemExit("train_24p.py: --multiscale keeps one captured step per input size (ep24.multiscale.MultiScaleStep); drop --no-graph")
    if world > 1:
        raise SystemExit("train_24p.py: --multiscale under WORLD_SIZE=%d: the gradient reducer plans its buckets for one engine; "
                         "multiscale training across ranks is out of scope (run a single process)" % world)
    if args.multiscale_interval < 1:
        raise SystemExit("train_24p.py: --multiscale-interval %d: a new size is drawn every N >= 1 steps" % args.multiscale_interval)
    if args.multiscale_plans < 0:
        raise SystemExit("train_24p.py: --multiscale-plans %d is negative (0 = as many plans as the device memory holds)" % args.multiscale_plans)
    if not getattr(exp, "multiscale_range", 0) and not hasattr(exp, "random_size"):
        raise SystemExit("train_24p.py: --multiscale with exp.multiscale_range == 0 and no exp.random_size: there is one size only")


def check_fisheye_args(args):
    """--fisheye-theta works on the raw uint8 batches, and the warp is not composed with mosaic / affine."""
    lo, hi = args.fisheye_theta
    if args.augment:
        raise SystemExit("train_24p.py: --fisheye-theta and --augment exclude each other (the sector warp is not composed with mosaic / affine)")
    if not args.raw_u8:
        raise SystemExit("train_24p.py: --fisheye-theta works on the raw uint8 batches behind the prefetcher (drop --no-prefetch / --fp32-batches)")
    if not 15 <= lo <= hi <= 180:
        raise SystemExit("train_24p.py: --fisheye-theta LO HI needs 15 <= LO <= HI <= 180")


def check_fisheye_lens_args(args):
    """--fisheye-lens works on the raw uint8 batches, one warp per run, and the lens is not composed with mosaic / affine."""
    if not getattr(args, "fisheye_lens", None):
        return
    if args.fisheye_theta is not None:
        raise SystemExit("train_24p.py: --fisheye-lens and --fisheye-theta exclude each other (a calibrated lens or the sector warp, not both)")
    if args.augment:
        raise SystemExit("train_24p.py: --fisheye-lens and --augment exclude each other (the lens model is not composed with mosaic / affine)")
    if args.no_prefetch or args.fp32_batches or not getattr(args, "raw_u8", True):
        raise SystemExit("train_24p.py: --fisheye-lens works on the raw uint8 batches behind the prefetcher (drop --no-prefetch / --fp32-batches)")
    for path in args.fisheye_lens:
        if not os.path.isfile(path):
            raise SystemExit("train_24p.py: --fisheye-lens %s: no such calibration file (JSON: K, D, pinhole, fov_deg, size)" % path)


EXP_VALUE = object()       # --weight-decay without a value (not a string: argparse would hand it to float())


def check_eval_tta_args(args):
    """--eval-tta implies --nms-iou poly24 (an explicit rect is refused); --eval-vote T >= 0 needs the polygon NMS, named by
    --nms-iou poly24 or implied by --eval-tta; --eval-tta-scales belongs to --eval-tta and starts with the canonical 1.0.
    Returns the message of the refusal, or None."""
    tta = getattr(args, "eval_tta", False)
    nms_iou = getattr(args, "nms_iou", None)
    if tta and nms_iou not in (None, "poly24"):
        return "--eval-tta merges the views by the polygon NMS: it implies --nms-iou poly24 (got --nms-iou %s)" % nms_iou
    scales = getattr(args, "eval_tta_scales", None)
    if scales is not None:
        if not tta:
            return "--eval-tta-scales names the views of --eval-tta (add --eval-tta)"
        if float(scales[0]) != 1.0 or any(not 0.0 < float(s) <= 1.0 for s in scales):
            return "--eval-tta-scales %s: the canonical view 1.0 first, then scales in (0, 1]" % (scales,)
    vote = getattr(args, "eval_vote", None)
    if vote is not None:
        if not tta and nms_iou != "poly24":
            return "--eval-vote finds its voters in the buffers of the polygon NMS: add --nms-iou poly24 or --eval-tta"
        if not vote >= 0.0:
            return "--eval-vote %r: the IoU threshold of the voters, at least 0" % vote
    return None


def apply_eval_args(exp, args):
    """The evaluation flags on the Exp: --eval-iou, --nms-iou, --eval-tta (with its scales; implies the polygon NMS), --eval-vote."""
    msg = check_eval_tta_args(args)
    if msg:
        raise SystemExit("train_24p.py: " + msg)
    if getattr(args, "eval_iou", None) is not None:
        exp.eval_iou_type = args.eval_iou
    if getattr(args, "nms_iou", None) is not None:
        exp.nms_iou_type = args.nms_iou
    if getattr(args, "eval_tta", False):
        exp.eval_tta = True
        exp.nms_iou_type = "poly24"
        if getattr(args, "eval_tta_scales", None) is not None:
            exp.eval_tta_scales = tuple(float(s) for s in args.eval_tta_scales)
    if getattr(args, "eval_vote", None) is not None:
        exp.eval_vote = float(args.eval_vote)
    msg = check_eval_strata_args(args)
    if msg:
        raise SystemExit("train_24p.py: " + msg)
    if getattr(args, "eval_areas", False):
        exp.eval_areas = True
    if getattr(args, "eval_zones", None) is not None:
        exp.eval_zones = args.eval_zones
        if getattr(args, "eval_zone_edges", None) is not None:
            exp.eval_zone_edges = tuple(float(e) for e in args.eval_zone_edges)
        if args.eval_zones == "lens":
            exp.eval_lens = args.eval_lens


def check_eval_strata_args(args):
    """--eval-zones lens needs its calibration file and --eval-lens belongs to it; --eval-zone-edges belongs to --eval-zones, ascends
    and leaves room for the area rows (8 strata in all).  Returns the message of what is wrong, or None."""
    zones, edges, lens = getattr(args, "eval_zones", None), getattr(args, "eval_zone_edges", None), getattr(args, "eval_lens", None)
    if zones == "lens" and not lens:
        return "--eval-zones lens takes the incidence angles from a calibration: add --eval-lens LENS.json"
    if lens and zones != "lens":
        return "--eval-lens is the calibration of --eval-zones lens (add --eval-zones lens)"
    if lens and not os.path.isfile(lens):
        return "--eval-lens %s: no such calibration file (JSON: K, D, pinhole, fov_deg, size)" % lens
    if edges is not None:
        if zones is None:
            return "--eval-zone-edges names the zones of --eval-zones (add --eval-zones radius or lens)"
        e = [float(x) for x in edges]
        if len(e) < 2 or any(not a < b for a, b in zip(e, e[1:])):
            return "--eval-zone-edges %s: at least two edges, ascending (the last may be inf)" % (" ".join(str(x) for x in edges),)
        if len(e) - 1 + (4 if getattr(args, "eval_areas", False) else 1) > 8:
            return "--eval-zone-edges: %d zones and the area rows make more than 8 strata" % (len(e) - 1)
    return None


class _Parser(argparse.ArgumentParser):
    def parse_args(self, args=None, namespace=None):
        a = super().parse_args(args, namespace)
        msg = check_eval_tta_args(a)
        if msg:
            self.error(msg)
        return a


def make_parser():
    p = _Parser("YOLOX train parser")
    p.add_argument("-b", "--batch_size", type=int, default=4, help="batch size (per GPU)")
    p.add_argument("-l", "--learn_rate", type=float, default=0.001, help="learn rate")
    p.add_argument("-s", "--start_device", default=0, type=int, help="device for start count")
    p.add_argument("-d", "--devices", default=1, type=int, help="device for training")
    p.add_argument("-f", "--exp_file", default=None, type=str, help="plz input your experiment description file")
    p.add_argument("--resume", default=False, action="store_true", help="resume training")
    p.add_argument("-c", "--ckpt", default=None, type=str, help="checkpoint file")
    p.add_argument("-e", "--start_epoch", default=None, type=int, help="resume training start epoch")
    p.add_argument("--num_machines", default=1, type=int, help="num of node for training")
    # additions of this build
    p.add_argument("--device", default="cuda", type=str, help="cuda or cuda:N (the ep24 path has no CPU fallback: cpu is refused)")
    p.add_argument("--synthetic", action="store_true", help="synthetic images / labels with the reference's layout (the source when no --data-dir is given)")
    p.add_argument("--data-dir", default=None, type=str, help="folder of training images <stem>.jpg (baseline JPEG; with --label-dir): "
                   "datasets.COCO24PFolderDataset, Huffman stage in the loader processes, IDCT / upsampling / colour on the GPU (ep24.jpeg)")
    p.add_argument("--label-dir", default=None, type=str, help="folder of COCO_24p_label/<stem>.txt files (labels_create_24p.py writes them)")
    p.add_argument("--val-data-dir", default=None, type=str, help="folder of validation images (with --val-label-dir) for --eval-interval")
    p.add_argument("--val-label-dir", default=None, type=str, help="folder of validation label files")
    p.add_argument("--jpeg-decoder", default=None, choices=["gpu", "pil", "device"], help="gpu (default): ep24.jpeg; pil: Pillow's decode in the "
                   "loader processes, for files the native path refuses (progressive, CMYK, 12-bit); device: as gpu, with the Huffman stage on "
                   "the GPU too (the loader processes hand over the scan bytes; a corrupt file is reported when its batch is handed out)")
    p.add_argument("--output-dir", default=None, type=str, help="overrides exp.output_dir")
    p.add_argument("--synthetic-len", default=0, type=int, help="images per synthetic epoch (overrides exp.synthetic_len; a checkpoint is written per epoch)")
    p.add_argument("--steps", default=0, type=int, help="stop after this many steps (0 = run all epochs)")
    p.add_argument("--log-interval", default=10, type=int)
    p.add_argument("--no-graph", action="store_true", help="reference-style eager loop instead of the captured step")
    p.add_argument("--sched", action="store_true", help="follow exp.get_lr_scheduler (yoloxwarmcos) instead of a constant rate")
    p.add_argument("--ema", action="store_true", help="keep a ModelEMA copy of the model (saved as ema_model)")
    p.add_argument("--l1", action="store_true", help="switch use_l1 on from epoch exp.L1_epoch")
    p.add_argument("--weight-decay", default=None, type=float, nargs="?", const=EXP_VALUE, metavar="W", help="stock YOLOX's optimizer "
                   "groups: weight decay W (without a value: exp.weight_decay) on every weight that is not a BatchNorm's, none on "
                   "BatchNorm weights and biases; saved with the optimizer state and restored by --resume (default: no decay)")
    p.add_argument("--prefetch", action="store_true", help="(default since round 4; kept for old command lines) upload the next batch on a side stream: ep24.input.DataPrefetcher")
    p.add_argument("--loader-workers", default=None, type=int, help="processes of the synthetic loader (default: the Exp's loader_workers)")
    p.add_argument("--loader-pin", default=None, type=int, choices=(0, 1), help="page-locked batches from the loader (default: with loader processes and fp32 batches)")
    p.add_argument("--no-prefetch", action="store_true", help="the reference's loop: upload every batch on the compute stream (train_24p.py:86-88)")
    p.add_argument("--raw-u8", action="store_true", help="(default since round 5; kept for old command lines) the synthetic source hands over uint8 HWC "
                   "images + normalised label rows; letterbox and label scaling run on the GPU behind the prefetcher (SURVEY 8f N1)")
    p.add_argument("--fp32-batches", action="store_true", help="the reference's form of the source: ready-made fp32 canvases [B,3,S,S] + label tables from "
                   "the loader (datasets/data_augment.py TrainTransform on the host side)")
    p.add_argument("--resident-batch", action="store_true", help="diagnostic: the epoch's first batch stays on the device and is fed again and again "
                   "(no upload, no letterbox after the first step): the entry point's rate without its input pipeline")
    p.add_argument("--dp-wire", default="fp32", choices=["fp32", "bf16"], help="wire format of the gradient all-reduce under torch.distributed.run")
    p.add_argument("--throughput-json", default=None, type=str, help="with --steps N: write images/s over the run's last --throughput-window steps "
                   "(synchronised at both ends) to this file")
    p.add_argument("--throughput-window", default=200, type=int)
    p.add_argument("--augment", action="store_true", help="mosaic, random affine, mirror and HSV on the GPU for 24-point labels (ep24.augment."
                   "MosaicTransform behind the prefetcher) with the Exp's mosaic_prob / degrees / translate / mosaic_scale / shear / flip_prob / "
                   "hsv_prob, for epochs < max_epoch - no_aug_epochs")
    p.add_argument("--mixup", action="store_true", help="with --augment: mixup on the GPU (a second image of the batch, letterboxed, "
                   "jittered, mirrored and cropped, averaged into every mosaic image; its 24-point labels re-cast and appended) with the "
                   "Exp's mixup_prob / mixup_scale, iff exp.enable_mixup")
    p.add_argument("--copy-paste", nargs="?", const=0.5, default=0.0, type=float, metavar="P", help="with --augment: copy-paste on the GPU "
                   "(YOLOv5's copy_paste for 24-point labels): with probability P (0.5 when the flag stands alone) an image pastes objects "
                   "of another image of the batch, shifted and possibly mirrored, where they hide less than 30 %% of every object already "
                   "there; their polygons are the masks.  Off when absent; goes off with the rest at no_aug_epochs")
    p.add_argument("--multiscale", action="store_true", help="stock YOLOX's multiscale training: a new input size from exp.random_resize "
                   "(multiples of 32 within exp.multiscale_range of input_size / 32) every --multiscale-interval steps, the batch and "
                   "its labels resized on the GPU behind loader and augmentation, one captured step per size; single process, captured step only")
    p.add_argument("--multiscale-interval", default=10, type=int, metavar="N", help="steps between two draws of the input size")
    p.add_argument("--multiscale-seed", default=0, type=int, metavar="S", help="the k-th size follows from (S, k): a resumed run continues the sequence")
    p.add_argument("--multiscale-plans", default=0, type=int, metavar="N", help="captured steps kept resident, least recently used evicted "
                   "(0: as many as the free device memory holds)")
    p.add_argument("--augment-seed", default=0, type=int, help="seed of the augmentation; a batch's parameters follow from (seed, epoch, iteration)")
    p.add_argument("--fisheye-theta", default=None, type=int, nargs=2, metavar=("LO", "HI"), help="fisheye sector warp of every image AND its "
                   "24-point labels on the GPU (ep24.fisheye.FisheyeTransform behind the prefetcher), one angle in [LO, HI] degrees per image, "
                   "reproducible from (--augment-seed, epoch, iteration); not together with --augment")
    p.add_argument("--fisheye-lens", default=None, nargs="+", metavar="FILE", help="calibrated fisheye lens (JSON of numbers: K 3x3 and D 4 in "
                   "OpenCV's cv2.fisheye layout, pinhole, fov_deg, size): every image AND its 24-point labels as the lens sees them, on the GPU "
                   "(ep24.lens.LensTransform behind the prefetcher); with several files one lens is drawn per image, reproducible from "
                   "(--augment-seed, epoch, iteration); not together with --fisheye-theta or --augment")
    p.add_argument("--eval-interval", default=0, type=int, help="every N epochs: COCO-style AP (exp.eval, ep24.evaluate) of the EMA model "
                   "(--ema) or the model, logged and saved as best_ckpt.pth when it improves (0 = off; single process only)")
    p.add_argument("--eval-iou", default=None, choices=["circle24", "rect", "poly24"], help="IoU type of the evaluation (ep24.evaluate): "
                   "overrides the Exp's eval_iou_type; poly24 is the exact area IoU of the 24-point polygons")
    p.add_argument("--nms-iou", default=None, choices=["rect", "poly24"], help="NMS of the evaluation: overrides the Exp's nms_iou_type; "
                   "rect is the reference's rectangle rule, poly24 suppresses by the exact area IoU of the 24-point polygons")
    p.add_argument("--eval-tta", action="store_true", help="test-time augmentation of the evaluation (ep24.tta): every batch at each of "
                   "--eval-tta-scales, plain and mirrored, the predictions brought back into one frame and merged by the polygon NMS "
                   "(implies --nms-iou poly24) over the canonical view's anchor count of candidates; one forward per view")
    p.add_argument("--eval-tta-scales", default=None, type=float, nargs="+", metavar="S", help="with --eval-tta: the views' scales, 1.0 "
                   "first (default: the Exp's eval_tta_scales, 1.0 0.85 0.7); each must keep the height a multiple of 32")
    p.add_argument("--eval-vote", default=None, type=float, metavar="T", help="polygon voting in the evaluation: every kept detection "
                   "becomes the score-weighted consensus of the candidates whose area IoU with it is above T (needs --nms-iou poly24 "
                   "or --eval-tta)")
    add_eval_strata_flags(p)
    return p


def add_eval_strata_flags(p):
    """The flags of the stratified evaluation (ep24.evaluate strata), shared with eval_24p.py."""
    p.add_argument("--eval-areas", action="store_true", help="evaluate by object size too: pycocotools' twelve lines (AP / AR for all, "
                   "small, medium, large objects in original-image pixels; maxDets 1, 10, 100)")
    p.add_argument("--eval-zones", default=None, choices=["radius", "lens"], help="AP per distortion zone of the objects' centres: "
                   "radius = distance from the image centre in units of half the diagonal, lens = incidence angle by --eval-lens")
    p.add_argument("--eval-zone-edges", default=None, type=float, nargs="+", metavar="E", help="with --eval-zones: the zones' edges, "
                   "ascending, the last may be inf (default 0 1/3 2/3 inf for radius, 0 30 60 90 degrees for lens)")
    p.add_argument("--eval-lens", default=None, type=str, metavar="LENS.json", help="with --eval-zones lens: the calibration of the "
                   "validation images (the JSON of --fisheye-lens), scaled to every image from its size")


def main(exp, args):
    if args.output_dir:
        exp.output_dir = args.output_dir
    apply_eval_args(exp, args)
    if args.synthetic_len:
        exp.synthetic_len = args.synthetic_len
    for name in ("data_dir", "label_dir", "val_data_dir", "val_label_dir", "jpeg_decoder"):
        if getattr(args, name, None) is not None:
            setattr(exp, name, getattr(args, name))
    trainer = Trainer(exp, args)
    trainer.train()
    return trainer


if __name__ == "__main__":
    args = make_parser().parse_args()
    exp = get_exp(args.exp_file)
    main(exp, args)
