"""``Exp``: model / data / optimizer factory of the 24p detector (reference exp/yolox_base.py:11-137) on top of the
MI355X-native path: ``get_model`` builds the ep24 parameter tree (HIP plan behind ``YOLOX.forward``),
``get_optimizer`` the fused nesterov SGD, ``get_data_loader`` a synthetic source with the reference's label layout, or - with
``data_dir`` / ``label_dir`` set - a folder of JPEG files and txt labels (``datasets.COCO24PFolderDataset``; the reference's
COCO24P loader reads hard-coded /home/gaoyu/... paths, coco24p.py:19-20)."""
import _path  # noqa: F401
import torch.nn as nn

from .base_exp import BaseExp


class Exp(BaseExp):
    def __init__(self):
        super().__init__()
        # model
        self.num_classes = 80
        self.depth = 1.00
        self.width = 1.00
        self.act = "silu"
        self.backbone_type = "darknet"   # 'darknet' | 'resnet' | 'densenet' | 'vgg': the switch of yolox/models/yolo_pafpn.py:31-38
        # data
        self.data_num_workers = 8
        self.input_size = (640, 640)
        self.multiscale_range = 5
        self.train_ann = "instances_train2017.json"
        self.val_ann = "instances_val2017.json"
        self.synthetic_len = 64          # images per synthetic epoch
        self.loader_workers = 4          # processes of the synthetic fp32 loader (train_24p.py --loader-workers)
        self.synthetic_gts = 10
        # a real dataset (datasets.COCO24PFolderDataset): folders of <stem>.jpg and of COCO_24p_label/<stem>.txt; None = the synthetic source.
        # train_24p.py --data-dir / --label-dir / --val-data-dir / --val-label-dir / --jpeg-decoder set them
        self.data_dir = None
        self.label_dir = None
        self.val_data_dir = None
        self.val_label_dir = None
        self.jpeg_decoder = "gpu"        # "gpu": Huffman stage in the loader processes, the rest on the GPU (ep24.jpeg); "pil": Pillow;
        #                                  "device": the loader processes only walk the markers, the Huffman stage runs on the GPU too
        self.data_seed = 0               # seed of the per-epoch shuffle of the folder dataset
        # augmentation (stock YOLOX's names and values; read by train_24p.py --augment only: ep24.augment.MosaicTransform)
        self.mosaic_prob = 1.0
        self.degrees = 10.0
        self.translate = 0.1
        self.mosaic_scale = (0.5, 1.5)
        self.shear = 2.0
        self.flip_prob = 0.5
        self.hsv_prob = 1.0
        self.enable_mixup = True         # with train_24p.py --mixup (ep24.augment.sample_mixup); stock YOLOX's names and values
        self.mixup_prob = 1.0
        self.mixup_scale = (0.5, 1.5)
        # copy-paste of 24-point objects between the images of a batch (ep24.augment.sample_paste).  A deviation: the reference has no
        # such attribute (stock YOLOX has no copy-paste; the rule is YOLOv5's copy_paste).  train_24p.py --copy-paste [P] sets it.
        self.copy_paste_prob = 0.0
        # training
        self.warmup_epochs = 5
        self.max_epoch = 300
        self.L1_epoch = 100
        self.warmup_lr = 0
        self.basic_lr_per_img = 0.01 / 64.0
        self.scheduler = "yoloxwarmcos"
        self.no_aug_epochs = 100
        self.min_lr_ratio = 0.05
        self.ema = True
        self.weight_decay = 5e-4
        self.momentum = 0.9
        self.print_interval = 10
        self.eval_interval = 10
        self.exp_name = "yolox_24p"
        # testing
        self.test_size = (640, 640)
        self.test_conf = 0.01
        self.nmsthre = 0.65
        self.eval_len = 64               # images of the synthetic validation set (get_eval_loader)
        self.eval_seed = 1               # its own seed: the training source uses 0
        self.eval_iou_type = "circle24"  # ep24.evaluate: "circle24" (the model's geometry), "rect" (bounding boxes) or "poly24" (polygon area)
        self.nms_iou_type = "rect"       # NMS of the evaluation: "rect" (the reference's rectangle rule) or "poly24" (the polygons' area IoU)
        self.eval_tta = False            # test-time augmentation of the evaluation (ep24.tta): needs nms_iou_type "poly24"
        self.eval_tta_scales = (1.0, 0.85, 0.7)   # its views: each scale of test_size, plain and mirrored, the canonical one first
        self.eval_vote = None            # polygon voting: the voters' IoU threshold, or None (needs nms_iou_type "poly24")
        self.eval_areas = False          # pycocotools' twelve lines: AP / AR by object size (small, medium, large), maxDets 1 / 10 / 100
        self.eval_zones = None           # AP per distortion zone: "radius" (distance from the image centre) or "lens" (incidence angle)
        self.eval_zone_edges = None      # the zones' edges; None: 0 1/3 2/3 inf (radius), 0 30 60 90 degrees (lens)
        self.eval_lens = None            # "lens" zones: an ep24.lens.LensModel or its JSON file, the calibration of the validation images

    def get_model(self):
        from models import YOLOX, YOLOPAFPN, YOLOXHead
        if getattr(self, "model", None) is None:
            in_channels = [256, 512, 1024]
            backbone = YOLOPAFPN(self.depth, self.width, in_channels=in_channels, act=self.act, backbone_type=self.backbone_type)
            head = YOLOXHead(self.num_classes, self.width, in_channels=in_channels, act=self.act)
            self.model = YOLOX(backbone, head)
        for m in self.model.modules():                    # init_yolo, yolox_base.py:58-62
            if isinstance(m, nn.BatchNorm2d):
                m.eps = 1e-3
                m.momentum = 0.03
        self.model.head.initialize_biases(1e-2)
        return self.model

    def get_data_loader(self, batch_size, raw_u8=False, workers=None, pin=None):
        """``workers``: loader processes (None: ``loader_workers`` of the Exp for ready-made fp32 batches - collating 98 MB per step in
        the training process itself left the trainer at 0.21 of bench.py, four processes + page-locked batches bring 0.91 - and 0 for
        the raw uint8 source, whose batches are lists of cached images: 0.96, profiles/r04_trainer.json); ``pin``: page-locked batches
        (None: with loader processes and fp32 batches only)."""
        from datasets import ResumableSampler, SyntheticDataset, raw_collate
        import torch
        import os
        if self.data_dir is not None:
            return self.folder_loader(batch_size, self.data_dir, self.label_dir, train=True, raw_u8=raw_u8, workers=workers, pin=pin)
        self.dataset = SyntheticDataset(self.synthetic_len, tuple(self.input_size), self.synthetic_gts, self.num_classes, raw=raw_u8)
        world, rank = int(os.environ.get("WORLD_SIZE", 1)), int(os.environ.get("RANK", 0))
        sampler = None
        if world > 1:                                     # every rank walks its own shard of the epoch
            sampler = torch.utils.data.distributed.DistributedSampler(self.dataset, num_replicas=world, rank=rank, shuffle=False)
        else:
            sampler = torch.utils.data.SequentialSampler(self.dataset)
        sampler = ResumableSampler(sampler)               # .start: indices a resumed run has already trained on (train_24p.py)
        if workers is None:
            workers = 0 if raw_u8 else getattr(self, "loader_workers", 0)
        workers = int(workers)
        if pin is None:
            pin = workers > 0 and not raw_u8
        kw = dict(batch_size=batch_size, num_workers=workers, drop_last=True, sampler=sampler, pin_memory=bool(pin))
        if workers > 0:
            kw.update(persistent_workers=True, prefetch_factor=2)
        if raw_u8:                                        # lists of uint8 images + label rows: letterboxed on the GPU by the prefetcher
            kw["collate_fn"] = raw_collate
        return torch.utils.data.DataLoader(self.dataset, **kw)

    def folder_loader(self, batch_size, data_dir, label_dir, train, raw_u8=True, workers=None, pin=None):
        """Raw batches of a ``COCO24PFolderDataset``: lists of ``JpegCoefficients`` (or of Pillow's BGR arrays with
        ``jpeg_decoder = "pil"``) + label rows, from ``data_num_workers`` loader processes (at most 16; ``workers`` overrides) that run
        the Huffman stage and never open the GPU.  Training: shuffled per epoch from ``data_seed`` by a ``DistributedSampler`` (one
        rank included, so ``ResumableSampler.set_epoch`` reshuffles), incomplete last batch dropped.  Validation: in order, all kept."""
        import os
        import torch
        from datasets import COCO24PFolderDataset, ResumableSampler, raw_collate
        from ep24._lib import Ep24Error
        if not raw_u8:
            raise Ep24Error("ep24: a folder dataset yields raw batches (images of any sizes), letterboxed on the GPU behind the prefetcher; "
                            "ready-made fp32 batches are the synthetic source's")
        if label_dir is None:
            raise Ep24Error("ep24: data_dir %s is set without a label_dir (train_24p.py --label-dir)" % data_dir)
        dataset = COCO24PFolderDataset(data_dir, label_dir, decoder=self.jpeg_decoder, report_cuda=getattr(self, "report_loader_cuda", False))
        workers = min(int(self.data_num_workers if workers is None else workers), 16)
        kw = dict(batch_size=batch_size, num_workers=workers, collate_fn=raw_collate, pin_memory=bool(pin) if pin is not None else False)
        if workers > 0:
            kw.update(persistent_workers=True, prefetch_factor=2)
        if not train:
            return torch.utils.data.DataLoader(dataset, shuffle=False, drop_last=False, generator=torch.Generator(), **kw)
        self.dataset = dataset
        world, rank = int(os.environ.get("WORLD_SIZE", 1)), int(os.environ.get("RANK", 0))
        sampler = torch.utils.data.distributed.DistributedSampler(dataset, num_replicas=world, rank=rank, shuffle=True, seed=int(self.data_seed))
        return torch.utils.data.DataLoader(dataset, sampler=ResumableSampler(sampler), drop_last=True, **kw)

    def random_resize(self, data_loader=None, epoch=None, rng=None):
        """A multiscale input size, multiple of 32, aspect ratio of input_size (exp/yolox_base.py:93-107); plans are cached per size.
        ``rng``: a ``random.Random`` to draw from (``ep24.multiscale.size_for``); None: the module-level ``random``."""
        import random
        size_factor = self.input_size[1] * 1.0 / self.input_size[0]
        if not hasattr(self, "random_size"):
            self.random_size = (int(self.input_size[0] / 32) - self.multiscale_range, int(self.input_size[0] / 32) + self.multiscale_range)
        size = (rng or random).randint(*self.random_size)
        return (int(32 * size), 32 * int(size * size_factor))

    def preprocess(self, inputs, targets, tsize, out=None):
        """``out=(images, labels)``: buffers the resized batch is written into (``MultiScaleStep.inputs(tsize)``).  CUDA fp32 batches
        are resized by ``ep24.multiscale.resize_batch`` (two HIP launches); CPU tensors keep the reference's ``interpolate``."""
        scale_y = tsize[0] / self.input_size[0]
        scale_x = tsize[1] / self.input_size[1]
        if scale_x != 1 or scale_y != 1:
            import torch
            if inputs.is_cuda and inputs.dtype == torch.float32:
                from ep24.multiscale import resize_batch
                out_images, out_labels = out if out is not None else (None, None)
                return resize_batch(inputs.contiguous(), targets.contiguous(), tsize, out_images=out_images, out_labels=out_labels)
            inputs = nn.functional.interpolate(inputs, size=tsize, mode="bilinear", align_corners=False)
            targets[..., 1::2] = targets[..., 1::2] * scale_x
            targets[..., 2::2] = targets[..., 2::2] * scale_y
        return inputs, targets

    def get_optimizer(self, lr, weight_decay=None):
        """Takes the learning rate (not the batch size), like the 24p trainer (yolox_base.py:120-124).  ``weight_decay`` None or 0:
        that trainer's optimizer, one group without decay (the default).  A positive value: stock YOLOX's three groups
        (``ep24.train.yolox_param_groups``: BatchNorm weights / every other weight, decayed / biases), in the same fused update."""
        from ep24.train import SGD, yolox_param_groups
        if weight_decay:
            self.optimizer = SGD(yolox_param_groups(self.model, weight_decay), lr=lr, momentum=self.momentum, nesterov=True, model=self.model)
        else:
            self.optimizer = SGD(self.model.parameters(), lr=lr, momentum=self.momentum, nesterov=True, model=self.model)
        return self.optimizer

    def get_lr_scheduler(self, lr, iters_per_epoch, **kwargs):
        from utils import LRScheduler
        return LRScheduler(self.scheduler, lr, iters_per_epoch, self.max_epoch, warmup_epochs=self.warmup_epochs,
                           warmup_lr_start=self.warmup_lr, no_aug_epochs=self.no_aug_epochs, min_lr_ratio=self.min_lr_ratio)

    def get_eval_loader(self, batch_size, is_distributed=False, testdev=False, legacy=False):
        """Raw uint8 validation batches (a ``SyntheticDataset`` with its own seed and ``eval_len`` images, in order, the last batch
        may be short): ``eval`` letterboxes them on the GPU with ``TrainTransform.batch``.  Any loader yielding raw batches
        ``(images, label rows, info, ids)`` can take its place."""
        import torch
        from datasets import SyntheticDataset, raw_collate
        if self.val_data_dir is not None:
            return self.folder_loader(batch_size, self.val_data_dir, self.val_label_dir, train=False)
        ds = SyntheticDataset(self.eval_len, tuple(self.test_size), self.synthetic_gts, self.num_classes, seed=self.eval_seed, raw=True)
        # a generator of its own: iterating the loader must not draw from the global RNG the training run relies on
        return torch.utils.data.DataLoader(ds, batch_size=batch_size, shuffle=False, num_workers=0, drop_last=False,
                                           collate_fn=raw_collate, generator=torch.Generator())

    def get_evaluator(self, batch_size, is_distributed=False, testdev=False, legacy=False):
        """``ep24.evaluate.Evaluator24`` (COCO-style AP over 24-point detections, matching on the GPU) with ``test_conf`` /
        ``nmsthre`` and the validation loader attached; the reference's signature (exp/yolox_base.py:199-214, commented out there)."""
        from ep24._lib import Ep24Error
        from ep24.evaluate import Evaluator24
        if is_distributed:
            raise Ep24Error("ep24: distributed evaluation (gathering records across ranks) is not implemented")
        max_candidates = None
        if getattr(self, "eval_tta", False):
            # the merged table holds every view's anchors; only the canonical view's count of them enters the polygon NMS, so that
            # the suppression matrix keeps the size it has without the views
            from ep24.tta import anchors_for
            max_candidates = anchors_for(tuple(self.test_size))
        strata, max_dets = self.eval_strata()
        evaluator = Evaluator24(self.num_classes, iou_type=self.eval_iou_type, max_dets=max_dets, conf_thre=self.test_conf,
                                nms_thre=self.nmsthre, nms_iou=self.nms_iou_type, max_candidates=max_candidates,
                                vote_thre=getattr(self, "eval_vote", None), strata=strata)
        evaluator.dataloader = self.get_eval_loader(batch_size)
        return evaluator

    ZONE_EDGES = {"radius": (0.0, 1.0 / 3.0, 2.0 / 3.0, float("inf")), "lens": (0.0, 30.0, 60.0, 90.0)}

    def eval_strata(self):
        """``(strata, max_dets)`` of ``eval_areas`` / ``eval_zones`` / ``eval_zone_edges``: the four COCO area rows at maxDets
        (1, 10, 100), then one stratum per zone; ``(None, 100)`` with none of them set - the evaluator as it was."""
        from ep24 import evaluate as E
        areas, zones = getattr(self, "eval_areas", False), getattr(self, "eval_zones", None)
        if not areas and zones is None:
            return None, 100
        if zones not in (None, "radius", "lens"):
            raise ValueError("eval_zones must be None, 'radius' or 'lens', got %r" % (zones,))
        strata = E.coco_area_strata() if areas else [E.Stratum("all")]
        if zones is not None:
            if zones == "lens" and getattr(self, "eval_lens", None) is None:
                raise ValueError("eval_zones 'lens' needs eval_lens: the calibration of the validation images")
            edges = getattr(self, "eval_zone_edges", None) or self.ZONE_EDGES[zones]
            strata = strata + E.zone_strata(edges, "r" if zones == "radius" else "deg")
        return strata, ((1, 10, 100) if areas else 100)

    def eval_tables(self, sizes):
        """``(scales, zones)`` of a validation batch from its raw images' ``sizes`` (h, w) and ``test_size``: the letterbox ratios, and
        the zone rows of ``eval_zones`` - for "lens" the calibration brought to ``test_size`` from its ``size`` (a file without one
        is taken as given for ``test_size``), as the trainer's lens transform scales its models."""
        from ep24 import evaluate as E
        S = (int(self.test_size[0]), int(self.test_size[1]))
        zones = getattr(self, "eval_zones", None)
        zt = None
        if zones == "radius":
            zt = E.radius_zones(sizes, S)
        elif zones == "lens":
            from ep24.lens import LensModel, image_model
            m = self.eval_lens if isinstance(self.eval_lens, LensModel) else LensModel.from_json(self.eval_lens)
            if m.size is not None and m.size != S:
                m = m.scaled(S[1] / m.size[1], S[0] / m.size[0])
            zt = E.lens_zones([image_model(m, h, w, S) for h, w in sizes])
        return E.letterbox_scales(sizes, S), zt

    def eval(self, model, evaluator, is_distributed, half=False):
        """Eval-mode forward of every validation batch, ``evaluator.update`` on the decoded predictions, ``summarize``.
        Returns ``(ap50_95, ap50, summary)`` as stock YOLOX does; the model's training flag is restored."""
        import torch
        from ep24._lib import Ep24Error
        from ep24.input import TrainTransform
        if is_distributed:
            raise Ep24Error("ep24: distributed evaluation (gathering records across ranks) is not implemented")
        if half:
            raise Ep24Error("ep24: the eval-mode network runs in bf16 with fp32 outputs; half=True is not a separate mode")
        transform = TrainTransform(max_labels=50)
        views = None
        if getattr(self, "eval_tta", False):
            from ep24 import tta
            views = tta.views_for(tuple(self.test_size), self.eval_tta_scales)
        was_training = model.training
        model.eval()
        evaluator.reset()
        try:
            with torch.no_grad():
                for images, targets, _, _ in evaluator.dataloader:
                    tables = ()
                    if evaluator.strata is not None:      # object sizes in original pixels, zones in the input frame
                        from ep24.jpeg import finish_checked
                        images = finish_checked(images)
                        tables = self.eval_tables([tuple(im.shape[:2]) for im in images])
                    imgs, labs = transform.batch(images, targets, tuple(self.test_size))
                    evaluator.update(model(imgs, train=False) if views is None else tta.predict(model, imgs, views), labs, *tables)
            stats = evaluator.summarize()
        finally:
            if views is not None:
                torch.cuda.synchronize()
                tta.release(model)                        # the views' eval plans go with the evaluation
            if was_training:
                model.train()
        return stats["AP"], stats["AP50"], evaluator.summary
