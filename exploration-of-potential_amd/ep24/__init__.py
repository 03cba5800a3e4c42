"""ep24 - MI355X-native training path of the YOLOX-24p detector (HIP kernels behind include/ep24.h).

Submodules: ``_lib`` (ctypes binding), ``nn`` (parameter tree with the reference's names), ``engine``
(static launch plan), ``loss`` (SimOTA + 24-circle loss), ``train`` (captured step, fused SGD), ``dp``
(RCCL gradient reduction), ``sector`` (fisheye sector warp), ``fisheye`` (the warp with its 24-point labels: ``warp_labels``, ``FisheyeTransform``), ``lens`` (a calibrated fisheye lens in cv2.fisheye's model: images, points and 24-point labels in both directions,
``LensModel``, ``LensTransform``), ``synth`` (synthetic inputs), ``evaluate`` (COCO-style AP), ``masks`` (polygons to
instance masks, mask IoU), ``draw`` (detections drawn on images), ``track`` (identity of detections across frames: ``Tracker24``),``featmap`` (FPN heat maps and their response inside the labels' regions).
"""
__all__ = ["nn", "engine", "loss", "train", "dp", "sector", "synth"]
