"""``COCO24PFolderDataset``: the reference's ``COCO24PDataset`` (datasets/coco24p.py:37-104) over a folder of JPEG files and a folder
of ``COCO_24p_label/*.txt`` files (``labels_create_24p.py`` writes them), for the raw path of the trainer.

Every ``*.txt`` of ``label_dir`` is one item; its image is ``<stem>.jpg`` in ``data_dir``; rows come through
``ep24.labels24.load_rows`` (an empty file is an image without objects); ``img_id = int(stem)``, or the item's index where the stem
is not a number.  Items are ``(image, rows [k, 51], (h, w), id)`` and are collated by ``raw_collate``.  With ``decoder="gpu"`` the
image is an ``ep24.jpeg.JpegCoefficients``: the loader process runs the Huffman stage only (host library, no GPU, no ``libep24.so``)
and ``TrainTransform.batch`` / ``MosaicTransform.batch`` finish the decode on the GPU.  ``decoder="pil"`` hands over Pillow's decode
as a uint8 HWC BGR array instead - for files the native path refuses (progressive, CMYK, ...).  With ``decoder="device"`` the image
is an ``ep24.jpeg.JpegScan``: the loader process only walks the markers and hands over the scan's bytes, the Huffman stage runs on
the GPU too; what the marker walk cannot see (corrupt entropy-coded data) is reported by ``DataPrefetcher.next()`` with the file's name.

``img_info`` is the TRUE ``(h, w)``: the reference returns ``(h, h)`` (coco24p.py:57, ``img.shape[0], img.shape[0]``), which is
wrong for every image that is not square; nothing downstream of it in the reference's trainer reads the second value.
"""
import os

import numpy as np
import torch

from ep24 import jpeg, labels24


class COCO24PFolderDataset(torch.utils.data.Dataset):
    def __init__(self, data_dir, label_dir, decoder="gpu", report_cuda=False):
        if decoder not in ("gpu", "pil", "device"):
            raise ValueError("COCO24PFolderDataset: decoder must be 'gpu', 'pil' or 'device', got %r" % (decoder,))
        if decoder == "pil":
            try:
                import PIL.Image  # noqa: F401
            except ImportError as e:
                raise ImportError("COCO24PFolderDataset(decoder='pil') needs Pillow, which is not installed; decoder='gpu' "
                                  "(ep24.jpeg) reads baseline JPEG files without it") from e
        self.data_dir, self.label_dir, self.decoder = str(data_dir), str(label_dir), decoder
        self.report_cuda = bool(report_cuda)              # tests: items carry torch.cuda.is_initialized() of the process that made them
        if not os.path.isdir(self.label_dir):
            raise FileNotFoundError("COCO24PFolderDataset: label directory %s does not exist" % self.label_dir)
        self.stems = sorted(os.path.splitext(f)[0] for f in os.listdir(self.label_dir) if f.endswith(".txt"))
        if not self.stems:
            raise FileNotFoundError("COCO24PFolderDataset: no *.txt label files in %s" % self.label_dir)
        missing = [s + ".jpg" for s in self.stems if not os.path.isfile(os.path.join(self.data_dir, s + ".jpg"))]
        if missing:
            raise FileNotFoundError("COCO24PFolderDataset: %d of %d label files have no image in %s: %s%s" % (
                len(missing), len(self.stems), self.data_dir, ", ".join(missing[:5]), ", ..." if len(missing) > 5 else ""))
        self.ids = [int(s) if s.isdigit() else i for i, s in enumerate(self.stems)]

    def __len__(self):
        return len(self.stems)

    def image_path(self, index):
        return os.path.join(self.data_dir, self.stems[index] + ".jpg")

    def load_rows(self, index):
        rows = np.asarray(labels24.load_rows(os.path.join(self.label_dir, self.stems[index] + ".txt")), dtype=np.float64)
        if rows.size == 0:
            return np.zeros((0, 51), dtype=np.float64)
        if rows.ndim != 2 or rows.shape[1] != 51:
            raise ValueError("COCO24PFolderDataset: %s.txt holds rows of %s values, not 51" % (self.stems[index], rows.shape[-1]))
        return rows

    def load_image(self, index):
        path = self.image_path(index)
        with open(path, "rb") as fh:
            data = fh.read()
        if self.decoder == "pil":
            import io
            from PIL import Image
            rgb = np.asarray(Image.open(io.BytesIO(data)).convert("RGB"), dtype=np.uint8)
            return np.ascontiguousarray(rgb[:, :, ::-1])                         # BGR, as cv2.imread returns it
        try:
            tag = torch.cuda.is_initialized() if self.report_cuda else None
            if self.decoder == "device":
                item = jpeg.scan(data, tag=tag)
                item.source = path                        # a corrupt scan shows only on the GPU: the prefetcher names the file
                return item
            return jpeg.entropy_decode(data, tag=tag)
        except jpeg.JpegError as e:
            raise jpeg.JpegError(e.code, "%s: %s - such files can be read with --jpeg-decoder pil (Pillow)" % (path, e.message)) from None

    def __getitem__(self, index):
        img = self.load_image(index)
        h, w = int(img.shape[0]), int(img.shape[1])
        return img, self.load_rows(index), (h, w), self.ids[index]
