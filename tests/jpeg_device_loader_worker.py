"""Child process of tests/test_gpu_jpeg_device.py::test_folder_dataset_with_the_device_decoder:

    python tests/jpeg_device_loader_worker.py TMP_DIR

A folder of 8 files from tools/make_jpeg_dataset.py goes through Exp.get_data_loader (2 loader processes, shuffled) and the
DataPrefetcher twice: with ``jpeg_decoder = "device"`` (the loader processes hand over JpegScan items, the Huffman stage runs on the
GPU) and with ``"gpu"`` (host Huffman stage).  The batches must be bit-equal, the device items must have been made without
initialising CUDA, and a file with a cut scan must make ``next()`` raise with its name."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
Y24 = os.path.join(ROOT, "exploration-of-potential_amd", "yolox_24p")
for p in (os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools"), os.path.join(ROOT, "exploration-of-potential_amd"), Y24):
    sys.path.insert(0, p)

import torch  # noqa: E402

import jpeg_device_streams as ds  # noqa: E402
import make_jpeg_dataset  # noqa: E402
from ep24 import jpeg  # noqa: E402
from ep24.input import DataPrefetcher, TrainTransform  # noqa: E402
from exp import Exp  # noqa: E402


class Recorder:
    def __init__(self, loader):
        self.loader, self.batches = loader, []

    def __iter__(self):
        for b in self.loader:
            self.batches.append(b)
            yield b


def run(tmp, decoder):
    exp = Exp()
    exp.data_dir, exp.label_dir = os.path.join(tmp, "images"), os.path.join(tmp, "COCO_24p_label")
    exp.data_num_workers, exp.report_loader_cuda, exp.jpeg_decoder = 2, True, decoder
    loader = exp.get_data_loader(4, raw_u8=True)
    assert loader.num_workers == 2 and loader.dataset.decoder == decoder
    loader.sampler.set_epoch(0)
    rec = Recorder(loader)
    pf = DataPrefetcher(rec, (128, 160), TrainTransform(max_labels=50))
    got = []
    while True:
        img, lab = pf.next()
        if img is None:
            break
        got.append((img.clone(), lab.clone()))
    torch.cuda.synchronize()
    return got, rec.batches


def main(tmp):
    make_jpeg_dataset.make(tmp, 8)
    torch.zeros(1, device="cuda")                         # the GPU is open in this process before the loader processes start
    dev, dev_batches = run(tmp, "device")
    host, host_batches = run(tmp, "gpu")
    assert len(dev) == len(host) == 2
    for (a_img, a_lab), (b_img, b_lab), db, hb in zip(dev, host, dev_batches, host_batches):
        assert db[3] == hb[3]                             # the same shuffled order
        assert all(isinstance(im, jpeg.JpegScan) and im.tag is False and im.source.endswith(".jpg") for im in db[0])
        assert all(isinstance(im, jpeg.JpegCoefficients) for im in hb[0])
        assert torch.equal(a_img, b_img) and torch.equal(a_lab, b_lab)
    # a cut scan passes the marker walk in the loader process; the batch that holds it is refused when it is handed out
    victim = os.path.join(tmp, "images", "%012d.jpg" % 3)
    with open(victim, "wb") as fh:
        fh.write(ds.truncated_scene())
    try:
        run(tmp, "device")
    except jpeg.JpegError as e:
        assert e.code == jpeg.EP24JPEG_E_DATA and "000000000003.jpg" in str(e) and "--jpeg-decoder pil" in str(e), str(e)
    else:
        raise AssertionError("the cut file was not reported")
    print("device loader worker ok: %d batches" % len(dev))


if __name__ == "__main__":
    main(sys.argv[1])
