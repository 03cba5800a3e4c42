"""Child process of tests/test_gpu_jpeg.py::test_folder_dataset_behind_the_prefetcher:

    python tests/jpeg_loader_worker.py TMP_DIR

A folder of 8 files from tools/make_jpeg_dataset.py goes through Exp.get_data_loader (2 loader processes, shuffled) and the
DataPrefetcher; the two batches must equal TrainTransform.batch fed libjpeg's decode of the same files (the committed .rgb.npy, as BGR),
bit for bit, and every item must report that its loader process had not initialised CUDA."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
Y24 = os.path.join(ROOT, "exploration-of-potential_amd", "yolox_24p")
for p in (os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools"), os.path.join(ROOT, "exploration-of-potential_amd"), Y24):
    sys.path.insert(0, p)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import jpeg_fixtures as fx  # noqa: E402
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


def main(tmp):
    made = make_jpeg_dataset.make(tmp, 8)
    by_id = {k: (name, rows) for k, name, rows in made}
    exp = Exp()
    exp.data_dir, exp.label_dir = os.path.join(tmp, "images"), os.path.join(tmp, "COCO_24p_label")
    exp.data_num_workers, exp.report_loader_cuda = 2, True
    torch.zeros(1, device="cuda")                         # the GPU is open in this process before the loader processes start
    loader = exp.get_data_loader(4, raw_u8=True)
    assert loader.num_workers == 2
    loader.sampler.set_epoch(0)
    rec = Recorder(loader)
    pf = DataPrefetcher(rec, (128, 160), TrainTransform(max_labels=50))
    got = []
    while True:
        img, lab = pf.next()
        if img is None:
            break
        got.append((img.clone(), lab.clone()))
    assert len(got) == 2 and len(rec.batches) == 2
    seen, tt = [], TrainTransform(max_labels=50)
    for (img, lab), (images, targets, infos, ids) in zip(got, rec.batches):
        assert all(isinstance(im, jpeg.JpegCoefficients) and im.tag is False for im in images)
        arrays = [np.ascontiguousarray(fx.rgb(by_id[i][0])[:, :, ::-1]) for i in ids]
        assert infos == [a.shape[:2] for a in arrays]
        for t, i in zip(targets, ids):
            assert np.array_equal(np.asarray(t).reshape(-1, 51), by_id[i][1])
        w_img, w_lab = tt.batch(arrays, [by_id[i][1] for i in ids], (128, 160))
        assert torch.equal(img, w_img) and torch.equal(lab, w_lab)
        seen += ids
    assert sorted(seen) == list(range(1, 9)) and seen != list(range(1, 9))              # shuffled
    torch.cuda.synchronize()
    print("loader worker ok: %d batches, order %s" % (len(got), seen))


if __name__ == "__main__":
    main(sys.argv[1])
