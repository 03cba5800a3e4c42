"""ep24.jpeg on the GPU: ep24_jpeg_idct + ep24_jpeg_color against libjpeg's decode of the committed fixtures (bit equality), the
transforms fed with entropy-decoded files, the folder dataset behind the prefetcher, and the entry point."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import jpeg_fixtures as fx
from ep24 import jpeg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
Y24 = os.path.join(ROOT, "exploration-of-potential_amd", "yolox_24p")
pytestmark = pytest.mark.gpu

MIXED = ("q90_420_33x50", "q90_444_17x23", "grey_q80_16x16", "q75rst_422_40x7")       # four sizes, four samplings


def _bgr(name):
    return np.ascontiguousarray(fx.rgb(name)[:, :, ::-1])


def _rows(k, seed, hw=(33, 50)):
    """k label rows (class + 24-point polygon, normalised) as tools/make_jpeg_dataset.py writes them."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import make_jpeg_dataset
    finally:
        sys.path.remove(os.path.join(ROOT, "tools"))
    return make_jpeg_dataset.label_rows(np.random.RandomState(seed), k, hw[0], hw[1])


@pytest.mark.parametrize("name", fx.decodable())
def test_every_fixture_alone(name):
    want = fx.rgb(name)
    rgb = jpeg.decode([fx.data(name)], bgr=False)
    assert len(rgb) == 1 and rgb[0].dtype == torch.uint8 and rgb[0].is_cuda and tuple(rgb[0].shape) == want.shape
    got = rgb[0].cpu().numpy()
    assert np.array_equal(got, want), "RGB: %d pixels differ, max %d" % (int((got != want).any(-1).sum()), int(np.abs(got.astype(int) - want).max()))
    got = jpeg.decode([fx.data(name)])[0].cpu().numpy()                               # BGR is the default: cv2.imread's order
    assert np.array_equal(got, want[:, :, ::-1])


def test_all_fixtures_in_one_call_in_two_orders():
    """Descriptor offsets and mixed sampling in one launch: every result equals its single-image result."""
    names = fx.decodable()
    items = {n: jpeg.entropy_decode(fx.data(n)) for n in names}
    single = {n: jpeg.finish([items[n]], bgr=False)[0].cpu().numpy() for n in names}
    for n in names:
        assert np.array_equal(single[n], fx.rgb(n)), n
    order_b = list(np.random.RandomState(3).permutation(names))
    for order in (names, order_b):
        out = jpeg.finish([items[n] for n in order], bgr=False)
        assert len(out) == len(order)
        for n, t in zip(order, out):
            assert np.array_equal(t.cpu().numpy(), single[n]), n
    assert names != order_b


def test_empty_list():
    assert jpeg.finish([]) == [] and jpeg.decode([]) == []


def test_finish_refuses_inconsistent_items():
    it = jpeg.entropy_decode(fx.data("q90_420_17x23"))
    bad = jpeg.JpegCoefficients(it.header, it.coef[:-64])
    with pytest.raises(jpeg.JpegError):
        jpeg.finish([bad])


def test_train_transform_takes_coefficients():
    """A mixed-size batch of four into a 128 x 160 canvas: bit-identical images and labels to the same call fed the expected arrays."""
    from ep24.input import TrainTransform
    items = [jpeg.entropy_decode(fx.data(n)) for n in MIXED]
    arrays = [_bgr(n) for n in MIXED]
    targets = [_rows(3, 1), _rows(1, 2), np.zeros((0, 51)), _rows(5, 3)]
    tt = TrainTransform(max_labels=50)
    a_img, a_lab = tt.batch(items, targets, (128, 160))
    b_img, b_lab = tt.batch(arrays, targets, (128, 160))
    assert a_img.shape == (4, 3, 128, 160) and a_img.dtype == torch.float32
    assert torch.equal(a_img, b_img) and torch.equal(a_lab, b_lab)
    # a batch may mix decoded arrays and coefficients
    c_img, _ = tt.batch([items[0], arrays[1], items[2], arrays[3]], targets, (128, 160))
    assert torch.equal(c_img, b_img)


def test_mosaic_transform_takes_coefficients():
    from ep24.augment import MosaicTransform
    items = [jpeg.entropy_decode(fx.data(n)) for n in MIXED]
    arrays = [_bgr(n) for n in MIXED]
    targets = [_rows(3, 1), _rows(1, 2), np.zeros((0, 51)), _rows(5, 3)]
    out = []
    for images in (items, arrays):
        mt = MosaicTransform(max_labels=50, seed=5, mixup_prob=1.0, copy_paste_prob=1.0)
        mt.set_position(0, 0)
        img, lab = mt.batch(images, targets, (128, 160))
        out.append((img.clone(), lab.clone(), mt.last_counts.clone()))
    assert torch.equal(out[0][0], out[1][0]) and torch.equal(out[0][1], out[1][1]) and torch.equal(out[0][2], out[1][2])
    assert bool(torch.isfinite(out[0][0]).all()) and float(out[0][0].std()) > 0


def test_folder_dataset_behind_the_prefetcher(tmp_path):
    """8 files -> Exp.get_data_loader with 2 loader processes -> DataPrefetcher: two batches equal the same transform fed libjpeg's
    decode; the loader processes ran the Huffman stage without initialising the GPU.  In a fresh process (tests/jpeg_loader_worker.py):
    forking loader processes out of a test session that has run hundreds of GPU tests takes most of a minute."""
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "jpeg_loader_worker.py"), str(tmp_path)], stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, text=True, timeout=300)
    assert p.returncode == 0 and "loader worker ok: 2 batches" in p.stdout, p.stdout[-4000:]


def test_entry_point_trains_on_a_folder(tmp_path):
    """``train_24p.py --data-dir ... --label-dir ... --steps 2`` with a small Exp at 128 x 128, in a fresh process."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import make_jpeg_dataset
    finally:
        sys.path.remove(os.path.join(ROOT, "tools"))
    make_jpeg_dataset.make(str(tmp_path / "data"), 8)
    (tmp_path / "small_jpeg_exp.py").write_text(
        "from exp import Exp as MyExp\n\n\nclass Exp(MyExp):\n    def __init__(self):\n        super().__init__()\n"
        "        self.depth, self.width, self.input_size, self.test_size = 0.33, 0.25, (128, 128), (128, 128)\n"
        "        self.data_num_workers, self.max_epoch, self.exp_name = 2, 2, 'small_jpeg'\n")
    env = dict(os.environ)
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK"):
        env.pop(k, None)
    cmd = [sys.executable, os.path.join(Y24, "train_24p.py"), "-f", str(tmp_path / "small_jpeg_exp.py"), "-b", "4", "-l", "0.01",
           "--data-dir", str(tmp_path / "data" / "images"), "--label-dir", str(tmp_path / "data" / "COCO_24p_label"), "--steps", "2",
           "--log-interval", "1", "--output-dir", str(tmp_path / "out")]
    p = subprocess.run(cmd, cwd=Y24, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
    assert p.returncode == 0, p.stdout[-4000:]
    steps = [ln for ln in p.stdout.splitlines() if ln.startswith("step ")]
    assert len(steps) == 2 and "out of scope" not in p.stdout, p.stdout[-2000:]
    losses = [float(ln.split("loss")[1].split()[0]) for ln in steps]
    assert all(np.isfinite(v) and 0 < v < 1e4 for v in losses), losses
    assert os.path.isfile(str(tmp_path / "out" / "small_jpeg" / "last_epoch_ckpt.pth"))
