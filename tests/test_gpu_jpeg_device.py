"""The Huffman stage on the GPU (csrc/jpeg_huff.hip: ep24_jpeg_huffman + ep24_jpeg_dc, through ep24.jpeg): every comparison is
``np.array_equal`` against ``jpeg.entropy_decode`` (coefficients) or against the committed Pillow decode (pixels) - no tolerances."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import jpeg_device_streams as ds
import jpeg_fixtures as fx
from ep24 import jpeg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
Y24 = os.path.join(ROOT, "exploration-of-potential_amd", "yolox_24p")
pytestmark = pytest.mark.gpu

MIXED = ("q90_420_33x50", "q90_444_17x23", "grey_q80_16x16", "q75rst_422_40x7")       # four sizes, four samplings
PHOTO = "photo_000000130566"


@functools.lru_cache(maxsize=None)
def _want(name):
    """The host decoder's coefficients of a fixture, computed once and left unchanged."""
    c = jpeg.entropy_decode(fx.data(name)).coef
    c.setflags(write=False)
    return c


def _same(got, want, what):
    assert got.dtype == np.int16 and got.shape == want.shape, what
    assert np.array_equal(got, want), "%s: %d coefficients differ, the first at %d" % (what, int((got != want).sum()), int(np.argmax(got != want)))


@pytest.mark.parametrize("name", fx.decodable())
def test_every_fixture_alone(name):
    out = jpeg.entropy_decode_device([fx.data(name)])
    assert len(out) == 1 and list(out.status) == [0]
    _same(out[0], _want(name), name)


def test_all_fixtures_in_one_call_in_two_orders():
    names = fx.decodable()
    assert len(names) == 67
    order_b = list(np.random.RandomState(3).permutation(names))
    assert names != order_b
    for order in (names, order_b):
        out = jpeg.entropy_decode_device([fx.data(n) for n in order])
        assert len(out) == 67 and not out.status.any()
        for n, got in zip(order, out):
            _same(got, _want(n), n)


def test_scan_items_mixed_with_coefficients_and_a_plain_array():
    bgr = lambda n: np.ascontiguousarray(fx.rgb(n)[:, :, ::-1])
    batch = [jpeg.scan(fx.data(MIXED[0])), jpeg.entropy_decode(fx.data(MIXED[1])), bgr(MIXED[2]), jpeg.scan(fx.data(MIXED[3]))]
    out = jpeg.finish_mixed(batch)
    assert isinstance(out, jpeg.Finished) and [i for i, _ in out.status_items] == [0, 3] and out[2] is batch[2]
    assert out.status.dtype == torch.int32 and out.status.is_cuda and out.status.cpu().tolist() == [0, 0]
    for i in (0, 1, 3):
        assert out[i].is_cuda and np.array_equal(out[i].cpu().numpy(), bgr(MIXED[i])), MIXED[i]
    # the other way round, in RGB, and in one finish: coefficients in front of and behind the device-decoded planes
    items = [jpeg.entropy_decode(fx.data(MIXED[0])), jpeg.scan(fx.data(MIXED[1])), jpeg.scan(fx.data(MIXED[2])), jpeg.entropy_decode(fx.data(MIXED[3]))]
    out = jpeg.finish(items, bgr=False)
    for n, t in zip(MIXED, out):
        assert np.array_equal(t.cpu().numpy(), fx.rgb(n)), n
    assert out.status.cpu().tolist() == [0, 0]
    plain = jpeg.finish(items[::3])                       # no JpegScan item: a plain list, as before
    assert type(plain) is list and len(plain) == 2


@pytest.mark.parametrize("S,tile", [(128, 1024), (16, 1024), (128, 64)])
def test_photo_crosses_tiles(S, tile):
    """About 2 350 subsequences at S = 128 and 18 800 at S = 16: more than any tile, so the end state, the block count and (in
    ep24_jpeg_dc) the DC value are carried from tile to tile."""
    it = jpeg.scan(fx.data(PHOTO))
    nsub = -(-it.data.size // S)
    assert len(it.segments) == 1 and nsub > 2 * tile and (2300 < nsub < 2400 if S == 128 else 18700 < nsub < 18900)
    assert max(it.header.nblocks) > 1024                  # the DC pass of a component crosses its tiles too
    out = jpeg.entropy_decode_device([it], subseq_bytes=S, tile=tile)
    assert list(out.status) == [0]
    _same(out[0], _want(PHOTO), "photo at S = %d in tiles of %d" % (S, tile))


def _crafted():
    files = {"tiny_grey": ds.tiny_grey(), "all_symbols": ds.all_symbols(), "flat_420": ds.flat_420()}
    for S in (16, 128):
        for delta in (-1, 0, 1):
            files["length_%d" % (2 * S + delta)] = ds.exact_length(2 * S + delta)
        for where in ("straddle", "inside", "first"):
            files["stuffed_%s_%d" % (where, S)] = ds.stuffed_at(S, where)[0]
    for interval in (1, 2, 7):
        files["restarts_%d" % interval] = ds.restarts(interval)
    return files


@pytest.mark.parametrize("S,tile", [(16, 64), (16, 1024), (128, 64), (128, 1024), (32, 256), (64, 128), (256, 512)])
def test_crafted_files(S, tile):
    """tests/jpeg_device_streams.py (their properties are asserted in test_jpeg_device_host.py): a scan shorter than a subsequence,
    scans of k S - 1, k S, k S + 1 bytes, FF 00 at a boundary, every DC size and AC symbol of both Annex K tables, restart intervals of
    1, 2 and 7 MCUs with segments shorter and longer than S, and the flat image that locks speculation to the wrong phase."""
    files = _crafted()
    out = jpeg.entropy_decode_device(list(files.values()), subseq_bytes=S, tile=tile)
    assert len(out) == len(files) and not out.status.any(), dict(zip(files, out.status))
    for (name, data), got in zip(files.items(), out):
        _same(got, jpeg.entropy_decode(data).coef, "%s at S = %d in tiles of %d" % (name, S, tile))


def test_launch_arguments_are_checked():
    with pytest.raises(jpeg.JpegError):
        jpeg.entropy_decode_device([fx.data(fx.SCENE)], subseq_bytes=100)
    with pytest.raises(jpeg.JpegError):
        jpeg.entropy_decode_device([fx.data(fx.SCENE)], tile=96)
    assert len(jpeg.entropy_decode_device([])) == 0 and jpeg.decode([], entropy="device") == []


@pytest.mark.parametrize("name", [fx.SCENE, "scene_420_rst", PHOTO])
def test_pixels_equal_the_host_path_and_pillow(name):
    for bgr in (True, False):
        dev = jpeg.decode([fx.data(name)], bgr=bgr, entropy="device")[0].cpu().numpy()
        host = jpeg.decode([fx.data(name)], bgr=bgr, entropy="host")[0].cpu().numpy()
        assert np.array_equal(dev, host), (name, bgr)
        assert np.array_equal(dev, fx.rgb(name)[:, :, ::-1] if bgr else fx.rgb(name)), (name, bgr)


def test_status_of_a_cut_scan():
    """scene_420 with the last 100 bytes of its scan cut and EOI appended again, between two whole files: the status words are
    [0, EP24JPEG_E_DATA, 0], the neighbours are exact, decode raises and names index 1.  (csrc/jpeg_device_check.cpp has walked the
    core over this file under the sanitizers: tests/test_jpeg_device_host.py.)"""
    cut = ds.truncated_scene()
    with pytest.raises(jpeg.JpegError):
        jpeg.entropy_decode(cut)
    batch = [fx.data("scene_420_rst"), cut, fx.data(fx.SCENE)]
    out = jpeg.entropy_decode_device(batch)
    assert out.status.tolist() == [0, jpeg.EP24JPEG_E_DATA, 0]
    _same(out[0], _want("scene_420_rst"), "left neighbour")
    _same(out[2], _want(fx.SCENE), "right neighbour")
    assert out[1].shape == _want(fx.SCENE).shape
    imgs = jpeg.finish([jpeg.scan(d) for d in batch], bgr=False)
    assert imgs.status.cpu().tolist() == [0, jpeg.EP24JPEG_E_DATA, 0]
    assert np.array_equal(imgs[0].cpu().numpy(), fx.rgb("scene_420_rst")) and np.array_equal(imgs[2].cpu().numpy(), fx.rgb(fx.SCENE))
    with pytest.raises(jpeg.JpegError) as e:
        jpeg.decode(batch, entropy="device")
    assert e.value.code == jpeg.EP24JPEG_E_DATA and "item 1" in e.value.message and "item 0" not in e.value.message
    tagged = [jpeg.scan(d, tag=t) for d, t in zip(batch, ("a.jpg", "b.jpg", "c.jpg"))]
    with pytest.raises(jpeg.JpegError, match="b.jpg"):
        jpeg.check_status(jpeg.finish(tagged).status.cpu().numpy(), [(i, jpeg._name(it, i)) for i, it in enumerate(tagged)])


def test_folder_dataset_with_the_device_decoder(tmp_path):
    """``COCO24PFolderDataset(decoder="device")`` through two loader processes and the prefetcher, bit-equal to ``decoder="gpu"``; a
    cut file is reported by ``DataPrefetcher.next()`` with its name.  In a fresh process (tests/jpeg_device_loader_worker.py)."""
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "jpeg_device_loader_worker.py"), str(tmp_path)], stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, text=True, timeout=300)
    assert p.returncode == 0 and "device loader worker ok: 2 batches" in p.stdout, p.stdout[-4000:]


def test_prefetcher_reads_the_status_words_in_next_and_not_in_its_upload(monkeypatch):
    """``DataPrefetcher`` finishes a batch of JpegScan items itself and hands the transform plain tensors: nothing in its upload reads
    the status words (that would be a host wait for the batch's Huffman launches, per batch, in the trainer's thread).  So the batch in
    front of a cut file is handed out although the cut file's batch is already enqueued, and the ``next()`` that would hand THAT batch
    out raises; ``finish_checked`` leaves a ``Finished`` list that it did not finish alone."""
    from ep24 import input as ep_input
    reads = []
    check = jpeg.check_status
    monkeypatch.setattr(jpeg, "check_status", lambda *a: (reads.append("transform"), check(*a)))        # finish_checked's
    monkeypatch.setattr(ep_input, "check_status", lambda *a: (reads.append("next"), check(*a)))         # DataPrefetcher.next's
    rows = [np.zeros((0, 51)), np.zeros((0, 51))]
    whole = [jpeg.scan(fx.data(fx.SCENE), tag="a.jpg"), jpeg.scan(fx.data("scene_420_rst"), tag="b.jpg")]
    bad = [jpeg.scan(fx.data(fx.SCENE), tag="whole.jpg"),jpeg.scan(ds.truncated_scene(), tag="cut.jpg")]
    tt = ep_input.TrainTransform(max_labels=50)
    want = tt.batch([jpeg.entropy_decode(fx.data(fx.SCENE)), jpeg.entropy_decode(fx.data("scene_420_rst"))], rows, (128, 160))[0].clone()
    pf = ep_input.DataPrefetcher([(whole, rows, None, None), (bad, rows, None, None)], (128, 160), tt)
    assert reads == []                                    # the first batch is enqueued, its words unread
    img, _ = pf.next()                                    # hands out the whole batch and enqueues the one with the cut file
    assert reads == ["next"] and torch.equal(img, want)
    with pytest.raises(jpeg.JpegError) as e:
        pf.next()
    assert reads == ["next", "next"] and e.value.code == jpeg.EP24JPEG_E_DATA
    assert "cut.jpg" in str(e.value) and "whole.jpg" not in str(e.value) and "--jpeg-decoder pil" in str(e.value)
    done = jpeg.finish_mixed(bad)
    assert jpeg.finish_checked(done) is done and reads == ["next", "next"]          # not its batch: no read, no wait
    with pytest.raises(jpeg.JpegError, match="cut.jpg"):
        jpeg.finish_checked(bad)                          # its own batch: read before the pixels are used
    assert reads[-1] == "transform"


def test_validation_with_the_device_decoder_reports_a_cut_file_by_name(tmp_path):
    """``Exp.eval`` does not go through the prefetcher: it hands the validation loader's batches to ``TrainTransform.batch``.  With
    ``jpeg_decoder = "device"`` those hold JpegScan items; the transform reads their status words before it uses the pixels, so whole
    files give the batches of ``"gpu"`` bit for bit and a cut file raises with its name and the pointer to ``--jpeg-decoder pil`` -
    in ``Exp.eval`` itself, with a small network, and in the mosaic and fisheye transforms."""
    for p in (Y24, os.path.join(ROOT, "tools")):
        if p not in sys.path:
            sys.path.insert(0, p)
    import make_jpeg_dataset
    from ep24.augment import MosaicTransform
    from ep24.fisheye import FisheyeTransform
    from ep24.input import TrainTransform
    from exp import Exp
    make_jpeg_dataset.make(str(tmp_path), 8)

    def loader(decoder):
        exp = Exp()
        exp.val_data_dir, exp.val_label_dir = str(tmp_path / "images"), str(tmp_path / "COCO_24p_label")
        exp.jpeg_decoder, exp.data_num_workers, exp.test_size = decoder, 0, (128, 160)
        return exp, exp.get_eval_loader(4)

    tt = TrainTransform(max_labels=50)
    (_, dev), (_, host) = loader("device"), loader("gpu")
    n = 0
    for (a_im, a_t, _, a_ids), (b_im, b_t, _, b_ids) in zip(dev, host):
        assert a_ids == b_ids and all(isinstance(im, jpeg.JpegScan) for im in a_im) and all(isinstance(im, jpeg.JpegCoefficients) for im in b_im)
        a, b = tt.batch(a_im, a_t, (128, 160)), tt.batch(b_im, b_t, (128, 160))
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
        n += len(a_ids)
    assert n == 8
    with open(str(tmp_path / "images" / ("%012d.jpg" % 6)), "wb") as fh:
        fh.write(ds.truncated_scene())
    exp, dev = loader("device")
    batches = list(dev)
    assert jpeg.scan(ds.truncated_scene()).data.size > 0              # the marker walk accepts it: only the GPU can tell
    tt.batch(batches[0][0], batches[0][1], (128, 160))                # files 1 .. 4: whole
    for transform in (tt, MosaicTransform(max_labels=50, seed=1), FisheyeTransform(max_labels=50, seed=1)):
        with pytest.raises(jpeg.JpegError) as e:
            transform.batch(batches[1][0], batches[1][1], (128, 160))
        assert e.value.code == jpeg.EP24JPEG_E_DATA and "000000000006.jpg" in str(e.value) and "--jpeg-decoder pil" in str(e.value), type(transform)
    exp.depth, exp.width = 0.33, 0.25
    model = exp.get_model().to("cuda")
    evaluator = exp.get_evaluator(4)
    with pytest.raises(jpeg.JpegError, match="000000000006.jpg"):
        exp.eval(model, evaluator, False)


def test_entry_point_trains_with_the_device_decoder(tmp_path):
    """``train_24p.py --data-dir ... --jpeg-decoder device --steps 3`` with a small Exp at 128 x 128, in a fresh process."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import make_jpeg_dataset
    finally:
        sys.path.remove(os.path.join(ROOT, "tools"))
    make_jpeg_dataset.make(str(tmp_path / "data"), 8)
    (tmp_path / "small_jpeg_exp.py").write_text(
        "from exp import Exp as MyExp\n\n\nclass Exp(MyExp):\n    def __init__(self):\n        super().__init__()\n"
        "        self.depth, self.width, self.input_size, self.test_size = 0.33, 0.25, (128, 128), (128, 128)\n"
        "        self.data_num_workers, self.max_epoch, self.exp_name = 2, 2, 'small_jpeg_device'\n")
    env = dict(os.environ)
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK"):
        env.pop(k, None)
    cmd = [sys.executable, os.path.join(Y24, "train_24p.py"), "-f", str(tmp_path / "small_jpeg_exp.py"), "-b", "4", "-l", "0.01",
           "--data-dir", str(tmp_path / "data" / "images"), "--label-dir", str(tmp_path / "data" / "COCO_24p_label"), "--jpeg-decoder", "device",
           "--steps", "3", "--log-interval", "1", "--output-dir", str(tmp_path / "out")]
    p = subprocess.run(cmd, cwd=Y24, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
    assert p.returncode == 0, p.stdout[-4000:]
    steps = [ln for ln in p.stdout.splitlines() if ln.startswith("step ")]
    assert len(steps) == 3, p.stdout[-2000:]
    losses = [float(ln.split("loss")[1].split()[0]) for ln in steps]
    assert all(np.isfinite(v) and 0 < v < 1e4 for v in losses), losses
