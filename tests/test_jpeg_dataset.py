"""datasets.COCO24PFolderDataset, the Exp attributes and the train_24p.py flags that select it (no GPU needed)."""
import os
import sys

import numpy as np
import pytest

import jpeg_fixtures as fx

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
Y24 = os.path.join(ROOT, "exploration-of-potential_amd", "yolox_24p")
for p in (Y24, os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)

import make_jpeg_dataset  # noqa: E402
from ep24 import jpeg  # noqa: E402


@pytest.fixture()
def folder(tmp_path):
    made = make_jpeg_dataset.make(str(tmp_path), 8)
    return str(tmp_path / "images"), str(tmp_path / "COCO_24p_label"), made


def test_pairing_ids_rows_and_true_size(folder):
    from datasets import COCO24PFolderDataset, raw_collate
    data_dir, label_dir, made = folder
    ds = COCO24PFolderDataset(data_dir, label_dir)
    assert len(ds) == 8 and ds.ids == list(range(1, 9))
    cases = {c["name"]: c for c in fx.cases()}
    items = [ds[i] for i in range(8)]
    for (img, rows, hw, ident), (k, name, want) in zip(items, made):
        assert ident == k and isinstance(img, jpeg.JpegCoefficients)
        assert hw == (cases[name]["height"], cases[name]["width"]) == img.shape[:2]       # the true (h, w), not the reference's (h, h)
        assert rows.dtype == np.float64 and rows.shape == (len(want), 51) and np.array_equal(rows, want)
        assert np.array_equal(img.coef, fx.oracle_coefficients(name)[1])
    assert hw[0] != hw[1]
    assert [len(m[2]) for m in made].count(0) == 1 and items[4][1].shape == (0, 51)      # an empty label file: an image without objects
    images, targets, infos, ids = raw_collate(items[:3])
    assert len(images) == len(targets) == 3 and infos == [it[2] for it in items[:3]] and ids == [1, 2, 3]


def test_single_row_files_stay_two_dimensional_and_names_that_are_no_numbers(tmp_path):
    from datasets import COCO24PFolderDataset
    (tmp_path / "i").mkdir()
    (tmp_path / "l").mkdir()
    for stem in ("b_frame", "a_frame"):
        (tmp_path / "i" / (stem + ".jpg")).write_bytes(fx.data("q90_420_17x23"))
    (tmp_path / "l" / "a_frame.txt").write_text(" ".join(["3"] + ["0.5"] * 50) + "\n")
    (tmp_path / "l" / "b_frame.txt").write_text("")
    (tmp_path / "l" / "notes.md").write_text("not a label file")
    ds = COCO24PFolderDataset(str(tmp_path / "i"), str(tmp_path / "l"))
    assert ds.stems == ["a_frame", "b_frame"] and ds.ids == [0, 1]
    assert ds[0][1].shape == (1, 51) and ds[0][1][0, 0] == 3.0 and ds[1][1].shape == (0, 51) and ds[0][2] == (17, 23)


def test_missing_images_are_reported_at_construction(folder):
    from datasets import COCO24PFolderDataset
    data_dir, label_dir, _ = folder
    for k in (2, 3, 5, 6, 7, 8):
        os.remove(os.path.join(data_dir, "%012d.jpg" % k))
    with pytest.raises(FileNotFoundError) as e:
        COCO24PFolderDataset(data_dir, label_dir)
    msg = str(e.value)
    assert "6 of 8" in msg and "000000000002.jpg" in msg and "000000000007.jpg" in msg and "000000000008.jpg" not in msg and "..." in msg


def test_refused_file_names_the_file_and_the_other_decoder(folder):
    from datasets import COCO24PFolderDataset
    data_dir, label_dir, _ = folder
    with open(os.path.join(data_dir, "000000000002.jpg"), "wb") as fh:
        fh.write(fx.data("refused_progressive"))
    ds = COCO24PFolderDataset(data_dir, label_dir)
    with pytest.raises(jpeg.JpegError) as e:
        ds[1]
    assert e.value.code == jpeg.EP24_E_UNSUPPORTED and "000000000002.jpg" in str(e.value) and "--jpeg-decoder pil" in str(e.value)


def test_pil_decoder(folder, monkeypatch):
    from datasets import COCO24PFolderDataset
    data_dir, label_dir, made = folder
    try:
        import PIL  # noqa: F401
        have = True
    except ImportError:
        have = False
    if have:
        ds = COCO24PFolderDataset(data_dir, label_dir, decoder="pil")
        img, rows, hw, ident = ds[0]
        assert isinstance(img, np.ndarray) and img.dtype == np.uint8 and img.flags["C_CONTIGUOUS"]
        assert np.array_equal(img, fx.rgb(made[0][1])[:, :, ::-1]) and hw == img.shape[:2]        # BGR, as cv2.imread returns it
    # without Pillow: refused at construction
    import builtins
    real = builtins.__import__

    def no_pil(name, *a, **k):
        if name == "PIL" or name.startswith("PIL."):
            raise ImportError("No module named 'PIL'")
        return real(name, *a, **k)
    for m in [m for m in sys.modules if m == "PIL" or m.startswith("PIL.")]:
        monkeypatch.delitem(sys.modules, m)
    monkeypatch.setattr(builtins, "__import__", no_pil)
    with pytest.raises(ImportError, match="Pillow"):
        COCO24PFolderDataset(data_dir, label_dir, decoder="pil")
    with pytest.raises(ValueError):
        COCO24PFolderDataset(data_dir, label_dir, decoder="cv2")


def test_exp_builds_the_folder_loader(folder):
    """Shuffled per epoch from the seed, resumable, raw batches; loader processes capped at 16."""
    from exp import Exp
    from datasets import COCO24PFolderDataset, ResumableSampler, SyntheticDataset
    import datasets
    data_dir, label_dir, _ = folder
    exp = Exp()
    assert exp.data_dir is None and exp.label_dir is None and exp.val_data_dir is None and exp.val_label_dir is None and exp.jpeg_decoder == "gpu"
    assert datasets.COCO24PDataset is SyntheticDataset                                    # the alias stays
    exp.data_dir, exp.label_dir, exp.val_data_dir, exp.val_label_dir = data_dir, label_dir, data_dir, label_dir
    exp.data_num_workers = 40
    loader = exp.get_data_loader(4, raw_u8=True)
    assert isinstance(loader.dataset, COCO24PFolderDataset) and loader.num_workers == 16 and isinstance(loader.sampler, ResumableSampler)
    loader = exp.get_data_loader(4, raw_u8=True, workers=0)
    orders = []
    for epoch in (0, 1, 0):
        loader.sampler.set_epoch(epoch)
        batches = list(loader)
        assert len(batches) == 2 and all(len(b[0]) == 4 and isinstance(b[0][0], jpeg.JpegCoefficients) for b in batches)
        orders.append([i for b in batches for i in b[3]])
        assert sorted(orders[-1]) == list(range(1, 9))
    assert orders[0] == orders[2] and orders[0] != orders[1]
    val = exp.get_eval_loader(3)
    assert [b[3] for b in val] == [[1, 2, 3], [4, 5, 6], [7, 8]]
    with pytest.raises(Exception, match="raw batches"):
        exp.get_data_loader(4, raw_u8=False)


def test_loader_processes_hand_over_coefficients(folder):
    """Two loader processes: the items cross the process boundary unchanged, made without initialising CUDA."""
    from exp import Exp
    data_dir, label_dir, made = folder
    exp = Exp()
    exp.data_dir, exp.label_dir, exp.data_num_workers, exp.report_loader_cuda = data_dir, label_dir, 2, True
    loader = exp.get_data_loader(4, raw_u8=True)
    assert loader.num_workers == 2
    by_id = {k: name for k, name, _ in made}
    n = 0
    for images, targets, infos, ids in loader:
        for im, i in zip(images, ids):
            assert isinstance(im, jpeg.JpegCoefficients) and isinstance(im.coef, np.ndarray) and im.coef.dtype == np.int16 and im.tag is False
            assert np.array_equal(im.coef, fx.oracle_coefficients(by_id[i])[1])
            n += 1
    assert n == 8
    del loader


def _args(*argv):
    import train_24p
    return train_24p, train_24p.make_parser().parse_args(list(argv))


def test_new_flags_parse_and_reach_the_exp():
    mod, a = _args("--data-dir", "/d", "--label-dir", "/l", "--val-data-dir", "/vd", "--val-label-dir", "/vl", "--jpeg-decoder", "pil")
    assert (a.data_dir, a.label_dir, a.val_data_dir, a.val_label_dir, a.jpeg_decoder) == ("/d", "/l", "/vd", "/vl", "pil")
    mod.check_data_args(a)
    _, b = _args()
    assert (b.data_dir, b.label_dir, b.val_data_dir, b.val_label_dir, b.jpeg_decoder) == (None,) * 5
    mod.check_data_args(b)
    with pytest.raises(SystemExit):
        _args("--jpeg-decoder", "cv2")


@pytest.mark.parametrize("extra", [("--synthetic",), ("--fp32-batches",), ("--no-prefetch",)])
def test_data_dir_excludes_the_other_sources(extra):
    mod, a = _args("--data-dir", "/d", "--label-dir", "/l", *extra)
    with pytest.raises(SystemExit) as e:
        mod.check_data_args(a)
    assert "--data-dir" in str(e.value)
    _, v = _args("--val-data-dir", "/d", "--val-label-dir", "/l", *extra)
    with pytest.raises(SystemExit):
        mod.check_data_args(v)


def test_data_dir_needs_label_dir():
    mod, a = _args("--data-dir", "/d")
    with pytest.raises(SystemExit, match="go together"):
        mod.check_data_args(a)
