"""``train_24p.py --copy-paste`` and the ``MosaicTransform`` / Exp wiring behind it, without a GPU."""
import argparse
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
Y24 = os.path.join(ROOT, "exploration-of-potential_amd", "yolox_24p")


@pytest.fixture
def mod():
    sys.path.insert(0, Y24)
    try:
        import importlib
        yield importlib.import_module("train_24p")
    finally:
        sys.path.remove(Y24)


def test_parser_defaults_leave_it_off(mod):
    d = mod.make_parser().parse_args([])
    assert d.copy_paste == 0.0 and not d.augment
    mod.check_copy_paste_args(d)                                                 # nothing to refuse
    assert mod.make_parser().parse_args(["--augment", "--copy-paste"]).copy_paste == 0.5      # the flag alone: const
    assert mod.make_parser().parse_args(["--augment", "--copy-paste", "0.25"]).copy_paste == 0.25
    a = mod.make_parser().parse_args(["--augment", "--mixup", "--multiscale", "--copy-paste", "0.4"])
    assert a.mixup and a.multiscale and a.copy_paste == 0.4                      # composes with the rest of the recipe
    mod.check_copy_paste_args(a)
    mod.check_mixup_args(a)


def test_copy_paste_without_augment_is_refused(mod):
    with pytest.raises(SystemExit, match="--copy-paste.*--augment"):
        mod.check_copy_paste_args(mod.make_parser().parse_args(["--copy-paste"]))
    with pytest.raises(SystemExit, match="--copy-paste.*--augment"):
        mod.check_copy_paste_args(mod.make_parser().parse_args(["--copy-paste", "0.3", "--mixup"]))
    for bad in ("1.5", "-0.1"):
        with pytest.raises(SystemExit, match="probability"):
            mod.check_copy_paste_args(mod.make_parser().parse_args(["--augment", "--copy-paste", bad]))
    mod.check_copy_paste_args(argparse.Namespace(augment=False))                 # a namespace from before the flag: off
    import inspect
    src = inspect.getsource(mod.Trainer.__init__)
    assert "check_copy_paste_args(args)" in src                                  # the trainer runs the check before it builds anything


def test_from_exp_wiring(mod):
    from exp import get_exp
    from ep24 import augment as aug
    exp = get_exp(os.path.join(Y24, "load_train", "yolox_24p_train.py"))
    assert exp.copy_paste_prob == 0.0                                            # the Exp's default: off
    off = aug.MosaicTransform.from_exp(exp, seed=3)
    assert off.copy_paste_prob == 0.0 and (off.copy_paste_obj_prob, off.copy_paste_ioa) == (0.5, 0.30)
    exp.copy_paste_prob = 0.7
    assert aug.MosaicTransform.from_exp(exp, seed=3).copy_paste_prob == 0.0       # only when asked for
    on = aug.MosaicTransform.from_exp(exp, seed=3, mixup=True, copy_paste=True)
    assert on.copy_paste_prob == 0.7 and on.mixup_prob == exp.mixup_prob
    sizes = [(120, 160)] * 4
    on.set_position(2, 5)
    p = on.sample(sizes, (128, 160), [3, 0, 2, 1])
    off.set_position(2, 5)
    q = off.sample(sizes, (128, 160), [3, 0, 2, 1])
    assert p.paste.any() and not q.paste.any()
    # the paste draws come from a generator of their own: mosaic, affine, mirror and HSV parameters are those of the transform without
    for name in ("mosaic", "centre", "partners", "M", "mirror", "hsv_on", "hsv"):
        assert (getattr(p, name) == getattr(q, name)).all(), name
    on.set_position(2, 5)
    again = on.sample(sizes, (128, 160), [3, 0, 2, 1])
    assert (again.paste_select == p.paste_select).all() and (again.paste_off == p.paste_off).all()   # set_position reseeds it
    on.set_position(2, 6)
    other = on.sample(sizes, (128, 160), [3, 0, 2, 1])
    assert (other.paste_select != p.paste_select).any()


def test_trainer_hands_the_probability_to_the_exp(mod):
    """``Trainer.augment_transform`` with --copy-paste P: the Exp's attribute becomes P, the transform reads it, and the transform goes
    off with the rest at no_aug_epochs."""
    import types
    from exp import get_exp
    exp = get_exp(os.path.join(Y24, "load_train", "yolox_24p_train.py"))
    exp.no_aug_epochs = 1
    tr = mod.Trainer.__new__(mod.Trainer)
    tr.exp, tr.args = exp, types.SimpleNamespace(mixup=False, copy_paste=0.5, augment_seed=0)
    tr.epoch, tr.max_epoch = 0, 3
    t = tr.augment_transform()
    assert exp.copy_paste_prob == 0.5 and t.copy_paste_prob == 0.5 and t.mixup_prob == 0.0 and t.enabled
    tr.epoch = 2
    assert tr.augment_transform() is t and not t.enabled
    tr2 = mod.Trainer.__new__(mod.Trainer)
    tr2.exp, tr2.args = get_exp(os.path.join(Y24, "load_train", "yolox_24p_train.py")), types.SimpleNamespace(mixup=False, augment_seed=0)
    tr2.epoch, tr2.max_epoch = 0, 3
    assert tr2.augment_transform().copy_paste_prob == 0.0
