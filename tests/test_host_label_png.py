"""--save_label / eval_labels, host side (no GPU): the flags and the default directory, the C ABI's declarations and bindings, and
excel_amd.tools.eval_labels on a temporary tree against a plain numpy bincount."""
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PNG_SYMBOLS = ("excel_png_labels_bound_bytes", "excel_png_encode_labels_ragged")


def test_parser_knows_the_flags_and_they_default_to_off():
    from excel_amd.tools import infer_lam
    a = infer_lam.get_parser().parse_args([])
    assert a.save_label is False and a.label_dir is None
    b = infer_lam.get_parser().parse_args(["--save_label", "true", "--label_dir", "/x/y"])
    assert b.save_label is True and b.label_dir == "/x/y"


def test_label_output_dir_sits_next_to_the_cam_directories():
    from excel_amd.tools import infer_lam
    d = infer_lam.label_output_dir("/w/exp/checkpoints/run7/model_iter_30000.pth", "train_aug", True, True)
    assert d == "/w/exp/train_aug/train_aug_run7/model_iter_30000_lam_training_free/aff_lam_label"
    cam = infer_lam.cam_output_dirs("/w/exp/checkpoints/run7/model_iter_30000.pth", "train_aug", True, True)["cam_dir"]
    assert os.path.dirname(d) == os.path.dirname(cam)
    assert infer_lam.label_output_dir("/w/run/model.pth", "val", False, False) == "/w/run/val/val_model_lam_optimized/seeds_lam_label"
    assert infer_lam.label_output_dir(None, "val") == os.path.join("lam_cams", "val", "val_none_lam_training_free/aff_lam_label")


def test_header_declares_the_entries_and_they_are_bound():
    from excel_amd import _lib
    header = open(os.path.join(ROOT, "include", "excel_hip.h")).read()
    for name in PNG_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert name in _lib.SIGNATURES, name
    assert "tools/infer_lam.py:95" in header and "tools/training_free_attr.py:225" in header
    # the encoder: 7 device pointers, the host sizes, two byte counts, the plan info and the stream
    res, args = _lib.SIGNATURES["excel_png_encode_labels_ragged"]
    assert res is _lib.c_i and len(args) == 11
    assert _lib.SIGNATURES["excel_png_labels_bound_bytes"] == (_lib.c_sz, [_lib.c_i, _lib.c_i])


def _write_palette_png(path, a):
    from PIL import Image
    from excel_amd.utils import imutils
    os.makedirs(os.path.dirname(path), exist_ok=True)
    im = Image.fromarray(a)
    im.putpalette(imutils.colormap().reshape(-1).tolist())
    im.save(path)


def _tree(tmp_path, n=7, nc=21, seed=3):
    rs = np.random.RandomState(seed)
    root, lists, pred = tmp_path / "VOC2012", tmp_path / "lists", tmp_path / "pred"
    names, gts, preds = [], [], []
    for i in range(n):
        h, w = int(rs.randint(5, 60)), int(rs.randint(5, 70))
        gt = rs.randint(0, nc, (h, w)).astype(np.uint8)
        gt[rs.rand(h, w) < 0.1] = 255
        pr = np.where(rs.rand(h, w) < 0.6, gt, rs.randint(0, nc, (h, w))).astype(np.uint8)
        pr[rs.rand(h, w) < 0.05] = 255
        name = f"2007_{i:06d}"
        _write_palette_png(str(root / "SegmentationClassAug" / (name + ".png")), gt)
        _write_palette_png(str(pred / (name + ".png")), pr)
        names.append(name), gts.append(gt), preds.append(pr)
    os.makedirs(lists, exist_ok=True)
    (lists / "val.txt").write_text("\n".join(names) + "\n")
    argv = ["--pred_dir", str(pred), "--data_folder", str(root), "--list_folder", str(lists), "--infer_set", "val", "--num_workers", "2",
            "--batch_size", "3"]
    return argv, names, gts, preds


def test_eval_labels_equals_numpy_bincount(tmp_path):
    """The matrix goes through ops.confusion_accumulate when a GPU is present and through eval_labels' numpy path otherwise
    (utils/evaluate.hist_from_labels has no CPU path); the expectation is a plain bincount either way, the score dict the metric
    arithmetic of utils/evaluate.scores (scores_from_hist) on that matrix."""
    from excel_amd.tools import eval_labels
    from excel_amd.utils import evaluate
    argv, names, gts, preds = _tree(tmp_path)
    out = eval_labels.validate(eval_labels.get_parser().parse_args(argv))
    nc = 21
    want = np.zeros((nc, nc), np.int64)
    for g, p in zip(gts, preds):
        g, p = g.reshape(-1).astype(np.int64), p.reshape(-1).astype(np.int64)
        m = (g < nc) & (p < nc)
        want += np.bincount(nc * g[m] + p[m], minlength=nc * nc).reshape(nc, nc)
    assert sorted(out) == ["hist", "images", "score", "seconds"]
    assert out["images"] == len(names)
    assert np.array_equal(out["hist"].numpy(), want) and out["hist"].dtype.is_floating_point is False
    np.testing.assert_equal(out["score"], evaluate.scores_from_hist(want))
    assert 0.0 < out["score"]["miou"] < 1.0


def test_eval_labels_names_a_missing_prediction(tmp_path):
    from excel_amd.tools import eval_labels
    argv, names, _, _ = _tree(tmp_path)
    os.remove(tmp_path / "pred" / (names[4] + ".png"))
    with pytest.raises(FileNotFoundError, match=names[4] + r"\.png"):
        eval_labels.validate(eval_labels.get_parser().parse_args(argv))


def test_eval_labels_names_a_prediction_of_the_wrong_size(tmp_path):
    from excel_amd.tools import eval_labels
    argv, names, gts, _ = _tree(tmp_path)
    _write_palette_png(str(tmp_path / "pred" / (names[2] + ".png")), np.zeros((gts[2].shape[0] + 1, gts[2].shape[1]), np.uint8))
    with pytest.raises(ValueError, match=names[2] + r"\.png"):
        eval_labels.validate(eval_labels.get_parser().parse_args(argv))


def test_eval_labels_coco_ground_truth_path():
    from excel_amd.tools import eval_labels
    a = eval_labels.get_parser().parse_args(["--pred_dir", "/p", "--data_folder", "/coco", "--list_folder", "/l", "--infer_set", "val",
                                             "--dataset_name", "ms_coco"])
    assert eval_labels.label_paths(a, "COCO_val2014_000000000042") == ("/p/COCO_val2014_000000000042.png",
                                                                     "/coco/SegmentationClass/val/000000000042.png")
