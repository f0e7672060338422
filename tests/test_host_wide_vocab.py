"""Custom vocabularies, host side (no GPU): infer_lam's --class_names / --bkg_names / --attr_bank parsing, every refusal before a model
is built, the text-row rule of the synthetic mode, ExCEL_model's class_names + bkg_names, and eval_labels on a 151-class tree."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

from excel_amd.tools import infer_lam, synthetic  # noqa: E402


def _names(n, stem="thing"):
    return [f"{stem} {i}" for i in range(n)]


def _write(path, names):
    path.write_text("\n".join(names) + "\n")
    return str(path)


def _parse(*argv):
    return infer_lam.get_parser().parse_args(list(argv))


@pytest.fixture
def no_model(monkeypatch):
    """The model constructor raises if it is reached: a refusal has to come first."""
    from excel_amd.model import model_excel

    def boom(*a, **k):
        raise AssertionError("a model was built before the vocabulary was checked")
    monkeypatch.setattr(model_excel, "ExCEL_model", boom)
    monkeypatch.setattr(infer_lam, "resolve_model_inputs", boom)


def test_vocabulary_files_are_parsed(tmp_path):
    from excel_amd.datasets.clip_text import BACKGROUND_CATEGORY
    fg = _write(tmp_path / "fg.txt", _names(150))
    a = _parse("--class_names", fg)
    assert a.num_classes == 21                                       # the parser's default, until the file is read
    v = infer_lam.resolve_vocabulary(a)
    assert a.num_classes == 151 and v["fg"] == _names(150) and v["bkg"] == list(BACKGROUND_CATEGORY) and v["bank"] is None
    assert infer_lam.class_names(a) == ["_background_"] + _names(150)
    b = _parse("--class_names", fg, "--num_classes", "151", "--bkg_names", _write(tmp_path / "bkg.txt", ["sky", "ground", "wall "]))
    assert infer_lam.resolve_vocabulary(b)["bkg"] == ["sky", "ground", "wall"] and b.num_classes == 151
    # without a file nothing changes
    c = _parse("--dataset_name", "ms_coco", "--num_classes", "81")
    assert infer_lam.resolve_vocabulary(c) == {"fg": None, "bkg": None, "bank": None} and c.num_classes == 81
    assert len(infer_lam.class_names(c)) == 81 and infer_lam.class_names(_parse()) == infer_lam.VOC_CLASSES


def test_attr_bank_files(tmp_path):
    rs = np.random.RandomState(0)
    bank = rs.standard_normal((64, 16)).astype(np.float32)
    np.savez(tmp_path / "bank.npz", bank=bank, flag=np.ones((3, 16), np.float32))
    torch.save([torch.from_numpy(bank), torch.ones(3, 16)], tmp_path / "bank.pth")
    for f in ("bank.npz", "bank.pth"):
        v = infer_lam.resolve_vocabulary(_parse("--attr_bank", str(tmp_path / f)))
        assert v["bank"].dtype == torch.float32 and np.array_equal(v["bank"].numpy(), bank)
    np.savez(tmp_path / "nobank.npz", centres=bank)
    with pytest.raises(ValueError, match="bank"):
        infer_lam.resolve_vocabulary(_parse("--attr_bank", str(tmp_path / "nobank.npz")))
    with pytest.raises(FileNotFoundError):
        infer_lam.resolve_vocabulary(_parse("--attr_bank", str(tmp_path / "missing.npz")))


def test_refusals_come_before_the_model(tmp_path, no_model):
    ok = _write(tmp_path / "ok.txt", _names(150))
    cases = [
        (["--class_names", _write(tmp_path / "dup.txt", ["cat", "dog", "cat"])], "appears on lines 1 and 3"),
        (["--class_names", _write(tmp_path / "empty.txt", ["cat", "", "dog"])], "line 2 is empty"),
        (["--class_names", _write(tmp_path / "f255.txt", _names(255))], "254"),
        (["--class_names", _write(tmp_path / "f254.txt", _names(254)), "--bkg_names", _write(tmp_path / "b259.txt", _names(259, "stuff"))], "512"),
        (["--class_names", ok, "--num_classes", "21"], "contradicts"),
        (["--class_names", ok, "--bkg_names", _write(tmp_path / "both.txt", ["sky", "thing 7"])], "both lists"),
        (["--class_names", ok, "--data_folder", str(tmp_path)], "needs --attr_bank"),
        (["--bkg_names", ok], "needs --class_names"),
        (["--num_classes", "256"], "255"),
    ]
    for argv, msg in cases:
        with pytest.raises(ValueError, match=msg):
            infer_lam.validate(_parse(*argv))
    # 254 names + 258 background names = 512 prompts are served
    a = _parse("--class_names", str(tmp_path / "f254.txt"), "--bkg_names", _write(tmp_path / "b258.txt", _names(258, "stuff")))
    v = infer_lam.resolve_vocabulary(a)
    assert a.num_classes == 255 and len(v["fg"]) + len(v["bkg"]) == 512


def test_pipeline_and_model_refuse_what_the_labels_cannot_hold():
    from excel_amd.model import ExCEL_model
    from excel_amd.pipeline import OptimisedLamPipeline, TrainingFreePipeline, check_num_classes
    check_num_classes(255)
    for cls in (TrainingFreePipeline, OptimisedLamPipeline):
        with pytest.raises(ValueError, match="uint8 with 255 as the ignore value"):
            cls(None, num_classes=256)
    with pytest.raises(ValueError, match="contradicts the 3 foreground"):
        ExCEL_model(clip_model="tiny", num_classes=21, class_names=["a", "b", "c"], bkg_names=["sky"])
    with pytest.raises(ValueError, match="needs class_names"):
        ExCEL_model(clip_model="tiny", num_classes=21, bkg_names=["sky"])


def test_synthetic_text_rows():
    assert synthetic.text_rows(21) == 45 and synthetic.text_rows(81) == 103           # the shipped vocabularies keep their rows
    assert synthetic.text_rows(5) == 45                                                # ... and the tiny training runs theirs
    assert synthetic.text_rows(151) == 150 + 25 and synthetic.text_rows(255) == 254 + 25
    assert synthetic.text_rows(172, n_bkg=30) == 201
    assert synthetic.text_rows(21, custom=True) == 45 and synthetic.text_rows(6, n_bkg=3, custom=True) == 8


def test_synthetic_model_inputs_follow_the_vocabulary(tmp_path, monkeypatch):
    monkeypatch.setattr(synthetic, "make_vit_state_dict", lambda seed=0: {"seed": seed})     # (86 M random weights are not the point)
    empty = str(tmp_path / "no_clip")
    for argv, T in ([[], 45], [["--num_classes", "81"], 103], [["--num_classes", "151"], 175],
                    [["--class_names", _write(tmp_path / "fg.txt", _names(150)), "--bkg_names", _write(tmp_path / "bkg.txt", _names(7, "stuff"))], 157]):
        a = _parse("--synthetic", "4", "--clip_root", empty, *argv)
        infer_lam.resolve_vocabulary(a)
        assert infer_lam.resolve_model_inputs(a)["text_features"].shape == (T, 512), argv


def test_eval_labels_scores_a_151_class_tree(tmp_path, caplog):
    """write_voc_tree(num_classes=151): the VOC-format reader's one-hot rows are 150 wide, the ground truth scored against itself is the
    diagonal matrix of its pixel counts, and the table carries the file's names."""
    import logging
    import shutil
    from excel_amd.tools import eval_labels
    root, lists = tmp_path / "VOC2012", tmp_path / "lists"
    ids, npix = synthetic.write_voc_tree(str(root), str(lists), 3, seed=2, split="val", num_classes=151)
    onehot = np.load(lists / "cls_labels_onehot.npy", allow_pickle=True).item()
    assert all(v.shape == (150,) for v in onehot.values())
    from excel_amd.datasets import voc
    ds = voc.VOC12SegDataset(root_dir=str(root), name_list_dir=str(lists), split="val", stage="val")
    assert len(ds) == 3 and np.asarray(ds[0][3]).shape[-1] == 150
    shutil.copytree(root / "SegmentationClassAug", tmp_path / "pred")
    names = _write(tmp_path / "fg.txt", _names(150))
    argv = ["--pred_dir", str(tmp_path / "pred"), "--data_folder", str(root), "--list_folder", str(lists), "--infer_set", "val", "--num_workers", "2"]
    with caplog.at_level(logging.INFO):
        out = eval_labels.validate(eval_labels.get_parser().parse_args(argv + ["--class_names", names]))
    h = out["hist"].numpy()
    assert h.shape == (151, 151) and int(h.sum()) == npix and int(np.trace(h)) == npix
    assert "| thing 149 " in "\n".join(r.getMessage() for r in caplog.records)
    out2 = eval_labels.validate(eval_labels.get_parser().parse_args(argv + ["--num_classes", "151"]))
    assert np.array_equal(out2["hist"].numpy(), h)
    with pytest.raises(ValueError, match="contradicts"):
        eval_labels.validate(eval_labels.get_parser().parse_args(argv + ["--class_names", names, "--num_classes", "21"]))
