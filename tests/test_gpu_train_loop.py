"""scripts/train_voc.train end to end on a tiny on-disk VOC tree and a tiny tower: device augmentation, training iterations,
checkpoints loadable by tools/infer_lam, validation, reproducibility."""
import logging
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

NUM_CLASSES = 5


def _voc_tree(tmp_path, n_train=8, n_val=2, seed=0):
    from PIL import Image
    rng = np.random.default_rng(seed)
    root = tmp_path / "VOC"
    (root / "JPEGImages").mkdir(parents=True)
    (root / "SegmentationClassAug").mkdir()
    onehot, names = {}, []
    for i in range(n_train + n_val):
        name = f"2008_{i:06d}"
        h, w = int(rng.integers(60, 150)), int(rng.integers(60, 150))
        im = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
        Image.fromarray(im).save(root / "JPEGImages" / f"{name}.jpg", quality=90)
        lab = np.zeros((h, w), np.uint8)
        c = 1 + i % (NUM_CLASSES - 1)
        lab[h // 4:3 * h // 4, w // 4:3 * w // 4] = c
        lab[h // 4, :] = 255
        png = Image.fromarray(lab, mode="P")
        png.putpalette(list(rng.integers(0, 256, 768, dtype=np.uint8)))
        png.save(root / "SegmentationClassAug" / f"{name}.png")
        oh = np.zeros(NUM_CLASSES - 1, np.float32)
        oh[c - 1] = 1
        onehot[name] = oh
        names.append(name)
    lists = tmp_path / "lists"
    lists.mkdir()
    (lists / "train.txt").write_text("\n".join(names[:n_train]) + "\n")
    (lists / "val.txt").write_text("\n".join(names[n_train:]) + "\n")
    np.save(lists / "cls_labels_onehot.npy", onehot)
    return str(root), str(lists)


def _tiny_model(dec=None):
    from oracle.vit import VitConfig, make_vit_weights
    from excel_amd.model import ExCEL_model, init_decoder_state_dict
    TINY = VitConfig(width=128, layers=8, heads=2, patch=16, out_dim=64, input_resolution=64, n_surgery=5)
    kw = dict(width=128, layers=8, heads=2, patch=16, output_dim=64, input_resolution=64)
    rs = np.random.RandomState(3)
    text = rs.standard_normal((9, 64)).astype(np.float32)
    text /= np.linalg.norm(text, axis=1, keepdims=True)
    if dec is None:
        dec = init_decoder_state_dict(num_classes=NUM_CLASSES, in_channels=128, embedding_dim=32, crop_size=96, seed=0, index=8)
    return ExCEL_model(clip_model="tiny", num_classes=NUM_CLASSES, img_size=96, mode="train", state_dict=make_vit_weights(TINY, seed=11),
                       vit_cfg=kw, text_attr=text.T.copy(), gemm_mode="f32", embedding_dim=32, in_channels=128, decoder_state_dict=dec)


def _args(root, lists, work_dir):
    from excel_amd.scripts.train_voc import get_parser
    return get_parser().parse_args(["--data_folder", root, "--list_folder", lists, "--train_set", "train", "--val_set", "val",
                                    "--crop_size", "96", "--spg", "2", "--max_iters", "6", "--eval_iters", "3", "--log_iters", "2",
                                    "--num_classes", str(NUM_CLASSES), "--radius", "2", "--work_dir", work_dir, "--num_workers", "2",
                                    "--seed", "5"])


@pytest.mark.timeout(600)
def test_train_loop_end_to_end(tmp_path, caplog):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from excel_amd.scripts.train_voc import train
    from excel_amd.tools import infer_lam
    root, lists = _voc_tree(tmp_path)
    caplog.set_level(logging.INFO)
    model = _tiny_model()
    res = train(_args(root, lists, str(tmp_path / "run1")), model=model)
    hist = res["history"]
    assert len(hist) == 6 and all(np.isfinite(h["seg_loss"]) and np.isfinite(h["diver_loss"]) for h in hist)
    ck = [str(tmp_path / "run1" / "checkpoints" / f"model_iter_{n}.pth") for n in (3, 6)]
    assert res["ckpts"] == ck and all(os.path.isfile(p) for p in ck)
    assert len(res["tables"]) == 2 and all("Seg_Preds" in t and "Attr_aff_Pseudo" in t for t in res["tables"])
    text = caplog.text
    assert "Iter: 2; Elasped:" in text and "seg_loss:" in text and "Seg_Preds" in text

    # the last checkpoint through the loader `infer_lam --model_path` uses reproduces the in-memory head's seg output
    a = infer_lam.get_parser().parse_args(["--training_free", "false", "--synthetic", "2", "--model_path", ck[1]])
    loaded = _tiny_model(dec=infer_lam.resolve_model_inputs(a)["decoder_state_dict"])
    x = torch.randn(2, 3, 96, 96, generator=torch.Generator().manual_seed(0)).cuda()
    seg_mem = model(x)[0]
    seg_ck = loaded(x)[0]
    assert torch.equal(seg_mem, seg_ck)

    # same seed, fresh model: the same loss log
    res2 = train(_args(root, lists, str(tmp_path / "run2")), model=_tiny_model())
    log1 = open(tmp_path / "run1" / "losses.txt").read()
    log2 = open(tmp_path / "run2" / "losses.txt").read()
    assert log1 == log2 and len(log1.splitlines()) == 6
    assert [h["seg_loss"] for h in res2["history"]] == [h["seg_loss"] for h in hist]
