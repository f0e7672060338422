"""--save_visual of the decoder training programs end to end on the tiny on-disk VOC / COCO trees and the tiny tower of
test_gpu_train_loop.py / test_gpu_train_coco.py (helpers copied): the PNG files of the progress panels, the ground-truth panel against
the augmented labels, and that rendering does not perturb training (the loss log is byte-identical to a run without it)."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

import _train_panels_ref as R  # noqa: E402

S, G, SPG = 96, 6, 2


def _voc_tree(tmp_path, n_train=8, n_val=2, seed=0, num_classes=5):
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
        c = 1 + i % (num_classes - 1)
        lab[h // 4:3 * h // 4, w // 4:3 * w // 4] = c
        lab[h // 4, :] = 255
        png = Image.fromarray(lab, mode="P")
        png.putpalette(list(rng.integers(0, 256, 768, dtype=np.uint8)))
        png.save(root / "SegmentationClassAug" / f"{name}.png")
        oh = np.zeros(num_classes - 1, np.float32)
        oh[c - 1] = 1
        onehot[name] = oh
        names.append(name)
    lists = tmp_path / "lists"
    lists.mkdir()
    (lists / "train.txt").write_text("\n".join(names[:n_train]) + "\n")
    (lists / "val.txt").write_text("\n".join(names[n_train:]) + "\n")
    np.save(lists / "cls_labels_onehot.npy", onehot)
    return str(root), str(lists)


def _coco_tree(tmp_path, n_train=4, seed=0):
    from PIL import Image
    rng = np.random.default_rng(seed)
    root = tmp_path / "COCO"
    for d in ("JPEGImages/train", "JPEGImages/val", "SegmentationClass/val"):
        (root / d).mkdir(parents=True)
    onehot, train = {}, []
    for i in range(n_train):
        name = f"COCO_train2014_{i:012d}"
        h, w = int(rng.integers(60, 150)), int(rng.integers(60, 150))
        Image.fromarray(rng.integers(0, 256, (h, w, 3), dtype=np.uint8)).save(root / "JPEGImages" / "train" / f"{name}.jpg", quality=90)
        oh = np.zeros(80, np.float32)
        oh[(7 * i) % 80] = 1
        onehot[name] = oh
        train.append(name)
    lists = tmp_path / "lists"
    lists.mkdir()
    (lists / "train.txt").write_text("\n".join(train) + "\n")
    (lists / "val_part.txt").write_text("")
    np.save(lists / "cls_labels_onehot.npy", onehot)
    return str(root), str(lists)


def _tiny_model(num_classes=5):
    from oracle.vit import VitConfig, make_vit_weights
    from excel_amd.model import ExCEL_model, init_decoder_state_dict
    TINY = VitConfig(width=128, layers=8, heads=2, patch=16, out_dim=64, input_resolution=64, n_surgery=5)
    kw = dict(width=128, layers=8, heads=2, patch=16, output_dim=64, input_resolution=64)
    rs = np.random.RandomState(3)
    text = rs.standard_normal((num_classes - 1 + 5, 64)).astype(np.float32)
    text /= np.linalg.norm(text, axis=1, keepdims=True)
    dec = init_decoder_state_dict(num_classes=num_classes, in_channels=128, embedding_dim=32, crop_size=S, seed=0, index=8)
    return ExCEL_model(clip_model="tiny", num_classes=num_classes, img_size=S, mode="train", state_dict=make_vit_weights(TINY, seed=11),
                       vit_cfg=kw, text_attr=text.T.copy(), gemm_mode="f32", embedding_dim=32, in_channels=128, decoder_state_dict=dec)


def _voc_args(root, lists, work_dir, save_visual):
    from excel_amd.scripts.train_voc import get_parser
    return get_parser().parse_args(["--data_folder", root, "--list_folder", lists, "--train_set", "train", "--val_set", "val",
                                    "--crop_size", str(S), "--spg", str(SPG), "--max_iters", "4", "--eval_iters", "100", "--log_iters", "2",
                                    "--num_classes", "5", "--radius", "2", "--work_dir", work_dir, "--num_workers", "2", "--seed", "5",
                                    "--save_visual", save_visual])


def _pngs(d):
    from PIL import Image
    out = {}
    for f in sorted(os.listdir(d)):
        im = Image.open(os.path.join(d, f))
        assert im.mode == "RGB", f
        out[f] = np.asarray(im)
    return out


@pytest.mark.timeout(300)
def test_voc_writes_six_panels_and_leaves_training_alone(tmp_path):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from excel_amd.scripts import train_voc
    root, lists = _voc_tree(tmp_path)
    seen = []

    class Recording(train_voc.TrainVariant):
        @staticmethod
        def augment_with_gt(images, plan, labels, args):
            inputs, gt = train_voc.TrainVariant.augment_with_gt(images, plan, labels, args)
            seen.append((inputs.cpu(), gt.cpu().numpy()))
            return inputs, gt

    class Tags:
        calls = []

        def add_image(self, tag, img, global_step=None):
            self.calls.append((tag, global_step, img.cpu().numpy()))

    run1 = tmp_path / "run1"
    res = train_voc.train(_voc_args(root, lists, str(run1), "true"), model=_tiny_model(), variant=Recording(), tb_writer=Tags())
    dirs = [str(run1 / "visual" / f"iter_{n}") for n in (2, 4)]
    assert res["visuals"] == dirs and len(seen) == 2
    plan = R.plan(SPG, S, G)[0]
    for d, (inputs, gt) in zip(dirs, seen):
        files = _pngs(d)
        assert sorted(files) == sorted(n + ".png" for n in R.PANELS)
        for n in R.PANELS:
            assert files[n + ".png"].shape == plan[n][:2] + (3,), n
        assert (gt == 255).any() and (gt > 0).any()
        assert np.array_equal(files["seg_gt.png"], R.make_grid(R.label_rgb(gt)))
        assert np.array_equal(files["img1.png"], R.make_grid(R.img1(inputs)))
    # the writer object got the same grids, CHW, under the reference's tags, at global_step = n_iter + 1
    assert [(t, s) for t, s, _ in Tags.calls] == [("visual/" + n, step) for step in (2, 4) for n in R.PANELS]
    last = _pngs(dirs[1])
    for (tag, _, chw), n in zip(Tags.calls[6:], R.PANELS):
        assert np.array_equal(chw.transpose(1, 2, 0), last[n + ".png"]), n

    # the same seed without the feature: the same loss log, no visual directory
    run2 = tmp_path / "run2"
    res2 = train_voc.train(_voc_args(root, lists, str(run2), "false"), model=_tiny_model())
    assert "visuals" not in res2 and not (run2 / "visual").exists()
    log1, log2 = (run1 / "losses.txt").read_bytes(), (run2 / "losses.txt").read_bytes()
    assert log1 == log2 and len(log1.splitlines()) == 4


@pytest.mark.timeout(300)
def test_coco_writes_five_panels(tmp_path):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from excel_amd.scripts import train_coco
    root, lists = _coco_tree(tmp_path)
    run = tmp_path / "run"
    a = train_coco.get_parser().parse_args(["--data_folder", root, "--list_folder", lists, "--crop_size", str(S), "--spg", str(SPG),
                                            "--max_iters", "2", "--eval_iters", "100", "--log_iters", "2", "--radius", "2", "--work_dir", str(run),
                                            "--num_workers", "2", "--seed", "5", "--save_visual", "true", "--visual_dir", str(tmp_path / "vis")])
    res = train_coco.train(a, model=_tiny_model(num_classes=81))
    assert res["visuals"] == [str(tmp_path / "vis" / "iter_2")] and not (run / "visual").exists()
    files = _pngs(res["visuals"][0])
    plan = R.plan(SPG, S, G, panels=[n for n in R.PANELS if n != "seg_gt"])[0]
    assert sorted(files) == sorted(n + ".png" for n in plan)
    for n in plan:
        assert files[n + ".png"].shape == plan[n][:2] + (3,), n
