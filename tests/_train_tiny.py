"""A tiny on-disk VOC tree, a tiny tower with a decoder head and the flags of a few-iteration run: what the training-program tests
share (the helpers of test_gpu_train_loop.py, as a module)."""
import numpy as np

NUM_CLASSES = 5


def voc_tree(tmp_path, n_train=8, n_val=2, seed=0):
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


def init_head():
    from excel_amd.model import init_decoder_state_dict
    return init_decoder_state_dict(num_classes=NUM_CLASSES, in_channels=128, embedding_dim=32, crop_size=96, seed=0, index=8)


def tiny_model(dec=None):
    """width 128, 8 layers, crop 96, gemm_mode f32; the head at its initial weights unless `dec` gives others"""
    from oracle.vit import VitConfig, make_vit_weights
    from excel_amd.model import ExCEL_model
    TINY = VitConfig(width=128, layers=8, heads=2, patch=16, out_dim=64, input_resolution=64, n_surgery=5)
    kw = dict(width=128, layers=8, heads=2, patch=16, output_dim=64, input_resolution=64)
    rs = np.random.RandomState(3)
    text = rs.standard_normal((9, 64)).astype(np.float32)
    text /= np.linalg.norm(text, axis=1, keepdims=True)
    if dec is None:
        dec = init_head()
    return ExCEL_model(clip_model="tiny", num_classes=NUM_CLASSES, img_size=96, mode="train", state_dict=make_vit_weights(TINY, seed=11),
                       vit_cfg=kw, text_attr=text.T.copy(), gemm_mode="f32", embedding_dim=32, in_channels=128, decoder_state_dict=dec)


def train_args(root, lists, work_dir, extra=(), **over):
    """--spg 2 over 8 training images: 4 batches per epoch.  `over`: flag values that replace the defaults below; `extra`: more flags."""
    from excel_amd.scripts.train_voc import get_parser
    flags = dict(data_folder=root, list_folder=lists, train_set="train", val_set="val", crop_size=96, spg=2, max_iters=7, eval_iters=3,
                 log_iters=2, num_classes=NUM_CLASSES, radius=2, work_dir=work_dir, num_workers=2, seed=5)
    flags.update(over)
    argv = [x for k, v in flags.items() for x in ("--" + k, str(v))]
    return get_parser().parse_args(argv + list(extra))
