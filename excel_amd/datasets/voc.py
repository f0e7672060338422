"""On-disk PASCAL VOC input format (the data side before the path): mirror of the inference-time parts of datasets/voc.py.

  load_img_name_list / load_cls_label_list   :21-27   (split .txt of image ids; cls_labels_onehot.npy = pickled {id: one-hot[20]})
  VOC12Dataset.__getitem__                   :49-70   (JPEGImages/<id>.jpg, SegmentationClassAug/<id>.png; test: no label)
  VOC12ClsDataset (stage train, aug on)     :73-139  (the transform of :110-117 runs on the DEVICE: samples carry the decoded
                                                        uint8 image and label plus the random draws; ops.train_augment)
  VOC12SegDataset (stage val/test, aug off)  :133-230 (normalize_img + HWC->CHW happen on the DEVICE here: samples carry the
                                                        decoded uint8 image, 3 B/pixel over PCIe; ops.normalize_img_u8)

Decoding uses PIL (the reference's imageio.v2.imread delegates to the same Pillow decoder for .jpg/.png).
"""
import os

import numpy as np

class_list = ["_background_", "aeroplane", "bicycle", "bird", "boat", "bottle", "bus", "car", "cat", "chair", "cow", "diningtable",
              "dog", "horse", "motorbike", "person", "pottedplant", "sheep", "sofa", "train", "tvmonitor"]


def load_img_name_list(img_name_list_path):
    return np.loadtxt(img_name_list_path, dtype=str, ndmin=1)


def load_cls_label_list(name_list_dir):
    return np.load(os.path.join(name_list_dir, "cls_labels_onehot.npy"), allow_pickle=True).item()


def _imread(path):
    from PIL import Image
    with Image.open(path) as im:
        return np.asarray(im)          # palette PNGs give the index map, JPEGs the RGB array (like imageio.v2.imread)


class VOC12Dataset:
    def __init__(self, root_dir=None, name_list_dir=None, split="train", stage="train"):
        self.root_dir, self.stage = root_dir, stage
        self.img_dir = os.path.join(root_dir, "JPEGImages")
        self.label_dir = os.path.join(root_dir, "SegmentationClassAug")
        self.name_list = load_img_name_list(os.path.join(name_list_dir, split + ".txt"))

    def __len__(self):
        return len(self.name_list)

    def __getitem__(self, idx):
        name = str(self.name_list[idx])
        image = _imread(os.path.join(self.img_dir, name + ".jpg"))
        if image.ndim == 2:
            image = np.stack([image] * 3, -1)
        label = image[:, :, 0] if self.stage == "test" else _imread(os.path.join(self.label_dir, name + ".png"))
        return name, image, label


class VOC12SegDataset(VOC12Dataset):
    """Inference-time samples: (name, image uint8 [h,w,3], label uint8 [h,w], cls_label f32 [20]).  `batch` keeps the calling
    convention of tools/synthetic.SyntheticSegDataset so tools/infer_lam.build_validation can consume either."""

    def __init__(self, root_dir=None, name_list_dir=None, split="val", stage="val", ignore_index=255, cls_labels_optional=False,
                 num_fg=None, **kwargs):
        """`cls_labels_optional` (a run that predicts its tags, tools/infer_lam --tags clip): without cls_labels_onehot.npy the samples
        carry rows of `num_fg` zeros and `has_cls_labels` is False; with the file nothing changes (its rows then score the tagger)."""
        super().__init__(root_dir, name_list_dir, split, stage)
        self.ignore_index = ignore_index
        self.num_fg = int(num_fg) if num_fg else len(class_list) - 1
        self.has_cls_labels = stage != "test"
        if cls_labels_optional and not os.path.isfile(os.path.join(name_list_dir, "cls_labels_onehot.npy")):
            self.has_cls_labels = False
        self.label_list = load_cls_label_list(name_list_dir) if self.has_cls_labels else None

    def __getitem__(self, idx):
        name, image, label = super().__getitem__(idx)
        cls = np.zeros(self.num_fg, np.float32) if self.label_list is None else np.asarray(self.label_list[name], np.float32)
        return name, np.ascontiguousarray(image[..., :3], np.uint8), np.ascontiguousarray(label, np.uint8), cls

    def max_k(self):
        return 6            # the largest number of present classes of a VOC train_aug image

    def batch(self, indices):
        items = [self[i] for i in indices]
        if len({it[1].shape for it in items}) != 1:
            raise ValueError("VOC images have different sizes: use batch_size 1 (tools/infer_lam.py:167 does) or resize first")
        return ([it[0] for it in items], np.stack([it[1] for it in items]), np.stack([it[2] for it in items]), np.stack([it[3] for it in items]))


class VOC12ClsDataset(VOC12Dataset):
    """Training samples of the reference's VOC12ClsDataset(aug=True): (name, image uint8 [h,w,3], label uint8 [h,w], cls one-hot f32 [20],
    params) where `params` is one ops.aug_params_dtype() record - the random draws of the transform (:110-117), which
    ops.train_augment applies on the device (random_scaling, random_fliplr, random_crop, normalize_img, HWC->CHW).

    The draws follow the reference's order and distributions (datasets/transforms.py): ratio ~ U(rescale_range) (:29), flip when
    random() > 0.5 (:75), H_pad ~ randint(H - h' + 1), W_pad ~ randint(W - w' + 1) (:127-128), then the crop candidates as
    (randrange(H - S + 1), randrange(W - S + 1)) pairs (:144-147).  They come from a generator seeded by (seed, epoch, index), so a
    run is reproducible whatever the number of decode workers.  The reference stops drawing candidates at the first accepted
    window; here all 10 are drawn up front (the device picks among them), so the random STREAM differs from the reference's while
    every draw has the same distribution.
    The reference builds a PhotoMetricDistortion (:95) but never calls it on this path; it is not applied here either.
    `img_fliplr=False` turns the flip off (the reference ignores the flag and always flips with probability 1/2); the default True is
    the reference's behaviour."""

    def __init__(self, root_dir=None, name_list_dir=None, split="train", stage="train", resize_range=(512, 640), rescale_range=(0.5, 2.0),
                 crop_size=512, img_fliplr=True, ignore_index=255, num_classes=21, aug=True, seed=0, **kwargs):
        if not aug:
            raise ValueError("VOC12ClsDataset mirrors the training transform (aug=True); evaluation data is VOC12SegDataset")
        super().__init__(root_dir, name_list_dir, split, stage)
        self.rescale_range, self.crop_size, self.img_fliplr = tuple(rescale_range), int(crop_size), img_fliplr
        self.ignore_index, self.num_classes, self.seed = ignore_index, num_classes, seed
        self.label_list = load_cls_label_list(name_list_dir)
        self.epoch = 0

    def set_epoch(self, epoch):
        self.epoch = int(epoch)

    def draw_params(self, idx, h, w, epoch=None):
        """The transform's random draws for sample `idx` of size h x w in `epoch` (default: the current one)."""
        from .. import ops
        rng = np.random.default_rng([int(self.seed), int(self.epoch if epoch is None else epoch), int(idx)])
        S = self.crop_size
        p = np.zeros((), ops.aug_params_dtype())
        ratio = rng.uniform(*self.rescale_range)
        flip = rng.random() > 0.5
        h2, w2 = int(ratio * h), int(ratio * w)
        H, W = max(S, h2), max(S, w2)
        p["ratio"] = ratio
        p["flip"] = int(flip and self.img_fliplr)
        p["h_pad"] = rng.integers(H - h2 + 1)
        p["w_pad"] = rng.integers(W - w2 + 1)
        cand = rng.integers(0, [H - S + 1, W - S + 1], size=(ops.AUG_CANDIDATES, 2))
        p["cand_h"], p["cand_w"] = cand[:, 0], cand[:, 1]
        return p

    def sample(self, idx, epoch=None):
        name, image, label = VOC12Dataset.__getitem__(self, idx)
        image = np.ascontiguousarray(image[..., :3], np.uint8)
        cls = np.asarray(self.label_list[name], np.float32)
        return name, image, np.ascontiguousarray(label, np.uint8), cls, self.draw_params(idx, image.shape[0], image.shape[1], epoch)

    def __getitem__(self, idx):
        return self.sample(idx)
