"""On-disk MS COCO input format: mirror of datasets/coco.py:22-230.

  JPEGImages/{train,val}/<COCO_train2014_000000xxxxxx>.jpg, SegmentationClass/{train,val}/<000000xxxxxx>.png (the label file name
  drops the "COCO_train2014_" / "COCO_val2014_" prefix, :62,:68), grey-scale JPEGs are replicated to 3 channels (:22-26).
Samples carry the decoded uint8 image (normalised on the device, ops.normalize_img_u8) like excel_amd/datasets/voc.py.
CocoClsDataset (stage train, aug on, :81-170) carries no label map: its transform runs on the DEVICE (ops.train_augment_image).
"""
import os

import numpy as np

from .voc import _imread, load_cls_label_list, load_img_name_list

# the 80 COCO category names in the reference's order (data)
class_list = ['_background_', 'person', 'bicycle', 'car', 'motorcycle', 'airplane', 'bus', 'train', 'truck', 'boat', 'traffic light', 'fire hydrant', 'stop sign', 'parking meter', 'bench', 'bird', 'cat', 'dog', 'horse', 'sheep', 'cow', 'elephant', 'bear', 'zebra', 'giraffe', 'backpack', 'umbrella', 'handbag', 'tie', 'suitcase', 'frisbee', 'skis', 'snowboard', 'sports ball', 'kite', 'baseball bat', 'baseball glove', 'skateboard', 'surfboard', 'tennis racket', 'bottle', 'wine glass', 'cup', 'fork', 'knife', 'spoon', 'bowl', 'banana', 'apple', 'sandwich', 'orange', 'broccoli', 'carrot', 'hot dog', 'pizza', 'donut', 'cake', 'chair', 'couch', 'potted plant', 'bed', 'dining table', 'toilet', 'tv', 'laptop', 'mouse', 'remote', 'keyboard', 'cell phone', 'microwave', 'oven', 'toaster', 'sink', 'refrigerator', 'book', 'clock', 'vase', 'scissors', 'teddy bear', 'hair drier', 'toothbrush']


def robust_read_image(path):
    image = _imread(path)
    return np.stack((image, image, image), axis=-1) if image.ndim < 3 else image


class CocoDataset:
    def __init__(self, root_dir=None, name_list_dir=None, split="train", stage="train"):
        self.root_dir, self.stage = root_dir, stage
        sub = "train" if "train" in split else ("val" if "val" in split else "")
        self.img_dir = os.path.join(root_dir, "JPEGImages", sub)
        self.label_dir = os.path.join(root_dir, "SegmentationClass", sub)
        self.name_list = load_img_name_list(os.path.join(name_list_dir, split + ".txt"))

    def __len__(self):
        return len(self.name_list)

    def __getitem__(self, idx):
        full = str(self.name_list[idx])
        image = robust_read_image(os.path.join(self.img_dir, full + ".jpg"))
        if self.stage == "test":
            return full, full, image, image[:, :, 0]
        short = full[15:] if self.stage == "train" else full[13:]          # strip "COCO_train2014_" / "COCO_val2014_"
        return full, short, image, _imread(os.path.join(self.label_dir, short + ".png"))


class CocoSegDataset(CocoDataset):
    """(name, image uint8 [h,w,3], label uint8 [h,w], cls_label f32 [80]); `batch` as in datasets/voc.VOC12SegDataset."""

    def __init__(self, root_dir=None, name_list_dir=None, split="val", stage="val", ignore_index=255, cls_labels_optional=False, **kwargs):
        """`cls_labels_optional`: as in datasets/voc.VOC12SegDataset (a run that predicts its tags needs no cls_labels_onehot.npy)."""
        super().__init__(root_dir, name_list_dir, split, stage)
        self.ignore_index = ignore_index
        self.has_cls_labels = stage != "test"
        if cls_labels_optional and not os.path.isfile(os.path.join(name_list_dir, "cls_labels_onehot.npy")):
            self.has_cls_labels = False
        self.label_list = load_cls_label_list(name_list_dir) if self.has_cls_labels else None

    def __getitem__(self, idx):
        full, short, image, label = super().__getitem__(idx)
        cls = np.zeros(len(class_list) - 1, np.float32) if self.label_list is None else np.asarray(self.label_list[full], np.float32)
        return full, np.ascontiguousarray(image[..., :3], np.uint8), np.ascontiguousarray(label, np.uint8), cls

    def max_k(self):
        return 18           # the largest number of present classes of a COCO 2014 image

    def batch(self, indices):
        items = [self[i] for i in indices]
        if len({it[1].shape for it in items}) != 1:
            raise ValueError("COCO images have different sizes: use batch_size 1 or resize first")
        return ([it[0] for it in items], np.stack([it[1] for it in items]), np.stack([it[2] for it in items]), np.stack([it[3] for it in items]))


class CocoClsDataset(CocoDataset):
    """Training samples of the reference's CocoClsDataset(aug=True): (name, image uint8 [h,w,3], None, cls one-hot f32 [80], params)
    where `params` is one ops.aug_params_dtype() record - the random draws of the transform (:112-142), which ops.train_augment_image
    applies on the device (random_scaling, random_fliplr, random_crop, normalize_img, HWC->CHW).

    The transform is the image-only one: random_crop(image, label=None) takes get_random_cropbox's FIRST draw (datasets/transforms.py:
    141-146), with no cat_max_ratio retry.  The draws follow the reference's order and distributions: ratio ~ U(rescale_range), flip
    when random() > 0.5, H_pad ~ randint(H - h' + 1), W_pad ~ randint(W - w' + 1), then ONE (H_start, W_start) pair; that origin fills
    every candidate slot of the record, so excel_train_aug_plan's range checks apply to it unchanged.  The generator is seeded by
    (seed, epoch, index) as in datasets/voc.VOC12ClsDataset.
    The reference's base class reads the label PNG and discards it; here it is not read at all, so a training tree needs no
    SegmentationClass/train.  PhotoMetricDistortion is built by the reference but never called; it is not applied here either."""

    def __init__(self, root_dir=None, name_list_dir=None, split="train", stage="train", resize_range=(512, 640), rescale_range=(0.5, 2.0),
                 crop_size=512, img_fliplr=True, ignore_index=255, num_classes=81, aug=True, seed=0, **kwargs):
        if not aug:
            raise ValueError("CocoClsDataset mirrors the training transform (aug=True); evaluation data is CocoSegDataset")
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
        hs, ws = rng.integers(0, [H - S + 1, W - S + 1])
        p["cand_h"], p["cand_w"] = hs, ws
        return p

    def sample(self, idx, epoch=None):
        full = str(self.name_list[idx])
        image = robust_read_image(os.path.join(self.img_dir, full + ".jpg"))
        image = np.ascontiguousarray(image[..., :3], np.uint8)
        cls = np.asarray(self.label_list[full], np.float32)
        return full, image, None, cls, self.draw_params(idx, image.shape[0], image.shape[1], epoch)

    def __getitem__(self, idx):
        return self.sample(idx)
