"""A plain folder of images: the data side of a label-free run (tools/infer_lam --unlabeled true).

  <root_dir>/JPEGImages/<id>.jpg   for the ids of <name_list_dir>/<split>.txt   (datasets/voc.py's layout without SegmentationClassAug)

Samples are (name, image uint8 [h,w,3], None, cls f32 [F]): no ground-truth map exists, so the ragged batches carry labels = None
(datasets/loader.pack_samples).  `cls` comes from `label_list` ({id: one-hot [F]}, the format of cls_labels_onehot.npy - e.g. the file
a --save_tags run wrote) or, without one, is a row of zeros that a pipeline with a tagger never reads.
"""
import os

import numpy as np

from .voc import _imread, load_img_name_list


class ImageListDataset:
    def __init__(self, root_dir, name_list_dir, split="train", num_fg=20, label_list=None):
        self.root_dir = root_dir
        self.img_dir = os.path.join(root_dir, "JPEGImages")
        self.name_list = load_img_name_list(os.path.join(name_list_dir, split + ".txt"))
        self.num_fg = int(num_fg)
        self.label_list = label_list
        self.has_cls_labels = label_list is not None
        if label_list is not None:
            missing = [str(n) for n in self.name_list if str(n) not in label_list]
            if missing:
                raise KeyError(f"{len(missing)} image ids of {split}.txt have no row in the image-level labels (first: {missing[0]})")
            bad = [str(n) for n in self.name_list if np.asarray(label_list[str(n)]).shape != (self.num_fg,)]
            if bad:
                raise ValueError(f"{bad[0]}: the image-level label row has shape {np.asarray(label_list[bad[0]]).shape}, the vocabulary "
                                 f"has {self.num_fg} foreground classes")

    def __len__(self):
        return len(self.name_list)

    def __getitem__(self, idx):
        name = str(self.name_list[idx])
        image = _imread(os.path.join(self.img_dir, name + ".jpg"))
        if image.ndim == 2:
            image = np.stack([image] * 3, -1)
        cls = np.zeros(self.num_fg, np.float32) if self.label_list is None else np.asarray(self.label_list[name], np.float32)
        return name, np.ascontiguousarray(image[..., :3], np.uint8), None, cls

    def max_k(self):
        """The largest number of present classes of any listed image (the pipeline's smax); 1 without image-level labels."""
        if self.label_list is None or not len(self.name_list):
            return 1
        return max(1, max(int((np.asarray(self.label_list[str(n)]) != 0).sum()) for n in self.name_list))
