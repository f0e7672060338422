"""Pillow + numpy restatement of CocoClsDataset(aug=True)'s transform (datasets/coco.py:112-142 over datasets/transforms.py) with the
random draws passed in: the yardstick ops.train_augment_image is compared against.  Test helper only: the package never imports it."""
import numpy as np
from PIL import Image

MEAN = (123.675, 116.28, 103.53)
STD = (58.395, 57.12, 57.375)


def transform(image, p, S):
    """-> dict(crop_u8 [S,S,3] uint8 (before normalisation), img_ref [3,S,S] f32 (the reference's float32 normalize_img), img_box [4]).
    random_scaling (image only, Pillow BILINEAR), random_fliplr, random_crop(label=None, mean_rgb=[0,0,0]): the FIRST crop draw, i.e.
    candidate 0 of the record."""
    h, w, _ = image.shape
    ratio = float(p["ratio"])
    im = np.asarray(Image.fromarray(image.astype(np.uint8)).resize([int(ratio * w), int(ratio * h)], resample=Image.BILINEAR))
    im = im.astype(np.float32)
    if int(p["flip"]):
        im = np.fliplr(im)
    h, w, _ = im.shape
    H, W = max(S, h), max(S, w)
    H_pad, W_pad = int(p["h_pad"]), int(p["w_pad"])
    assert 0 <= H_pad <= H - h and 0 <= W_pad <= W - w
    pad_image = np.zeros((H, W, 3), np.float32)
    pad_image[H_pad:H_pad + h, W_pad:W_pad + w, :] = im
    H_start, W_start = int(p["cand_h"][0]), int(p["cand_w"][0])
    H_end, W_end = H_start + S, W_start + S
    crop = pad_image[H_start:H_end, W_start:W_end, :]
    img_box = np.asarray([max(H_pad - H_start, 0), min(H_end, H_pad + h), max(W_pad - W_start, 0), min(W_end, W_pad + w)], np.int16)
    proc = np.empty_like(crop, np.float32)                     # normalize_img (transforms.py:7-14)
    for c in range(3):
        proc[..., c] = (crop[..., c] - MEAN[c]) / STD[c]
    return dict(crop_u8=crop.astype(np.uint8), img_ref=np.ascontiguousarray(proc.transpose(2, 0, 1)), img_box=img_box, rescaled=(h, w))


def params(rng, hw, S, ratios=None, flips=None, distinct=False):
    """Records with the reference's distributions; ratios / flips override per image (None: drawn).  distinct=False: one crop origin in
    every slot (CocoClsDataset's records); True: 10 independent origins (only slot 0 matters to the image-only transform)."""
    from excel_amd import ops
    out = np.zeros(len(hw), ops.aug_params_dtype())
    for b, (h, w) in enumerate(hw):
        r = rng.uniform(0.5, 2.0) if ratios is None or ratios[b] is None else ratios[b]
        h2, w2 = int(r * h), int(r * w)
        H, W = max(S, h2), max(S, w2)
        out[b]["ratio"] = r
        out[b]["flip"] = int(rng.random() > 0.5) if flips is None else flips[b]
        out[b]["h_pad"] = rng.integers(H - h2 + 1)
        out[b]["w_pad"] = rng.integers(W - w2 + 1)
        n = 10 if distinct else 1
        out[b]["cand_h"] = rng.integers(0, H - S + 1, n)
        out[b]["cand_w"] = rng.integers(0, W - S + 1, n)
    return out
