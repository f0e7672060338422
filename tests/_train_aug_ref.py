"""Pillow + numpy restatement of VOC12ClsDataset(aug=True)'s transform (datasets/voc.py:110-117 over datasets/transforms.py) with the
random draws passed in: the yardstick ops.train_augment is compared against.  Test helper only: the package never imports it."""
import numpy as np
from PIL import Image

MEAN = (123.675, 116.28, 103.53)
STD = (58.395, 57.12, 57.375)


def make_params(B):
    from excel_amd import ops
    return np.zeros(B, ops.aug_params_dtype())


def rescale(image, label, ratio):
    """_img_rescaling (transforms.py:32-50): Pillow BILINEAR for the image, NEAREST for the label, size (int(r w), int(r h))."""
    h, w, _ = image.shape
    new_scale = [int(ratio * w), int(ratio * h)]
    im = np.asarray(Image.fromarray(image.astype(np.uint8)).resize(new_scale, resample=Image.BILINEAR))
    lab = np.asarray(Image.fromarray(label).resize(new_scale, resample=Image.NEAREST))
    return im, lab


def choose_window(label, H, W, S, cand_h, cand_w, ignore_index=255, cat_max_ratio=0.75):
    """get_random_cropbox (transforms.py:141-159) over the given candidate origins; slices the UNPADDED label like the reference."""
    for i in range(10):
        H_start, W_start = int(cand_h[i]), int(cand_w[i])
        temp_label = label[H_start:H_start + S, W_start:W_start + S]
        index, cnt = np.unique(temp_label, return_counts=True)
        cnt = cnt[index != ignore_index]
        if len(cnt > 1) and np.max(cnt) / np.sum(cnt) < cat_max_ratio:
            break
    return H_start, W_start, i


def transform(image, label, p, S, ignore_index=255):
    """-> dict(crop_u8 [S,S,3] uint8 (before normalisation), img_ref [3,S,S] f32 (the reference's float32 normalize_img),
    label [S,S] uint8, img_box [4], window (H_start, W_start), cand (index of the chosen candidate))."""
    im, lab = rescale(image, label, float(p["ratio"]))
    if int(p["flip"]):
        im, lab = np.fliplr(im), np.fliplr(lab)
    h, w, _ = im.shape
    H, W = max(S, h), max(S, w)
    H_pad, W_pad = int(p["h_pad"]), int(p["w_pad"])
    assert 0 <= H_pad <= H - h and 0 <= W_pad <= W - w
    pad_image = np.zeros((H, W, 3), np.float32)
    pad_image[H_pad:H_pad + h, W_pad:W_pad + w, :] = im
    H_start, W_start, cand = choose_window(lab, H, W, S, p["cand_h"], p["cand_w"], ignore_index)
    H_end, W_end = H_start + S, W_start + S
    crop = pad_image[H_start:H_end, W_start:W_end, :]
    img_box = np.asarray([max(H_pad - H_start, 0), min(H_end, H_pad + h), max(W_pad - W_start, 0), min(W_end, W_pad + w)], np.int16)
    pad_label = np.ones((H, W), np.float32) * ignore_index
    pad_label[H_pad:H_pad + h, W_pad:W_pad + w] = lab
    lab_crop = pad_label[H_start:H_end, W_start:W_end]
    proc = np.empty_like(crop, np.float32)                     # normalize_img (transforms.py:7-14)
    for c in range(3):
        proc[..., c] = (crop[..., c] - MEAN[c]) / STD[c]
    return dict(crop_u8=crop.astype(np.uint8), img_ref=np.ascontiguousarray(proc.transpose(2, 0, 1)), label=lab_crop.astype(np.uint8),
                img_box=img_box, window=(H_start, W_start), cand=cand, rescaled=(h, w))


def draw_params(rng, hw, S, rescale_range=(0.5, 2.0)):
    """Random params with the reference's distributions (for tests that do not care about a particular draw)."""
    out = make_params(len(hw))
    for b, (h, w) in enumerate(hw):
        r = rng.uniform(*rescale_range)
        h2, w2 = int(r * h), int(r * w)
        H, W = max(S, h2), max(S, w2)
        out[b]["ratio"] = r
        out[b]["flip"] = int(rng.random() > 0.5)
        out[b]["h_pad"] = rng.integers(H - h2 + 1)
        out[b]["w_pad"] = rng.integers(W - w2 + 1)
        out[b]["cand_h"] = rng.integers(0, H - S + 1, 10)
        out[b]["cand_w"] = rng.integers(0, W - S + 1, 10)
    return out
