"""torch (CPU, float32) + numpy restatement of the training-progress panels (scripts/train_voc.py:233-246 over utils/tbutils.py:28-61,
:88-93) for the train-panel tests: the oracle the kernel of trainviz.hip is held to.

    make_grid          torchvision.utils.make_grid's default layout (padding 2, pad value 0), restated in numpy
    img1               tbutils.denormalize_img: ((x * std_c) + mean_c) * 255 in float32, truncated to uint8
    cam1               F.interpolate(bilinear, align_corners=False) of attr_maps_raw as [B,F,g,g], * cls_label, torch.max over classes,
                       the jet rules of tests/_cam_overlay_ref.py, (jet * 255) * 0.5 + img1 * 0.5 in float64, truncated
    label panels       COLORMAP[label] (the VOC palette, 255 -> (224, 224, 192))
"""
import numpy as np
import torch
import torch.nn.functional as F

from _cam_overlay_ref import jet_rgb

PANELS = ("img1", "cam1", "pseu_aff", "pseu_mid", "seg_gt", "seg_pred")
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)


def colormap():
    """utils/tbutils.py:8-22"""
    cmap = np.zeros((256, 3), np.uint8)
    for i in range(256):
        r = g = b = 0
        c = i
        for j in range(8):
            r |= ((c >> 0) & 1) << (7 - j)
            g |= ((c >> 1) & 1) << (7 - j)
            b |= ((c >> 2) & 1) << (7 - j)
            c >>= 3
        cmap[i] = (r, g, b)
    return cmap


def grid_shape(B, h, w, nrow=2):
    """-> (Hg, Wg, xmaps, ymaps, pad)"""
    if B == 1:
        return h, w, 1, 1, 0
    xmaps = min(nrow, B)
    ymaps = -(-B // xmaps)
    return (h + 2) * ymaps + 2, (w + 2) * xmaps + 2, xmaps, ymaps, 2


def make_grid(imgs, nrow=2):
    """imgs uint8 [B,h,w,3] -> uint8 [Hg,Wg,3]"""
    B, h, w = imgs.shape[:3]
    Hg, Wg, xmaps, _, pad = grid_shape(B, h, w, nrow)
    if B == 1:
        return imgs[0].copy()
    grid = np.zeros((Hg, Wg, 3), np.uint8)
    for k in range(B):
        y, x = (k // xmaps) * (h + 2) + 2, (k % xmaps) * (w + 2) + 2
        grid[y:y + h, x:x + w] = imgs[k]
    return grid


def plan(B, S, g, panels=PANELS, nrow=2):
    """-> ({name: (Hg, Wg, byte offset)}, total bytes): the requested panels tight, in PANELS order"""
    out, off = {}, 0
    for n in PANELS:
        if n in panels:
            h = g if n == "pseu_mid" else S
            Hg, Wg = grid_shape(B, h, h, nrow)[:2]
            out[n] = (Hg, Wg, off)
            off += 3 * Hg * Wg
    return out, off


def img1(inputs):
    """inputs f32 [B,3,S,S] -> uint8 [B,S,S,3]"""
    out = torch.zeros_like(inputs)
    for i in range(3):
        out[:, i] = inputs[:, i] * STD[i] + MEAN[i]
    out = (out * 255).clamp(0, 255).to(torch.uint8)           # in range for every input the tests build: the clamp changes nothing there
    return out.permute(0, 2, 3, 1).contiguous().numpy()


def cam_max(attr, cls_label, S):
    """attr f32 [B,P,F], cls_label f32 [B,F] -> float32 [B,S,S]"""
    B, P, F_ = attr.shape
    g = int(round(P ** 0.5))
    cam = attr.permute(0, 2, 1).reshape(B, F_, g, g)
    cam = F.interpolate(cam, size=(S, S), mode="bilinear", align_corners=False)
    cam = cam * cls_label.unsqueeze(2).unsqueeze(3)
    return torch.max(cam, dim=1)[0].numpy()


def jet_blend(idx_or_cam, img_u8, lut, by_index=False):
    """(jet * 255) * 0.5 + img * 0.5 truncated; by_index: idx_or_cam holds jet indices (0..255) instead of cam values"""
    rgb = lut[idx_or_cam] if by_index else jet_rgb(idx_or_cam, lut)
    return ((rgb * 255) * 0.5 + img_u8.astype(np.float32) * np.float32(0.5)).astype(np.uint8)


def label_rgb(label):
    return colormap()[np.asarray(label).astype(int), :]
