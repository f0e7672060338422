"""float64 numpy restatement of the two-threshold pseudo labels (include/excel_hip.h, "confident labels"; utils/affutils.py:101-158
with utils/PAR.py:26-92 between its two ends).  Everything, the source coordinates of the resizes included, is computed in float64;
tests/test_host_conf_labels.py pins it to tests/golden/conf_labels.npz (the reference's own float32 planes and float64 labels)."""
import numpy as np

DILATIONS = (1, 2, 4, 8, 12, 24)
# utils/PAR.py:13-21 get_kernel: the eight neighbours as (dy, dx), in tap order
NEIGHBOURS = ((-1, -1), (-1, 0), (-1, 1), (0, -1), (0, 1), (1, -1), (1, 0), (1, 1))


def _taps(out_size, in_size):
    """F.interpolate(bilinear, align_corners=False): (i0, i1, weight of i1) per output index."""
    src = np.maximum((in_size / out_size) * (np.arange(out_size, dtype=np.float64) + 0.5) - 0.5, 0.0)
    i0 = np.minimum(np.floor(src).astype(np.int64), in_size - 1)
    return i0, np.minimum(i0 + 1, in_size - 1), src - i0


def resize_planes(x, H, W):
    """x [..., h, w] -> [..., H, W] float64"""
    x = np.asarray(x, np.float64)
    y0, y1, ly = _taps(H, x.shape[-2])
    x0, x1, lx = _taps(W, x.shape[-1])
    r0, r1 = x[..., y0, :], x[..., y1, :]
    top = (1 - lx) * r0[..., :, x0] + lx * r0[..., :, x1]
    bot = (1 - lx) * r1[..., :, x0] + lx * r1[..., :, x1]
    return (1 - ly)[:, None] * top + ly[:, None] * bot


def softmax0(x):
    e = np.exp(x - x.max(0, keepdims=True))
    return e / e.sum(0, keepdims=True)


def conf_planes_ref(cams, high_thre, low_thre, down_scale=2):
    """cams [k, h, w] (the present classes) -> (softmax([high, m_1..m_k]), softmax([low, m_1..m_k])), each [k+1, h//ds, w//ds]"""
    k, h, w = cams.shape
    m = resize_planes(cams, h // down_scale, w // down_scale)
    bkg = np.ones((1,) + m.shape[1:])
    return softmax0(np.concatenate([bkg * high_thre, m], 0)), softmax0(np.concatenate([bkg * low_thre, m], 0))


def _neighbours(x, dilations):
    """x [C, H, W] -> [C, 8 * ndil, H, W], replicate padding (utils/PAR.py:38-48)"""
    C, H, W = x.shape
    out = []
    for d in dilations:
        p = np.pad(x, ((0, 0), (d, d), (d, d)), mode="edge")
        for dy, dx in NEIGHBOURS:
            out.append(p[:, d + dy * d:d + dy * d + H, d + dx * d:d + dx * d + W])
    return np.stack(out, 1)


def par_ref(guide, masks, dilations=DILATIONS, num_iter=10, w1=0.3, w2=0.01):
    """utils/PAR.py:64-92 with the guide already at the mask size: guide [3, H, W], masks [C, H, W] -> [C, H, W] float64"""
    guide, masks = np.asarray(guide, np.float64), np.asarray(masks, np.float64)
    nb = _neighbours(guide, dilations)                                                  # [3, T, H, W]
    std = nb.std(1, ddof=1, keepdims=True)
    aff = -((np.abs(nb - guide[:, None]) / (std + 1e-8) / w1) ** 2)
    aff = aff.mean(0)                                                                   # [T, H, W]
    # the reference keeps its distances in a float32 tensor (:50-62): sqrt(2) as float32
    r2 = float(np.float32(np.sqrt(2)))
    pos = np.array([d * (r2 if dy and dx else 1.0) for d in dilations for dy, dx in NEIGHBOURS], np.float64)
    pos_aff = -((pos / (pos.std(ddof=1) + 1e-8) / w1) ** 2)
    wgt = softmax0(aff) + w2 * softmax0(pos_aff)[:, None, None]
    for _ in range(num_iter):
        masks = (_neighbours(masks, dilations) * wgt[None]).sum(1)
    return masks


def merge_ref(par_h, par_l, keys, hw, ignore_index=255, img_box=None):
    """par_h / par_l [k+1, hh, wh] -> labels [h, w] int64: per pass resize + arg-max + keys (:94-96), the merge (:154-156), the box (:146-149);
    keys = [0, c_1 + 1, ..., c_k + 1]"""
    keys = np.asarray(keys, np.int64)
    lab_h = keys[resize_planes(par_h, *hw).argmax(0)]
    lab_l = keys[resize_planes(par_l, *hw).argmax(0)]
    lab = lab_h.copy()
    lab[lab_h == 0] = ignore_index
    lab[(lab_h == 0) & (lab_l == 0)] = 0
    if img_box is not None:
        y0, y1, x0, x1 = (int(v) for v in img_box)
        boxed = np.full_like(lab, ignore_index)
        boxed[y0:y1, x0:x1] = lab[y0:y1, x0:x1]
        lab = boxed
    return lab


def conf_labels_ref(image, cams, cls_onehot, high_thre, low_thre, ignore_index=255, img_box=None, down_scale=2, num_iter=10):
    """One image of refine_cams_with_bkg_v2 in float64: image [3, h, w], cams [F, h, w], cls_onehot [F]
    -> (labels [h, w], planes_h, planes_l, par_h, par_l)"""
    present = np.flatnonzero(np.asarray(cls_onehot) != 0)
    h, w = cams.shape[-2:]
    ph, pl = conf_planes_ref(np.asarray(cams, np.float64)[present], high_thre, low_thre, down_scale)
    guide = resize_planes(image, h // down_scale, w // down_scale)
    qh, ql = par_ref(guide, ph, num_iter=num_iter), par_ref(guide, pl, num_iter=num_iter)
    keys = np.concatenate([[0], present + 1])
    return merge_ref(qh, ql, keys, (h, w), ignore_index, img_box), ph, pl, qh, ql
