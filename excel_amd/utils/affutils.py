"""Mirror of the hot functions of utils/affutils.py over the HIP kernels.

  compute_trans_mat            :8-24
  refine_cams_with_aff         :177-223 (both branches; seg_attn needs per-layer maps: model(img, n_attn_out>=6))
  refine_cams_with_bkg_weclip  :161-174  (+ generate_cam_label/scale_cam_image :55-78, _refine_cams :80-89)
  refine_cams_with_bkg_v2      :101-158  (+ _refine_cams2 :91-98; the twin at utils/camutils.py:264-304)

The reference hops to the host per class (numpy + OpenCV, :207-217, :59-66); here everything stays on the device:
scoremap2bbox (:26-53) runs as one workgroup per (image, class) inside excel_refine_cams_with_aff.
"""
import numpy as np
import torch

from .. import ops
from ..clip.clip import LazyAttnWeights


def compute_trans_mat(attn_weight):
    return ops.compute_trans_mat(attn_weight)


def _w_aff_of(attn_weights, attn_layers):
    if isinstance(attn_weights, LazyAttnWeights):
        if attn_weights.aff_layers != attn_layers:
            raise ValueError("attention mean was reduced over a different number of layers")
        return attn_weights.w_aff
    aw = attn_weights
    if aw.dim() == 3:                  # [L,N,N] of one image, as tools/infer_lam.py:90 passes it
        aw = aw[:, None]
    return ops.attn_layer_mean(aw, attn_layers)          # mean(attn[-layers:, 1:, 1:])  (:180,:197)


@torch.no_grad()
def refine_cams_with_aff(attr_map, attn_weights, cls_label, size, caa_thre=0.79, attn_layers=6, seg_attn=None):
    """attr_map [P,F], attn_weights [L,N,N] | LazyAttnWeights, cls_label [F] -> (list of k x [g,g], cls_lst cpu int64)."""
    h, w = size
    g = h // 16
    if seg_attn is not None:                                                                  # :182-195
        stacked = attn_weights.stacked if isinstance(attn_weights, LazyAttnWeights) else attn_weights
        if stacked is None or stacked.shape[0] < attn_layers:
            raise ValueError("the seg_attn branch needs the per-layer attention maps: call model(img, n_attn_out=%d)" % attn_layers)
        if stacked.dim() == 3:
            stacked = stacked[:, None]
        w_aff = ops.attn_select_mean(stacked[:, :1].contiguous(), seg_attn.reshape(1, g * (w // 16), -1), attn_layers)
    else:
        w_aff = _w_aff_of(attn_weights, attn_layers)
    cls_label = torch.as_tensor(cls_label)
    cls_lst = torch.where(cls_label.detach().cpu() != 0)[0]                                   # :203
    k = int(cls_lst.numel())
    if k == 0:
        return [], cls_lst
    idx, n = ops.cls_compact(cls_label.reshape(1, -1).float().to(attr_map.device), k)
    refined = ops.refine_cams_with_aff_batched(attr_map.reshape(1, g * g, -1), w_aff[:1], idx, n, g, caa_thre)
    return [refined[0, s].reshape(g, w // 16) for s in range(k)], cls_lst


@torch.no_grad()
def refine_cams_with_bkg_weclip(cam_refined_list, inputs_denorm, cls_lst, par, size):
    """-> (cam_labels [1,H,W] int64, cams [k+1,H,W])   (:161-174)"""
    H, W = int(size[0]), int(size[1])
    k = len(cam_refined_list)
    g = cam_refined_list[0].shape[0]
    dev = cam_refined_list[0].device
    refined = torch.stack([c.reshape(-1) for c in cam_refined_list], 0)[None].contiguous()       # [1,k,P]
    ncls = torch.tensor([k], dtype=torch.int32, device=dev)
    cams = ops.cam_upsample_bkg(refined, ncls, g, H, W)                                           # [1,k+1,H,W]
    out = par(inputs_denorm[None].float(), cams)                                                  # _refine_cams :80-84
    idx = torch.as_tensor(np.asarray(cls_lst), dtype=torch.int32).reshape(1, k).to(dev)
    _, lab = ops.argmax_label(out, None, idx, want_i64=True)                                      # :86-87, :168
    return lab, cams[0]


def _pitched(x):
    """[B,K,h,w] -> the flat pitched planes of a uniform ragged plan (rows padded to 4 floats)."""
    w = x.shape[-1]
    return torch.nn.functional.pad(x, (0, -w % 4)).contiguous().view(-1)


@torch.no_grad()
def _bkg_v2(ref_mod, images, cams, cls_labels, high_thre, low_thre, ignore_index, img_box, down_scale):
    """refine_cams_with_bkg_v2's work -> (flat uint8 labels, planes, PAR output, plan, half plan, smax, nchan): the intermediates are
    what the tests compare with the reference's."""
    from ..pipeline import conf_labels_ragged
    B, _, h, w = images.shape
    dev = cams.device
    F_ = cams.shape[1]
    plan = ops.RaggedPlan([(h, w)] * B, dev)
    half = ops.conf_half_plan(plan, down_scale)
    guide = ops.bilinear_resize(images.float(), h // int(down_scale), w // int(down_scale), align_corners=False)    # :113
    onehot = (cls_labels != 0).float().to(dev)
    smax = max(1, int(onehot.sum(1).max().item()))
    idx, ncls, nchan = ops.cls_compact(onehot, smax, want_nchan=True)                               # :139 (valid_key without the background)
    slot = torch.arange(smax, device=dev)[None] < ncls[:, None]
    take = torch.where(slot, idx, torch.zeros_like(idx)).long().clamp_(0, F_ - 1)
    planes = torch.gather(cams.float(), 1, take[:, :, None, None].expand(B, smax, h, w))
    packed = _pitched(torch.cat([torch.zeros_like(planes[:, :1]), planes], 1))                      # plane 0 = background: never read
    box = None if img_box is None else torch.as_tensor(img_box).to(device=dev, dtype=torch.int32).reshape(B, 4).contiguous()
    labels, conf_planes, par_out = conf_labels_ragged(guide, packed, plan, half, smax, nchan, idx, float(high_thre), float(low_thre),
                                                      ref_mod.dilations, ref_mod.num_iter, w1=ref_mod.w1, w2=ref_mod.w2, img_box=box,
                                                      ignore_index=int(ignore_index))
    return labels, conf_planes, par_out, plan, half, smax, nchan


def refine_cams_with_bkg_v2(ref_mod=None, images=None, cams=None, cls_labels=None, high_thre=None, low_thre=None, ignore_index=False,
                            img_box=None, down_scale=2):
    """images [B,3,h,w], cams [B,F,h,w] over the whole class list, cls_labels [B,F] one-hot -> labels [B,h,w] float32 like the
    reference's (:101-158): lab_h where the strict pass (background score high_thre) names a class, 0 where the pass with low_thre
    says background too, ignore_index between, and outside img_box [B,4] = (y0, y1, x0, x1).  `ref_mod` = the project's PAR object
    (its num_iter, dilations and weights are used).  The two PAR passes of an image run as one over 2 (k + 1) planes at
    (h // down_scale, w // down_scale); the guide is the image halved with align_corners=False (:113), handed to PAR at the mask
    size, where PAR's own resize is the identity.  Compacting the present classes goes through torch gathers: not a hot path."""
    labels = _bkg_v2(ref_mod, images, cams, cls_labels, high_thre, low_thre, ignore_index, img_box, down_scale)[0]
    return labels.view(images.shape[0], images.shape[2], images.shape[3]).float()


@torch.no_grad()
def conf_labels_image(par, image, cams, cls_lst, high_thre, low_thre, ignore_index=255, down_scale=2):
    """The confident labels of ONE image the way the batched step computes them (pipeline.conf_labels_ragged over a plan of one
    image): image [3,S,S] = the network input PAR reads, cams [k+1,H,W] = refine_cams_with_bkg_weclip's second result (plane 0
    is not read), cls_lst = its class list.  -> uint8 [H,W]."""
    from ..pipeline import conf_labels_ragged
    k, (H, W) = cams.shape[0] - 1, cams.shape[-2:]
    dev = cams.device
    plan = ops.RaggedPlan([(int(H), int(W))], dev)
    half = ops.conf_half_plan(plan, down_scale)
    idx = torch.as_tensor(np.asarray(cls_lst), dtype=torch.int32).reshape(1, k).to(dev)
    nchan = torch.tensor([k + 1], dtype=torch.int32, device=dev)
    labels, _, _ = conf_labels_ragged(image[None].float(), _pitched(cams[None].float()), plan, half, k, nchan, idx, float(high_thre),
                                      float(low_thre), par.dilations, par.num_iter, w1=par.w1, w2=par.w2, ignore_index=int(ignore_index))
    return labels.view(int(H), int(W))
