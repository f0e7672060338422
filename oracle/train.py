"""One training iteration of the decoder head restated in torch CPU float64 with autograd (oracle; test infrastructure only).

The numpy twin of the forward is oracle/decoder.py; this module adds what training needs on top of it, in double precision so that
the HIP kernels' fp32 results can be checked against it at the production shapes:

  SegFormerHead.forward        model/segformer_head.py:66-77   (MLP :22-27: Linear, ReLU, Linear per ViT layer; channel concat :73;
                                                                 1x1 linear_fuse :74; Dropout2d :75 with an explicit keep mask)
  attn_pred                    model/model_excel.py:70-76      (from the post-dropout fts: F.normalize over channels, bmm, the GLOBAL
                                                                 torch.mean over all B*P*P entries, sigmoid((x - mean) * 3))
  DecoderTransformer.forward   model/decoder/TransDecoder.py:81-84, :114-124 (pre-LN MHA + QuickGELU MLP per block, 1x1 linear_pred)
  seg_loss                     scripts/train_voc.py:202-203    (F.interpolate bilinear, align_corners=False; model/losses.py:4-18)
  aff_mask                     utils/camutils.py:438-476       (cams_to_affinity_label with nearest down-sampling, get_mask_by_radius)
  diver_loss                   model/losses.py:20-31           (get_aff_loss with its +1 counts), loss = w_seg*seg + w_diver*diver :215

Weights are dicts keyed like the reference modules' state_dict, prefixed "fuse." / "dec." (as in oracle/decoder.py), with the
reference shapes (1x1 convolutions [out, in, 1, 1]).  Inputs are taken as given (fp32 values are widened, not re-rounded).
"""
import numpy as np
import torch
import torch.nn.functional as F

F64 = torch.float64


def _d(a):
    return torch.as_tensor(np.ascontiguousarray(np.asarray(a))).to(F64)


def mask_by_radius(g, radius):
    """get_mask_by_radius(g, g, radius) (utils/camutils.py:459-476) as bool [P,P]: token pairs whose rows and columns both lie
    within `radius` (the reference's window is symmetric, so mask[i, j] = mask[j, i])."""
    r, c = np.divmod(np.arange(g * g), g)
    return torch.from_numpy((np.abs(r[:, None] - r[None, :]) <= radius) & (np.abs(c[:, None] - c[None, :]) <= radius))


def affinity_label(labels, g, radius, ignore_index=255):
    """cams_to_affinity_label(labels, mask=get_mask_by_radius(g, g, radius)) (utils/camutils.py:438-456) -> int64 [B,P,P]:
    1 same class, 0 different class, ignore_index outside the window or where either token is ignored.  labels [B,H,W] are
    nearest-down-sampled to the g x g token grid (:442; the reference's h//16 is g at its patch size)."""
    lab = torch.as_tensor(np.asarray(labels)).to(torch.float32)
    B = lab.shape[0]
    small = F.interpolate(lab[:, None], size=[g, g], mode="nearest").reshape(B, -1)        # :442-444
    aff = (small[:, None, :] == small[:, :, None]).long()                                    # :445-447
    aff[:, ~mask_by_radius(g, radius)] = ignore_index                                        # :451
    ign = small == ignore_index
    for b in range(B):                                                                       # :453-454
        aff[b, :, ign[b]] = ignore_index
        aff[b, ign[b], :] = ignore_index
    return aff


def seg_loss(pred, label, ignore_index=255):
    """get_seg_loss (model/losses.py:4-18): per-pixel cross entropy, background and foreground sums each over (count + 1e-6)."""
    ce = lambda t: F.cross_entropy(pred, t, ignore_index=ignore_index, reduction="none").sum()
    bg = label.clone()
    bg[label != 0] = ignore_index
    fg = label.clone()
    fg[label == 0] = ignore_index
    bg_n = (bg != ignore_index).sum().to(F64)
    fg_n = (fg != ignore_index).sum().to(F64)
    return (ce(bg) / (bg_n + 1e-6) + ce(fg) / (fg_n + 1e-6)) * 0.5


def aff_loss(inputs, targets):
    """get_aff_loss (model/losses.py:20-31) -> (loss, pos_count, neg_count); the counts include the reference's +1."""
    pos = (targets == 1).to(F64)
    neg = (targets == 0).to(F64)
    pc, nc = pos.sum() + 1, neg.sum() + 1
    return 0.5 * torch.sum(pos * (1 - inputs)) / pc + 0.5 * torch.sum(neg * inputs) / nc, int(pc), int(nc)


def train_losses(seg, attn_pred, pseudo, radius, w_seg=1.0, w_diver=0.1, ignore_index=255, aff_labels=None):
    """scripts/train_voc.py:202-215 on float64 tensors seg [B,nc,g,g] and attn_pred [B,P,P] -> (loss, seg_loss, diver_loss, aff_mask,
    pos_count, neg_count).  aff_labels: the map the affinity target comes from (default the pseudo labels; :210 later uses the seg
    arg-max)."""
    g = seg.shape[-1]
    pseudo = torch.as_tensor(np.asarray(pseudo)).long()
    up = F.interpolate(seg, size=tuple(pseudo.shape[-2:]), mode="bilinear", align_corners=False)            # :202
    sl = seg_loss(up, pseudo, ignore_index)                                                                  # :203
    aff = affinity_label(pseudo if aff_labels is None else aff_labels, g, radius, ignore_index)              # :207-210
    dl, pc, nc = aff_loss(attn_pred, aff)                                                                    # :212
    return w_seg * sl + w_diver * dl, sl, dl, aff, pc, nc                                                   # :215


def losses_and_grads(seg, attn_pred, pseudo, radius, **kw):
    """train_losses on leaf copies of seg / attn_pred -> dict(seg_loss, diver_loss, aff_mask, pos_count, neg_count, d_seg, d_attn_pred)."""
    s, a = _d(seg).requires_grad_(), _d(attn_pred).requires_grad_()
    loss, sl, dl, aff, pc, nc = train_losses(s, a, pseudo, radius, **kw)
    loss.backward()
    return dict(seg_loss=float(sl.detach()), diver_loss=float(dl.detach()), aff_mask=aff.numpy(), pos_count=pc, neg_count=nc, d_seg=s.grad.numpy(),
                d_attn_pred=a.grad.numpy())


def _ln(x, w, b):
    return F.layer_norm(x, (x.shape[-1],), w, b, 1e-5)


def head_forward(all_feats, w, heads, keep=None, dropout_p=0.0, attn_mean="global"):
    """all_feats [L,B,N,D] (float64) -> (fts [B,P,E] after Dropout2d, seg [B,nc,g,g], attn_pred [B,P,P]).
    keep: [B,E] 0/1 Dropout2d mask (kept channels are scaled by 1/(1-dropout_p)); None = no dropout.
    attn_mean: "global" (the reference) or "per_image" (a deliberate mistake, for negative controls only)."""
    L, B, N, D = all_feats.shape
    g = int(round((N - 1) ** 0.5))
    P = g * g
    tok = all_feats[:, :, 1:, :]                                                             # model_excel.py:64-66
    outs = []
    for l in range(L):                                                                       # segformer_head.py:68-72
        p = f"fuse.linears_modulelist.{l}."
        h = F.relu(F.linear(tok[l], w[p + "proj.weight"], w[p + "proj.bias"]))              # :24-25
        outs.append(F.linear(h, w[p + "proj_2.weight"], w[p + "proj_2.bias"]))              # :26
    cat = torch.cat(outs, -1)                                                                # :73 channel concat, layer-major
    Wf = w["fuse.linear_fuse.weight"]
    fts = F.linear(cat, Wf.reshape(Wf.shape[0], -1), w["fuse.linear_fuse.bias"])             # :74 1x1 conv
    if keep is not None:                                                                     # :75 Dropout2d: whole (image, channel) planes
        fts = fts * (_d(keep)[:, None, :] / (1.0 - dropout_p))
    E = fts.shape[-1]
    fl = F.normalize(fts.transpose(1, 2), dim=1)                                             # model_excel.py:72-73 [B,E,P]
    sim = fl.transpose(2, 1).bmm(fl)                                                         # :74
    mean = sim.mean() if attn_mean == "global" else sim.mean(dim=(1, 2), keepdim=True)
    attn_pred = torch.sigmoid((sim - mean * 1.0) * 3.0)                                      # :75-76
    x = fts
    hd = E // heads
    layer = 0
    while f"dec.transformer.resblocks.{layer}.ln_1.weight" in w:                             # TransDecoder.py:81-84
        p = f"dec.transformer.resblocks.{layer}."
        y = _ln(x, w[p + "ln_1.weight"], w[p + "ln_1.bias"])
        qkv = F.linear(y, w[p + "attn.in_proj_weight"], w[p + "attn.in_proj_bias"])
        q, k, v = (qkv[..., i * E:(i + 1) * E].reshape(B, P, heads, hd).transpose(1, 2) for i in range(3))
        a = torch.softmax((q * hd ** -0.5) @ k.transpose(-1, -2), dim=-1)
        o = (a @ v).transpose(1, 2).reshape(B, P, E)
        x = x + F.linear(o, w[p + "attn.out_proj.weight"], w[p + "attn.out_proj.bias"])
        z = F.linear(_ln(x, w[p + "ln_2.weight"], w[p + "ln_2.bias"]), w[p + "mlp.c_fc.weight"], w[p + "mlp.c_fc.bias"])
        x = x + F.linear(z * torch.sigmoid(1.702 * z), w[p + "mlp.c_proj.weight"], w[p + "mlp.c_proj.bias"])   # QuickGELU :58-60
        layer += 1
    Wp = w["dec.linear_pred.weight"]
    seg = F.linear(x, Wp.reshape(Wp.shape[0], -1), w["dec.linear_pred.bias"])                # :122 1x1 conv
    return fts, seg.transpose(1, 2).reshape(B, -1, g, g), attn_pred


def train_iteration(all_feats, weights, pseudo, heads, radius, w_seg=1.0, w_diver=0.1, ignore_index=255, aff_labels=None, keep=None,
                    dropout_p=0.0, attn_mean="global"):
    """scripts/train_voc.py:186-215 for the head alone, float64 autograd -> dict of numpy float64 arrays:
    seg, attn_pred, fts (post-dropout, [B,E,g,g]), seg_loss, diver_loss, aff_mask, pos_count, neg_count, d_seg, d_attn_pred, d_fts and
    grads {state_dict key: d loss / d parameter} for every key of `weights`."""
    params = {k: _d(v).requires_grad_() for k, v in weights.items()}
    fts, seg, ap = head_forward(_d(all_feats), params, heads, keep, dropout_p, attn_mean)
    for t in (fts, seg, ap):
        t.retain_grad()
    loss, sl, dl, aff, pc, nc = train_losses(seg, ap, pseudo, radius, w_seg, w_diver, ignore_index, aff_labels)
    loss.backward()
    B, P, E = fts.shape
    g = seg.shape[-1]
    chw = lambda t: t.detach().transpose(1, 2).reshape(B, E, g, g).numpy()
    return dict(seg=seg.detach().numpy(), attn_pred=ap.detach().numpy(), fts=chw(fts), seg_loss=float(sl.detach()), diver_loss=float(dl.detach()),
                aff_mask=aff.numpy(), pos_count=pc, neg_count=nc, d_seg=seg.grad.numpy(), d_attn_pred=ap.grad.numpy(), d_fts=chw(fts.grad),
                grads={k: v.grad.numpy() for k, v in params.items()})
