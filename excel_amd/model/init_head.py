"""Initial weights of the trainable head (model/model_excel.py:28-30): SegFormerHead(index=12) + DecoderTransformer(layers=3, heads=8)
at the reference modules' own initialisation, so that ExCEL_model(mode="train", decoder_state_dict=...) can start training from
nothing.  torch CPU modules of the same shapes draw the values (torch is plumbing here; nothing runs on them)."""
import torch
from torch import nn


def init_decoder_state_dict(num_classes=21, in_channels=768, embedding_dim=256, crop_size=320, seed=0, index=12, layers=3, heads=8):
    """-> {"decoder_fts_fuse.*", "decoder.*": float32 CPU tensor} with the reference model's state_dict keys and shapes.

      decoder_fts_fuse.linears_modulelist.{l}.proj / proj_2   nn.Linear default init (segformer_head.py:17-18), l < index
      decoder_fts_fuse.linear_fuse                            nn.Conv2d 1x1 default init (:66)
      decoder.transformer.resblocks.{l}.attn                  MultiheadAttention: xavier_uniform in_proj, zero in_proj / out_proj
                                                              biases, nn.Linear default out_proj weight (decoder/myAtt.py:408-418)
      decoder.transformer.resblocks.{l}.ln_1 / ln_2           ones / zeros
      decoder.transformer.resblocks.{l}.mlp.c_fc / c_proj     nn.Linear default init (TransDecoder.py:72-76)
      decoder.linear_pred                                     nn.Conv2d 1x1 default init (:113)

    `index` = number of fused tower layers (12 for ViT-B/16), `in_channels` = the tower's width.  Values are drawn in the
    reference's construction order from torch's generator seeded with `seed` (the global generator is left as it was).
    `crop_size` is accepted for the reference's calling convention but changes nothing: the head holds no size-dependent tensor
    (TransDecoder.py:14's randn / sqrt(d) positional embedding belongs to AttentionPool2d, which DecoderTransformer never builds, and
    the reference's state_dict has no such key)."""
    del crop_size
    with torch.random.fork_rng(devices=[]):
        torch.manual_seed(int(seed))
        fuse = {}
        mods = []
        for l in range(index):
            proj, proj2 = nn.Linear(in_channels, embedding_dim), nn.Linear(embedding_dim, embedding_dim)
            mods.append((f"linears_modulelist.{l}.proj", proj))
            mods.append((f"linears_modulelist.{l}.proj_2", proj2))
        mods.append(("linear_fuse", nn.Conv2d(embedding_dim * index, embedding_dim, kernel_size=1)))
        for name, m in mods:
            fuse[name + ".weight"], fuse[name + ".bias"] = m.weight, m.bias
        dec = {}
        for l in range(layers):
            p = f"transformer.resblocks.{l}."
            attn = nn.MultiheadAttention(embedding_dim, heads)
            ln1 = nn.LayerNorm(embedding_dim)
            c_fc, c_proj = nn.Linear(embedding_dim, embedding_dim * 4), nn.Linear(embedding_dim * 4, embedding_dim)
            ln2 = nn.LayerNorm(embedding_dim)
            dec.update({p + "attn.in_proj_weight": attn.in_proj_weight, p + "attn.in_proj_bias": attn.in_proj_bias,
                        p + "attn.out_proj.weight": attn.out_proj.weight, p + "attn.out_proj.bias": attn.out_proj.bias,
                        p + "ln_1.weight": ln1.weight, p + "ln_1.bias": ln1.bias,
                        p + "mlp.c_fc.weight": c_fc.weight, p + "mlp.c_fc.bias": c_fc.bias,
                        p + "mlp.c_proj.weight": c_proj.weight, p + "mlp.c_proj.bias": c_proj.bias,
                        p + "ln_2.weight": ln2.weight, p + "ln_2.bias": ln2.bias})
        pred = nn.Conv2d(embedding_dim, num_classes, kernel_size=1)
        dec["linear_pred.weight"], dec["linear_pred.bias"] = pred.weight, pred.bias
    out = {"decoder_fts_fuse." + k: v.detach().float().clone() for k, v in fuse.items()}
    out.update({"decoder." + k: v.detach().float().clone() for k, v in dec.items()})
    return out
