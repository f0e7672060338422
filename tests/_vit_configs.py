"""Shared by test_gpu_vit_configs.py (GPU sweep) and test_host_vit_configs.py (the gates' own sensitivity, on the CPU): the ViT geometries
excel_vit_create accepts (width = 64 heads, patch % 4 == 0, out_dim % 4 == 0, 0 <= n_surgery <= layers) away from the two the rest of the
suite runs (width 128 / 2 heads and width 768 / 12 heads, both patch 16, out_dim 64 or 512).

Every case: B = 2, square inputs of g * patch pixels, a stored positional grid of 4 x 4 (input_resolution = 4 * patch; reload_self_attn or
the library resizes it to g), w_aff over the last min(6, layers) layers.  Nets, references and gates are those of tests/_attn_shapes.py
with cfg= / aff_layers= set: nothing is restated here.

    id     heads (width)  patch  out_dim  layers / n_surgery  g (N)     what it is there for
    h1      1   (64)       16      64        3 / 2             6 (37)   one head: the strip kernel's second sweep is a single phase; 16 LayerNorm lanes
    h3      3  (192)       16      36        3 / 2             6 (37)   odd head count, D < 256 (48 lanes), out_dim % 32 != 0
    h5p8    5  (320)        8     100        3 / 2             9 (82)   a second ln_row trip on 16 lanes, Kc = 192, 3 key tiles
    h4      4  (256)       16      64        2 / 2             8 (65)   D = 256 exactly; no plain block (first_surgery = 0); 1 key in the last tile
    h16    16 (1024)       16     768        2 / 1             6 (37)   ViT-L width, out_dim > 512 (24 x 32 transpose tiles)
    h20    20 (1280)       16      64        2 / 1             6 (37)   5 ln_row trips (ViT-H width)
    p32     2  (128)       32       4        3 / 3             6 (37)   Kc = 3072 > 4 D: the im2col matrix sizes hbuf; out_dim = 4
    p4      2  (128)        4      64        1 / 0             6 (37)   Kc = 48 (no split-plane mode); one layer; aff_layers == layers == 1
    h12    12  (768)       16     512        2 / 1             9 (82)   the register LayerNorm arm (ln_row_reg<3>) at the same depth, as anchor
"""
import collections

from oracle.vit import VitConfig

import _attn_shapes as A

ALL = ("bf16x3", "f16x3", "f32")
B = 2
POS_GRID = 4

Case = collections.namedtuple("Case", "cfg g modes")


def _cfg(heads, patch, out_dim, layers, n_surgery):
    return VitConfig(width=64 * heads, layers=layers, heads=heads, patch=patch, out_dim=out_dim, input_resolution=POS_GRID * patch,
                     n_surgery=n_surgery)


CASES = {
    "h1": Case(_cfg(1, 16, 64, 3, 2), 6, ALL),
    "h3": Case(_cfg(3, 16, 36, 3, 2), 6, ALL),
    "h5p8": Case(_cfg(5, 8, 100, 3, 2), 9, ALL),
    "h4": Case(_cfg(4, 16, 64, 2, 2), 8, ALL),
    "h16": Case(_cfg(16, 16, 768, 2, 1), 6, ALL),
    "h20": Case(_cfg(20, 16, 64, 2, 1), 6, ("bf16x3", "f32")),
    "p32": Case(_cfg(2, 32, 4, 3, 3), 6, ALL),
    "p4": Case(_cfg(2, 4, 64, 1, 0), 6, ("f32",)),
    "h12": Case(_cfg(12, 16, 512, 2, 1), 9, ("bf16x3", "f32")),
}

# The kernels of attn.hip (row pass with 4 score types + attn_accum_bf_kernel) at H = 3: h3 at g = 36 (N = 1297 = 41 key tiles), one image
TWOPASS = Case(CASES["h3"].cfg, 36, ("bf16x3",))

# The floors of _attn_shapes.floor_of() were set for the width-128 net; every case here passes on them (worst measured err / o on an MI355X,
# both nets, every quantity: bf16x3 25.8 - p32 -, f16x3 3.4 and f32 3.3 - p32 again, errors of 1.5e-6 under the 5e-5 floor), so no case has
# a floor of its own.


def aff_layers(cfg):
    return min(6, cfg.layers)


def reference(case, net, batch=B):
    """_attn_shapes.reference() for one case: through reload_self_attn(feat_size=g, "train") when the net has surgery blocks, else on the
    native 4 x 4 grid (the oracle and the library both resize it)."""
    return A.reference(net, case.g, batch, reload=case.cfg.n_surgery > 0, cfg=case.cfg, aff_layers=aff_layers(case.cfg))


def weights(case, net):
    return A.net_weights(net, case.g if case.cfg.n_surgery > 0 else None, case.cfg)
