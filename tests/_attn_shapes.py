"""Shared by test_gpu_attn_shapes.py (GPU sweep) and test_host_attn_plan.py (the gates' own sensitivity, on the CPU): the dispatch
arithmetic of the ViT attention as a table, the two test nets with their float64 references, and the comparison functions.  The nets,
references and gates take the ViT as cfg= (default: TINY, what those two files run); tests/_vit_configs.py runs them at other geometries.

Dispatch (attn_plan.hip), for N = g*g + 1 tokens, cdiv(a, b) = ceil(a / b):
    tiles = cdiv(N, 32)                         key tiles of 32 (= KP / 32; also the number of 32-row query strips)
    last  = N - 32 * (tiles - 1)                valid keys in the last tile
    split modes, tiles <= 40: strip kernel, instance ntw = cdiv(tiles, 8), waves nw = cdiv(tiles, ntw),
                              full = tiles - nw * (ntw - 1) waves own ntw tiles, the other nw - full own ntw - 1
    split modes, tiles  > 40: row pass with 4 score types + attn_accum_bf_kernel (attn.hip, one binary per split type)
    f32, whatever N:          attn_rowpass_f32_kernel + attn_accum_kernel (attn_f32.hip, one binary)
"""
import numpy as np

import oracle
from oracle.vit import VitConfig, make_vit_weights

TINY = VitConfig(width=128, layers=8, heads=2, patch=16, out_dim=64, input_resolution=64, n_surgery=5)

# g: (N, tiles, ntw, waves, waves with ntw tiles, valid keys in the last tile); ntw = 0: the two-pass fallback.  Written out by hand from
# the formulae above, not read back from the library.
DISPATCH = {
    1: (2, 1, 1, 1, 1, 2),
    2: (5, 1, 1, 1, 1, 5),
    3: (10, 1, 1, 1, 1, 10),
    4: (17, 1, 1, 1, 1, 17),
    5: (26, 1, 1, 1, 1, 26),
    6: (37, 2, 1, 2, 2, 5),
    7: (50, 2, 1, 2, 2, 18),
    8: (65, 3, 1, 3, 3, 1),
    9: (82, 3, 1, 3, 3, 18),
    10: (101, 4, 1, 4, 4, 5),
    11: (122, 4, 1, 4, 4, 26),
    12: (145, 5, 1, 5, 5, 17),
    13: (170, 6, 1, 6, 6, 10),
    14: (197, 7, 1, 7, 7, 5),
    15: (226, 8, 1, 8, 8, 2),
    16: (257, 9, 2, 5, 4, 1),
    17: (290, 10, 2, 5, 5, 2),
    18: (325, 11, 2, 6, 5, 5),
    19: (362, 12, 2, 6, 6, 10),
    20: (401, 13, 2, 7, 6, 17),
    21: (442, 14, 2, 7, 7, 26),
    22: (485, 16, 2, 8, 8, 5),
    23: (530, 17, 3, 6, 5, 18),
    24: (577, 19, 3, 7, 5, 1),
    25: (626, 20, 3, 7, 6, 18),
    26: (677, 22, 3, 8, 6, 5),
    27: (730, 23, 3, 8, 7, 26),
    28: (785, 25, 4, 7, 4, 17),
    29: (842, 27, 4, 7, 6, 10),
    30: (901, 29, 4, 8, 5, 5),
    31: (962, 31, 4, 8, 7, 2),
    32: (1025, 33, 5, 7, 5, 1),
    33: (1090, 35, 5, 7, 7, 2),
    34: (1157, 37, 5, 8, 5, 5),
    35: (1226, 39, 5, 8, 7, 10),
    36: (1297, 41, 0, 0, 0, 17),
    37: (1370, 43, 0, 0, 0, 26),
    38: (1445, 46, 0, 0, 0, 5),
    39: (1522, 48, 0, 0, 0, 18),
    40: (1601, 51, 0, 0, 0, 1),
    41: (1682, 53, 0, 0, 0, 18),
    42: (1765, 56, 0, 0, 0, 5),
    43: (1850, 58, 0, 0, 0, 26),
    44: (1937, 61, 0, 0, 0, 17),
    45: (2026, 64, 0, 0, 0, 10),
    46: (2117, 67, 0, 0, 0, 5),
    47: (2210, 70, 0, 0, 0, 2),
    48: (2305, 73, 0, 0, 0, 1),
}

NETS = {"flat": 0.25, "peaked": None}       # attn_gain of make_vit_weights(cfg, seed=31): 0.25 = nearly uniform rows, None = the default (4.0)


def net_weights(net, feat_size=None, cfg=TINY):
    gain = NETS[net]
    w = make_vit_weights(cfg, seed=31) if gain is None else make_vit_weights(cfg, seed=31, attn_gain=gain)
    return w if feat_size is None else oracle.vit.reload_self_attn(w, cfg, feat_size=feat_size, mode="train")


def images(g, B, patch=TINY.patch):
    return np.random.RandomState(1000 + g).standard_normal((B, 3, patch * g, patch * g)).astype(np.float32)


def ex_features(g, B, C=24):
    return np.random.RandomState(2000 + g).standard_normal((B, C, g, g)).astype(np.float32)


def layer_rowsum(l, cfg=TINY):
    """Row sum of layer l's attention output: head-MEAN of an nn.MultiheadAttention block, head-SUM of a surgery block."""
    return float(cfg.heads) if l >= cfg.layers - cfg.n_surgery else 1.0


def maxabs(a, b):
    return float(np.max(np.abs(np.asarray(a, np.float64) - np.asarray(b, np.float64))))


def relmax(a, b):
    return maxabs(a, b) / max(float(np.max(np.abs(b))), 1e-30)


def token_normalize(x):
    return x / np.sqrt((x * x).sum(axis=1, keepdims=True))


def errors(out, ref):
    """Every compared quantity of one forward against the float64 reference -> {name: error}.  `out` / `ref`: dicts of attn [L,B,N,N]
    (optional), feats [L,B,N,D] (optional), w_aff [B,P,P] (optional), x_raw, image_features [B,N,C].  Attention: max-abs per layer
    ("attn<l>") and max-abs row-sum error per layer ("rowsum<l>", sums taken in float64); everything else relative to the reference's
    largest magnitude."""
    e = {}
    if out.get("attn") is not None:
        for l in range(ref["attn"].shape[0]):
            a = np.asarray(out["attn"][l], np.float64)
            e[f"attn{l}"] = float(np.abs(a - ref["attn"][l]).max())
            e[f"rowsum{l}"] = float(np.abs(a.sum(-1) - ref["attn"][l].sum(-1)).max())
    if out.get("feats") is not None:
        for l in range(ref["feats"].shape[0]):
            e[f"feats{l}"] = relmax(out["feats"][l], ref["feats"][l])
    for k in ("w_aff", "x_raw", "image_features"):
        if out.get(k) is not None:
            e[k] = relmax(out[k], ref[k])
    return e


def pack(x, attn, feats, aff_layers=6):
    """One oracle forward (vit_forward's x, attn, feats) as the dict errors() compares: w_aff is the mean of the last aff_layers layers."""
    return dict(attn=attn, feats=feats, x_raw=x, image_features=token_normalize(x), w_aff=attn[-aff_layers:, :, 1:, 1:].mean(0))


def reference(net, g, B, ex=False, reload=True, cfg=TINY, aff_layers=6):
    """float64 run of the oracle -> (ref dict, o dict, pmin list): the judge, the fp32 oracle's own deviation from it for every quantity
    of errors(), and every layer's smallest reference probability.  reload=False: the weights keep their native positional grid and the
    oracle resizes it itself, as the library does for a handle used at another size.  cfg: the ViT (its weights come from net_weights(cfg=cfg),
    its inputs are g * cfg.patch pixels wide); aff_layers: how many of the last layers w_aff averages."""
    w = net_weights(net, g if reload else None, cfg)
    imgs = images(g, B, cfg.patch)
    exf = ex_features(g, B) if ex else None

    with oracle.vit.precision(np.float64):
        x, attn, feats = oracle.vit.vit_forward(imgs.astype(np.float64), {k: np.asarray(v, np.float64) for k, v in w.items()}, cfg,
                                                ex_feats=None if exf is None else exf.astype(np.float64))
        assert x.dtype == np.float64 and attn.dtype == np.float64
    ref = pack(x, attn, feats, aff_layers)
    x32, attn32, feats32 = oracle.vit.vit_forward(imgs, w, cfg, ex_feats=exf)
    o = errors(pack(x32, attn32, feats32, aff_layers), ref)
    pmin = [float(attn[l].min()) for l in range(cfg.layers)]
    return ref, o, pmin


# ---------------------------------------------------------------------------------------------------------------- gates
# k: the factors of test_vit_b16_448_clip_like_outlier_net (an fp32-grade mode stays within 3x the fp32 oracle's own deviation from float64,
# bf16x3 within 40x); floors: the suite's tolerances for this net (_check_vit, test_vit_tiny_strip_three_tiles_per_wave_bf16x3)
K_FACTOR = {"f32": 3.0, "f16x3": 3.0, "f16x2": 3.0, "bf16x3": 40.0}


def floor_of(mode, name, cfg=TINY):
    if name.startswith("attn") or name.startswith("rowsum"):
        l = int(name.lstrip("attnrowsum"))
        return (2e-4 if mode == "bf16x3" else 5e-4) * layer_rowsum(l, cfg)
    if mode != "bf16x3":
        return 5e-5
    return 3e-4 if name == "w_aff" else 5e-4


def numerics_failures(err, o, mode, cfg=TINY):
    """Quantities of `err` beyond max(floor, k x the fp32 oracle's own deviation) -> list of messages (empty = accepted).  Row sums are
    left to the masking gate (the floors are per-element tolerances)."""
    bad = []
    for name, e in err.items():
        if name.startswith("rowsum"):
            continue
        bound = max(floor_of(mode, name, cfg), K_FACTOR[mode] * o[name])
        if not e <= bound:
            bad.append(f"{name}: err {e:.3e} > {bound:.3e} (o {o[name]:.3e})")
    return bad


def masking_precondition(o, pmin, N, cfg=TINY):
    """On the reference alone: the flat net is flat (every valid key holds >= 0.3 of a uniform row's share) and the fp32 oracle's own
    noise is at most a quarter of the gate -> list of messages (empty = the regime is there)."""
    bad = []
    for l, p in enumerate(pmin):
        if not p * N / layer_rowsum(l, cfg) >= 0.3:
            bad.append(f"layer {l}: pmin*N/rowsum = {p * N / layer_rowsum(l, cfg):.3f} < 0.3")
        for q in (f"attn{l}", f"rowsum{l}"):
            if not 4 * o[q] <= p / 4:
                bad.append(f"{q}: fp32 oracle deviation {o[q]:.3e} x 4 > pmin/4 = {p / 4:.3e}")
    return bad


def masking_failures(err, pmin):
    """A key that is wrongly admitted or dropped moves one element and its row sum by >= pmin: both must stay within pmin / 4."""
    bad = []
    for l, p in enumerate(pmin):
        for q in (f"attn{l}", f"rowsum{l}"):
            if not err[q] <= p / 4:
                bad.append(f"{q}: err {err[q]:.3e} > pmin/4 = {p / 4:.3e}")
    return bad


def report(tag, err, o, pmin=None, cfg=TINY):
    L = cfg.layers
    worst = lambda d, p: max(d[f"{p}{l}"] for l in range(L)) if f"{p}0" in d else float("nan")
    ratio = lambda q: max((err[k] / max(o[k], 1e-300) for k in err if k.startswith(q)), default=float("nan"))
    line = (f"[attn-shapes] {tag}: attn err {worst(err, 'attn'):.2e} (o {worst(o, 'attn'):.2e}, err/o {ratio('attn'):.1f}) "
            f"rowsum err {worst(err, 'rowsum'):.2e} (o {worst(o, 'rowsum'):.2e}) feats err {worst(err, 'feats'):.2e} (o {worst(o, 'feats'):.2e}, "
            f"err/o {ratio('feats'):.1f})")
    for k in ("w_aff", "x_raw", "image_features"):
        if k in err:
            line += f" {k} err {err[k]:.2e} (o {o[k]:.2e}, err/o {err[k] / max(o[k], 1e-300):.1f})"
    if pmin is not None:
        line += f" pmin {min(pmin):.2e}"
    print(line)
