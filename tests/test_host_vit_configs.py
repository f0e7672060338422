"""The ViT geometry sweep's own tools (tests/_vit_configs.py over tests/_attn_shapes.py), on the oracle alone - no GPU.

First: the generalised helpers with a cfg other than TINY give, on the fp32 oracle against the float64 oracle, the regime the GPU sweep
relies on at h1 (1 head), h3 (3 heads) and p32 (patch 32): the flat net holds pmin N / rowsum between the gate's 0.3 and 0.82, the fp32
oracle deviates from float64 by at most 1.2e-7 (attention) and 7.5e-7 (x_raw, feats), and 4 o <= pmin / 4 holds with three orders to spare.

Second: the gates notice, at these geometries, the mistakes the sweep is there to find.  A float64 forward is corrupted three ways -
  one head's contribution is dropped from the head-summed attention of a surgery layer (a phase lost from a sweep over H heads),
  the im2col column order is swapped in px and py,
  one token's LayerNorm statistics are taken over the first D / 2 columns only (lanes that never entered ln_row's loop),
- and each must fail the numerics gate in every mode (and the head drop the masking gate) while the clean fp32 oracle passes both."""
import numpy as np
import pytest

import _attn_shapes as A
import _vit_configs as V

vit = A.oracle.vit
IDS = ("h1", "h3", "p32")
MODES = ("f32", "f16x3", "bf16x3")


@pytest.fixture(scope="module")
def refs():
    return {(cid, net): V.reference(V.CASES[cid], net) for cid in IDS for net in ("flat", "peaked")}


def forward64(case, net):
    """A float64 forward of the case's net as errors() wants it (whatever oracle.vit functions are patched at the moment)."""
    w = {k: np.asarray(v, np.float64) for k, v in V.weights(case, net).items()}
    imgs = A.images(case.g, V.B, case.cfg.patch).astype(np.float64)
    with vit.precision(np.float64):
        x, attn, feats = vit.vit_forward(imgs, w, case.cfg)
    assert x.dtype == np.float64
    return A.pack(x, attn, feats, V.aff_layers(case.cfg)), w


@pytest.mark.parametrize("cid", IDS)
def test_precondition_numbers_at_other_geometries(refs, cid):
    case = V.CASES[cid]
    cfg, N = case.cfg, case.g * case.g + 1
    ref, o, pmin = refs[cid, "flat"]
    assert len(pmin) == cfg.layers and ref["attn"].shape == (cfg.layers, V.B, N, N) and ref["feats"].shape == (cfg.layers, V.B, N, cfg.width)
    assert ref["x_raw"].shape == (V.B, N, cfg.out_dim) and ref["w_aff"].shape == (V.B, N - 1, N - 1)
    assert not A.masking_precondition(o, pmin, N, cfg), A.masking_precondition(o, pmin, N, cfg)
    for l, p in enumerate(pmin):
        share = p * N / A.layer_rowsum(l, cfg)
        assert 0.3 <= share <= 0.82, (l, share)
        assert o[f"attn{l}"] <= 1.2e-7 and o[f"feats{l}"] <= 7.5e-7, (l, o[f"attn{l}"], o[f"feats{l}"])
        assert 4e3 * o[f"attn{l}"] <= p / 4 and 4e3 * o[f"rowsum{l}"] <= p / 4, (l, o[f"attn{l}"], o[f"rowsum{l}"], p)
    assert o["x_raw"] <= 7.5e-7, o["x_raw"]
    # the rows of a surgery layer sum to the head count, those of a plain layer to 1: layer_rowsum follows cfg, not TINY
    for l in range(cfg.layers):
        assert np.allclose(ref["attn"][l].sum(-1), A.layer_rowsum(l, cfg), rtol=0, atol=1e-12)
    assert np.array_equal(ref["w_aff"], ref["attn"][-V.aff_layers(cfg):, :, 1:, 1:].mean(0))


def gates(case, out, ref, o, pmin, net):
    """-> (numerics failures per mode, masking failures (flat net only))"""
    err = A.errors(out, ref)
    return {m: A.numerics_failures(err, o, m, case.cfg) for m in MODES}, (A.masking_failures(err, pmin) if net == "flat" else [])


@pytest.mark.parametrize("net", ["flat", "peaked"])
@pytest.mark.parametrize("cid", IDS)
def test_gates_accept_the_fp32_oracle_and_reject_three_corruptions(refs, monkeypatch, cid, net):
    case = V.CASES[cid]
    cfg = case.cfg
    ref, o, pmin = refs[cid, net]
    x32, a32, f32 = vit.vit_forward(A.images(case.g, V.B, cfg.patch), V.weights(case, net), cfg)
    num, mask = gates(case, A.pack(x32, a32, f32, V.aff_layers(cfg)), ref, o, pmin, net)
    assert not mask and not any(num.values()), (num, mask)
    # the uncorrupted float64 forward is the reference itself (the patches below are the only difference)
    same, _ = forward64(case, net)
    assert all(np.array_equal(same[k], ref[k]) for k in ref)

    # 1. one head's probabilities missing from the head sum of every surgery layer's reported attention
    orig_surgery = vit.surgery_attention

    def one_head_dropped(y, p, w, cfg_, ex_attn=None):
        x, x_ori, a = orig_surgery(y, p, w, cfg_, ex_attn)
        q, k, _ = vit._qkv(y, p, w, cfg_.heads)
        return x, x_ori, a - vit.softmax((q[-1] @ k[-1].T) * vit.F32(cfg_.head_dim ** -0.5))

    with monkeypatch.context() as m:
        m.setattr(vit, "surgery_attention", one_head_dropped)
        out, _ = forward64(case, net)
    num, mask = gates(case, out, ref, o, pmin, net)
    first = cfg.layers - cfg.n_surgery
    for mode in MODES:
        assert any(s.startswith(f"attn{first}:") for s in num[mode]) and any(s.startswith("w_aff:") for s in num[mode]), (mode, num[mode])
    if net == "flat":
        assert any(s.startswith(f"rowsum{cfg.layers - 1}:") for s in mask), mask
    assert np.array_equal(out["x_raw"], ref["x_raw"])                 # (only the reported weights: x_raw cannot see it)

    # 2. im2col columns ordered (c, px, py) where conv1's weight has (c, py, px)
    def patch_embed_swapped(img, w, cfg_):
        ps = cfg_.patch
        C, S, _ = img.shape
        g = S // ps
        patches = img.reshape(C, g, ps, g, ps).transpose(1, 3, 0, 4, 2).reshape(g * g, C * ps * ps)
        return (patches @ w["conv1.weight"].reshape(cfg_.width, -1).T).astype(vit.F32)

    with monkeypatch.context() as m:
        m.setattr(vit, "patch_embed", patch_embed_swapped)
        out, _ = forward64(case, net)
    num, _ = gates(case, out, ref, o, pmin, net)
    for mode in MODES:
        assert any(s.startswith("x_raw:") for s in num[mode]) and any(s.startswith("feats0:") for s in num[mode]), (mode, num[mode])

    # 3. token 1's LayerNorm statistics over the first D / 2 columns, in ONE LayerNorm of the forward: ln_pre (everything downstream
    # moves), the first block's ln_1, and ln_post (one token of x_raw is all that moves)
    orig_ln = vit.layer_norm
    for name, seen in (("ln_pre.weight", "feats0:"), ("transformer.resblocks.0.ln_1.weight", "feats0:"), ("ln_post.weight", "x_raw:")):
        target = []

        def ln_half_row(x, w, b, eps=1e-5):
            y = orig_ln(x, w, b, eps)
            if target and w is target[0]:
                h = x[1, :x.shape[1] // 2]
                mu = h.mean()
                y[1] = (x[1] - mu) / np.sqrt(((h - mu) ** 2).mean() + eps) * w + b
            return y

        with monkeypatch.context() as m:
            m.setattr(vit, "layer_norm", ln_half_row)
            w64 = {k: np.asarray(v, np.float64) for k, v in V.weights(case, net).items()}
            target.append(w64[name])
            with vit.precision(np.float64):
                x, attn, feats = vit.vit_forward(A.images(case.g, V.B, cfg.patch).astype(np.float64), w64, cfg)
        num, _ = gates(case, A.pack(x, attn, feats, V.aff_layers(cfg)), ref, o, pmin, net)
        for mode in MODES:
            assert any(s.startswith(seen) for s in num[mode]), (name, mode, num[mode])
