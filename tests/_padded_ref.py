"""float64 restatements of the operations of tests/test_gpu_padded_shapes.py, and its seeded inputs (importable without a GPU).

The GPU tests compare the kernels with the project's fp32 numpy oracle at the bounds of the existing tests; these float64 forms are
the yardstick of the yardstick: tests/test_host_padded_shapes.py measures the fp32 oracle against them at the same shapes, so a bound
is known to be a statement about the kernel and not about the reference's own rounding."""
import numpy as np

from _scratch_cases import block_weights, decoder_weights, text_tokens, text_weights  # noqa: F401

F64 = np.float64


def _ln(x, w, b, eps=1e-5):
    mu = x.mean(-1, keepdims=True)
    xc = x - mu
    return xc / np.sqrt((xc * xc).mean(-1, keepdims=True) + eps) * w + b


def _softmax(x):
    e = np.exp(x - x.max(-1, keepdims=True))
    return e / e.sum(-1, keepdims=True)


def _blocks(x, w, prefix, heads, causal):
    B, P, E = x.shape
    hd = E // heads
    mask = np.triu(np.full((P, P), -np.inf), 1) if causal else 0.0
    layer = 0
    while f"{prefix}transformer.resblocks.{layer}.ln_1.weight" in w:
        p = f"{prefix}transformer.resblocks.{layer}."
        g = lambda k: w[p + k].astype(F64)
        qkv = _ln(x, g("ln_1.weight"), g("ln_1.bias")) @ g("attn.in_proj_weight").T + g("attn.in_proj_bias")
        q, k, v = (qkv[..., i * E:(i + 1) * E].reshape(B, P, heads, hd).transpose(0, 2, 1, 3) for i in range(3))
        a = _softmax(q @ k.transpose(0, 1, 3, 2) * hd ** -0.5 + mask)
        x = x + (a @ v).transpose(0, 2, 1, 3).reshape(B, P, E) @ g("attn.out_proj.weight").T + g("attn.out_proj.bias")
        h = _ln(x, g("ln_2.weight"), g("ln_2.bias")) @ g("mlp.c_fc.weight").T + g("mlp.c_fc.bias")
        x = x + (h / (1 + np.exp(-1.702 * h))) @ g("mlp.c_proj.weight").T + g("mlp.c_proj.bias")
        layer += 1
    return x


def decoder_f64(all_feats, w, heads):
    """all_feats [L,B,N,D] -> (fts [B,E,g,g], seg [B,nc,g,g]) in float64 (oracle.decoder.segformer_fuse + decoder_transformer)."""
    L, B, N, D = all_feats.shape
    g_ = int(round((N - 1) ** 0.5))
    tok = all_feats.astype(F64)[:, :, 1:, :]
    outs = []
    for l in range(L):
        p = f"fuse.linears_modulelist.{l}."
        h = np.maximum(tok[l] @ w[p + "proj.weight"].astype(F64).T + w[p + "proj.bias"], 0)
        outs.append(h @ w[p + "proj_2.weight"].astype(F64).T + w[p + "proj_2.bias"])
    Wf = w["fuse.linear_fuse.weight"].astype(F64)
    x = np.concatenate(outs, -1) @ Wf.reshape(Wf.shape[0], -1).T + w["fuse.linear_fuse.bias"]
    fts = x.transpose(0, 2, 1).reshape(B, -1, g_, g_)
    x = _blocks(x, w, "dec.", heads, False)
    Wp = w["dec.linear_pred.weight"].astype(F64)
    seg = x @ Wp.reshape(Wp.shape[0], -1).T + w["dec.linear_pred.bias"]
    return fts, seg.transpose(0, 2, 1).reshape(B, -1, g_, g_)


def text_f64(tokens, w, heads):
    tokens = np.asarray(tokens)
    x = w["token_embedding.weight"].astype(F64)[tokens] + w["positional_embedding"].astype(F64)[None]
    x = _blocks(x, w, "", heads, True)
    x = _ln(x, w["ln_final.weight"].astype(F64), w["ln_final.bias"].astype(F64))
    return x[np.arange(len(tokens)), tokens.argmax(-1)] @ w["text_projection"].astype(F64)


def similarity_f64(feats, beta=1.0, gamma=3.0):
    f = np.asarray(feats, F64)
    f = f.reshape(f.shape[0], f.shape[1], -1)
    f = f / np.maximum(np.sqrt((f * f).sum(1, keepdims=True)), 1e-12)
    sim = np.einsum("bcm,bcn->bmn", f, f)
    return (sim - sim.mean() * beta) * gamma


def affinity_f64(feats, mode):
    z = similarity_f64(feats)
    if mode == "sigmoid":
        return 1 / (1 + np.exp(-z))
    with np.errstate(invalid="ignore"):
        return _softmax(np.where(z < 0, -np.inf, z))           # a row of all -inf: NaN, like torch.softmax


# ------------------------------------------------------------------ seeded inputs
def decoder_case(g, nc):
    rs = np.random.RandomState(100 * g + nc)
    w = decoder_weights(rs, nc=nc)
    return w, rs.standard_normal((3, 2, g * g + 1, 64)).astype(np.float32)


def text_case():
    rs = np.random.RandomState(9)
    return text_weights(rs), text_tokens(rs)


def affinity_case(C, kind="plain"):
    """feats [4, C, 25].  "zero": token 7 of image 1 is all zero (the 1e-12 clamp of F.normalize; with the batch mean above zero its
    mask_softmax row ends below zero everywhere: NaN).  The features are shifted so that the batch mean of the similarity is positive."""
    rs = np.random.RandomState(C + (17 if kind == "zero" else 0))
    f = (rs.standard_normal((4, C, 25)) + 0.5).astype(np.float32)
    if kind == "zero":
        f[1, :, 7] = 0
    return f


def relmax(a, b):
    return float(np.max(np.abs(np.asarray(a, F64) - np.asarray(b, F64)))) / max(float(np.max(np.abs(b))), 1e-30)


def maxabs(a, b):
    with np.errstate(invalid="ignore"):
        d = np.abs(np.asarray(a, F64) - np.asarray(b, F64))
    return float(np.nanmax(d))
