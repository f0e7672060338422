"""GPU parity tests, op level: every C-ABI entry point against the numpy oracle on seeded inputs
(and against the committed golden fixtures where one exists).  Run with `pytest -m gpu` on an MI355X."""
import numpy as np
import pytest

import oracle
from oracle.vit import VitConfig, make_vit_weights

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

TINY = VitConfig(width=128, layers=8, heads=2, patch=16, out_dim=64, input_resolution=64, n_surgery=5)


def dev(a, dtype=None):
    t = torch.as_tensor(np.ascontiguousarray(a))
    if dtype is not None:
        t = t.to(dtype)
    return t.cuda()


def host(t):
    return t.detach().cpu().numpy()


def maxabs(a, b):
    return float(np.max(np.abs(np.asarray(a, np.float64) - np.asarray(b, np.float64))))


def relmax(a, b):
    return maxabs(a, b) / max(float(np.max(np.abs(b))), 1e-30)


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from excel_amd import ops as _ops
    return _ops


def make_handle(ops, cfg, w, mode="f32"):
    """exact-fp32 numerics by default: the tight oracle tolerances below are statements about that path; the bf16x3
    (product default) path is checked against the north-star gates in the *_bf16x3_* tests."""
    return ops.VitHandle(w, cfg.width, cfg.layers, cfg.heads, cfg.patch, cfg.out_dim, n_surgery=cfg.n_surgery, gemm_mode=mode)


# ------------------------------------------------------------------ GEMM / LN
@pytest.mark.parametrize("M,N,K", [(128, 128, 32), (300, 45, 512), (257, 384, 768), (785, 2304, 768), (37, 64, 128)])
def test_gemm_nt(ops, M, N, K):
    rs = np.random.RandomState(M + N + K)
    A = rs.standard_normal((M, K)).astype(np.float32)
    W = rs.standard_normal((N, K)).astype(np.float32)      # asymmetric operands: a transposed write cannot pass
    bias = rs.standard_normal(N).astype(np.float32)
    res = rs.standard_normal((M, N)).astype(np.float32)
    ref = A.astype(np.float64) @ W.T.astype(np.float64)
    out = host(ops.gemm(dev(A), dev(W)))
    assert relmax(out, ref) < 2e-6
    y = ref + bias
    y = y * (1.0 / (1.0 + np.exp(-1.702 * y))) + res
    out2 = host(ops.gemm(dev(A), dev(W), bias=dev(bias), residual=dev(res), act=1))
    assert relmax(out2, y) < 3e-6


def test_gemm_identity_detects_transpose(ops):
    I = np.eye(64, dtype=np.float32)
    Bm = np.arange(64 * 64, dtype=np.float32).reshape(64, 64) / 100.0     # asymmetric
    out = host(ops.gemm(dev(I), dev(Bm)))           # I @ Bm^T
    assert np.array_equal(out, Bm.T)


@pytest.mark.parametrize("M,N,K", [(785, 64, 788), (100, 128, 64), (37, 64, 40)])
def test_gemm_nn_batched(ops, M, N, K):
    rs = np.random.RandomState(7)
    A = rs.standard_normal((3, M, K)).astype(np.float32)
    Bm = rs.standard_normal((3, K, N)).astype(np.float32)
    ref = A.astype(np.float64) @ Bm.astype(np.float64)
    out = host(ops.gemm(dev(A), dev(Bm), b_kmajor=False))
    assert relmax(out, ref) < 2e-6


def test_layernorm(ops):
    rs = np.random.RandomState(3)
    x = (rs.standard_normal((300, 768)) * 3 + 1).astype(np.float32)
    w = rs.standard_normal(768).astype(np.float32)
    b = rs.standard_normal(768).astype(np.float32)
    ref = oracle.vit.layer_norm(x, w, b)
    assert maxabs(host(ops.layernorm(dev(x), dev(w), dev(b))), ref) < 2e-5


def _layernorm_f64(x, w, b, eps=1e-5):
    """LayerNorm restated in float64: mean, biased variance, eps inside the root."""
    x = np.asarray(x, np.float64)
    mu = x.mean(-1, keepdims=True)
    var = ((x - mu) ** 2).mean(-1, keepdims=True)
    return (x - mu) / np.sqrt(var + eps) * np.asarray(w, np.float64) + np.asarray(b, np.float64)


@pytest.mark.parametrize("D", [4, 64, 128, 252, 256, 260, 768, 1024, 1280])
def test_layernorm_widths_rows_and_special_rows(ops, D):
    """layernorm_rows_kernel against float64 at every trip count of ln_row's lane loop (D = 4: one lane; 64: 16 lanes; 128: 32; 252 / 256 /
    260: the last lane's first trip missing, present, and lane 0's second trip; 1024 / 1280: 4 and 5 full trips) and on the register arm
    (768), with 1, 5 and 301 rows: none a multiple of the 4 rows of a workgroup, so the last workgroup is partial.

    Two special rows per row count (with one row: one call each).  OFFSET: 1e3 + standard_normal.  A one-pass variance E[x^2] - E[x]^2
    loses everything on it (1e6 against 1), and so does a mean kept as one fp32 number: its last place around 1e3 is 6e-5, which
    (x - mean) * w passes on as up to 1e-4 (what the fp32 oracle delivers on this row, see `o` below).  CONSTANT: every element 2.5, so the
    sum 2.5 D and the mean are exact in fp32 in any summation order, x - mean = 0 exactly, the variance is 0, rstd = eps^-1/2, and the
    output is 0 * rstd * w + b = the bias, bit for bit.

    Bound (max-abs): 2e-5, test_layernorm's, at D = 768; elsewhere max(2e-5, 3 x the fp32 oracle.vit.layer_norm's own deviation from
    float64 on the same input)."""
    rs = np.random.RandomState(100 + D)
    w = rs.standard_normal(D).astype(np.float32)
    b = rs.standard_normal(D).astype(np.float32)
    plain = lambda n: (rs.standard_normal((n, D)) * 3 + 1).astype(np.float32)
    offset = lambda: (1e3 + rs.standard_normal(D)).astype(np.float32)
    const = np.full(D, 2.5, np.float32)
    inputs = [("rows=1 plain", plain(1), None), ("rows=1 offset", offset()[None], None), ("rows=1 constant", const[None].copy(), 0)]
    for rows in (5, 301):
        x = plain(rows)
        x[rows - 1] = offset()                    # both in the partial last workgroup (rows % 4 == 1: the offset row is alone in it at
        x[rows - 2] = const                       # 5 and 301; the constant row closes the last full one)
        inputs.append((f"rows={rows}", x, rows - 2))
    for tag, x, const_row in inputs:
        ref = _layernorm_f64(x, w, b)
        o = maxabs(oracle.vit.layer_norm(x, w, b), ref)
        bound = 2e-5 if D == 768 else max(2e-5, 3 * o)
        got = host(ops.layernorm(dev(x), dev(w), dev(b)))
        assert got.shape == x.shape and got.dtype == np.float32
        err = maxabs(got, ref)
        print(f"[layernorm] D={D} {tag}: err {err:.2e} (fp32 oracle {o:.2e}, bound {bound:.2e})")
        assert err <= bound, (tag, err, bound)
        if const_row is not None:
            assert np.array_equal(got[const_row], b), (tag, maxabs(got[const_row], b))


# ------------------------------------------------------------------ ViT
def _check_vit(ops, cfg, w, imgs, tol_rel, check_feats=True):
    L = cfg.layers
    h = make_handle(ops, cfg, w)
    nl = min(6, L)
    r = h.forward(dev(imgs), want_w_aff=True, aff_layers=nl, n_attn_out=L, want_feats=check_feats, want_raw=True)
    x, attn, feats = oracle.vit.vit_forward(imgs, w, cfg)
    f_ref, _, _ = oracle.cam.generate_clip_fts(imgs, w, cfg)
    got_attn = host(r["attn"])
    for l in range(L):
        assert maxabs(got_attn[l], attn[l]) < tol_rel * max(1.0, cfg.heads if l >= L - cfg.n_surgery else 1.0) * 10, f"attn layer {l}"
    if check_feats:
        got_feats = host(r["feats"])
        for l in range(L):
            assert relmax(got_feats[l], feats[l]) < tol_rel, f"feats layer {l}"
    assert relmax(host(r["x_raw"]), x) < tol_rel
    assert relmax(host(r["image_features"]), f_ref) < tol_rel
    w_ref = attn[-nl:, :, 1:, 1:].mean(0, dtype=np.float32)
    assert relmax(host(r["w_aff"]), w_ref) < tol_rel
    return r, (x, attn, feats, f_ref)


def test_vit_tiny_vs_oracle(ops):
    w = make_vit_weights(TINY, seed=11)
    imgs = np.random.RandomState(21).standard_normal((2, 3, 96, 96)).astype(np.float32)
    _check_vit(ops, TINY, w, imgs, 5e-5)


def test_vit_tiny_vs_golden(ops, golden):
    g = golden("vit_cam_tiny.npz")
    w = make_vit_weights(TINY, seed=int(g["seed_w"]))
    for mode in ("train", "val"):
        wm = oracle.vit.reload_self_attn(w, TINY, feat_size=6, mode=mode)
        h = make_handle(ops, TINY, wm)
        r = h.forward(dev(g["imgs"]), n_attn_out=TINY.layers, want_raw=True, want_feats=True)
        assert relmax(host(r["x_raw"]), g[f"{mode}_x"]) < 5e-5
        assert relmax(host(r["image_features"]), g[f"{mode}_image_features"]) < 5e-5
        assert maxabs(host(r["attn"]), g[f"{mode}_attn"]) < 2e-4
        assert relmax(host(r["feats"])[-1], g[f"{mode}_feat_last"]) < 5e-5
        full, _ = ops.clip_feature_surgery(r["image_features"], dev(g[f"{mode}_text"]))
        assert maxabs(host(full), g[f"{mode}_cam"]) < 1e-3      # north-star CAM gate
        assert maxabs(host(full), g[f"{mode}_cam"]) < 1e-4      # what fp32 actually delivers
    # second resolution through the pre-resized grid (quirk Q5)
    wm = oracle.vit.reload_self_attn(w, TINY, feat_size=6, mode="train")
    h = make_handle(ops, TINY, wm)
    r = h.forward(dev(g["res2_imgs"]), n_attn_out=1, want_raw=True)
    assert relmax(host(r["x_raw"]), g["res2_x"]) < 5e-5
    assert maxabs(host(r["attn"])[0], g["res2_attn_last"]) < 2e-4


@pytest.mark.parametrize("S", [384, 416])
def test_vit_tiny_strip_three_tiles_per_wave_bf16x3(ops, S):
    """The attention strip kernel's 3-tiles-per-wave instantiation (513 <= N <= 768: 384^2 -> N = 577 = 19 key tiles on 7 waves with 3 or 2
    tiles each; 416^2 -> N = 677 = 22 tiles, the last one ragged) - the benchmark shape runs 4 per wave, the tiny tests 1: per-layer attention
    weights, the affinity mean and the features of the tiny net in the default bf16x3 mode against the oracle."""
    w = make_vit_weights(TINY, seed=31)
    imgs = np.random.RandomState(S).standard_normal((2, 3, S, S)).astype(np.float32)
    wm = oracle.vit.reload_self_attn(w, TINY, feat_size=S // 16, mode="train")
    h = make_handle(ops, TINY, wm, mode="bf16x3")
    r = h.forward(dev(imgs), want_w_aff=True, aff_layers=6, n_attn_out=TINY.layers, want_raw=True)
    x, attn, _ = oracle.vit.vit_forward(imgs, wm, TINY)
    got = host(r["attn"])
    for l in range(TINY.layers):
        assert maxabs(got[l], attn[l]) < 2e-4 * (TINY.heads if l >= TINY.layers - TINY.n_surgery else 1.0), f"attn layer {l}"
    # 3e-4: bf16x3's accumulated rounding in this tiny net (width 128) lands at 1.8-2.3e-4 depending on the GEMM's accumulation order - with
    # the K = 32 MFMA form 2.30e-4 / 2.19e-4, while the GEMM's own error against float64 is unchanged to three digits (rms 4.43e-6, max 2.7e-5 of
    # the output's rms for both forms: tools_dev/gemm_accuracy.py)
    assert relmax(host(r["w_aff"]), attn[-6:, :, 1:, 1:].mean(0, dtype=np.float32)) < 3e-4
    assert relmax(host(r["x_raw"]), x) < 5e-4


def test_vit_odd_batch_and_no_surgery(ops):
    cfg = VitConfig(width=128, layers=3, heads=2, patch=16, out_dim=64, input_resolution=64, n_surgery=0)
    w = make_vit_weights(cfg, seed=5)
    imgs = np.random.RandomState(2).standard_normal((3, 3, 80, 80)).astype(np.float32)
    _check_vit(ops, cfg, w, imgs, 5e-5)


def test_vit_b16_448_single_image_vs_oracle(ops):
    """BASELINE shape (ViT-B/16, 448x448, N=785) on one image, seeded weights."""
    cfg = VitConfig(width=768, layers=12, heads=12, patch=16, out_dim=512, input_resolution=224, n_surgery=5)
    w = make_vit_weights(cfg, seed=1, attn_gain=2.0)
    imgs = np.random.RandomState(4).standard_normal((1, 3, 448, 448)).astype(np.float32)
    h = make_handle(ops, cfg, w)
    r = h.forward(dev(imgs), want_w_aff=True, n_attn_out=6, want_raw=True)
    x, attn, _ = oracle.vit.vit_forward(imgs, w, cfg)
    f_ref, _, _ = oracle.cam.generate_clip_fts(imgs, w, cfg)
    assert relmax(host(r["x_raw"]), x) < 2e-4
    assert relmax(host(r["image_features"]), f_ref) < 2e-4
    assert maxabs(host(r["attn"]), attn[-6:]) < 2e-3
    assert relmax(host(r["w_aff"]), attn[-6:, :, 1:, 1:].mean(0, dtype=np.float32)) < 2e-4
    # CAM gate on the full-size features
    rs = np.random.RandomState(8)
    text = rs.standard_normal((45, 512)).astype(np.float32)
    text /= np.linalg.norm(text, axis=1, keepdims=True)
    full, sl = ops.clip_feature_surgery(r["image_features"], dev(text), num_fg=20)
    ref = oracle.cam.clip_feature_surgery(f_ref, text)
    assert maxabs(host(full), ref) < 1e-3
    assert np.array_equal(host(sl), host(full)[:, 1:, :20])


# ------------------------------------------------------------------ CAM
@pytest.mark.parametrize("B,N,C,T,F", [(2, 37, 64, 9, 4), (3, 785, 512, 45, 20), (1, 1025, 512, 103, 80)])
def test_clip_feature_surgery(ops, B, N, C, T, F):
    rs = np.random.RandomState(N + T)
    f = rs.standard_normal((B, N, C)).astype(np.float32)
    f = f / np.linalg.norm(f, axis=1, keepdims=True)
    t = rs.standard_normal((T, C)).astype(np.float32)
    t /= np.linalg.norm(t, axis=1, keepdims=True)
    ref = oracle.cam.clip_feature_surgery(f, t)
    full, sl = ops.clip_feature_surgery(dev(f), dev(t), num_fg=F)
    assert maxabs(host(full), ref) < 2e-5
    assert maxabs(host(sl), ref[:, 1:, :F]) < 2e-5


@pytest.mark.parametrize("mode,tol", [("f32", 2e-5), ("bf16x3", 6e-5)])
@pytest.mark.parametrize("B,N,C,T,F", [(3, 785, 512, 45, 20), (1, 1025, 512, 103, 80), (2, 37, 64, 9, 4), (1, 17, 32, 33, 33)])
def test_patch_text_cam_fused(ops, B, N, C, T, F, mode, tol):
    """excel_patch_text_cam: token-axis L2 norm (clip.py:353) + similarity on the matrix core + surgery epilogue (clip.py:288-310)
    in one launch from the UN-normalised token features, against the oracle's generate_clip_fts tail + clip_feature_surgery."""
    rs = np.random.RandomState(N + T + C)
    x = (rs.standard_normal((B, N, C)) * (1 + rs.rand(1, 1, C) * 3)).astype(np.float32)      # uneven column norms
    t = rs.standard_normal((T, C)).astype(np.float32)
    t /= np.linalg.norm(t, axis=1, keepdims=True)
    f = (x / np.sqrt((x * x).sum(axis=1, keepdims=True, dtype=np.float32))).astype(np.float32)   # clip.py:353
    ref = oracle.cam.clip_feature_surgery(f, t)
    full, sl, feats = ops.patch_text_cam(dev(x), dev(t), num_fg=F, want_full=True, want_features=True, mode=mode)
    assert maxabs(host(feats), f) < 1e-6
    assert maxabs(host(full), ref) < tol and maxabs(host(sl), ref[:, 1:, :F]) < tol
    # the two-launch path on the normalised features gives the same maps
    full2, _ = ops.clip_feature_surgery(dev(f), dev(t), num_fg=F)
    assert maxabs(host(full), host(full2)) < tol
    _, sl_only, none = ops.patch_text_cam(dev(x), dev(t), num_fg=F, mode=mode)                # slice only, no feature write
    assert none is None and torch.equal(sl_only, sl)


@pytest.mark.parametrize("mode", ["bf16x3", "f32"])
def test_patch_text_cam_is_batch_invariant(ops, mode):
    """The attribute maps of an image do not depend on its position in the batch or on the batch size, bit for bit: the token-axis
    norms are reduced over image-aligned blocks in a fixed order, the class-prior weights in fixed fp32 chains, min / max exactly."""
    rs = np.random.RandomState(21)
    x = dev((rs.standard_normal((5, 785, 512)) * (1 + rs.rand(1, 1, 512) * 3)).astype(np.float32))
    t = rs.standard_normal((45, 512)).astype(np.float32)
    t = dev(t / np.linalg.norm(t, axis=1, keepdims=True))
    full, sl, _ = ops.patch_text_cam(x, t, num_fg=20, want_full=True, mode=mode)
    for b in (0, 3, 4):
        f1, s1, _ = ops.patch_text_cam(x[b:b + 1].contiguous(), t, num_fg=20, want_full=True, mode=mode)
        assert torch.equal(f1[0], full[b]) and torch.equal(s1[0], sl[b])
    full2, _, _ = ops.patch_text_cam(x, t, num_fg=20, want_full=True, mode=mode)
    assert torch.equal(full2, full)                                                     # run to run


def test_clip_feature_surgery_redundant_feats_branch(ops):
    """clip.py:289-290: similarity = image_features @ (text_features - redundant_feats).t() (the reference then returns an
    unassigned name, :310; the evident intent - the similarity - is returned here)."""
    from excel_amd import clip as xclip
    rs = np.random.RandomState(5)
    f = rs.standard_normal((2, 37, 64)).astype(np.float32)
    t = rs.standard_normal((9, 64)).astype(np.float32)
    red = rs.standard_normal((1, 64)).astype(np.float32)
    out = host(xclip.clip_feature_surgery(dev(f), dev(t), redundant_feats=dev(red)))
    assert out.shape == (2, 37, 9) and maxabs(out, f @ (t - red).T) < 1e-4


def test_clip_feature_surgery_golden(ops, golden):
    g = golden("ops.npz")
    full, _ = ops.clip_feature_surgery(dev(g["cfs_f"]), dev(g["cfs_t"]))
    assert maxabs(host(full), g["cfs_out"]) < 2e-5


# ------------------------------------------------------------------ affinity
def test_compute_trans_mat(ops, golden):
    g = golden("ops.npz")
    out = host(ops.compute_trans_mat(dev(g["tm_in"])))
    np.testing.assert_allclose(out, g["tm_out"], rtol=5e-5, atol=1e-9)
    rs = np.random.RandomState(1)
    a = (rs.rand(2, 784, 784).astype(np.float32) ** 4 + 1e-4)
    ref = np.stack([oracle.aff.compute_trans_mat(x) for x in a])
    out = host(ops.compute_trans_mat(dev(a)))
    np.testing.assert_allclose(out, ref, rtol=1e-4, atol=1e-12)


def test_attn_layer_mean(ops):
    rs = np.random.RandomState(0)
    attn = rs.rand(8, 2, 37, 37).astype(np.float32)
    out = host(ops.attn_layer_mean(dev(attn), 6))
    assert maxabs(out, attn[-6:, :, 1:, 1:].mean(0)) < 1e-6


def _smooth_maps(rs, B, g, F):
    """Random smooth-ish maps in [0,1] with several blobs per class."""
    yy, xx = np.mgrid[0:g, 0:g].astype(np.float32)
    out = np.zeros((B, g * g, F), np.float32)
    for b in range(B):
        for f in range(F):
            m = np.zeros((g, g), np.float32)
            for _ in range(rs.randint(1, 5)):
                cy, cx, s = rs.uniform(0, g), rs.uniform(0, g), rs.uniform(0.8, 4.0)
                m += rs.uniform(0.3, 1.0) * np.exp(-((yy - cy) ** 2 + (xx - cx) ** 2) / (2 * s * s))
            m += 0.05 * rs.rand(g, g)
            m = (m - m.min()) / (m.max() - m.min())
            out[b, :, f] = m.reshape(-1)
    return out


from _known_boxes import GRADED, KNOWN  # noqa: E402


def _check_box_case(ops, m, thr, e):
    g = m.shape[0]
    assert m.shape == (g, g)
    assert np.array_equal(oracle.aff.box_mask(m, thr).astype(np.uint8), e), "oracle known-answer"
    attr = dev(m.reshape(1, g * g, 1))
    idx, n = ops.cls_compact(dev(np.ones((1, 1), np.float32)), 2)
    v, mask = ops.scoremap_box_mask(attr, idx, n, g, thr, want_mask=True)
    assert np.array_equal(host(mask)[0, 0].reshape(g, g), e)
    assert np.array_equal(host(v)[0, 0].reshape(g, g), m * e)


@pytest.mark.parametrize("name", sorted(KNOWN))
def test_box_mask_known_answers(ops, name):
    rows, exp = KNOWN[name]
    _check_box_case(ops, np.array([[float(c) for c in r] for r in rows], np.float32), 0.5, np.array([[int(c) for c in r] for r in exp], np.uint8))


@pytest.mark.parametrize("name", sorted(GRADED))
def test_box_mask_graded_known_answers(ops, name):
    vals, thr, exp = GRADED[name]
    _check_box_case(ops, np.array(vals, np.float32), thr, np.array([[int(c) for c in r] for r in exp], np.uint8))


@pytest.mark.parametrize("g", [6, 28, 32])
def test_box_mask_random(ops, g):
    rs = np.random.RandomState(g)
    B, F = 4, 5
    attr = _smooth_maps(rs, B, g, F)
    onehot = (rs.rand(B, F) < 0.6).astype(np.float32)
    onehot[:, 0] = 1
    idx, n = ops.cls_compact(dev(onehot), F)
    assert np.array_equal(host(n), onehot.sum(1).astype(np.int32))
    v, mask = ops.scoremap_box_mask(dev(attr), idx, n, g, 0.79, want_mask=True)
    idx_h, mask_h = host(idx), host(mask)
    for b in range(B):
        present = np.where(onehot[b])[0]
        assert np.array_equal(idx_h[b, :len(present)], present)
        for s, cls in enumerate(present):
            ref = oracle.aff.box_mask(attr[b, :, cls].reshape(g, g), 0.79)
            assert np.array_equal(mask_h[b, s].reshape(g, g), ref.astype(np.uint8)), (b, cls)


def test_box_mask_snake_converges(ops):
    """A long 1-pixel-wide serpentine: worst case for label propagation."""
    g = 28
    m = np.zeros((g, g), np.float32)
    for y in range(0, g, 2):
        m[y, :] = 1
        if y + 1 < g:
            m[y + 1, (g - 1) if (y // 2) % 2 == 0 else 0] = 1
    ref = oracle.aff.box_mask(m, 0.5)
    idx, n = ops.cls_compact(dev(np.ones((1, 1), np.float32)), 1)
    _, mask = ops.scoremap_box_mask(dev(m.reshape(1, g * g, 1)), idx, n, g, 0.5, want_mask=True)
    assert np.array_equal(host(mask)[0, 0].reshape(g, g), ref.astype(np.uint8))


def test_refine_cams_with_aff_batched(ops):
    rs = np.random.RandomState(12)
    B, g, F = 3, 28, 20
    P = g * g
    attr = _smooth_maps(rs, B, g, F)
    w_aff = (rs.rand(B, P, P).astype(np.float32) ** 6 + 1e-4)
    onehot = np.zeros((B, F), np.float32)
    onehot[0, [3]] = 1
    onehot[1, [0, 7, 19]] = 1
    onehot[2, [5, 6]] = 1
    idx, n = ops.cls_compact(dev(onehot), 3)
    out = host(ops.refine_cams_with_aff_batched(dev(attr), dev(w_aff), idx, n, g, 0.79))
    for b in range(B):
        present = np.where(onehot[b])[0]
        trans = oracle.aff.compute_trans_mat(w_aff[b])
        for s, cls in enumerate(present):
            gmap = attr[b, :, cls].reshape(g, g)
            mask = oracle.aff.box_mask(gmap, 0.79).reshape(1, -1)
            ref = ((trans * mask) @ gmap.reshape(-1, 1)).reshape(-1)
            assert relmax(out[b, s], ref) < 2e-5, (b, cls)
        assert not out[b, len(present):].any()


@pytest.mark.parametrize("g,H,W", [(6, 40, 56), (28, 448, 448), (28, 375, 500), (32, 333, 512)])
def test_cam_upsample_bkg(ops, g, H, W):
    rs = np.random.RandomState(H)
    B, smax = 2, 3
    r = rs.rand(B, smax, g * g).astype(np.float32) * 0.3
    ncls = np.array([3, 1], np.int32)
    cams = host(ops.cam_upsample_bkg(dev(r), dev(ncls), g, H, W))
    for b in range(B):
        maps = np.stack([oracle.aff.scale_cam_image(r[b, s].reshape(g, g), (W, H)) for s in range(ncls[b])])
        bg = 1 - maps.max(0)
        assert maxabs(cams[b, 1:1 + ncls[b]], maps) < 2e-6
        assert maxabs(cams[b, 0], bg) < 2e-6


# ------------------------------------------------------------------ PAR / labels / metric
def test_par_golden(ops, golden):
    g = golden("ops.npz")
    out = host(ops.par_forward(dev(g["par_img"]), dev(g["par_mask"]), num_iter=20))
    assert maxabs(out, g["par_out"]) < 1e-4
    out2 = host(ops.par_forward(dev(g["par2_img"]), dev(g["par2_mask"]), num_iter=3))
    assert maxabs(out2, g["par2_out"]) < 2e-5


@pytest.mark.parametrize("B,C,H,W,it", [(2, 3, 64, 80, 5), (1, 7, 96, 96, 20), (2, 9, 50, 33, 2)])
def test_par_vs_oracle(ops, B, C, H, W, it):
    rs = np.random.RandomState(C * H)
    img = rs.standard_normal((B, 3, H, W)).astype(np.float32)
    masks = rs.rand(B, C, H, W).astype(np.float32)
    ref = oracle.par.PAR([1, 2, 4, 8, 12, 24], it)(img, masks)
    out = host(ops.par_forward(dev(img), dev(masks), num_iter=it))
    assert maxabs(out, ref) < 5e-5


def test_par_ragged_channels(ops):
    rs = np.random.RandomState(2)
    B, Cmax, H, W = 3, 4, 40, 48
    img = rs.standard_normal((B, 3, H, W)).astype(np.float32)
    masks = rs.rand(B, Cmax, H, W).astype(np.float32)
    nchan = np.array([2, 4, 3], np.int32)
    out = host(ops.par_forward(dev(img), dev(masks), num_iter=4, nchan=dev(nchan)))
    par = oracle.par.PAR([1, 2, 4, 8, 12, 24], 4)
    for b in range(B):
        ref = par(img[b:b + 1], masks[b:b + 1, :nchan[b]])
        assert maxabs(out[b, :nchan[b]], ref[0]) < 5e-5


def test_par_guide_resize_align_corners(ops):
    rs = np.random.RandomState(3)
    img = rs.standard_normal((1, 3, 24, 30)).astype(np.float32)
    masks = rs.rand(1, 2, 41, 37).astype(np.float32)
    ref = oracle.par.PAR([1, 2, 4, 8, 12, 24], 2)(img, masks)
    out = host(ops.par_forward(dev(img), dev(masks), num_iter=2))
    assert maxabs(out, ref) < 5e-5


def test_argmax_label(ops):
    rs = np.random.RandomState(5)
    B, smax, H, W = 3, 3, 17, 29
    cams = rs.rand(B, smax + 1, H, W).astype(np.float32)
    cams[0, 1] = cams[0, 2]                      # exact ties -> first index wins
    onehot = np.zeros((B, 20), np.float32)
    onehot[0, [2, 5, 9]] = 1
    onehot[1, [0]] = 1
    onehot[2, [18, 19]] = 1
    idx, n, nchan = ops.cls_compact(dev(onehot), smax, want_nchan=True)
    l8, l64 = ops.argmax_label(dev(cams), nchan, idx, want_i64=True)
    l8, l64 = host(l8), host(l64)
    for b in range(B):
        cls = np.where(onehot[b])[0]
        key = np.pad(cls + 1, (1, 0))
        ref = key[cams[b, :len(cls) + 1].argmax(0)]
        assert np.array_equal(l8[b], ref.astype(np.uint8))
        assert np.array_equal(l64[b], ref.astype(np.int64))


@pytest.mark.parametrize("nc,n", [(21, 448 * 448 * 3 + 5), (81, 100003), (5, 7)])
def test_confusion(ops, nc, n):
    rs = np.random.RandomState(nc)
    gt = rs.randint(0, nc, n).astype(np.uint8)
    gt[rs.rand(n) < 0.03] = 255
    pred = rs.randint(0, nc, n).astype(np.uint8)
    hist = ops.confusion_accumulate(dev(gt), dev(pred), nc)
    hist = ops.confusion_accumulate(dev(gt), dev(pred), nc, hist)        # accumulates
    ref = oracle.evaluate.fast_hist(gt, pred, nc)
    assert np.array_equal(host(hist), 2 * ref)


@pytest.mark.parametrize("B,C,H,W,dil,it", [(2, 3, 64, 80, (1, 2, 4, 8, 12, 24), 5), (1, 7, 96, 96, (1, 2, 4, 8, 12, 24), 20),
                                            (3, 2, 52, 36, (1, 2, 4, 8, 12, 24), 3), (2, 4, 448, 448, (1, 2, 4, 8, 12, 24), 2)])
def test_par_recompute_equals_streamed_affinities(ops, B, C, H, W, dil, it):
    """The default PAR step recomputes its 48 weights per pixel from the guide image and 5 per-pixel statistics (same operations in
    the same order as the affinity kernel); streaming the 48 planes (a per-call flag) must give the SAME BITS, ragged channel counts
    included."""
    rs = np.random.RandomState(H + C)
    img = dev(rs.standard_normal((B, 3, H, W)).astype(np.float32))
    masks = dev(rs.rand(B, C, H, W).astype(np.float32))
    nchan = dev(np.array([max(1, C - b) for b in range(B)], np.int32))
    ref = ops.par_forward(img, masks, dil, it, nchan=nchan, stream_affinities=True)
    got = ops.par_forward(img, masks, dil, it, nchan=nchan)
    for b in range(B):
        k = int(host(nchan)[b])
        assert torch.equal(got[b, :k], ref[b, :k])
    lo = oracle.par.PAR(list(dil), it)(host(img)[:1], host(masks)[:1, :int(host(nchan)[0])])
    assert maxabs(host(got)[0, :int(host(nchan)[0])], lo[0]) < 2e-4


def test_par_other_dilation_sets_use_the_streamed_kernel(ops):
    """Dilation sets other than the reference's [1,2,4,8,12,24] (1..8 entries, any values) go through the streamed-plane kernel."""
    rs = np.random.RandomState(9)
    img = rs.standard_normal((2, 3, 33, 47)).astype(np.float32)
    masks = rs.rand(2, 3, 33, 47).astype(np.float32)
    for dil in ((1, 2, 4, 8), (3,), (1, 2, 3, 5, 6, 7, 9, 11)):
        ref = oracle.par.PAR(list(dil), 3)(img, masks)
        assert maxabs(host(ops.par_forward(dev(img), dev(masks), dil, 3)), ref) < 5e-5


# ------------------------------------------------------------------ ragged batches (images of different label sizes in one launch)
RAGGED_SIZES = [(375, 500), (500, 375), (333, 500), (96, 64), (17, 29), (448, 448), (500, 334), (281, 500)]


def _pack_planes(plan, arrs, K):
    """list of [K,H,W] arrays -> packed pitched float tensor (padding columns filled with NaN: nothing may read them as data)."""
    out = np.full(K * plan.total_pix, np.nan, np.float32)
    for b, a in enumerate(arrs):
        H, W = a.shape[-2:]
        Wp = (W + 3) // 4 * 4
        v = out[K * plan.poff[b]:K * plan.poff[b] + K * H * Wp].reshape(K, H, Wp)
        v[:, :, :W] = a
    return out


def test_ragged_plan_matches_the_documented_layout(ops):
    plan = ops.RaggedPlan(RAGGED_SIZES, "cuda")
    rec = plan.table_host[:8 * (plan.B + 1)].reshape(-1, 8)
    pix = lab = tiles = 0
    for b, (H, W) in enumerate(RAGGED_SIZES):
        assert tuple(rec[b, :5]) == (H, W, pix, tiles, lab)
        nt = -(-W // 64) * -(-H // 16)
        assert np.all(plan.table_host[8 * (plan.B + 1) + tiles:8 * (plan.B + 1) + tiles + nt] == b)
        pix += H * ((W + 3) // 4 * 4); lab += H * W; tiles += nt
    assert (plan.total_pix, plan.total_label_pix, plan.total_tiles) == (pix, lab, tiles)
    assert tuple(rec[plan.B, 2:5]) == (pix, tiles, lab)


def test_ragged_normalize_resize_equals_two_step(ops):
    """excel_normalize_resize_u8_ragged == excel_normalize_img_u8 + excel_bilinear_resize per image, bit for bit; and the oracle."""
    rs = np.random.RandomState(4)
    imgs = [rs.randint(0, 256, (H, W, 3)).astype(np.uint8) for H, W in RAGGED_SIZES]
    plan = ops.RaggedPlan(RAGGED_SIZES, "cuda")
    packed = dev(np.concatenate([im.reshape(-1) for im in imgs]))
    S = 128
    got = ops.normalize_resize_u8_ragged(packed, plan, S)
    for b, im in enumerate(imgs):
        two = ops.bilinear_resize(ops.normalize_img_u8(dev(im[None])), S, S, align_corners=False)
        assert torch.equal(got[b], two[0])
    mean, std = np.array([123.675, 116.28, 103.53]), np.array([58.395, 57.12, 57.375])
    x = ((imgs[0].astype(np.float64) - mean) / std).astype(np.float32).transpose(2, 0, 1)
    ref = torch.nn.functional.interpolate(torch.from_numpy(x)[None], size=(S, S), mode="bilinear", align_corners=False)[0].numpy()
    assert maxabs(host(got[0]), ref) < 2e-5


def test_ragged_upsample_par_argmax_equal_per_image_calls(ops):
    """The ragged entry points (cam_upsample_bkg / PAR / arg-max over packed, pitched planes of 8 different sizes, odd widths included)
    give the SAME BITS as the uniform entry points called per image - streamed-plane PAR included for widths that are not multiples
    of 4 - and the confusion matrix over the flat label arrays equals the sum of the per-image ones."""
    rs = np.random.RandomState(11)
    B, smax, g, S = len(RAGGED_SIZES), 3, 8, 128
    plan = ops.RaggedPlan(RAGGED_SIZES, "cuda")
    refined = dev(rs.rand(B, smax, g * g).astype(np.float32))
    onehot = np.zeros((B, 20), np.float32)
    for b in range(B):
        onehot[b, rs.choice(20, 1 + b % smax, replace=False)] = 1
    idx, ncls, nchan = ops.cls_compact(dev(onehot), smax, want_nchan=True)
    imgs = dev(rs.standard_normal((B, 3, S, S)).astype(np.float32))
    gts = [rs.randint(0, 21, hw).astype(np.uint8) for hw in RAGGED_SIZES]
    gt_packed = dev(np.concatenate([x.reshape(-1) for x in gts]))
    cams = ops.cam_upsample_bkg_ragged(refined, ncls, g, plan)
    par = ops.par_forward_ragged(imgs, cams, plan, smax + 1, num_iter=3, nchan=nchan)
    lab = ops.argmax_label_ragged(par, plan, smax + 1, nchan, idx)
    hist = ops.confusion_accumulate(gt_packed, lab, 21)
    hist_ref = None
    for b, (H, W) in enumerate(RAGGED_SIZES):
        k = int(host(nchan)[b])
        c1 = ops.cam_upsample_bkg(refined[b:b + 1], ncls[b:b + 1], g, H, W)
        assert torch.equal(plan.planes(cams, b, smax + 1)[:k], c1[0, :k])
        p1 = ops.par_forward(imgs[b:b + 1], c1, num_iter=3, nchan=nchan[b:b + 1])
        assert torch.equal(plan.planes(par, b, smax + 1)[:k], p1[0, :k]), (H, W)
        l1 = ops.argmax_label(p1, nchan[b:b + 1], idx[b:b + 1])
        assert torch.equal(plan.label(lab, b), l1[0])
        hist_ref = ops.confusion_accumulate(dev(gts[b]), l1[0], 21, hist_ref)
    assert torch.equal(hist, hist_ref)
    # ... and the oracle, on the smallest image
    b = 4
    k = int(host(nchan)[b])
    ref = oracle.par.PAR([1, 2, 4, 8, 12, 24], 3)(host(imgs[b:b + 1]), host(plan.planes(cams, b, smax + 1))[None, :k])
    assert maxabs(host(plan.planes(par, b, smax + 1))[:k], ref[0]) < 5e-5


def test_ragged_tiny_images(ops):
    """Degenerate sizes in a ragged batch (1x1, a single row, a single column, widths below one float4): the tile map has one tile per
    image and every stage still equals the uniform entry points (which take the streamed PAR kernel for these shapes), bit for bit."""
    rs = np.random.RandomState(17)
    sizes = [(1, 1), (3, 2), (1, 9), (11, 1), (5, 7), (2, 3)]
    B, smax, g = len(sizes), 2, 4
    plan = ops.RaggedPlan(sizes, "cuda")
    assert plan.total_tiles == B
    refined = dev(rs.rand(B, smax, g * g).astype(np.float32))
    onehot = np.zeros((B, 20), np.float32)
    for b in range(B):
        onehot[b, rs.choice(20, 1 + b % smax, replace=False)] = 1
    idx, ncls, nchan = ops.cls_compact(dev(onehot), smax, want_nchan=True)
    imgs = dev(rs.standard_normal((B, 3, 16, 16)).astype(np.float32))
    cams = ops.cam_upsample_bkg_ragged(refined, ncls, g, plan)
    par = ops.par_forward_ragged(imgs, cams, plan, smax + 1, num_iter=2, nchan=nchan)
    lab = ops.argmax_label_ragged(par, plan, smax + 1, nchan, idx)
    for b, (H, W) in enumerate(sizes):
        k = int(host(nchan)[b])
        c1 = ops.cam_upsample_bkg(refined[b:b + 1], ncls[b:b + 1], g, H, W)
        p1 = ops.par_forward(imgs[b:b + 1], c1, num_iter=2, nchan=nchan[b:b + 1])
        assert torch.equal(plan.planes(cams, b, smax + 1)[:k], c1[0, :k]) and torch.equal(plan.planes(par, b, smax + 1)[:k], p1[0, :k]), (H, W)
        assert torch.equal(plan.label(lab, b), ops.argmax_label(p1, nchan[b:b + 1], idx[b:b + 1])[0])
    u8 = [rs.randint(0, 256, (H, W, 3)).astype(np.uint8) for H, W in sizes]
    x = ops.normalize_resize_u8_ragged(dev(np.concatenate([a.reshape(-1) for a in u8])), plan, 32)
    for b, a in enumerate(u8):
        assert torch.equal(x[b], ops.bilinear_resize(ops.normalize_img_u8(dev(a[None])), 32, 32, align_corners=False)[0])


def test_ragged_par_ignores_row_padding(ops):
    """The padding columns of the pitched layout are never read as data: NaN there must not reach a pixel."""
    rs = np.random.RandomState(12)
    sizes = [(40, 30), (33, 61), (64, 64)]
    plan = ops.RaggedPlan(sizes, "cuda")
    masks = [rs.rand(2, H, W).astype(np.float32) for H, W in sizes]
    imgs = dev(rs.standard_normal((3, 3, 32, 32)).astype(np.float32))
    out = ops.par_forward_ragged(imgs, dev(_pack_planes(plan, masks, 2)), plan, 2, num_iter=2)
    for b, (H, W) in enumerate(sizes):
        ref = ops.par_forward(imgs[b:b + 1], dev(masks[b][None]), num_iter=2)
        assert torch.equal(plan.planes(out, b, 2), ref[0])


@pytest.mark.parametrize("H,W,C,params,kind", [(24, 30, 3, (10, 3, 1, 4, 67, 3), "noise_half"), (37, 29, 5, (5, 3, 3, 10, 80, 13), "noise_half"),
                                               (50, 64, 2, (10, 3, 1, 4, 67, 3), "noise_half"), (37, 29, 5, (10, 3, 3, 10, 80, 13), "smooth"),
                                               (24, 30, 3, (10, 3, 1, 4, 67, 3), "uniform")],
                         ids=["24-30-3-params0", "37-29-5-params1", "50-64-2-params2", "37-29-5-smooth", "24-30-3-uniform"])
def test_dcrf_vs_oracle(ops, H, W, C, params, kind):
    """excel_dcrf_inference (utils/dcrf.py:42-68 with the parameter sets of tools/infer_lam.py:191-198 and utils/dcrf.py:20-21) against
    the numpy restatement of the published mean-field / permutohedral-lattice algorithm; marginals within 2e-4, labels equal except
    where the two top marginals tie.  `smooth` and `uniform` (tests/_dcrf_filter_ref.py) give long vertex lists per lattice point; one
    message at a time is held far tighter in tests/test_gpu_dcrf_filter.py."""
    rs = np.random.RandomState(H + C)
    img = (rs.rand(H, W, 3) * 255).astype(np.uint8)
    img[:, : W // 2] = (img[:, : W // 2] * 0.15 + 140).astype(np.uint8)           # a smooth half and a noisy half
    if kind != "noise_half":
        import _dcrf_filter_ref
        img = _dcrf_filter_ref.image(kind, H, W, H + C)
    p = rs.rand(C, H, W).astype(np.float32) ** 2 + 1e-3
    p /= p.sum(0, keepdims=True)
    ref = oracle.dcrf.dense_crf_2d(img, oracle.dcrf.unary_from_softmax(p), *params)
    got = host(ops.dcrf_inference(dev(img, torch.uint8), dev(p), *params))
    assert maxabs(got, ref) < 1e-3 and float(np.abs(got - ref).mean()) < 2e-5      # ten softmax iterations amplify fp32 round-off at a few pixels
    np.testing.assert_allclose(got.sum(0), 1.0, atol=1e-5)
    top2 = np.sort(ref, 0)[-2:]
    clear = (top2[1] - top2[0]) > 1e-3
    assert np.array_equal(got.argmax(0)[clear], ref.argmax(0)[clear])
    again = host(ops.dcrf_inference(dev(img, torch.uint8), dev(p), *params))
    assert np.array_equal(got, again)                                             # fixed-point splat: bit-reproducible


def test_dcrf_device_properties(ops):
    """Properties of the device mean field that hold for the model whatever the implementation (parity with pydensecrf itself stays
    UNPINNED: the package is absent from the reference snapshot and from this image, tests/test_oracle_golden.py says the same):
      * both pairwise weights 0                -> Q = softmax(-U) = the (clipped, renormalised) input probabilities, at any iteration count
      * Potts compatibility is label-symmetric -> permuting the classes of the input permutes the output
      * a class that is nowhere likely stays nowhere likely; marginals are a distribution at every pixel
      * smoothing: on a two-region image with noisy unaries the label map gets more homogeneous inside a region, never less
      * the launch-batched message passing (both kernels per launch, 8 launches per step) is bit-reproducible"""
    rs = np.random.RandomState(31)
    H, W, C = 36, 44, 4
    img = np.zeros((H, W, 3), np.uint8)
    img[:, : W // 2] = (40, 60, 200)
    img[:, W // 2:] = (220, 180, 30)
    img = (img.astype(np.int16) + rs.randint(-6, 7, img.shape)).clip(0, 255).astype(np.uint8)
    p = rs.rand(C, H, W).astype(np.float32) + 0.05
    p[0, :, : W // 2] += 0.6                                   # class 0 on the left, class 1 on the right, noisy
    p[1, :, W // 2:] += 0.6
    p[3] = 1e-4                                                # class 3 nowhere likely
    p /= p.sum(0, keepdims=True)
    par = (10, 3, 1, 4, 67, 3)
    q = host(ops.dcrf_inference(dev(img, torch.uint8), dev(p), *par))
    np.testing.assert_allclose(q.sum(0), 1.0, atol=1e-5)
    assert q[3].max() < 1e-3
    # zero pairwise weights: the unary alone
    q0 = host(ops.dcrf_inference(dev(img, torch.uint8), dev(p), 5, 0.0, 1, 0.0, 67, 3))
    pc = np.clip(p, 1e-5, 1.0)
    assert maxabs(q0, pc / pc.sum(0, keepdims=True)) < 1e-6
    # label permutation
    perm = np.array([2, 0, 3, 1])
    qp = host(ops.dcrf_inference(dev(img, torch.uint8), dev(np.ascontiguousarray(p[perm])), *par))
    assert maxabs(qp, q[perm]) < 2e-6
    # smoothing inside the regions
    lab_in, lab_out = p.argmax(0), q.argmax(0)
    left_in, left_out = (lab_in[:, : W // 2 - 2] == 0).mean(), (lab_out[:, : W // 2 - 2] == 0).mean()
    right_in, right_out = (lab_in[:, W // 2 + 2:] == 1).mean(), (lab_out[:, W // 2 + 2:] == 1).mean()
    assert left_out >= left_in and right_out >= right_in and left_out > 0.99 and right_out > 0.99
    assert np.array_equal(q, host(ops.dcrf_inference(dev(img, torch.uint8), dev(p), *par)))


def test_dcrf_mirror_api(ops):
    """excel_amd.utils.dcrf keeps the reference module's surface (DenseCRF class, crf_inference, crf_inference_label) on numpy inputs."""
    from excel_amd.utils import dcrf
    rs = np.random.RandomState(2)
    H, W = 30, 41
    img = (rs.rand(H, W, 3) * 255).astype(np.uint8)
    p = rs.rand(4, H, W).astype(np.float32)
    q = dcrf.DenseCRF(iter_max=10, pos_w=3, pos_xy_std=1, bi_w=4, bi_xy_std=67, bi_rgb_std=3)(img, p)      # un-normalised "probabilities" like valid_lam
    assert isinstance(q, np.ndarray) and maxabs(q, oracle.dcrf.DenseCRF(10, 3, 1, 4, 67, 3)(img, p)) < 1e-3
    assert maxabs(dcrf.crf_inference(img, p / p.sum(0), t=3), oracle.dcrf.crf_inference(img, p / p.sum(0), t=3)) < 1e-3
    lab = rs.randint(0, 4, (H, W))
    assert np.mean(dcrf.crf_inference_label(img, lab, t=3, n_labels=4) == oracle.dcrf.crf_inference_label(img, lab, t=3, n_labels=4)) > 0.995


def test_confusion_unaligned_slices(ops):
    """gt / pred views that do not start on a 16-byte boundary (labels_u8[i], gts[lo:hi] of an odd-sized image): same
    misalignment -> scalar head + vector body; different misalignment -> scalar path.  Both equal fast_hist."""
    rs = np.random.RandomState(9)
    nc, n = 21, 5003
    gt = rs.randint(0, nc, n + 40).astype(np.uint8)
    gt[rs.rand(n + 40) < 0.05] = 255
    pr = rs.randint(0, nc, n + 40).astype(np.uint8)
    G, P = dev(gt), dev(pr)
    for og, op_ in ((3, 3), (5, 5), (1, 6), (0, 7), (13, 13)):
        hist = ops.confusion_accumulate(G[og:og + n], P[op_:op_ + n], nc)
        assert np.array_equal(host(hist), oracle.evaluate.fast_hist(gt[og:og + n], pr[op_:op_ + n], nc)), (og, op_)
    assert int(host(ops.confusion_accumulate(G[3:10], P[3:10], nc)).sum()) == int((gt[3:10] < nc).sum())     # shorter than the head


def test_confusion_golden(ops, golden):
    g = golden("ops.npz")
    gts = g["sc_gts"].astype(np.int64)
    gts[gts == 255] = 255
    hist = None
    for gt, pr in zip(gts, g["sc_preds"]):
        hist = ops.confusion_accumulate(dev(gt.astype(np.uint8)), dev(pr.astype(np.uint8)), 21, hist)
    assert np.array_equal(host(hist), g["sc_hist"])


# ------------------------------------------------------------------ bf16x3 mode (split-bf16 operands, 3 MFMAs / product)
def _bf16_round(x):
    u = np.asarray(x, np.float32).view(np.uint32).astype(np.uint64)
    r = ((u >> 16) & 1) + 0x7FFF
    return (((u + r) & 0xFFFF0000).astype(np.uint32)).view(np.float32)


def _unsplit(t):
    """split tensor [R,2,K] (int16 view) -> (hi, lo) fp32 [R,K]; layout: per block of 32 k, 32 hi then 32 lo."""
    R = t.shape[0]
    K = t.shape[2]
    u = t.reshape(R, K // 32, 2, 32).view(np.uint16).astype(np.uint32) << 16
    f = u.view(np.float32)
    return f[:, :, 0, :].reshape(R, K), f[:, :, 1, :].reshape(R, K)


def test_split_bf16_format(ops):
    rs = np.random.RandomState(0)
    x = (rs.standard_normal((37, 96)) * np.exp(rs.uniform(-20, 20, (37, 96)))).astype(np.float32)
    hi, lo = _unsplit(host(ops.split_bf16(dev(x))))
    ref_hi = _bf16_round(x)
    assert np.array_equal(hi, ref_hi)
    assert np.array_equal(lo, _bf16_round(x - ref_hi))
    assert np.max(np.abs((hi.astype(np.float64) + lo) - x) / np.abs(x)) < 2.0 ** -16


@pytest.mark.parametrize("M,N,K", [(128, 128, 32), (300, 64, 512), (785, 2304, 768), (37, 64, 128), (257, 768, 3072), (2100, 384, 96)])
def test_gemm_bf16x3(ops, M, N, K):
    rs = np.random.RandomState(M + N)
    A = rs.standard_normal((M, K)).astype(np.float32)
    W = (rs.standard_normal((N, K)) * 0.05).astype(np.float32)
    bias = rs.standard_normal(N).astype(np.float32)
    res = rs.standard_normal((M, N)).astype(np.float32)
    ref = A.astype(np.float64) @ W.T.astype(np.float64)
    As, Ws = ops.split_bf16(dev(A)), ops.split_bf16(dev(W))
    out = host(ops.gemm_bf16x3(As, Ws))
    scale = np.sqrt(K) * 0.05
    assert maxabs(out, ref) < 3e-5 * scale            # ~2^-17 per product, random accumulation
    y = ref + bias
    y = y * (1.0 / (1.0 + np.exp(-1.702 * y))) + res
    out2 = host(ops.gemm_bf16x3(As, Ws, bias=dev(bias), residual=dev(res), act=1))
    assert maxabs(out2, y) < 3e-5 * scale + 2e-6
    # split output == split of the fp32 output
    hi, _ = _unsplit(host(ops.gemm_bf16x3(As, Ws, split_out=True)))
    assert np.array_equal(hi, _bf16_round(out))


def _plan(ops, M, N, K, **kw):
    """The kernel instance the split-plane GEMM launcher picks for this problem on this device (host arithmetic, ops.gemm_plan)."""
    return ops.gemm_plan(M, N, K, torch.cuda.get_device_properties(0).multi_processor_count, **kw)


@pytest.mark.parametrize("M,N,K", [(25120, 768, 768), (25120, 2304, 768), (25120, 3072, 768), (25120, 768, 3072), (12560, 3072, 768),
                                   (12560, 768, 768), (25120, 512, 768), (12560, 2304, 768), (12560, 768, 3072), (16400, 768, 768),
                                   (16400, 3072, 768), (12500, 776, 896)])
def test_gemm_bf16x3_bench_shapes(ops, M, N, K):
    """The GEMM instances the benchmark configurations actually run (B = 32 / 16 at 448^2: M = B * 785; B = 16 at 512^2: M = 16 400): the
    four-wave kernel gemm_w4.hip in its 320-row (M = 25 120 with N = 768), 160-row (M = 12 560 with N = 768: 237 tiles) and 256-row
    (M = 16 400, N = 768: 195 tiles) instances, and one or two of its instances for the other shapes - proj, QKV, fc1, fc2, the final
    projection, and one ragged shape (M, N not multiples of the tile, K % 128 == 0) - against a float64 product, plain and with bias +
    QuickGELU + residual, and with the split output (whose residual form runs on the 8-wave tiles).  The plans are asserted."""
    plan = _plan(ops, M, N, K)
    if N == 768 and M in (12560, 16400, 25120):
        nt_m, tiles = {12560: (5, 237), 16400: (8, 195), 25120: (10, 237)}[M]
        assert plan["kernel"] == "w4" and plan["nt_m"] == nt_m and plan["grid_x"] == tiles, plan
    else:
        assert plan["kernel"] in ("w4", "w4_mix"), plan
    if N % 32 == 0:
        assert _plan(ops, M, N, K, out="split", residual=True)["kernel"] in ("8wave", "8wave_mixed")
    rs = np.random.RandomState(M % 1000 + N + K)
    A = rs.standard_normal((M, K)).astype(np.float32)
    W = (rs.standard_normal((N, K)) * 0.05).astype(np.float32)
    bias = rs.standard_normal(N).astype(np.float32)
    res = rs.standard_normal((M, N)).astype(np.float32)
    ref = A.astype(np.float64) @ W.T.astype(np.float64)
    As, Ws = ops.split_bf16(dev(A)), ops.split_bf16(dev(W))
    out = host(ops.gemm_bf16x3(As, Ws))
    scale = np.sqrt(K) * 0.05
    assert maxabs(out, ref) < 3e-5 * scale
    y = ref + bias
    y = y * (1.0 / (1.0 + np.exp(-1.702 * y))) + res
    out2 = host(ops.gemm_bf16x3(As, Ws, bias=dev(bias), residual=dev(res), act=1))
    assert maxabs(out2, y) < 3e-5 * scale + 2e-6
    if N % 32 == 0:
        hi, lo = _unsplit(host(ops.gemm_bf16x3(As, Ws, split_out=True)))
        assert np.array_equal(hi, _bf16_round(out)) and np.array_equal(lo, _bf16_round(out - hi))
        # the fc1 form (bias + QuickGELU, split output: the stage-wise packed QuickGELU of the four-wave epilogue) must carry the bits of the
        # plain-output launch of the same problem, and residual + split output (which the four-wave kernel hands to the 8-wave one) those
        # of the plain residual launch: every instance and every output mode computes the same values
        g_plain = host(ops.gemm_bf16x3(As, Ws, bias=dev(bias), act=1))
        hi, lo = _unsplit(host(ops.gemm_bf16x3(As, Ws, bias=dev(bias), act=1, split_out=True)))
        assert np.array_equal(hi, _bf16_round(g_plain)) and np.array_equal(lo, _bf16_round(g_plain - hi))
        assert maxabs(g_plain, y - res) < 3e-5 * scale + 2e-6
        hi, lo = _unsplit(host(ops.gemm_bf16x3(As, Ws, bias=dev(bias), residual=dev(res), act=1, split_out=True)))
        assert np.array_equal(hi, _bf16_round(out2)) and np.array_equal(lo, _bf16_round(out2 - hi))


@pytest.mark.parametrize("M,N,K", [(25120, 1001, 64), (12560, 2302, 64), (25120, 770, 96)])
def test_gemm_bf16x3_scalar_epilogue_big_tiles(ops, M, N, K):
    """N not a multiple of 4 sends the big tiles (256 / 320 rows, mixed-height row tiles included) through the scalar epilogue
    (round-4 advisor finding: a short 256-row tile of the mixed-height launch stored wave row 1 thirty-two rows too low and wrote
    bias-only values into the next row tile).  Plain and bias + QuickGELU + residual, against a float64 product."""
    rs = np.random.RandomState(N)
    A = rs.standard_normal((M, K)).astype(np.float32)
    W = (rs.standard_normal((N, K)) * 0.05).astype(np.float32)
    bias = rs.standard_normal(N).astype(np.float32)
    res = rs.standard_normal((M, N)).astype(np.float32)
    ref = A.astype(np.float64) @ W.T.astype(np.float64)
    As, Ws = ops.split_bf16(dev(A)), ops.split_bf16(dev(W))
    tol = 4e-5                                           # outputs ~N(0, 0.4^2), 2^-17 per product; max over 25 M entries measured 1.5e-5
    out = host(ops.gemm_bf16x3(As, Ws))
    assert out.shape == (M, N) and maxabs(out, ref) < tol
    y = ref + bias
    y = y * (1.0 / (1.0 + np.exp(-1.702 * y))) + res
    out2 = host(ops.gemm_bf16x3(As, Ws, bias=dev(bias), residual=dev(res), act=1))
    assert maxabs(out2, y) < tol


@pytest.mark.timeout(300)
@pytest.mark.parametrize("M,N,K,mode", [(12560, 768, 768, "bf16x3"), (16400, 768, 768, "bf16x3"), (25120, 768, 768, "bf16x3"),
                                        (12560, 768, 768, "f16x2"), (12560, 2304, 768, "f16x2"), (16400, 3072, 768, "bf16x3")])
def test_gemm_bf16x3_with_neighbours_on_other_streams(ops, M, N, K, mode):
    """The four-wave GEMM instances (160- / 256- / 320-row tiles for these shapes) while ANOTHER kernel's waves share their CUs: the 160- and
    256-row instances leave registers and LDS for a neighbour, and with one the timing of their LDS reads changes.  Round 5 found the
    kernel's post-loop wait scheduled BEHIND the epilogue's lane-id computation - whose register was still the destination of an in-flight
    ds_read: a garbage lane id and wild addresses, only under such a neighbour (memory fault in `bench.py --split 2`).  Two GEMM streams + a
    LayerNorm stream, every result bit-identical to the serial launch."""
    # (round 6: the same with the two-product kernels - "f16x2" - and with launches made of two instances: N = 2304 / 3072)
    f16 = mode == "f16x2"
    for kw in (dict(residual=True), dict(out="split")):
        plan = _plan(ops, M, N, K, mode=mode, half=f16, **kw)
        assert plan["kernel"] == ("w4" if N == 768 else "w4_mix") and plan["x2"] == (2 if f16 else 0), plan
        if N == 768:
            assert plan["nt_m"] == {12560: 5, 16400: 8, 25120: 10}[M], plan
    g = torch.Generator(device="cuda").manual_seed(M)
    As = [ops.split_bf16(torch.randn(M, K, device="cuda", generator=g), f16=f16) for _ in range(2)]
    Wf = (torch.randn(N, K, device="cuda", generator=g) * 0.05).half().float()
    W = ops.split_bf16(Wf, f16=f16)
    Wh = ops.pack_f16(Wf)[0] if f16 else None
    bias = torch.randn(N, device="cuda", generator=g)
    res = torch.randn(M, N, device="cuda", generator=g)
    _ops = ops

    class _G:                                   # the mode's GEMM behind the name the body below uses
        @staticmethod
        def gemm_bf16x3(a, w, **kw):
            return _ops.gemm_f16x2(a, w, Wh, **kw) if f16 else _ops.gemm_bf16x3(a, w, **kw)
        layernorm = staticmethod(_ops.layernorm)
    ops = _G
    ref = [ops.gemm_bf16x3(a, W, bias=bias, residual=res, act=1) for a in As]
    refs = [ops.gemm_bf16x3(a, W, bias=bias, split_out=True).clone() for a in As]
    x = torch.randn(25120, 768, device="cuda", generator=g)
    lw, lb = torch.ones(768, device="cuda"), torch.zeros(768, device="cuda")
    torch.cuda.synchronize()
    streams = [torch.cuda.Stream() for _ in range(3)]
    for rep in range(3):
        outs = [[], []]
        for i in (0, 1):
            with torch.cuda.stream(streams[i]):
                for _ in range(6):
                    outs[i].append(ops.gemm_bf16x3(As[i], W, bias=bias, residual=res, act=1))
                    outs[i].append(ops.gemm_bf16x3(As[i], W, bias=bias, split_out=True))
        with torch.cuda.stream(streams[2]):
            for _ in range(16):
                ops.layernorm(x, lw, lb)
        torch.cuda.synchronize()
        for i in (0, 1):
            for j, o in enumerate(outs[i]):
                assert torch.equal(o, refs[i] if j % 2 else ref[i]), (rep, i, j)


@pytest.mark.parametrize("sharp", [1.6, 2.0])
def test_vit_b16_448_clip_like_outlier_net(ops, sharp):
    """Full-size ViT-B/16 @448 on a CLIP-LIKE STRESS NET (oracle.vit.make_vit_weights(outliers=True): 3-6 massive-activation channels at
    50-100x the rest of the residual stream, log-normal LayerNorm gains, peaked attention rows) instead of the benign random net of the
    other tests.  The judge of all three - the fp32 oracle, the exact-fp32 GPU mode, the default bf16x3 mode - is the SAME restatement
    run in float64 (oracle.vit.precision), because in this regime fp32 arithmetic has a visible error of its own.
      sharp 1.6  peaked rows; the fp32 oracle is 3e-5 (CAM) off float64.  ALL THREE GPU modes hold the north-star gate (CAM <= 1e-3): the
                 exact mode and f16x3 (IEEE-half planes, 22 bits) stay within 3x the fp32 oracle's own deviation (measured 0.9x / 1.5x);
                 bf16x3 (16 mantissa bits per operand) measures ~12x.
      sharp 2.0  every head near one-hot; the fp32 oracle itself is 2e-4 off.  The exact mode and f16x3 still hold the gate (1.6e-4 /
                 2.3e-4); bf16x3 does NOT (2.6e-3) - which is what ExCEL_model.check_numerics / infer_lam --gemm_check exist for: the
                 difference between a fast mode and the exact one exposes it on the user's own weights and the run moves down the ladder
                 bf16x3 -> f16x3 -> f32 (tested at the end: it lands on f16x3)."""
    cfg = VitConfig(width=768, layers=12, heads=12, patch=16, out_dim=512, input_resolution=224, n_surgery=5)
    w = make_vit_weights(cfg, seed=1, attn_gain=2.0, outliers=True, sharp=sharp)
    imgs = np.random.RandomState(4).standard_normal((1, 3, 448, 448)).astype(np.float32)
    text = np.random.RandomState(8).standard_normal((45, 512)).astype(np.float32)
    text /= np.linalg.norm(text, axis=1, keepdims=True)

    def cam_of(x, dt):
        f = x / np.sqrt((x * x).sum(axis=1, keepdims=True))
        return f, oracle.cam.clip_feature_surgery(f.astype(dt), text.astype(dt))

    with oracle.vit.precision(np.float64):
        x64, attn64, feats64 = oracle.vit.vit_forward(imgs.astype(np.float64), {k: np.asarray(v, np.float64) for k, v in w.items()}, cfg)
        assert x64.dtype == np.float64
    resid = np.abs(feats64[-1]).max(axis=(0, 1))
    assert np.sort(resid)[-3] > 10 * np.median(resid) and np.sort(resid)[-3] > 40 * np.median(np.abs(feats64[-1]))   # the stress regime is there
    f64, cam64 = cam_of(x64, np.float64)
    aff64 = attn64[-6:, :, 1:, 1:].mean(0)
    x32, attn32, _ = oracle.vit.vit_forward(imgs, w, cfg)
    f32_, cam32 = cam_of(x32, np.float32)
    o_feat, o_aff, o_cam = relmax(f32_, f64), relmax(attn32[-6:, :, 1:, 1:].mean(0, dtype=np.float32), aff64), maxabs(cam32, cam64)
    print(f"outlier net sharp {sharp}, fp32 oracle vs float64: feature rel err {o_feat:.2e}, w_aff rel err {o_aff:.2e}, CAM max-abs err {o_cam:.2e}")
    err = {}
    for mode in ("f32", "f16x3", "bf16x3"):
        h = make_handle(ops, cfg, w, mode=mode)
        r = h.forward(dev(imgs), want_w_aff=True, n_attn_out=6, want_raw=True)
        e_feat = relmax(host(r["image_features"]), f64)
        e_aff = relmax(host(r["w_aff"]), aff64)
        full, _ = ops.clip_feature_surgery(r["image_features"], dev(text), num_fg=20)
        e_cam = maxabs(host(full), cam64)
        err[mode] = (e_feat, e_aff, e_cam)
        print(f"outlier net sharp {sharp}, GPU {mode} vs float64: feature rel err {e_feat:.2e}, w_aff rel err {e_aff:.2e}, CAM max-abs err {e_cam:.2e}")
        del h
    for mode in ("f32", "f16x3"):
        e_feat, e_aff, e_cam = err[mode]
        assert e_cam < 1e-3 and e_aff < max(5e-4, 3 * o_aff) and e_feat < max(5e-4, 3 * o_feat), mode
    if sharp <= 1.6:
        assert err["bf16x3"][2] < 1e-3                                  # the north-star gate holds in the default mode
        assert err["bf16x3"][2] < 40 * max(o_cam, 1e-6)                 # ... at its known distance from fp32 arithmetic (~14x)
    # the self-check a user runs on his own weights (no float64 at hand): bf16x3 against the exact mode
    from excel_amd.model import ExCEL_model
    model = ExCEL_model(clip_model="ExCEL_ViT-B/16", num_classes=21, img_size=448, mode="train", state_dict=w,
                        text_attr=np.ascontiguousarray(text.T), gemm_mode="bf16x3")
    res = model.check_numerics(dev(imgs), tol=5e-4)
    print(f"outlier net sharp {sharp}: check_numerics {res}")
    if sharp <= 1.6:
        assert res["max_abs_diff"] < 5e-4 and res["mode_after"] == "bf16x3"
    else:
        assert err["bf16x3"][2] > 1e-3                                  # (if this ever passes, tighten the comment above)
        assert res["max_abs_diff"] > 5e-4 and res["mode_after"] == "f16x3" and model.encoder.visual.handle().gemm_mode() == "f16x3"
        assert res["ladder"][1][0] == "f16x3" and res["ladder"][1][1] < 5e-4


def test_baseline_batch16_vit_cam(ops):
    """BASELINE configs[1] on its own terms: 448x448, batch 16, ViT-B/16 surgery forward + patch-text CAM only (the GEMM tile the
    launcher picks for M = 16 * 785 differs from B = 32's).  Batch invariance bit for bit against B = 1 for three of the 16 images,
    the oracle on two of them (CAM gate 1e-3)."""
    from excel_amd.model import ExCEL_model
    from excel_amd.tools import synthetic
    sd = synthetic.make_vit_state_dict(seed=0)
    text = synthetic.make_text_features(45)
    model = ExCEL_model(clip_model="ExCEL_ViT-B/16", num_classes=21, img_size=448, mode="train", state_dict=sd, text_features=text)
    ds = synthetic.SyntheticSegDataset(16, (448, 448), seed=555)
    _, imgs, _, _ = ds.batch(range(16))
    x = dev(imgs)
    _, _, attr, attn_w, _ = model(x)
    assert attr.shape == (16, 784, 20)
    for b in (0, 7, 15):
        _, _, a1, w1, _ = model(x[b:b + 1])
        assert torch.equal(a1[0], attr[b]) and torch.equal(w1.w_aff[0], attn_w.w_aff[b])
    cfg = VitConfig(width=768, layers=12, heads=12, patch=16, out_dim=512, input_resolution=224, n_surgery=5)
    wo = oracle.vit.reload_self_attn({k: np.asarray(v) for k, v in sd.items()}, cfg, 28, "train")
    text_attr = host(model.text_attr)
    for b in (3, 12):
        f_ref, _, _ = oracle.cam.generate_clip_fts(imgs[b:b + 1], wo, cfg)
        cam = oracle.cam.clip_feature_surgery(f_ref, text_attr.T.copy())[:, 1:, :20]
        assert maxabs(host(attr[b]), cam[0]) < 1e-3


def test_par_uniform_narrow_images(ops):
    """The recomputing PAR tile kernel on UNIFORM batches narrower than 8 pixels (W = 4: the pitch the ragged path already runs it at):
    same results as the oracle and as the streamed-affinity kernel (EXCEL_PAR_STREAM_AFFINITIES)."""
    rs = np.random.RandomState(23)
    for (H, W) in ((9, 4), (33, 4), (5, 8)):
        img = rs.standard_normal((2, 3, H, W)).astype(np.float32)
        masks = rs.rand(2, 3, H, W).astype(np.float32)
        out = ops.par_forward(dev(img), dev(masks), num_iter=3)
        ref = oracle.par.PAR([1, 2, 4, 8, 12, 24], 3)
        for b in range(2):
            assert maxabs(host(out)[b], ref(img[b:b + 1], masks[b:b + 1])[0]) < 5e-5, (H, W)
        streamed = ops.par_forward(dev(img), dev(masks), num_iter=3, stream_affinities=True)
        assert torch.equal(out, streamed), (H, W)


def test_vit_b16_448_outlier_net_checkpoint_like_weights_start_in_f16x2(ops):
    """The extreme stress net of the test above (sharp 2.0: every head near one-hot, where bf16x3 exceeds the 1e-3 gate) with its weights
    rounded through IEEE half - the form every published CLIP archive has (clip/build_model.py:72).  A model built on such weights starts
    in f16x2 BY ITSELF and that mode holds the gate against a float64 run of the oracle on the same weights, within 3x the fp32 oracle's own
    deviation; the start-up check keeps it (no fall-back needed): on real checkpoints the fast default is the accurate mode."""
    cfg = VitConfig(width=768, layers=12, heads=12, patch=16, out_dim=512, input_resolution=224, n_surgery=5)
    w = {k: np.asarray(v, np.float32).astype(np.float16).astype(np.float32) for k, v in make_vit_weights(cfg, seed=1, attn_gain=2.0, outliers=True, sharp=2.0).items()}
    imgs = np.random.RandomState(4).standard_normal((1, 3, 448, 448)).astype(np.float32)
    text = np.random.RandomState(8).standard_normal((45, 512)).astype(np.float32)
    text /= np.linalg.norm(text, axis=1, keepdims=True)

    def cam_of(x, dt):
        f = x / np.sqrt((x * x).sum(axis=1, keepdims=True))
        return oracle.cam.clip_feature_surgery(f.astype(dt), text.astype(dt))

    with oracle.vit.precision(np.float64):
        x64, _, _ = oracle.vit.vit_forward(imgs.astype(np.float64), {k: np.asarray(v, np.float64) for k, v in w.items()}, cfg)
    cam64 = cam_of(x64, np.float64)
    x32, _, _ = oracle.vit.vit_forward(imgs, w, cfg)
    o_cam = maxabs(cam_of(x32, np.float32), cam64)
    from excel_amd.model import ExCEL_model
    model = ExCEL_model(clip_model="ExCEL_ViT-B/16", num_classes=21, img_size=448, mode="train", state_dict=w, text_attr=np.ascontiguousarray(text.T))
    h = model.encoder.visual.handle()
    assert h.weights_fp16_exact() and h.gemm_mode() == "f16x2"
    r = h.forward(dev(imgs), want_raw=True)
    full, _ = ops.clip_feature_surgery(r["image_features"], dev(text), num_fg=20)
    e_cam = maxabs(host(full), cam64)
    print(f"checkpoint-like outlier net (sharp 2.0): fp32 oracle vs float64 CAM {o_cam:.2e}, GPU f16x2 vs float64 CAM {e_cam:.2e}")
    assert e_cam < 1e-3 and e_cam < max(5e-4, 3 * o_cam)
    res = model.check_numerics(dev(imgs), tol=5e-4)
    assert res["mode_before"] == res["mode_after"] == "f16x2" and res["max_abs_diff"] < 5e-4


def _unsplit_f16(t):
    """split tensor [R,2,K] (int16 view) with IEEE-half planes -> (hi, lo) fp32 [R,K]."""
    R, K = t.shape[0], t.shape[2]
    f = t.reshape(R, K // 32, 2, 32).view(np.float16).astype(np.float32)
    return f[:, :, 0, :].reshape(R, K), f[:, :, 1, :].reshape(R, K)


@pytest.mark.parametrize("M,N,K", [(300, 64, 512), (785, 2304, 768), (25120, 768, 768), (12560, 3072, 768), (12560, 768, 768), (16400, 768, 768)])
def test_gemm_f16x3(ops, M, N, K):
    """The split-plane building blocks with IEEE-half planes ("f16x3"): hi = half(x), lo = half(x - hi) exactly as numpy rounds them, and
    the three-MFMA product against float64 - 22 mantissa bits instead of bf16x3's 16: the bound is 16x tighter."""
    rs = np.random.RandomState(M % 1000 + N + K + 1)
    A = rs.standard_normal((M, K)).astype(np.float32)
    W = (rs.standard_normal((N, K)) * 0.05).astype(np.float32)
    bias = rs.standard_normal(N).astype(np.float32)
    res = rs.standard_normal((M, N)).astype(np.float32)
    As, Ws = ops.split_bf16(dev(A), f16=True), ops.split_bf16(dev(W), f16=True)
    hi, lo = _unsplit_f16(host(As))
    ref_hi = A.astype(np.float16).astype(np.float32)
    assert np.array_equal(hi, ref_hi) and np.array_equal(lo, (A - ref_hi).astype(np.float16).astype(np.float32))
    ref = A.astype(np.float64) @ W.T.astype(np.float64)
    scale = np.sqrt(K) * 0.05
    out = host(ops.gemm_bf16x3(As, Ws, f16=True))
    assert maxabs(out, ref) < 5e-6 * scale + 2e-6          # (bf16x3: 3e-5 * scale; the weights' lo planes are denormal halves: ~19 bits)
    y = ref + bias
    y = y * (1.0 / (1.0 + np.exp(-1.702 * y))) + res
    out2 = host(ops.gemm_bf16x3(As, Ws, bias=dev(bias), residual=dev(res), act=1, f16=True))
    assert maxabs(out2, y) < 5e-6 * scale + 4e-6
    hi2, lo2 = _unsplit_f16(host(ops.gemm_bf16x3(As, Ws, split_out=True, f16=True)))
    h16 = out.astype(np.float16).astype(np.float32)
    assert np.array_equal(hi2, h16) and np.array_equal(lo2, (out - h16).astype(np.float16).astype(np.float32))      # (four-wave kernel: split_pair)


@pytest.mark.parametrize("M,N,K", [(300, 64, 512), (785, 2304, 768), (2100, 384, 96), (25120, 768, 768), (25120, 2304, 768), (25120, 3072, 768),
                                   (25120, 768, 3072), (25120, 512, 768), (12560, 768, 768), (12560, 3072, 768), (16400, 768, 768),
                                   (16400, 3072, 768), (12500, 776, 896), (12560, 768, 832)])
def test_gemm_f16x2_equals_f16x3_bitwise(ops, M, N, K):
    """"f16x2": fp16-VALUED weights (what every published CLIP archive holds, clip/build_model.py:72) have an all-zero lo plane, so the
    a.hi x w.lo pass of the three-product scheme multiplies zeros and the two-product kernels leave it out.  Adding exact zeros to an fp32
    accumulator changes nothing: every instance (the four-wave kernel on the compact half weights - 320- / 256- / 160-row tiles -, the
    four-wave kernel on split-layout weights, the 8-wave tiles for small / ragged shapes; K = 832 is not a multiple of 128: no compact
    instance) and every epilogue mode must reproduce the f16x3 result BIT FOR BIT, and the f16x3 result is checked against float64."""
    rs = np.random.RandomState(M % 1000 + N + K + 2)
    A = rs.standard_normal((M, K)).astype(np.float32)
    W = (rs.standard_normal((N, K)) * 0.05).astype(np.float16).astype(np.float32)            # fp16-valued
    bias = rs.standard_normal(N).astype(np.float32)
    res = rs.standard_normal((M, N)).astype(np.float32)
    As, Ws = ops.split_bf16(dev(A), f16=True), ops.split_bf16(dev(W), f16=True)
    _, wlo = _unsplit_f16(host(Ws))
    assert not wlo.any()                                                                     # the precondition, seen in the planes
    Wh, inexact = ops.pack_f16(dev(W))
    assert inexact == 0 and np.array_equal(host(Wh).view(np.float16).astype(np.float32), W)
    ref = A.astype(np.float64) @ W.T.astype(np.float64)
    db, dr = dev(bias), dev(res)
    forms = [dict(), dict(bias=db, residual=dr, act=1), dict(bias=db, residual=dr)]
    if N % 32 == 0:
        forms += [dict(split_out=True), dict(bias=db, act=1, split_out=True), dict(bias=db, residual=dr, act=1, split_out=True)]
    for kw in forms:
        x3 = ops.gemm_bf16x3(As, Ws, f16=True, **kw)
        for wh in (None, Wh):
            x2 = ops.gemm_f16x2(As, Ws, wh, **kw)
            assert torch.equal(x2, x3), (kw.keys(), wh is not None)
    out = host(ops.gemm_f16x2(As, Ws, Wh))
    assert maxabs(out, ref) < 1e-5 * np.sqrt(K) * 0.05 + 2e-6          # (K = 3072: 2.1e-5 measured, fp32 accumulation over 96 steps)


@pytest.mark.parametrize("M,N,K", [(16400, 3072, 768), (25120, 2304, 768), (12560, 2304, 768), (25120, 3072, 768), (14001, 2000, 768)])
def test_gemm_two_instance_launch_equals_row_slices(ops, M, N, K):
    """Round 6: for these shapes the launcher makes ONE launch of two instances of the four-wave GEMM (full rounds of 320-row tiles, the rest in
    256- / 160-row tiles: gemm_w4_kernel_mix / gemm_w4x2_kernel_mix).  Every output element is accumulated in the same k order whatever
    instance computes it, so the launch must equal, BIT FOR BIT, the same problem computed as row slices of other heights (which the launcher
    runs on other instances: a 4 000-row slice takes the 8-wave / short tiles) - for bf16x3, f16x3 and f16x2, plain / bias + QuickGELU + split /
    bias + residual."""
    rs = np.random.RandomState(M % 997 + N)
    A = rs.standard_normal((M, K)).astype(np.float32)
    W = (rs.standard_normal((N, K)) * 0.05).astype(np.float16).astype(np.float32)
    bias = dev(rs.standard_normal(N).astype(np.float32))
    res = dev(rs.standard_normal((M, N)).astype(np.float32))
    cuts = [0, 4000, 4000 + 7520, M]
    Wh, _ = ops.pack_f16(dev(W))
    for name in ("bf16x3", "f16x3", "f16x2"):
        f16 = name != "bf16x3"
        As, Ws = ops.split_bf16(dev(A), f16=f16), ops.split_bf16(dev(W), f16=f16)
        def run(a_split, r, **kw):
            if name == "f16x2":
                return ops.gemm_f16x2(a_split, Ws, Wh, residual=r, **kw)
            return ops.gemm_bf16x3(a_split, Ws, residual=r, f16=f16, **kw)
        # (14001 x 2000: a ragged last row AND column tile - 32 x 160 + 160-row tiles by the model -, N % 32 != 0: no split output)
        for kw, use_res in ((dict(), False), (dict(bias=bias, act=1, split_out=N % 32 == 0), False), (dict(bias=bias), True)):
            form = dict(mode=name, half=name == "f16x2", out="split" if kw.get("split_out") else "plain", residual=use_res)
            assert _plan(ops, M, N, K, **form)["kernel"] == "w4_mix", (name, form)
            short = _plan(ops, 4000, N, K, **form)
            assert short["kernel"] == "8wave" or (short["kernel"] == "w4" and short["nt_m"] in (8, 5)), (name, form, short)
            whole = run(As, res if use_res else None, **kw)
            for lo, hi in zip(cuts[:-1], cuts[1:]):
                part = run(As[lo:hi].contiguous(), res[lo:hi].contiguous() if use_res else None, **kw)
                assert torch.equal(whole[lo:hi], part), (name, kw.keys(), lo, hi)


def test_pack_f16_counts_inexact_values(ops):
    """excel_pack_f16's counter: 0 exactly for fp16-valued matrices; every value with a non-zero lo plane (and a NaN) counts."""
    rs = np.random.RandomState(5)
    W = rs.standard_normal((96, 64)).astype(np.float16).astype(np.float32)
    assert ops.pack_f16(dev(W))[1] == 0
    W2 = W.copy()
    W2[3, 5] += 2.0 ** -14
    W2[7, 0] = 1.0e5                   # beyond the half range
    W2[9, 9] = np.nan
    assert ops.pack_f16(dev(W2))[1] == 3
    assert ops.pack_f16(dev(rs.standard_normal((96, 64)).astype(np.float32)))[1] > 6000


def test_split_f16_overflow_is_loud(ops):
    """IEEE-half planes have a range of 65 504.  Inside it the split is the plain round-to-nearest pair; beyond it hi becomes +-inf and
    lo the opposite infinity, so every product the value enters is a NaN - an overflow of the f16 modes cannot pass as a finite wrong
    number (ExCEL_model.check_numerics treats NaN as a failed rung and moves to exact fp32); a NaN input stays NaN in both planes;
    bf16 planes are unaffected (fp32 range).  (Rounds 4-5 saturated instead, at three times the VALU cost per value.)"""
    x = np.array([[7.0e4, -1.2e5, 6.0e4, np.nan, 65504.0] + [1.0] * 27], np.float32)
    hi, lo = _unsplit_f16(host(ops.split_bf16(dev(x), f16=True)))
    assert hi[0, 0] == np.inf and lo[0, 0] == -np.inf and hi[0, 1] == -np.inf and lo[0, 1] == np.inf
    assert abs((hi + lo)[0, 2] - 6.0e4) <= 1 and hi[0, 4] == 65504.0 and lo[0, 4] == 0.0
    assert np.isnan(hi[0, 3]) and np.isnan(lo[0, 3])
    assert np.array_equal(hi[0, 5:], np.ones(27, np.float32)) and not lo[0, 5:].any()
    # the product of an overflowing row is NaN, the rows next to it are untouched
    A = np.ones((64, 32), np.float32)
    A[3, 7] = 1.0e5
    W = np.full((64, 32), 0.5, np.float32)
    out = host(ops.gemm_bf16x3(ops.split_bf16(dev(A), f16=True), ops.split_bf16(dev(W), f16=True), f16=True))
    assert np.all(np.isnan(out[3])) and np.array_equal(np.delete(out, 3, 0), np.full((63, 64), 16.0, np.float32))
    xb = np.where(np.isnan(x), np.float32(1.0), x)
    hb, lb = _unsplit(host(ops.split_bf16(dev(xb))))
    assert np.max(np.abs((hb.astype(np.float64) + lb) - xb) / np.abs(xb)) < 2.0 ** -16


def test_vit_b16_448_bf16x3_mode(ops):
    """Same BASELINE-shape check as the fp32 test, with the linear layers on the bf16x3 path: the CAM gate (1e-3)
    must hold with a wide margin (measured ~1e-5)."""
    cfg = VitConfig(width=768, layers=12, heads=12, patch=16, out_dim=512, input_resolution=224, n_surgery=5)
    w = make_vit_weights(cfg, seed=1, attn_gain=2.0)
    imgs = np.random.RandomState(4).standard_normal((1, 3, 448, 448)).astype(np.float32)
    h = make_handle(ops, cfg, w)
    h.set_gemm_mode("bf16x3")
    assert h.gemm_mode() == "bf16x3"
    r = h.forward(dev(imgs), want_w_aff=True, n_attn_out=6, want_raw=True)
    x, attn, _ = oracle.vit.vit_forward(imgs, w, cfg)
    f_ref, _, _ = oracle.cam.generate_clip_fts(imgs, w, cfg)
    e_feat = relmax(host(r["image_features"]), f_ref)
    e_aff = relmax(host(r["w_aff"]), attn[-6:, :, 1:, 1:].mean(0, dtype=np.float32))
    rs = np.random.RandomState(8)
    text = rs.standard_normal((45, 512)).astype(np.float32)
    text /= np.linalg.norm(text, axis=1, keepdims=True)
    full, _ = ops.clip_feature_surgery(r["image_features"], dev(text), num_fg=20)
    e_cam = maxabs(host(full), oracle.cam.clip_feature_surgery(f_ref, text))
    print(f"bf16x3: feature rel err {e_feat:.2e}, w_aff rel err {e_aff:.2e}, CAM max-abs err {e_cam:.2e}")
    assert e_feat < 5e-4 and e_aff < 5e-4
    assert e_cam < 1e-3
    assert e_cam < 2e-4
    h.set_gemm_mode("f32")
    r32 = h.forward(dev(imgs), want_raw=True)
    e32 = maxabs(host(ops.clip_feature_surgery(r32["image_features"], dev(text))[0]), oracle.cam.clip_feature_surgery(f_ref, text))
    print(f"f32   : CAM max-abs err {e32:.2e}")


def test_vit_tiny_bf16x3_mode_vs_golden(ops, golden):
    g = golden("vit_cam_tiny.npz")
    w = oracle.vit.reload_self_attn(make_vit_weights(TINY, seed=int(g["seed_w"])), TINY, feat_size=6, mode="train")
    h = make_handle(ops, TINY, w)
    h.set_gemm_mode("bf16x3")
    r = h.forward(dev(g["imgs"]), want_raw=True)
    full, _ = ops.clip_feature_surgery(r["image_features"], dev(g["train_text"]))
    assert maxabs(host(full), g["train_cam"]) < 1e-3


# ------------------------------------------------------------------ error conventions and degenerate inputs
def test_abi_error_conventions(ops):
    """C ABI: int status (0 ok, < 0 bad argument / launch failure) + excel_last_error(); Python raises RuntimeError with it."""
    import ctypes as C
    from excel_amd._lib import lib
    L = lib()
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    a = torch.zeros(8, 8, device="cuda")
    # K not a multiple of 4 in NT mode
    rc = L.excel_gemm_f32(a.data_ptr(), a.data_ptr(), a.data_ptr(), None, None, 8, 8, 7, 8, 8, 8, 0, 1, 0, 1, 0, 0, 0, 0, st)
    assert rc < 0 and b"multiple of 4" in L.excel_last_error()
    # null pointers
    assert L.excel_compute_trans_mat(None, 1, 36, a.data_ptr(), a.data_ptr(), st) < 0
    assert L.excel_par_forward(None, 8, 8, None, None, 1, 1, 8, 8, (C.c_int32 * 1)(1), 1, 1, 0.3, 0.01, None, None, 0, st) < 0
    # bad layer range
    assert L.excel_attn_layer_mean(a.data_ptr(), 2, 1, 4, 1, 5, a.data_ptr(), st) < 0 and b"layer" in L.excel_last_error()
    # a good call after failures returns 0 (errors are not sticky)
    assert L.excel_layernorm(a.data_ptr(), a[0].data_ptr(), a[0].data_ptr(), a.data_ptr(), 8, 8, 1e-5, st) == 0
    with pytest.raises(RuntimeError, match="head_dim|heads|width"):
        make_handle(ops, VitConfig(width=96, layers=2, heads=2, patch=16, out_dim=32, input_resolution=32, n_surgery=1),
                    make_vit_weights(VitConfig(width=96, layers=2, heads=2, patch=16, out_dim=32, input_resolution=32, n_surgery=1), seed=1)
                    ).forward(torch.zeros(1, 3, 32, 32, device="cuda"))
    with pytest.raises(RuntimeError, match="ndil"):
        ops.par_forward(torch.zeros(1, 3, 8, 8, device="cuda"), torch.zeros(1, 1, 8, 8, device="cuda"), dilations=(1,) * 9)


def test_degenerate_inputs_follow_the_reference(ops):
    """Silent-NaN conventions of the reference: a constant similarity column gives 0/0 in clip_feature_surgery's
    min-max (clip.py:308); scale_cam_image is eps-guarded (affutils.py:73); a zero row in the affinity gives NaN in Sinkhorn
    (affutils.py:11-12).  The oracle (numpy) produces the same patterns."""
    rs = np.random.RandomState(0)
    f = np.tile(rs.standard_normal((1, 1, 16)).astype(np.float32), (1, 10, 1))       # every token identical
    f /= np.linalg.norm(f, axis=1, keepdims=True)
    t = rs.standard_normal((3, 16)).astype(np.float32)
    with np.errstate(all="ignore"):
        ref = oracle.cam.clip_feature_surgery(f, t)                                      # every column constant -> (x - min) / 0
    got = host(ops.clip_feature_surgery(dev(f), dev(t))[0])
    assert np.isnan(ref).all() and np.array_equal(np.isnan(got), np.isnan(ref))
    # constant refined map -> eps-guarded min-max -> zeros, background 1
    refined = np.full((1, 1, 36), 0.25, np.float32)
    cams = host(ops.cam_upsample_bkg(dev(refined), dev(np.array([1]), torch.int32), 6, 12, 12))
    assert np.allclose(cams[0, 0], 1.0) and np.allclose(cams[0, 1], 0.0)
    # zero row -> NaN through the row/column normalisation, like the reference's plain divisions
    a = (rs.rand(1, 36, 36).astype(np.float32) + 0.1)
    a[0, 5, :] = 0
    a[0, :, 5] = 0
    with np.errstate(all="ignore"):
        tref = oracle.aff.compute_trans_mat(a[0])
    tgot = host(ops.compute_trans_mat(dev(a)))[0]
    assert np.isnan(tref).any() and np.array_equal(np.isnan(tgot), np.isnan(tref))


def test_denormalize_img(ops):
    """utils/imutils.py:11-25 restated: v = img*std + mean, float -> uint8 truncation; img2 = that / 255."""
    from excel_amd.utils import imutils
    rs = np.random.RandomState(1)
    mean, std = np.array([123.675, 116.28, 103.53], np.float32), np.array([58.395, 57.12, 57.375], np.float32)
    u8 = rs.randint(0, 256, (2, 3, 9, 13)).astype(np.float32)
    x = ((u8 + 0.4) - mean[None, :, None, None]) / std[None, :, None, None]          # decodes back to u8 + 0.4 -> truncates to u8
    got = host(imutils.denormalize_img(dev(x.astype(np.float32))))
    ref = (x.astype(np.float32) * std[None, :, None, None] + mean[None, :, None, None]).astype(np.uint8)
    assert got.dtype == np.uint8 and np.array_equal(got, ref)
    got2 = host(imutils.denormalize_img2(dev(x.astype(np.float32))))
    assert np.allclose(got2, ref.astype(np.float32) / 255.0, atol=1e-7)


def test_normalize_img_u8(ops):
    """datasets/transforms.normalize_img followed by the HWC->CHW transpose (datasets/voc.py:115-116), bit-exact vs numpy."""
    rs = np.random.RandomState(2)
    img = rs.randint(0, 256, (2, 11, 7, 3)).astype(np.uint8)
    mean, std = [123.675, 116.28, 103.53], [58.395, 57.12, 57.375]
    ref = np.empty(img.shape, np.float32)
    for c in range(3):
        ref[..., c] = (img[..., c] - mean[c]) / std[c]
    ref = ref.transpose(0, 3, 1, 2)
    got = host(ops.normalize_img_u8(dev(img)))
    assert np.array_equal(got, ref)


def test_lam_to_label(ops):
    """utils/camutils.py:123-145 restated in numpy (both threshold modes, image boxes)."""
    rs = np.random.RandomState(4)
    B, F_, H, W = 3, 5, 9, 11
    cam = rs.rand(B, F_, H, W).astype(np.float32)
    cls = (rs.rand(B, F_) < 0.5).astype(np.float32)
    cls[0] = 0
    box = np.array([[0, 9, 0, 11], [2, 7, 1, 9], [0, 4, 5, 11]], np.int32)
    for ignore_mid in (False, True):
        valid = cls[:, :, None, None] * cam
        val, arg = valid.max(1), valid.argmax(1)
        lab = arg + 1
        if ignore_mid:
            lab[val <= 0.7] = 255
            lab[val <= 0.25] = 0
        else:
            lab[val <= 0.5] = 0
        ref = np.full_like(lab, 255)
        for b in range(B):
            y0, y1, x0, x1 = box[b]
            ref[b, y0:y1, x0:x1] = lab[b, y0:y1, x0:x1]
        v, l = ops.lam_to_label(dev(cam), dev(cls), img_box=box, bkg_thre=0.5, high_thre=0.7, low_thre=0.25, ignore_mid=ignore_mid)
        assert np.array_equal(host(l), ref.astype(np.uint8)) and np.array_equal(host(v), valid)
        _, l2 = ops.lam_to_label(dev(cam), dev(cls), bkg_thre=0.5, high_thre=0.7, low_thre=0.25, ignore_mid=ignore_mid)
        assert np.array_equal(host(l2), lab.astype(np.uint8))
