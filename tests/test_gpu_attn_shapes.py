"""The ViT attention kernels at every token count they dispatch on, against a float64 run of the oracle.

The launchers pick a kernel instance per range of N = g*g + 1 (excel_attn_plan; formulae in tests/_attn_shapes.py).  Grid sides run here
(square inputs of 16 g pixels), with what each one exercises - tiles = key tiles of 32, waves = full x ntw + rest x (ntw - 1):

    g    N   tiles  instance  waves (tiles each)   keys in last tile  batch  extras
    8    65    3    <1>       3 x 1                 1                  3      f32, cls_only, NaN workspace    (N mod 128 = 65)
   15   226    8    <1>       8 x 1                 2                  1
   16   257    9    <2>       4 x 2 + 1 x 1         1                  3      f32, cls_only, NaN workspace    (N mod 128 = 1)
   17   290   10    <2>       5 x 2                 2                  3
   20   401   13    <2>       6 x 2 + 1 x 1        17                  3      (the decoder's training crop, 320^2), LVC, f16x2
   21   442   14    <2>       7 x 2                26                  1      (336^2 = 0.75 x 448)
   22   485   16    <2>       8 x 2                 5                  3
   23   530   17    <3>       5 x 3 + 1 x 2        18                  3      f32, cls_only, NaN workspace    (N mod 128 = 18)
   27   730   23    <3>       7 x 3 + 1 x 2        26                  1
   29   842   27    <4>       6 x 4 + 1 x 3        10                  3      f32, cls_only, NaN workspace    (N mod 128 = 74)
   31   962   31    <4>       7 x 4 + 1 x 3         2                  1
   32  1025   33    <5>       5 x 5 + 2 x 4         1                  1      LVC
   35  1226   39    <5>       7 x 5 + 1 x 4        10                  3      f32, cls_only, NaN workspace    (N mod 128 = 74)
   36  1297   41    two-pass  -                    17                  3      f32, cls_only, NaN workspace, LVC, f16x2 (N mod 128 = 17)
   40  1601   51    two-pass  -                     1                  1
   42  1765   56    two-pass  -                     5                  3      (672^2 = 1.5 x 448)
(the LVC cue also runs at g = 28, instance <4>; the size-reuse test adds g = 14 and 28)

B = 3 makes B x strips no multiple of 8 for the strip kernel's split grid and gives blockIdx.z > 0 in the two-pass kernels.  bf16x3 and
f16x3 run everywhere (the two namespaces are different binaries); f32 - always attn_rowpass_f32_kernel + attn_accum_kernel, attn_f32.hip -
on one shape per row, for the row pass's 128-row query-block edges.

Two nets (TINY, seed 31), each through reload_self_attn(feat_size=g, "train"):
  flat    attn_gain 0.25: nearly uniform rows, every valid key holds >= 0.3 of a uniform share.  One wrongly admitted or dropped key
          moves an element and its row sum by >= pmin (the smallest reference probability of the layer), four orders above arithmetic
          noise: the MASKING gate is per-element and row-sum error <= pmin / 4, in every mode.  Asserted first on the reference alone:
          pmin N / rowsum >= 0.3 and 4 o <= pmin / 4 (o = the fp32 oracle's own deviation from float64).
  peaked  the default gain (the net of test_vit_tiny_strip_three_tiles_per_wave_bf16x3): numerics.
NUMERICS gate, both nets, every quantity q: err <= max(floor_q, k o_q) with k = 3 (f32, f16x3) / 40 (bf16x3), the factors of
test_vit_b16_448_clip_like_outlier_net, and the floors the suite already holds this net to (_attn_shapes.floor_of).  bf16x3 `feats` and
`image_features` share x_raw's floor (the same residual stream, one projection apart).  `-s` prints err, o and pmin per case.
"""
import collections

import numpy as np
import pytest

import _attn_shapes as A

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

TINY = A.TINY
L = TINY.layers
# g: batch; FULL: the one shape per dispatch row that also runs f32, the cls_only second call and the NaN-workspace check
BATCH = {8: 3, 15: 1, 16: 3, 17: 3, 20: 3, 21: 1, 22: 3, 23: 3, 27: 1, 29: 3, 31: 1, 32: 1, 35: 3, 36: 3, 40: 1, 42: 3}
FULL = (8, 16, 23, 29, 35, 36)
SWEEP = [(net, g, mode) for net in ("flat", "peaked") for g in BATCH for mode in ("bf16x3", "f16x3", "f32") if mode != "f32" or g in FULL]


def dev(a, dtype=None):
    t = torch.as_tensor(np.ascontiguousarray(a))
    if dtype is not None:
        t = t.to(dtype)
    return t.cuda()


def host(t):
    return t.detach().cpu().numpy()


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from excel_amd import ops as _ops
    return _ops


def make_handle(ops, w, mode):
    return ops.VitHandle(w, TINY.width, TINY.layers, TINY.heads, TINY.patch, TINY.out_dim, n_surgery=TINY.n_surgery, gemm_mode=mode)


_REFS = collections.OrderedDict()      # (net, g, B, ex, reload) -> reference(); the sweep visits a key's modes back to back, two entries are kept


def reference(net, g, B, ex=False, reload=True):
    key = (net, g, B, ex, reload)
    if key not in _REFS:
        while len(_REFS) >= 2:
            _REFS.popitem(last=False)
        _REFS[key] = A.reference(net, g, B, ex=ex, reload=reload)
    _REFS.move_to_end(key)
    return _REFS[key]


def assert_plan(ops, g, B, mode):
    """The case runs the instance the table claims: every layer kind (plain / surgery, all with weights wanted here)."""
    N, tiles, ntw, nw, full, _ = A.DISPATCH[g]
    for surgery in (False, True):
        p = ops.attn_plan(B, TINY.heads, N, mode=mode, surgery=surgery, want_w=True)
        if mode == "f32":
            assert p["path"] == "twopass_f32" and p["rowpass_ntypes"] == (4 if surgery else 1), p
            assert p["grid"] == (-(-N // 64), -(-N // 64), B) and p["rowpass_grid"][0] == -(-N // 128)
        elif ntw:
            assert (p["path"], p["ntiles"], p["ntw"], p["waves"], p["waves_full"], p["rowpass_ntypes"]) == ("strip", tiles, ntw, nw, full, 1), p
            assert p["block"] == 64 * nw and (p["split_c"] > 0) == surgery
        else:
            assert (p["path"], p["ntiles"], p["ntw"]) == ("twopass_split", tiles, 0) and p["rowpass_ntypes"] == (4 if surgery else 1), p
            assert p["grid"] == (-(-N // 64), -(-N // 128), B) and p["block"] == 512


def outputs(r):
    return {k: host(v) for k, v in r.items() if v is not None}


def forward_all(h, x, **kw):
    return h.forward(x, want_w_aff=True, aff_layers=6, n_attn_out=L, want_raw=True, want_feats=True, **kw)


@pytest.mark.parametrize("net,g,mode", SWEEP, ids=[f"{n}-g{g}-{m}" for n, g, m in SWEEP])
def test_attention_shape_sweep(ops, net, g, mode):
    B = BATCH[g]
    N = g * g + 1
    assert_plan(ops, g, B, mode)
    ref, o, pmin = reference(net, g, B)
    if net == "flat":
        pre = A.masking_precondition(o, pmin, N)
        assert not pre, pre
    x = dev(A.images(g, B))
    h = make_handle(ops, A.net_weights(net, g), mode)
    out = outputs(forward_all(h, x))
    err = A.errors(out, ref)
    A.report(f"{net} g={g} N={N} B={B} {mode}", err, o, pmin if net == "flat" else None)
    bad = A.numerics_failures(err, o, mode)
    if net == "flat":
        bad += A.masking_failures(err, pmin)
    if g in FULL:
        # the cls_only branch of the last block (no feature maps wanted: flash_nq = 1, the compact [B, D] MLP)
        r2 = h.forward(x, want_w_aff=True, aff_layers=6, n_attn_out=L, want_raw=True, want_feats=False)
        assert r2["feats"] is None
        err2 = A.errors(outputs(r2), ref)
        A.report(f"{net} g={g} N={N} B={B} {mode} cls_only", err2, o)
        bad += ["cls_only " + m for m in A.numerics_failures(err2, o, mode)]
        if net == "flat":
            bad += ["cls_only " + m for m in A.masking_failures(err2, pmin)]
    del h
    assert not bad, bad


@pytest.mark.parametrize("mode", ["bf16x3", "f16x3"])
@pytest.mark.parametrize("g", FULL)
def test_workspace_padding_is_never_read_as_data(ops, g, mode):
    """A_sum's padded keys (KP = 32 tiles), the V^T padding columns and the padded q / k rows live in the caller-owned, grow-only
    workspace, a torch.empty that is reused across sizes.  Every byte set to 0xFF (a NaN in every fp32 / bf16 / f16 lane) before a
    forward must not change one bit of any output: nothing persists in the workspace between calls, and 0 x NaN = NaN on the matrix core."""
    B, S = BATCH[g], 16 * g
    x = dev(A.images(g, B))
    h = make_handle(ops, A.net_weights("peaked", g), mode)
    first = forward_all(h, x)
    torch.cuda.synchronize()
    ws, need = h.workspace(B, S)
    assert ws.dtype == torch.uint8 and ws.numel() >= need
    ws.fill_(0xFF)
    again = forward_all(h, x)
    ws2, _ = h.workspace(B, S)
    assert ws2.data_ptr() == ws.data_ptr()                    # the same tensor served both calls
    for k, v in first.items():
        assert torch.isfinite(v).all(), k
        assert torch.equal(v, again[k]), (k, float((v - again[k]).abs().max()))
    del h


def test_one_handle_many_sizes_bf16x3(ops):
    """What multi_scale_lam does: ONE handle with its native positional grid (the library resizes it per size and caches the result; the
    workspace only grows) run at g = 42 -> 14 -> 21 -> 28 -> 16.  Every result is bit-identical to a fresh handle's at that size and meets
    the numerics gate against the oracle on the un-reloaded weights (which resizes the grid itself)."""
    B = 2
    w = A.net_weights("peaked")
    h = make_handle(ops, w, "bf16x3")
    bad = []
    for g in (42, 14, 21, 28, 16):
        x = dev(A.images(g, B))
        r = forward_all(h, x)
        fresh = make_handle(ops, w, "bf16x3")
        r1 = forward_all(fresh, x)
        for k, v in r.items():
            assert torch.equal(v, r1[k]), (g, k)
        del fresh, r1
        ref, o, _ = reference("peaked", g, B, reload=False)
        err = A.errors(outputs(r), ref)
        A.report(f"reused handle g={g} B={B} bf16x3", err, o)
        bad += [f"g={g} " + m for m in A.numerics_failures(err, o, "bf16x3")]
    del h
    assert not bad, bad


@pytest.mark.parametrize("mode", ["bf16x3", "f16x3"])
@pytest.mark.parametrize("g", [20, 28, 32, 36])
def test_lvc_cue_shapes(ops, g, mode):
    """The LVC cue (ex_attn added to every head's attn[1:, 1:] of the surgery blocks) is applied in the strip kernel's and in
    attn_accum_bf_kernel's epilogue: instances <2>, <4>, <5> and the two-pass path, against vit_forward(ex_feats=...) in float64.
    The cue features are +-1 valued, so every similarity is a multiple of 2 / C and none sits at the `< 0 -> -inf` threshold of the
    masked softmax, where fp32 and float64 could disagree about a key (asserted on the reference: the margin is >= 1e-4)."""
    B = 2
    N = g * g + 1
    p = ops.attn_plan(B, TINY.heads, N, mode=mode)
    assert (p["path"], p["ntw"]) == {20: ("strip", 2), 28: ("strip", 4), 32: ("strip", 5), 36: ("twopass_split", 0)}[g]
    ex = np.sign(A.ex_features(g, B)).astype(np.float32)
    with A.oracle.vit.precision(np.float64):
        sim = A.oracle.vit.feature_similarity(ex.astype(np.float64), 1.0, 3.0)
    assert np.abs(sim).min() >= 1e-4, np.abs(sim).min()
    key = ("lvc", g)
    if key not in _REFS:
        while len(_REFS) >= 2:
            _REFS.popitem(last=False)
        w = A.net_weights("peaked", g)
        imgs = A.images(g, B)
        with A.oracle.vit.precision(np.float64):
            x64, a64, f64 = A.oracle.vit.vit_forward(imgs.astype(np.float64), {k: np.asarray(v, np.float64) for k, v in w.items()}, TINY,
                                                     ex_feats=ex.astype(np.float64))
            ex64 = A.oracle.vit.ex_attention(ex.astype(np.float64))
        pack = lambda x_, a_, f_: dict(attn=a_, feats=f_, x_raw=x_, image_features=A.token_normalize(x_), w_aff=a_[-6:, :, 1:, 1:].mean(0))
        ref = pack(x64, a64, f64)
        _REFS[key] = (ref, A.errors(pack(*A.oracle.vit.vit_forward(imgs, w, TINY, ex_feats=ex)), ref), ex64)
    ref, o, ex64 = _REFS[key]
    ex_attn = ops.feature_affinity(dev(ex), "mask_softmax")
    e_ex = A.maxabs(host(ex_attn), ex64)
    assert e_ex < 1e-6, e_ex                                    # the cue itself (fp32 kernel; rows sum to 1, entries <= 1)
    h = make_handle(ops, A.net_weights("peaked", g), mode)
    err = A.errors(outputs(forward_all(h, dev(A.images(g, B)), ex_attn=ex_attn)), ref)
    A.report(f"LVC g={g} N={N} B={B} {mode} (cue err {e_ex:.1e})", err, o)
    del h
    bad = A.numerics_failures(err, o, mode)
    assert not bad, bad


@pytest.mark.parametrize("g", [20, 36])
def test_f16x2_whole_forward_equals_f16x3(ops, g):
    """On weights rounded through fp16 (what every published CLIP archive holds) the lo plane of every weight is zero and f16x2 skips the
    products with it: the WHOLE forward - strip instance <2> at g = 20, the two-pass path at g = 36 - equals f16x3 bit for bit."""
    B = 2
    w = {k: np.asarray(v, np.float32).astype(np.float16).astype(np.float32) for k, v in A.net_weights("peaked", g).items()}
    x = dev(A.images(g, B))
    h3 = make_handle(ops, w, "f16x3")
    assert h3.weights_fp16_exact()
    r3 = forward_all(h3, x)
    del h3
    h2 = make_handle(ops, w, "f16x2")
    assert h2.gemm_mode() == "f16x2"
    r2 = forward_all(h2, x)
    del h2
    for k, v in r3.items():
        assert torch.isfinite(v).all() and torch.equal(v, r2[k]), k
