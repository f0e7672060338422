"""The ViT forward at every width, head count, patch size and out_dim class the library accepts, against a float64 run of the oracle.

The rest of the suite runs two geometries (width 128 / 2 heads and width 768 / 12 heads, patch 16, out_dim 64 or 512) and varies the token
count; here the token count stays small and the geometry moves (table and reasons: tests/_vit_configs.py).  What a case reaches that no
other test does:

    norm.hip         ln_row with 16 / 48 active lanes (D = 64, 192), an uneven second trip (D = 320), exactly one trip (D = 256), 4 and 5
                     trips (D = 1024, 1280); assemble_ln_pre, the cls_src swap of ln_post and the split-plane output at each of them
    attn_strip.hip   3H and H phases per workgroup with H = 1 (one phase in the second sweep), odd H (3, 5), H = 4, 16, 20
    attn.hip / attn_f32.hip   B * H in blockIdx.y and the batched f32 A_sum.V GEMM (zdiv = H) away from H = 2 and 12; the two-pass split
                     path at H = 3 (test_two_pass_path_three_heads)
    im2col_kernel    ps = 8 (Kc = 192), ps = 32 (Kc = 3072 > 4 D: hbuf is sized by the im2col matrix), ps = 4 (Kc = 48: f32 only)
    token_axis_*, transpose_kernel   C = 4, 36, 100 (no multiple of 32 or 64), 768 (wider than any other case)
    vit_forward      n_surgery == layers (first_surgery = 0), layers = 1, aff_layers == layers, n_surgery = 0
    GEMMs            N = 3 D, 4 D, D and C, K = D, 4 D and Kc for D = 64 ... 1280

Every case runs forward(want_w_aff, aff_layers = min(6, layers), n_attn_out = layers, want_raw, want_feats) on B = 2 images with the two
nets of the attention sweep (tests/_attn_shapes.py: "flat", attn_gain 0.25, and "peaked", the default gain; seed 31) and is held to that
sweep's gates, unchanged:
  MASKING, flat net: per-element and row-sum attention error <= pmin / 4.  Its precondition (pmin N / rowsum >= 0.3, 4 o <= pmin / 4) is
           asserted on the reference alone before the library is called.
  NUMERICS, both nets, every quantity: err <= max(floor, k o), o = the fp32 oracle's own deviation from float64 for the same case, k = 3
           (f32, f16x3) / 40 (bf16x3), floors of _attn_shapes.floor_of (no case needs one of its own: _vit_configs.py).
`-s` prints err, o and pmin per case.  The float64 reference of the largest case (the two-pass one, N = 1297) takes 1.4 s on a CPU, so
nothing here is skipped.
"""
import collections

import numpy as np
import pytest

import _attn_shapes as A
import _vit_configs as V

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

SWEEP = [(cid, net, mode) for cid, case in V.CASES.items() for net in ("flat", "peaked") for mode in case.modes]


def dev(a):
    return torch.as_tensor(np.ascontiguousarray(a)).cuda()


def host(t):
    return t.detach().cpu().numpy()


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from excel_amd import ops as _ops
    return _ops


def make_handle(ops, cfg, w, mode):
    return ops.VitHandle(w, cfg.width, cfg.layers, cfg.heads, cfg.patch, cfg.out_dim, n_surgery=cfg.n_surgery, gemm_mode=mode)


_REFS = collections.OrderedDict()      # (case tag, net) -> (reference(), weights); the sweep visits a key's modes back to back, two are kept


def reference(tag, case, net, batch):
    key = (tag, net)
    if key not in _REFS:
        while len(_REFS) >= 2:
            _REFS.popitem(last=False)
        _REFS[key] = V.reference(case, net, batch) + (V.weights(case, net),)
    _REFS.move_to_end(key)
    return _REFS[key]


def forward_all(h, x, cfg):
    r = h.forward(x, want_w_aff=True, aff_layers=V.aff_layers(cfg), n_attn_out=cfg.layers, want_raw=True, want_feats=True)
    return {k: host(v) for k, v in r.items() if v is not None}


def run_case(ops, tag, case, net, mode, batch=V.B):
    cfg, g = case.cfg, case.g
    N = g * g + 1
    ref, o, pmin, w = reference(tag, case, net, batch)
    if net == "flat":                                       # on the reference alone, before any GPU call
        pre = A.masking_precondition(o, pmin, N, cfg)
        assert not pre, pre
    h = make_handle(ops, cfg, w, mode)
    assert h.gemm_mode() == mode
    out = forward_all(h, dev(A.images(g, batch, cfg.patch)), cfg)
    del h
    assert out["attn"].shape == (cfg.layers, batch, N, N) and out["feats"].shape == (cfg.layers, batch, N, cfg.width)
    assert out["x_raw"].shape == out["image_features"].shape == (batch, N, cfg.out_dim) and out["w_aff"].shape == (batch, N - 1, N - 1)
    err = A.errors(out, ref)
    A.report(f"{tag} {net} H={cfg.heads} ps={cfg.patch} C={cfg.out_dim} L={cfg.layers}/{cfg.n_surgery} N={N} B={batch} {mode}", err, o,
             pmin if net == "flat" else None, cfg)
    bad = A.numerics_failures(err, o, mode, cfg)
    if net == "flat":
        bad += A.masking_failures(err, pmin)
    assert not bad, bad


@pytest.mark.parametrize("cid,net,mode", SWEEP, ids=[f"{c}-{n}-{m}" for c, n, m in SWEEP])
def test_vit_config_sweep(ops, cid, net, mode):
    case = V.CASES[cid]
    N = case.g * case.g + 1
    p = ops.attn_plan(V.B, case.cfg.heads, N, mode=mode, surgery=case.cfg.n_surgery > 0, want_w=True)
    assert p["path"] == ("twopass_f32" if mode == "f32" else "strip") and p["ntiles"] == A.DISPATCH[case.g][1]
    assert p["rowpass_grid"][1] == V.B * case.cfg.heads
    run_case(ops, cid, case, net, mode)


@pytest.mark.parametrize("net", ["flat", "peaked"])
def test_two_pass_path_three_heads(ops, net):
    """h3 at g = 36 (N = 1297 = 41 key tiles), one image, bf16x3: the row pass with 4 score types and attn_accum_bf_kernel (attn.hip),
    which every other test runs with 2 heads."""
    case = V.TWOPASS
    p = ops.attn_plan(1, case.cfg.heads, case.g * case.g + 1, mode="bf16x3", surgery=True, want_w=True)
    assert (p["path"], p["ntiles"], p["rowpass_ntypes"], p["rowpass_grid"][1]) == ("twopass_split", 41, 4, 3), p
    run_case(ops, "h3-twopass", case, net, "bf16x3", batch=1)


def test_patch4_split_mode_request_falls_back_to_f32(ops):
    """Kc = 3 * 4 * 4 = 48 is no multiple of 32, so there are no split planes of conv1's weight: a handle asked for bf16x3 runs - and
    reports - f32, and the library itself refuses the split modes for it."""
    case = V.CASES["p4"]
    h = make_handle(ops, case.cfg, V.weights(case, "peaked"), "bf16x3")
    assert h.gemm_mode() == "f32"
    assert not h.weights_fp16_exact()
    with pytest.raises(RuntimeError, match="multiples of 32"):
        h.set_gemm_mode("f16x3")
    assert h.gemm_mode() == "f32"
    del h


@pytest.mark.parametrize("cid", ["h3", "h16"])
def test_f16x2_whole_forward_equals_f16x3(ops, cid):
    """On weights rounded through fp16 the lo plane of every weight is zero and f16x2 skips the products with it: the whole forward equals
    f16x3 bit for bit (as test_gemm_f16x2_equals_f16x3_bitwise has it for one GEMM), at 3 and at 16 heads."""
    case = V.CASES[cid]
    w = {k: np.asarray(v, np.float32).astype(np.float16).astype(np.float32) for k, v in V.weights(case, "peaked").items()}
    x = dev(A.images(case.g, V.B, case.cfg.patch))
    h3 = make_handle(ops, case.cfg, w, "f16x3")
    assert h3.weights_fp16_exact()
    r3 = forward_all(h3, x, case.cfg)
    del h3
    h2 = make_handle(ops, case.cfg, w, "f16x2")
    assert h2.gemm_mode() == "f16x2"
    r2 = forward_all(h2, x, case.cfg)
    del h2
    for k, v in r3.items():
        assert np.isfinite(v).all() and np.array_equal(v, r2[k]), k
