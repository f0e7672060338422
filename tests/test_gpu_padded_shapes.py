"""The padded code paths against a reference: shapes at which the decoder's Pp / ncp padding, the text tower's Pp padding, the LVC
similarity's Cp padding and the fp32 GEMM's edge tiles are in use.  tests/test_gpu_scratch_contract.py shows that these paths do not
depend on what their scratch memory held; this file shows that they compute the right thing.

Bounds are the project's own, from the named existing tests.  The fp32 numpy oracle itself differs from the float64 restatement by at
most 4.8e-7 (decoder), 2.2e-7 (text) and 2.8e-7 (affinity) at these shapes; tests/test_host_padded_shapes.py asserts on the CPU that it
stays within 1e-6 / 2e-6 (decoder fts / seg), 2e-6 (text) and 5e-7 (affinity).  That is far inside every bound, so none is widened."""
import os
import sys

import numpy as np
import pytest

import oracle

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _padded_ref as R  # noqa: E402
import _scratch as S  # noqa: E402
from _scratch_cases import decoder_handle, dev  # noqa: E402


def host(t):
    return t.detach().cpu().numpy()


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from excel_amd import ops as _ops
    return _ops


# ------------------------------------------------------------------ decoder head: P % 4 != 0 (Pp), nc % 4 != 0 (ncp)
@pytest.mark.parametrize("g,nc", [(5, 21), (5, 2), (7, 21), (7, 2)])
def test_decoder_padded_grid_vs_oracle(ops, g, nc):
    """g = 5 (P = 25, Pp = 28) and g = 7 (P = 49, Pp = 52), nc = 21 (ncp = 24) and nc = 2 (ncp = 4), E = 32, 8 heads of 4, two layers:
    the bounds of test_decoder_head_matches_golden (relative max error 1e-5 for fts, 2e-5 for seg)."""
    w, feats = R.decoder_case(g, nc)
    fts, seg = decoder_handle(ops, w).forward(dev(feats))
    ref_fts = oracle.decoder.segformer_fuse(feats, w)
    ref_seg, _ = oracle.decoder.decoder_transformer(ref_fts, w, heads=8)
    assert seg.shape == (2, nc, g, g)
    e_fts, e_seg = R.relmax(host(fts), ref_fts), R.relmax(host(seg), ref_seg)
    print(f"decoder g={g} nc={nc}: fts {e_fts:.3g} seg {e_seg:.3g}")
    assert e_fts < 1e-5
    assert e_seg < 2e-5


def test_text_tower_context_9_vs_oracle(ops):
    """context 9 (Pp = 12), width 32, 2 heads, 2 layers, EOT at positions 2, 5 and 8: the bound of test_text_tower_matches_golden's
    oracle comparison (2e-5)."""
    w, tok = R.text_case()
    got = host(ops.TextHandle(w, heads=2).encode(tok))
    ref = oracle.text.encode_text(tok, w, heads=2)
    err = R.relmax(got, ref)
    print(f"text ctx=9: {err:.3g}")
    assert err < 2e-5


# ------------------------------------------------------------------ feature affinity: C % 4 != 0 (Cp), P = 25
@pytest.mark.parametrize("C", [30, 6])
@pytest.mark.parametrize("kind", ["plain", "zero"])
def test_feature_affinity_padded_channels_vs_oracle(ops, C, kind):
    """C = 30 (Cp = 32) and C = 6 (Cp = 8), P = 25, B = 4, the bound of test_feature_affinity_vs_golden_and_oracle (1e-6).  "zero": one
    token whose feature column is all zero - the 1e-12 clamp of F.normalize; its mask_softmax row ends below zero in every entry and is
    NaN like torch.softmax, position by position.  No similarity of these inputs lies within 3e-4 of the sign test's threshold."""
    f = R.affinity_case(C, kind)
    assert np.abs(R.similarity_f64(f)).min() > 3e-4
    sig = host(ops.feature_affinity(dev(f), "sigmoid"))
    ref = oracle.cam.attn_pred(f)
    assert np.isfinite(sig).all()
    e_sig = R.maxabs(sig, ref)
    msm = host(ops.feature_affinity(dev(f.reshape(4, C, 5, 5)), "mask_softmax"))
    with np.errstate(invalid="ignore"):
        ref = oracle.vit.ex_attention(f)
    nan = np.isnan(ref)
    assert int(nan.sum()) == (25 if kind == "zero" else 0) and (kind != "zero" or nan[1, 7].all())
    assert np.array_equal(np.isnan(msm), nan)
    e_msm = R.maxabs(msm[~nan], ref[~nan])
    print(f"feature_affinity C={C} {kind}: sigmoid {e_sig:.3g} mask_softmax {e_msm:.3g}")
    assert e_sig < 1e-6
    assert e_msm < 1e-6
    np.testing.assert_allclose(msm[~nan].reshape(-1, 25).sum(-1), 1.0, atol=1e-5)
    if kind == "zero":
        assert not msm[1, np.arange(25) != 7, 7].any()          # nobody attends to the empty token
    # the grouped form with one group over the whole batch is the same op
    assert torch.equal(ops.feature_affinity_grouped(dev(f), "sigmoid", group=4), ops.feature_affinity(dev(f), "sigmoid"))


# ------------------------------------------------------------------ ops.gemm at its edges
def _gemm_ref(A, Bm, nt, bias=None, res=None, act=0):
    A64, B64 = A.astype(np.float64), Bm.astype(np.float64)
    y = A64 @ (np.swapaxes(B64, -1, -2) if nt else B64)
    if bias is not None:
        y = y + bias
    if act == 1:
        y = y * (1.0 / (1.0 + np.exp(-1.702 * y)))
    elif act == 2:
        y = np.maximum(y, 0)
    return y if res is None else y + res


GEMM_SHAPES = [("nt", 1, 45, 36), ("nt", 129, 45, 4), ("nt", 129, 45, 36), ("nt", 1, 4, 4), ("nn", 1, 4, 36), ("nn", 129, 4, 4), ("nn", 129, 4, 36),
               ("nn", 1, 48, 4)]


@pytest.mark.parametrize("form,M,N,K", GEMM_SHAPES)
def test_gemm_edges_vs_float64(ops, form, M, N, K):
    """One row, one row past a tile (M = 129), the narrowest legal N of each form (NN needs N % 4 == 0: 4; NT takes 45), one k-step of
    4 and K = 36 (one full 32-wide k tile and a 4-wide rest): test_gemm_nt's bounds, relmax < 2e-6 plain and 3e-6 with an epilogue -
    QuickGELU as there, and ReLU (act = 2, what the decoder's fuse MLP runs) with bias and residual."""
    nt = form == "nt"
    rs = np.random.RandomState(1000 * M + 10 * N + K)
    A = rs.standard_normal((M, K)).astype(np.float32)
    Bm = rs.standard_normal((N, K) if nt else (K, N)).astype(np.float32)
    bias = rs.standard_normal(N).astype(np.float32)
    res = rs.standard_normal((M, N)).astype(np.float32)
    e0 = R.relmax(host(ops.gemm(dev(A), dev(Bm), b_kmajor=nt)), _gemm_ref(A, Bm, nt))
    e1 = R.relmax(host(ops.gemm(dev(A), dev(Bm), bias=dev(bias), residual=dev(res), act=1, b_kmajor=nt)), _gemm_ref(A, Bm, nt, bias, res, 1))
    relu = host(ops.gemm(dev(A), dev(Bm), bias=dev(bias), residual=dev(res), act=2, b_kmajor=nt))
    e2 = R.relmax(relu, _gemm_ref(A, Bm, nt, bias, res, 2))
    print(f"gemm {form} M={M} N={N} K={K}: plain {e0:.3g} quickgelu {e1:.3g} relu {e2:.3g}")
    assert e0 < 2e-6
    assert e1 < 3e-6
    assert e2 < 3e-6
    if M > 1:
        clipped = (_gemm_ref(A, Bm, nt, bias) < -1e-3)            # (clear of the fp32 rounding of the sum around zero)
        assert clipped.any() and not clipped.all()                # both sides of the ReLU are in the data ...
        assert np.array_equal(relu[clipped], res[clipped])        # ... and a clipped element is exactly its residual


@pytest.mark.parametrize("form,N", [("nt", 45), ("nn", 4)])
def test_gemm_broadcast_b_vs_float64(ops, form, N):
    """3-D A with a 2-D B: the one B serves every batch entry (sB = 0), with a per-entry residual and the ReLU epilogue."""
    nt = form == "nt"
    rs = np.random.RandomState(N)
    A = rs.standard_normal((3, 129, 36)).astype(np.float32)
    Bm = rs.standard_normal((N, 36) if nt else (36, N)).astype(np.float32)
    bias = rs.standard_normal(N).astype(np.float32)
    res = rs.standard_normal((3, 129, N)).astype(np.float32)
    out = ops.gemm(dev(A), dev(Bm), b_kmajor=nt)
    assert out.shape == (3, 129, N)
    e0 = R.relmax(host(out), _gemm_ref(A, Bm, nt))
    e2 = R.relmax(host(ops.gemm(dev(A), dev(Bm), bias=dev(bias), residual=dev(res), act=2, b_kmajor=nt)), _gemm_ref(A, Bm, nt, bias, res, 2))
    print(f"gemm broadcast {form} N={N}: plain {e0:.3g} relu {e2:.3g}")
    assert e0 < 2e-6
    assert e2 < 3e-6
    for b in range(3):                                             # every entry equals the 2-D call on its slice, bit for bit
        assert torch.equal(out[b], ops.gemm(dev(A[b]), dev(Bm), b_kmajor=nt))


@pytest.mark.parametrize("form,M,N,K", [("nt", 37, 45, 38), ("nn", 37, 45, 36), ("nn", 37, 48, 38)])
def test_gemm_refuses_unpadded_shapes_without_a_launch(ops, form, M, N, K):
    """NT with K % 4 != 0 and NN with N % 4 != 0 (or K % 4 != 0) raise; the output buffer, allocated as 0xFF bytes, is untouched after
    the stream has drained: nothing was launched."""
    nt = form == "nt"
    rs = np.random.RandomState(K)
    A = dev(rs.standard_normal((M, K)).astype(np.float32))
    Bm = dev(rs.standard_normal((N, K) if nt else (K, N)).astype(np.float32))
    made = []
    with S.poisoned_allocations(0xFF):
        poisoned = torch.empty

        def keep(*a, **kw):
            made.append(poisoned(*a, **kw))
            return made[-1]
        torch.empty = keep
        with pytest.raises(RuntimeError, match="multiple of 4|multiples of 4"):
            ops.gemm(A, Bm, b_kmajor=nt)
    torch.cuda.synchronize()
    assert len(made) == 1 and made[0].shape == (1, M, N)
    S.assert_holds(made[0], 0xFF)
