"""The references of tests/test_gpu_padded_shapes.py against float64, on the CPU.  At the padded shapes the fp32 numpy oracle differs
from the float64 restatement by at most 4.8e-7 (decoder, relative), 2.2e-7 (text, relative) and 2.8e-7 (affinity, absolute), so the
bounds the kernels are held to there are statements about the kernels.  Asserted: a tenth of the kernels' bound for the decoder
(1e-6 fts, 2e-6 seg) and the text tower (2e-6), half of it for the affinity (5e-7)."""
import os
import sys

import numpy as np
import pytest

import oracle

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _padded_ref as R  # noqa: E402


@pytest.mark.parametrize("g,nc", [(5, 21), (5, 2), (7, 21), (7, 2)])
def test_decoder_oracle_vs_float64(g, nc):
    w, feats = R.decoder_case(g, nc)
    fts = oracle.decoder.segformer_fuse(feats, w)
    seg, _ = oracle.decoder.decoder_transformer(fts, w, heads=8)
    f64, s64 = R.decoder_f64(feats, w, 8)
    assert seg.shape == (2, nc, g, g)
    assert R.relmax(fts, f64) < 1e-6 and R.relmax(seg, s64) < 2e-6


def test_text_oracle_vs_float64():
    w, tok = R.text_case()
    assert sorted(tok.argmax(-1)) == [2, 5, 8]                     # EOT at three different positions, one of them the last slot
    assert R.relmax(oracle.text.encode_text(tok, w, heads=2), R.text_f64(tok, w, 2)) < 2e-6


@pytest.mark.parametrize("C", [30, 6])
@pytest.mark.parametrize("kind", ["plain", "zero"])
def test_affinity_oracle_vs_float64(C, kind):
    f = R.affinity_case(C, kind)
    z = R.similarity_f64(f)
    assert np.abs(z).min() > 3e-4                                  # no entry near the z < 0 test of the mask: fp32 and float64 agree on it
    assert (z / 3 + z.mean()).mean() > -1 and float(np.einsum("bcm,bcn->bmn", f, f).mean()) > 0
    assert R.maxabs(oracle.cam.attn_pred(f), R.affinity_f64(f, "sigmoid")) < 5e-7
    with np.errstate(invalid="ignore"):
        got, ref = oracle.vit.ex_attention(f), R.affinity_f64(f, "mask_softmax")
    assert np.array_equal(np.isnan(got), np.isnan(ref))
    assert int(np.isnan(ref).sum()) == (25 if kind == "zero" else 0)
    assert R.maxabs(got[~np.isnan(ref)], ref[~np.isnan(ref)]) < 5e-7
