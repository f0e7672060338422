"""Pin the float64 autograd oracle of the training iteration (oracle/train.py) against tests/golden/train_tiny.npz, which the
reference's own modules, losses, affinity-label code and autograd minted in fp32 (tests/golden/make_goldens.py gold_train).  CPU only.

The oracle runs in float64 on the golden's fp32 inputs, so the two differ by the golden's own fp32 round-off: measured worst
relative errors (max abs error over the golden's max abs): 3.2e-7 for the parameter gradients, 4.3e-7 for seg and attn_pred,
1.2e-6 for d_seg, 1e-7 for the losses; bounded here at 1e-5."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
from oracle import train as otrain  # noqa: E402


def relmax(a, b):
    return float(np.max(np.abs(np.asarray(a, np.float64) - np.asarray(b, np.float64)))) / max(float(np.max(np.abs(b))), 1e-30)


@pytest.fixture(scope="module")
def run(golden):
    g, gd = golden("train_tiny.npz"), golden("decoder_tiny.npz")
    w = {k[3:]: g[k] for k in g.files if k.startswith("w0.")}
    return g, otrain.train_iteration(gd["all_feats"], w, g["pseudo"], heads=8, radius=2, w_seg=1.0, w_diver=0.1)


def test_forward_and_losses(run):
    g, o = run
    assert relmax(o["seg"], g["seg"]) < 1e-5
    assert relmax(o["attn_pred"], g["attn_pred"]) < 1e-5
    assert abs(o["seg_loss"] - float(g["seg_loss"])) < 1e-5 * float(g["seg_loss"])
    assert abs(o["diver_loss"] - float(g["diver_loss"])) < 1e-5 * float(g["diver_loss"])


def test_affinity_labels(run):
    g, o = run
    assert np.array_equal(o["aff_mask"], g["aff_mask"].astype(np.int64))
    assert o["pos_count"] == int(g["pos_count"]) and o["neg_count"] == int(g["neg_count"])
    assert np.array_equal(otrain.mask_by_radius(6, 2).numpy(), g["attn_mask"].astype(bool))


def test_loss_gradients(run):
    g, o = run
    assert relmax(o["d_seg"], g["d_seg"]) < 1e-5
    assert relmax(o["d_attn_pred"], g["d_attn_pred"]) < 1e-5
    assert relmax(o["d_fts"], g["d_fts"]) < 1e-5


def test_every_parameter_gradient(run):
    g, o = run
    keys = sorted(k[2:] for k in g.files if k.startswith("g."))
    assert sorted(o["grads"]) == keys
    errs = {k: relmax(o["grads"][k], g["g." + k]) for k in keys}
    worst = max(errs, key=errs.get)
    print("worst gradient mismatch", worst, errs[worst])
    assert errs[worst] < 1e-5, (worst, errs[worst])


def test_losses_alone_match_full_iteration(run):
    """losses_and_grads on the golden's seg / attn_pred gives the golden's loss gradients (the path the GPU sweep compares with)."""
    g, _ = run
    o = otrain.losses_and_grads(g["seg"], g["attn_pred"], g["pseudo"], 2, w_seg=1.0, w_diver=0.1)
    assert relmax(o["d_seg"], g["d_seg"]) < 1e-5 and relmax(o["d_attn_pred"], g["d_attn_pred"]) < 1e-5
    assert abs(o["seg_loss"] - float(g["seg_loss"])) < 1e-5 * float(g["seg_loss"])
