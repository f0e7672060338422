"""ops.train_augment (aug.hip) against the Pillow + numpy restatement of VOC12ClsDataset(aug=True)'s transform (tests/_train_aug_ref.py)."""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _train_aug_ref as R  # noqa: E402


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from excel_amd import ops as _ops
    return _ops


def _params(hw, S, ratios, flips, rng):
    p = R.draw_params(rng, hw, S)
    for b, (h, w) in enumerate(hw):
        if ratios[b] is not None:
            r = ratios[b]
            h2, w2 = int(r * h), int(r * w)
            H, W = max(S, h2), max(S, w2)
            p[b]["ratio"] = r
            p[b]["h_pad"], p[b]["w_pad"] = rng.integers(H - h2 + 1), rng.integers(W - w2 + 1)
            p[b]["cand_h"], p[b]["cand_w"] = rng.integers(0, H - S + 1, 10), rng.integers(0, W - S + 1, 10)
        p[b]["flip"] = flips[b]
    return p


def _batch(ops, images, labels, params, S, stream=None):
    from excel_amd.datasets.loader import pack_samples
    rb = pack_samples([(str(i), im, lab, np.zeros(4, np.float32)) for i, (im, lab) in enumerate(zip(images, labels))])
    plan = ops.RaggedPlan(rb.hw, "cuda")
    return ops.train_augment(rb.images.cuda(), plan, rb.labels.cuda(), params, S)


def _check(ops, images, labels, params, S):
    img, lab, box = _batch(ops, images, labels, params, S)
    refs = [R.transform(im, l, params[b], S) for b, (im, l) in enumerate(zip(images, labels))]
    crops = torch.from_numpy(np.stack([r["crop_u8"] for r in refs])).cuda()
    want = ops.normalize_img_u8(crops)
    for b, r in enumerate(refs):
        assert torch.equal(img[b], want[b]), (b, S, float(params[b]["ratio"]), int(params[b]["flip"]))
        assert np.array_equal(lab[b].cpu().numpy(), r["label"]), b
        assert box[b].cpu().numpy().tolist() == r["img_box"].astype(int).tolist(), b
    ref32 = np.stack([r["img_ref"] for r in refs])
    assert float(np.abs(img.cpu().numpy() - ref32).max()) <= 2.4e-7          # the reference's float32 normalize_img
    return refs


def _images(rng, hw, gray=()):
    ims, labs = [], []
    for b, (h, w) in enumerate(hw):
        im = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
        if b in gray:
            im = np.repeat(rng.integers(0, 256, (h, w, 1), dtype=np.uint8), 3, axis=2)     # VOC12Dataset's grayscale expansion
        lab = rng.integers(0, 6, (h, w), dtype=np.uint8)
        lab[rng.random((h, w)) < 0.1] = 255
        ims.append(im)
        labs.append(lab)
    return ims, labs


@pytest.mark.parametrize("S", [320, 448, 96])
def test_bit_identity_with_pillow(ops, S):
    rng = np.random.default_rng(S)
    hw = [(375, 500), (500, 333), (120, 90), (281, 500), (333, 500), (64, 75), (366, 480)]
    ims, labs = _images(rng, hw, gray=(3,))
    ratios = [0.5, 2.0, 1.0 + 0.5 / 90, None, None, 0.5, 1.0]      # 2: width unchanged (no horizontal pass); 5: smaller than any crop
    flips = [0, 1, 1, 0, 1, 0, 1]
    refs = _check(ops, ims, labs, _params(hw, S, ratios, flips, rng), S)
    h, w = refs[5]["rescaled"]
    assert h < S and w < S                                             # padded on both axes


def test_normalisation_convention_all_values(ops):
    """Every uint8 value through the kernel: equal to ops.normalize_img_u8, within 2.4e-7 of the reference's float32 normalize_img."""
    S = 16
    v = np.arange(256, dtype=np.uint8).reshape(16, 16)
    im = np.stack([v, v[::-1], v.T], -1).copy()
    p = R.make_params(1)
    p[0]["ratio"] = 1.0
    img, _, _ = _batch(ops, [im], [np.zeros((16, 16), np.uint8)], p, S)
    want = ops.normalize_img_u8(torch.from_numpy(im)[None].cuda())
    assert torch.equal(img, want)
    ref = R.transform(im, np.zeros((16, 16), np.uint8), p[0], S)["img_ref"]
    d = np.abs(img[0].cpu().numpy() - ref)
    assert float(d.max()) <= 2.4e-7 and int((d > 0).sum()) > 0        # the two conventions do differ, by one float32 ulp at most


def test_crop_rule(ops):
    rng = np.random.default_rng(5)
    S, h, w = 64, 100, 160
    base = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    ignore = np.full((h, w), 255, np.uint8)                           # every window all ignore: the 10th candidate
    single = np.full((h, w), 7, np.uint8)                             # one class everywhere: rejected every time, the 10th wins
    stripes = ((np.arange(w)[None, :] // 8) % 3).astype(np.uint8).repeat(h, 0)   # mixed: the first candidate is accepted
    early = np.zeros((h, w), np.uint8)
    early[:, 60:] = 3                                                 # flipped: columns 0-99 class 3, 100-159 class 0
    labs = [ignore, single, stripes, early]
    p = R.make_params(4)
    for b in range(4):
        p[b]["ratio"] = 1.0
        p[b]["flip"] = b == 3
        p[b]["cand_h"] = rng.integers(0, h - S + 1, 10)
        p[b]["cand_w"] = rng.integers(0, w - S + 1, 10)
    p[3]["cand_w"][:3] = [0, 5, 10]                                   # class 3 only: rejected
    p[3]["cand_w"][3] = 70                                            # 30 x class 3 + 34 x class 0 per row: accepted as the 4th
    refs = _check(ops, [base] * 4, labs, p, S)
    assert [r["cand"] for r in refs] == [9, 9, 0, 3]


def test_non_default_stream_queued_behind_work(ops):
    rng = np.random.default_rng(9)
    hw = [(375, 500), (200, 180), (500, 375)]
    ims, labs = _images(rng, hw)
    p = _params(hw, 320, [None] * 3, [1, 0, 1], rng)
    ref = _batch(ops, ims, labs, p, 320)
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    a = torch.randn(4096, 4096, device="cuda")
    with torch.cuda.stream(s):
        for _ in range(4):
            a = a @ a * 1e-3                                          # keeps the stream busy while the call is queued behind it
        got = _batch(ops, ims, labs, p, 320)
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    for x, y in zip(got, ref):
        assert torch.equal(x, y)


def test_train_step_on_device_augmented_inputs(ops):
    """One DecoderTrainer.train_step on ops.train_augment's output = on the restatement's uint8 crops through ops.normalize_img_u8."""
    from oracle.vit import VitConfig, make_vit_weights
    from excel_amd.model import ExCEL_model, init_decoder_state_dict
    from excel_amd.scripts.train_voc import DecoderTrainer
    from excel_amd.utils.PAR import PAR
    TINY = VitConfig(width=128, layers=8, heads=2, patch=16, out_dim=64, input_resolution=64, n_surgery=5)
    kw = dict(width=128, layers=8, heads=2, patch=16, output_dim=64, input_resolution=64)
    w = make_vit_weights(TINY, seed=11)
    rs = np.random.RandomState(3)
    text = rs.standard_normal((9, 64)).astype(np.float32)
    text /= np.linalg.norm(text, axis=1, keepdims=True)
    dec = init_decoder_state_dict(num_classes=5, in_channels=128, embedding_dim=32, crop_size=96, seed=0, index=8)
    rng = np.random.default_rng(2)
    hw = [(120, 150), (90, 70)]
    ims, labs = _images(rng, hw)
    p = _params(hw, 96, [None, None], [1, 0], rng)
    img, _, _ = _batch(ops, ims, labs, p, 96)
    crops = np.stack([R.transform(im, l, p[b], 96)["crop_u8"] for b, (im, l) in enumerate(zip(ims, labs))])
    ref = ops.normalize_img_u8(torch.from_numpy(crops).cuda())
    cls = torch.tensor([[1, 0, 1, 0], [0, 1, 0, 0]], dtype=torch.float32, device="cuda")
    out = []
    for x in (img, ref):
        model = ExCEL_model(clip_model="tiny", num_classes=5, img_size=96, mode="train", state_dict=w, vit_cfg=kw, text_attr=text.T.copy(),
                            gemm_mode="f32", embedding_dim=32, in_channels=128, decoder_state_dict=dec)
        tr = DecoderTrainer(model, PAR(num_iter=10, dilations=[1, 2, 4, 8, 12, 24]), lr=1e-3, warmup_iters=2, max_iters=100, radius=2)
        out.append(tr.train_step(x, cls))
    assert np.isfinite(out[0]["seg_loss"]) and np.isfinite(out[0]["diver_loss"])
    assert out[0]["seg_loss"] == out[1]["seg_loss"] and out[0]["diver_loss"] == out[1]["diver_loss"]
