"""COCO decoder training on the device: ops.train_augment_image (aug.hip) against the Pillow + numpy restatement of
CocoClsDataset(aug=True)'s transform (tests/_coco_aug_ref.py), against the labelled transform, on a busy stream; DecoderTrainer with COCO's
settings; scripts/train_coco.train end to end with checkpoint reload through infer_seg_coco."""
import logging
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _coco_aug_ref as R  # noqa: E402

COCO_HW = [(480, 640), (640, 480), (427, 640), (200, 150)]      # the last one is smaller than any crop at ratio 0.5
NUM_CLASSES = 81


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from excel_amd import ops as _ops
    return _ops


def _images(rng, hw, grey=()):
    ims = []
    for b, (h, w) in enumerate(hw):
        im = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
        if b in grey:
            im = np.repeat(rng.integers(0, 256, (h, w, 1), dtype=np.uint8), 3, axis=2)
        ims.append(im)
    return ims


def _packed(ops, images, labels=None):
    from excel_amd.datasets.loader import pack_samples
    labels = labels or [None] * len(images)
    rb = pack_samples([(str(i), im, lab, np.zeros(80, np.float32)) for i, (im, lab) in enumerate(zip(images, labels))])
    return rb, ops.RaggedPlan(rb.hw, "cuda")


def _image_only(ops, images, p, S):
    rb, plan = _packed(ops, images)
    return ops.train_augment_image(rb.images.cuda(), plan, p, S)


@pytest.mark.parametrize("S", [320, 448])
def test_bit_identity_with_pillow(ops, S):
    rng = np.random.default_rng(S)
    ims = _images(rng, COCO_HW, grey=(2,))
    for ratios, flips in (([0.5, 2.0, None, 0.5], [0, 1, 1, 0]), ([2.0, 0.5, 1.0, 2.0], [1, 0, 0, 1])):
        p = R.params(rng, COCO_HW, S, ratios, flips)
        img, box = _image_only(ops, ims, p, S)
        refs = [R.transform(im, p[b], S) for b, im in enumerate(ims)]
        want = ops.normalize_img_u8(torch.from_numpy(np.stack([r["crop_u8"] for r in refs])).cuda())
        for b, r in enumerate(refs):
            assert torch.equal(img[b], want[b]), (b, S, float(p[b]["ratio"]), int(p[b]["flip"]))
            assert box[b].cpu().numpy().tolist() == r["img_box"].astype(int).tolist(), b
        assert float(np.abs(img.cpu().numpy() - np.stack([r["img_ref"] for r in refs])).max()) <= 2.4e-7
        if ratios[3] == 0.5:
            h, w = refs[3]["rescaled"]
            assert h < S and w < S                                     # padded on both axes
    assert img.shape == (4, 3, S, S) and img.dtype == torch.float32 and box.dtype == torch.int32


def test_equals_labelled_transform_when_candidate_0_is_accepted(ops):
    """Labels that let the cat_max_ratio rule accept candidate 0 (7-pixel stripes of two classes, balanced in every window at every
    scale): train_augment, with 10 different candidates, gives the image-only result bit for bit.  A single-class label rejects every
    candidate there (the 10th is taken), and the two then differ."""
    S = 320
    rng = np.random.default_rng(4)
    ims = _images(rng, COCO_HW)
    checker = [np.broadcast_to(((np.arange(w) // 7) % 2 + 1).astype(np.uint8), (h, w)).copy() for h, w in COCO_HW]
    p = R.params(rng, COCO_HW, S, [0.5, 2.0, 1.3, 0.5], [1, 0, 1, 0], distinct=True)
    img, box = _image_only(ops, ims, p, S)
    rb, plan = _packed(ops, ims, checker)
    img_l, _, box_l = ops.train_augment(rb.images.cuda(), plan, rb.labels.cuda(), p, S)
    assert torch.equal(img, img_l) and torch.equal(box, box_l)
    single = [np.full((h, w), 3, np.uint8) for h, w in COCO_HW]
    rb, plan = _packed(ops, ims, single)
    img_s, _, box_s = ops.train_augment(rb.images.cuda(), plan, rb.labels.cuda(), p, S)
    assert not torch.equal(box, box_s) or not torch.equal(img, img_s)


def test_refusals(ops):
    rng = np.random.default_rng(0)
    ims = _images(rng, [(60, 80)])
    rb, plan = _packed(ops, ims)
    p = R.params(rng, [(60, 80)], 32)
    with pytest.raises(ValueError, match="images_u8"):
        ops.train_augment_image(rb.images[:-3].cuda(), plan, p, 32)
    with pytest.raises(ValueError, match="crop_size"):
        ops.train_augment_image(rb.images.cuda(), plan, p, 0)


def test_non_default_stream_queued_behind_work(ops):
    rng = np.random.default_rng(9)
    hw = [(480, 640), (200, 180), (640, 427)]
    ims = _images(rng, hw)
    p = R.params(rng, hw, 320, flips=[1, 0, 1])
    ref = _image_only(ops, ims, p, 320)
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    a = torch.randn(4096, 4096, device="cuda")
    with torch.cuda.stream(s):
        for _ in range(4):
            a = a @ a * 1e-3                                          # keeps the stream busy while the call is queued behind it
        got = _image_only(ops, ims, p, 320)
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    for x, y in zip(got, ref):
        assert torch.equal(x, y)


def _tiny_model(num_classes=NUM_CLASSES, dec=None):
    from oracle.vit import VitConfig, make_vit_weights
    from excel_amd.model import ExCEL_model, init_decoder_state_dict
    TINY = VitConfig(width=128, layers=8, heads=2, patch=16, out_dim=64, input_resolution=64, n_surgery=5)
    kw = dict(width=128, layers=8, heads=2, patch=16, output_dim=64, input_resolution=64)
    rs = np.random.RandomState(3)
    text = rs.standard_normal((num_classes - 1 + 5, 64)).astype(np.float32)
    text /= np.linalg.norm(text, axis=1, keepdims=True)
    if dec is None:
        dec = init_decoder_state_dict(num_classes=num_classes, in_channels=128, embedding_dim=32, crop_size=96, seed=0, index=8)
    return ExCEL_model(clip_model="tiny", num_classes=num_classes, img_size=96, mode="train", state_dict=make_vit_weights(TINY, seed=11),
                       vit_cfg=kw, text_attr=text.T.copy(), gemm_mode="f32", embedding_dim=32, in_channels=128, decoder_state_dict=dec)


def test_trainer_with_coco_settings(ops, monkeypatch):
    """caa_thre 0.88, LVC from 30000 on (seg_attn + cure_attr_map on the head's features), the affinity target never the seg arg-max."""
    from excel_amd.scripts import train_coco, train_voc
    from excel_amd.utils.PAR import PAR
    calls = dict(cure=0, seg_attn=[], caa=set(), aff_src=[])
    real_cure, real_refine, real_losses = train_voc.cure_attr_map, train_voc.refine_cams_with_aff, ops.train_losses

    def cure(*a, **k):
        calls["cure"] += 1
        return real_cure(*a, **k)

    def refine(*a, seg_attn=None, caa_thre=None, **k):
        calls["seg_attn"].append(seg_attn is not None)
        calls["caa"].add(caa_thre)
        return real_refine(*a, seg_attn=seg_attn, caa_thre=caa_thre, **k)

    def losses(*a, aff_labels_u8=None, **k):
        calls["aff_src"].append(aff_labels_u8 is not None)
        return real_losses(*a, aff_labels_u8=aff_labels_u8, **k)

    monkeypatch.setattr(train_voc, "cure_attr_map", cure)
    monkeypatch.setattr(train_voc, "refine_cams_with_aff", refine)
    monkeypatch.setattr(ops, "train_losses", losses)
    rng = np.random.default_rng(2)
    x = ops.normalize_img_u8(torch.from_numpy(rng.integers(0, 256, (2, 96, 96, 3), dtype=np.uint8)).cuda())
    cls = torch.zeros((2, 80), dtype=torch.float32, device="cuda")
    cls[0, [0, 17]] = 1
    cls[1, 55] = 1
    C = train_coco.COCO
    tr = train_voc.DecoderTrainer(_tiny_model(), PAR(num_iter=10, dilations=[1, 2, 4, 8, 12, 24]), lr=1e-3, warmup_iters=2,
                                  max_iters=100000, radius=2, caa_thre=C.caa_thre, lvc_iter=C.lvc_iter, seg_aff_iter=C.seg_aff_iter)
    for n_iter in (29999, 30000, 99999):
        out = tr.train_step(x, cls, n_iter)
        assert np.isfinite(out["seg_loss"]) and np.isfinite(out["diver_loss"])
    assert calls["cure"] == 2                                         # 30000 and 99999, not 29999
    assert calls["seg_attn"] == [False, False, True, True, True, True]
    assert calls["caa"] == {0.88}
    assert calls["aff_src"] == [False, False, False]                  # the affinity loss always takes the pseudo labels
    # control: the VOC settings do switch the affinity target at 24000
    tv = train_voc.DecoderTrainer(_tiny_model(), PAR(num_iter=10, dilations=[1, 2, 4, 8, 12, 24]), lr=1e-3, warmup_iters=2,
                                  max_iters=100000, radius=2)
    tv.train_step(x, cls, 30000)
    assert calls["aff_src"][-1] is True


def _coco_tree(tmp_path, n_train=8, n_val=3, seed=0):
    """The reference's layout: JPEGImages/{train,val}, SegmentationClass/val only, COCO_train2014_ / COCO_val2014_ names."""
    from PIL import Image
    rng = np.random.default_rng(seed)
    root = tmp_path / "COCO"
    for d in ("JPEGImages/train", "JPEGImages/val", "SegmentationClass/val"):
        (root / d).mkdir(parents=True)
    onehot, train, val = {}, [], []
    for i in range(n_train + n_val):
        is_val = i >= n_train
        name = f"COCO_val2014_{i:012d}" if is_val else f"COCO_train2014_{i:012d}"
        h, w = int(rng.integers(60, 150)), int(rng.integers(60, 150))
        yy, xx = np.mgrid[0:h, 0:w]
        base = 127 + 100 * np.sin(xx / (3.0 + i)) * np.cos(yy / 4.0)
        im = np.clip(base[..., None] + rng.integers(-30, 30, (h, w, 3)), 0, 255).astype(np.uint8)
        Image.fromarray(im[..., 0] if i == 2 else im).save(root / "JPEGImages" / ("val" if is_val else "train") / f"{name}.jpg", quality=90)
        c = 1 + (7 * i) % 80
        oh = np.zeros(80, np.float32)
        oh[c - 1] = 1
        if is_val:
            lab = np.zeros((h, w), np.uint8)
            lab[h // 4:3 * h // 4, w // 4:3 * w // 4] = c
            lab[0, :] = 255
            Image.fromarray(lab, mode="L").save(root / "SegmentationClass" / "val" / f"{name[13:]}.png")
        onehot[name] = oh
        (val if is_val else train).append(name)
    lists = tmp_path / "lists"
    lists.mkdir()
    (lists / "train.txt").write_text("\n".join(train) + "\n")
    (lists / "val_part.txt").write_text("\n".join(val) + "\n")
    np.save(lists / "cls_labels_onehot.npy", onehot)
    return str(root), str(lists)


def _args(root, lists, work_dir):
    from excel_amd.scripts.train_coco import get_parser
    return get_parser().parse_args(["--data_folder", root, "--list_folder", lists, "--crop_size", "96", "--spg", "2", "--max_iters", "6",
                                    "--eval_iters", "3", "--log_iters", "2", "--radius", "2", "--work_dir", work_dir, "--num_workers", "2",
                                    "--seed", "5", "--save_ckpt_from", "6"])


@pytest.mark.timeout(900)
def test_train_coco_end_to_end(ops, tmp_path, caplog):
    from excel_amd.datasets import coco
    from excel_amd.scripts.train_coco import train
    from excel_amd.tools import infer_lam, infer_seg_coco
    root, lists = _coco_tree(tmp_path)
    assert not os.path.exists(os.path.join(root, "SegmentationClass", "train"))
    caplog.set_level(logging.INFO)
    model = _tiny_model()
    a = _args(root, lists, str(tmp_path / "run1"))
    assert (a.num_classes, a.train_set, a.val_set) == (81, "train", "val_part")
    res = train(a, model=model)
    hist = res["history"]
    assert len(hist) == 6 and all(np.isfinite(h["seg_loss"]) and np.isfinite(h["diver_loss"]) for h in hist)
    ck = str(tmp_path / "run1" / "checkpoints" / "model_iter_6.pth")
    assert res["ckpts"] == [ck] and os.path.isfile(ck)                # iteration 3 validates but is below --save_ckpt_from
    assert len(res["tables"]) == 2
    for t in res["tables"]:
        assert "Seg_Preds" in t and "Attr_aff_Pseudo" in t and "traffic light" in t and "toothbrush" in t
    assert "Iter: 2; Elasped:" in caplog.text

    # the checkpoint through infer_seg_coco: the loader of --model_path, then the COCO evaluation on the val tree
    sd = torch.load(ck, map_location="cpu")
    ns = infer_lam.get_parser().parse_args(["--training_free", "false", "--synthetic", "2", "--model_path", ck])
    loaded = _tiny_model(dec=infer_lam.resolve_model_inputs(ns)["decoder_state_dict"])
    assert set(infer_lam.resolve_model_inputs(ns)["decoder_state_dict"]) == {k for k in sd if k.startswith(("decoder_fts_fuse.", "decoder."))}
    x = torch.randn(2, 3, 96, 96, generator=torch.Generator().manual_seed(0)).cuda()
    assert torch.equal(model.seg_logits(x), loaded.seg_logits(x))
    ev = infer_seg_coco.get_parser().parse_args(["--data_folder", root, "--list_folder", lists, "--model_path", ck, "--infer_set",
                                                 "val_part", "--resize_size", "96", "--scales", "1.0,0.5", "--gemm_check", "false",
                                                 "--num_workers", "2", "--batch_size", "2", "--crf_post", "false"])
    r_loaded = infer_seg_coco.validate(ev, model=loaded)
    r_mem = infer_seg_coco.validate(ev, model=model)
    assert r_loaded["images"] == 3 and torch.equal(r_loaded["hist"], r_mem["hist"])
    assert int(r_loaded["hist"].sum()) == sum(int(np.asarray(coco.CocoSegDataset(root, lists, "val_part")[i][2] != 255).sum())
                                              for i in range(3))

    # same seed, fresh model: the same loss history and the same checkpoint
    res2 = train(_args(root, lists, str(tmp_path / "run2")), model=_tiny_model())
    assert open(tmp_path / "run1" / "losses.txt").read() == open(tmp_path / "run2" / "losses.txt").read()
    assert [(h["seg_loss"], h["diver_loss"]) for h in res2["history"]] == [(h["seg_loss"], h["diver_loss"]) for h in hist]
    sd2 = torch.load(res2["ckpts"][0], map_location="cpu")
    assert set(sd2) == set(sd) and all(torch.equal(sd[k], sd2[k]) for k in sd)
