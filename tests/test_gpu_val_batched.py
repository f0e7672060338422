"""The batched, rank-sharded validation pass of the training programs (engine/validatation_engine.build_validation_ragged over
pipeline.ValidationPipeline) against the reference's per-image loop (build_validation): the same two confusion matrices bit for bit and the
same table, for VOC- and COCO-like trees, batch sizes 1 / 3 / larger than the set, f32 and the handle's default fast mode; sharding over
ranks; the uniform-source seg resize + arg-max kernel; the training programs with either validation path."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

VOC_NC = 5
# all different, one portrait, one square, one whose size differs from every other in both axes (33 x 47)
VOC_VAL_HW = [(75, 100), (100, 75), (64, 64), (90, 120), (57, 83), (120, 90), (33, 47), (96, 96)]
COCO_VAL_HW = [(80, 110), (110, 80), (70, 70), (96, 130), (50, 61)]


@pytest.fixture(scope="module")
def gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import excel_amd.ops  # noqa: F401  (raises if libexcel_hip.so is missing: no fallback)
    return True


def _image(rng, h, w, i):
    yy, xx = np.mgrid[0:h, 0:w]
    base = 127 + 100 * np.sin(xx / (3.0 + i)) * np.cos(yy / (4.0 + i % 3))
    return np.clip(base[..., None] + rng.integers(-30, 30, (h, w, 3)), 0, 255).astype(np.uint8)


def _label(rng, h, w, classes):
    """background, one vertical band per present class, a 255 row band and scattered 255 pixels"""
    lab = np.zeros((h, w), np.uint8)
    k = len(classes)
    for j, c in enumerate(classes):
        lab[h // 6:5 * h // 6, (j * w) // (k + 1) + w // (2 * (k + 1)):((j + 1) * w) // (k + 1) + w // (2 * (k + 1))] = c
    lab[h // 3:h // 3 + 2, :] = 255
    lab[rng.random((h, w)) < 0.02] = 255
    return lab


def _voc_tree(tmp_path, val_hw=VOC_VAL_HW, n_train=8, seed=0):
    """VOC layout (JPEGImages/, SegmentationClassAug/, <split>.txt, cls_labels_onehot.npy) with VOC_NC classes; val image i has
    1 + i % 4 present classes."""
    from PIL import Image
    rng = np.random.default_rng(seed)
    root = tmp_path / "VOC"
    (root / "JPEGImages").mkdir(parents=True)
    (root / "SegmentationClassAug").mkdir()
    onehot, train, val = {}, [], []
    hws = [(int(rng.integers(60, 150)), int(rng.integers(60, 150))) for _ in range(n_train)] + list(val_hw)
    for i, (h, w) in enumerate(hws):
        is_val = i >= n_train
        name = f"2008_{i:06d}"
        k = 1 + (i - n_train) % 4 if is_val else 1
        classes = sorted(rng.choice(np.arange(1, VOC_NC), size=k, replace=False).tolist())
        Image.fromarray(_image(rng, h, w, i)).save(root / "JPEGImages" / f"{name}.jpg", quality=90)
        png = Image.fromarray(_label(rng, h, w, classes), mode="P")
        png.putpalette(list(rng.integers(0, 256, 768, dtype=np.uint8)))
        png.save(root / "SegmentationClassAug" / f"{name}.png")
        oh = np.zeros(VOC_NC - 1, np.float32)
        oh[np.asarray(classes) - 1] = 1
        onehot[name] = oh
        (val if is_val else train).append(name)
    lists = tmp_path / "lists"
    lists.mkdir()
    (lists / "train.txt").write_text("\n".join(train) + "\n")
    (lists / "val.txt").write_text("\n".join(val) + "\n")
    np.save(lists / "cls_labels_onehot.npy", onehot)
    return str(root), str(lists)


def _coco_tree(tmp_path, val_hw=COCO_VAL_HW, n_train=8, seed=1):
    """COCO layout (JPEGImages/{train,val}, SegmentationClass/val); val images carry 7..11 present classes of 80."""
    from PIL import Image
    rng = np.random.default_rng(seed)
    root = tmp_path / "COCO"
    for d in ("JPEGImages/train", "JPEGImages/val", "SegmentationClass/val"):
        (root / d).mkdir(parents=True)
    onehot, train, val = {}, [], []
    hws = [(int(rng.integers(60, 150)), int(rng.integers(60, 150))) for _ in range(n_train)] + list(val_hw)
    for i, (h, w) in enumerate(hws):
        is_val = i >= n_train
        name = f"COCO_val2014_{i:012d}" if is_val else f"COCO_train2014_{i:012d}"
        k = 7 + (i - n_train) % 5 if is_val else 1
        classes = sorted(rng.choice(np.arange(1, 81), size=k, replace=False).tolist())
        im = _image(rng, h, w, i)
        Image.fromarray(im[..., 0] if i == n_train + 1 else im).save(root / "JPEGImages" / ("val" if is_val else "train") / f"{name}.jpg",
                                                                      quality=90)
        if is_val:
            Image.fromarray(_label(rng, h, w, classes), mode="L").save(root / "SegmentationClass" / "val" / f"{name[13:]}.png")
        oh = np.zeros(80, np.float32)
        oh[np.asarray(classes) - 1] = 1
        onehot[name] = oh
        (val if is_val else train).append(name)
    lists = tmp_path / "lists"
    lists.mkdir()
    (lists / "train.txt").write_text("\n".join(train) + "\n")
    (lists / "val_part.txt").write_text("\n".join(val) + "\n")
    np.save(lists / "cls_labels_onehot.npy", onehot)
    return str(root), str(lists)


def _tiny_model(num_classes=VOC_NC, gemm_mode="f32", head_seed=0):
    from oracle.vit import VitConfig, make_vit_weights
    from excel_amd.model import ExCEL_model, init_decoder_state_dict
    TINY = VitConfig(width=128, layers=8, heads=2, patch=16, out_dim=64, input_resolution=64, n_surgery=5)
    kw = dict(width=128, layers=8, heads=2, patch=16, output_dim=64, input_resolution=64)
    rs = np.random.RandomState(3)
    text = rs.standard_normal((num_classes - 1 + 5, 64)).astype(np.float32)
    text /= np.linalg.norm(text, axis=1, keepdims=True)
    dec = init_decoder_state_dict(num_classes=num_classes, in_channels=128, embedding_dim=32, crop_size=96, seed=head_seed, index=8)
    return ExCEL_model(clip_model="tiny", num_classes=num_classes, img_size=96, mode="train", state_dict=make_vit_weights(TINY, seed=11),
                       vit_cfg=kw, text_attr=text.T.copy(), gemm_mode=gemm_mode, embedding_dim=32, in_channels=128, decoder_state_dict=dec)


def _par():
    from excel_amd.utils.PAR import PAR
    return PAR(num_iter=20, dilations=[1, 2, 4, 8, 12, 24])


def _per_image(model, dataset, nc, class_list=None, S=96):
    """build_validation as train() runs it with --val_api_path true -> (table, aff hist, seg hist)"""
    from excel_amd.engine.validatation_engine import build_validation
    from excel_amd.scripts.train_voc import _val_batches
    from excel_amd.utils import evaluate
    captured = []
    orig = evaluate.scores_from_hist

    def spy(h):
        captured.append(h.clone())
        return orig(h)
    evaluate.scores_from_hist = spy
    try:
        table = build_validation(model=model, par=_par(), val_loader=_val_batches(dataset, "cuda"), device="cuda", num_classes=nc,
                                 resize_size=S, class_list=class_list)[0]
    finally:
        evaluate.scores_from_hist = orig
    assert len(captured) == 2
    return table, captured[0], captured[1]


def _batched(model, dataset, nc, batch_size, class_list=None, S=96, rank=0, world=1):
    from excel_amd.engine.validatation_engine import build_validation_ragged
    return build_validation_ragged(model=model, par=_par(), dataset=dataset, device="cuda", num_classes=nc, resize_size=S,
                                   class_list=class_list, batch_size=batch_size, num_workers=2, rank=rank, world=world, group=None)


def _voc_val(root, lists):
    from excel_amd.datasets import voc
    return voc.VOC12SegDataset(root_dir=root, name_list_dir=lists, split="val", stage="val")


def _scored_pixels(dataset):
    return sum(int((np.asarray(dataset[i][2]) != 255).sum()) for i in range(len(dataset)))


# ------------------------------------------------------------------ the kernel entry
def test_seg_resize_argmax_uniform_equals_resize_then_argmax(gpu):
    """excel_seg_resize_argmax_uniform over a tight [B,nc,g,g] source (g = 6: no multiple of 4, so NOT the pitched layout) equals
    bilinear_resize + argmax_label per image, for 5 and 81 classes and label sizes smaller and larger than the source."""
    from excel_amd import ops
    rng = np.random.default_rng(7)
    hw = [(75, 100), (5, 4), (33, 47), (6, 6), (120, 90)]
    plan = ops.RaggedPlan(hw, "cuda")
    for nc, g in ((5, 6), (81, 6), (21, 20)):
        segs = torch.from_numpy(rng.standard_normal((len(hw), nc, g, g)).astype(np.float32)).cuda()
        segs[0, 1] = segs[0, 0]                                        # ties: the first maximum wins in both
        lab = ops.seg_resize_argmax_uniform(segs, plan)
        assert lab.dtype == torch.uint8 and lab.numel() == plan.total_label_pix
        for b, (h, w) in enumerate(hw):
            want = ops.argmax_label(ops.bilinear_resize(segs[b:b + 1], h, w, align_corners=False))[0]
            assert torch.equal(plan.label(lab, b), want), (nc, g, b)
    with pytest.raises(ValueError):
        ops.seg_resize_argmax_uniform(segs[:2], plan)


# ------------------------------------------------------------------ bit-identity with the per-image loop
@pytest.mark.parametrize("gemm_mode", ["f32", None])
def test_voc_batched_equals_per_image(gpu, tmp_path, gemm_mode):
    """VOC-like set, 8 images of 8 sizes, 1-4 present classes: batch sizes 1, 3 and 16 (> the set) give build_validation's two
    matrices and table bit for bit, in exact f32 and in the handle's default fast mode."""
    from excel_amd.datasets import voc
    root, lists = _voc_tree(tmp_path)
    ds = _voc_val(root, lists)
    assert len(ds) == len(VOC_VAL_HW) and sorted({int(ds[i][3].sum()) for i in range(len(ds))}) == [1, 2, 3, 4]
    model = _tiny_model(gemm_mode=gemm_mode)
    mode = model.encoder.visual.handle().gemm_mode()
    assert mode == "f32" if gemm_mode == "f32" else mode != "f32"
    cats = voc.class_list[:VOC_NC]
    table, h_aff, h_seg = _per_image(model, ds, VOC_NC, cats)
    assert int(h_aff.sum()) == int(h_seg.sum()) == _scored_pixels(ds)
    assert int(h_aff.diagonal().sum()) > 0
    for bs in (1, 3, 16):
        t, _, _, out = _batched(model, ds, VOC_NC, bs, cats)
        assert out["images"] == len(ds)
        assert torch.equal(out["hist_aff"], h_aff), (bs, mode)
        assert torch.equal(out["hist_seg"], h_seg), (bs, mode)
        assert t == table


@pytest.mark.parametrize("gemm_mode", ["f32", None])
def test_coco_config_batched_equals_per_image(gpu, tmp_path, gemm_mode):
    """81 classes, 7-11 present classes per image (more than VOC's 6), COCO's reader and class names: the same equality."""
    from excel_amd.datasets import coco
    root, lists = _coco_tree(tmp_path)
    ds = coco.CocoSegDataset(root_dir=root, name_list_dir=lists, split="val_part", stage="val")
    assert min(int(ds[i][3].sum()) for i in range(len(ds))) > 6
    model = _tiny_model(num_classes=81, gemm_mode=gemm_mode)
    table, h_aff, h_seg = _per_image(model, ds, 81, coco.class_list)
    assert int(h_aff.sum()) == _scored_pixels(ds)
    for bs in (3, 8):
        t, _, _, out = _batched(model, ds, 81, bs, coco.class_list)
        assert torch.equal(out["hist_aff"], h_aff) and torch.equal(out["hist_seg"], h_seg), bs
        assert t == table


# ------------------------------------------------------------------ sharding
def test_sharded_ranks_sum_to_the_unsharded_pass(gpu, tmp_path, monkeypatch):
    """Ranks r of world 2 and 3 (called in one process, no process group): disjoint shards r, r+R, ... that cover the set, matrices
    that sum to the unsharded run's; world 10 > 8 images: the empty ranks return zero matrices."""
    from excel_amd.datasets import loader
    root, lists = _voc_tree(tmp_path)
    ds = _voc_val(root, lists)
    model = _tiny_model()
    _, _, _, full = _batched(model, ds, VOC_NC, 3)
    seen = []
    orig = loader.threaded_batches

    def spy(dataset, indices, *a, **k):
        seen.append([int(i) for i in indices])
        return orig(dataset, indices, *a, **k)
    monkeypatch.setattr(loader, "threaded_batches", spy)
    for world in (2, 3, 10):
        seen.clear()
        aff = torch.zeros_like(full["hist_aff"])
        seg = torch.zeros_like(full["hist_seg"])
        nimg = 0
        for r in range(world):
            _, _, _, out = _batched(model, ds, VOC_NC, 2, rank=r, world=world)
            aff += out["hist_aff"]
            seg += out["hist_seg"]
            nimg += out["images"]
            if r >= len(ds):
                assert out["images"] == 0 and int(out["hist_aff"].abs().sum()) == 0 and int(out["hist_seg"].abs().sum()) == 0
        flat = [i for s in seen for i in s]
        assert sorted(flat) == list(range(len(ds))) and len(set(flat)) == len(flat), world      # disjoint, covering
        assert all(s == list(range(r, len(ds), world)) for r, s in enumerate(seen)), world
        assert nimg == len(ds)
        assert torch.equal(aff, full["hist_aff"]) and torch.equal(seg, full["hist_seg"]), world


def test_pipeline_refuses_a_model_without_decoder(gpu):
    from oracle.vit import VitConfig, make_vit_weights
    from excel_amd.model import ExCEL_model
    from excel_amd.pipeline import ValidationPipeline
    TINY = VitConfig(width=128, layers=8, heads=2, patch=16, out_dim=64, input_resolution=64, n_surgery=5)
    model = ExCEL_model(clip_model="tiny", num_classes=5, img_size=96, mode="train", state_dict=make_vit_weights(TINY, seed=11),
                        vit_cfg=dict(width=128, layers=8, heads=2, patch=16, output_dim=64, input_resolution=64),
                        text_attr=np.eye(64, 9, dtype=np.float32))
    with pytest.raises(ValueError, match="decoder"):
        ValidationPipeline(model, num_classes=5)


def test_too_many_present_classes_is_refused(gpu, tmp_path):
    """An image with more present classes than dataset.max_k() is refused on the host (not silently truncated), and the decode
    threads and the feeder are gone afterwards."""
    import threading
    root, lists = _voc_tree(tmp_path)
    ds = _voc_val(root, lists)
    ds.max_k = lambda: 2
    before = {t.ident for t in threading.enumerate()}
    with pytest.raises(RuntimeError, match="present classes"):
        _batched(_tiny_model(), ds, VOC_NC, 3)
    left = [t for t in threading.enumerate() if t.ident not in before and t.is_alive()]
    assert not left, [t.name for t in left]


# ------------------------------------------------------------------ the programs
def _program_args(prog, root, lists, work_dir, extra):
    base = ["--data_folder", root, "--list_folder", lists, "--crop_size", "96", "--spg", "2", "--max_iters", "6", "--eval_iters", "3",
            "--log_iters", "2", "--radius", "2", "--work_dir", work_dir, "--num_workers", "2", "--seed", "5"]
    if prog.__name__.endswith("train_voc"):
        base += ["--train_set", "train", "--val_set", "val", "--num_classes", str(VOC_NC)]
    else:
        base += ["--save_ckpt_from", "3"]
    return prog.get_parser().parse_args(base + extra)


@pytest.mark.timeout(1200)
@pytest.mark.parametrize("program", ["voc", "coco"])
def test_programs_same_results_with_either_validation_path(gpu, tmp_path, program):
    """train_voc.train / train_coco.train with the default (batched) validation and with --val_api_path true: identical tables,
    identical losses.txt, bit-identical checkpoints; the per-pass seconds are reported."""
    from excel_amd.scripts import train_coco, train_voc
    prog = train_voc if program == "voc" else train_coco
    nc = VOC_NC if program == "voc" else 81
    root, lists = (_voc_tree if program == "voc" else _coco_tree)(tmp_path)
    runs = {}
    for tag, extra in (("batched", []), ("api", ["--val_api_path", "true"])):
        a = _program_args(prog, root, lists, str(tmp_path / tag), extra)
        assert a.val_api_path is (tag == "api")
        runs[tag] = prog.train(a, model=_tiny_model(num_classes=nc))
    b, p = runs["batched"], runs["api"]
    assert len(b["tables"]) == 2 and b["tables"] == p["tables"]
    assert all("Seg_Preds" in t and "Attr_aff_Pseudo" in t for t in b["tables"])
    assert len(b["val_seconds"]) == len(p["val_seconds"]) == 2 and all(s > 0 for s in b["val_seconds"] + p["val_seconds"])
    assert [(h["seg_loss"], h["diver_loss"], h["lr"]) for h in b["history"]] == [(h["seg_loss"], h["diver_loss"], h["lr"]) for h in p["history"]]
    lb = open(tmp_path / "batched" / "losses.txt").read()
    assert lb == open(tmp_path / "api" / "losses.txt").read() and len(lb.splitlines()) == 6
    assert [os.path.basename(c) for c in b["ckpts"]] == [os.path.basename(c) for c in p["ckpts"]] == ["model_iter_3.pth", "model_iter_6.pth"]
    for cb, cp in zip(b["ckpts"], p["ckpts"]):
        sb, sp = torch.load(cb, map_location="cpu"), torch.load(cp, map_location="cpu")
        assert set(sb) == set(sp) and sb and all(torch.equal(sb[k], sp[k]) for k in sb), cb
