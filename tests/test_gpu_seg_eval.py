"""Segmentation evaluation on the device: the three ragged kernels of segeval.hip against the existing per-image chain (bit for bit) and
float64 restatements, ExCEL_model.seg_logits, and the VOC / COCO evaluation programs end to end on tiny on-disk trees."""
import os
import time

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

# ragged sizes: W % 4 != 0, W = 1 and 2, H = 1, and both up- and down-sampling against the g values below
SIZES = [(37, 50), (5, 2), (16, 1), (70, 131), (1, 7)]
GS = [4, 9, 13, 6]


@pytest.fixture(scope="module")
def gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from excel_amd import _lib
    _lib.lib()
    return torch.device("cuda")


def _chain(segs, flips, b, B, H, W):
    """Image b alone through the existing per-scale excel_seg_scale_accumulate calls (tools/infer_seg_voc.multi_scale_seg's chain)."""
    from excel_amd import ops
    acc = None
    ns = len(segs)
    for i, (s, f) in enumerate(zip(segs, flips)):
        two = s[[b, B + b]].contiguous()
        acc = ops.seg_scale_accumulate(two, acc, H, W, flip_mean=f, init=(i == 0), scale=(1.0 / ns) if i == ns - 1 else 1.0)
    return acc


def _oracle_fuse(segs, flips, b, B, H, W):
    from oracle.interp import bilinear_resize
    acc = 0.0
    for s, f in zip(segs, flips):
        a = s[b].cpu().numpy()
        v = bilinear_resize(a, H, W).astype(np.float64)
        if f:
            v = (v + bilinear_resize(s[B + b].cpu().numpy(), H, W).astype(np.float64)[..., ::-1]) / 2
        acc = acc + v
    return acc / len(segs)


@pytest.mark.parametrize("nc", [5, 21, 81])
@pytest.mark.parametrize("flavour", ["voc", "coco"])
def test_msc_fuse_matches_per_image_chain(gpu, nc, flavour):
    from excel_amd import ops
    B = len(SIZES)
    g = torch.Generator().manual_seed(nc)
    segs = [(torch.randn(2 * B, nc, k, k, generator=g) * 3).to(gpu) for k in GS]
    flips = [True] * len(GS) if flavour == "coco" else [False, True, True, True]
    plan = ops.RaggedPlan(SIZES, gpu)
    planes, labels = ops.seg_msc_fuse_ragged(segs, flips, plan, want_planes=True, want_labels=True, label_hw=SIZES)
    _, labels_only = ops.seg_msc_fuse_ragged(segs, flips, plan, want_planes=False, want_labels=True, label_hw=SIZES)
    assert torch.equal(labels, labels_only)
    for b, (H, W) in enumerate(SIZES):
        ref = _chain(segs, flips, b, B, H, W)
        got = plan.planes(planes, b, nc)
        assert torch.equal(got, ref[0]), f"image {b} ({H}x{W}): planes differ from the seg_scale_accumulate chain"
        assert torch.equal(plan.label(labels, b), ops.argmax_label(ref)[0])
        o = _oracle_fuse(segs, flips, b, B, H, W)
        err = np.abs(got.cpu().numpy().astype(np.float64) - o).max() / np.abs(o).max()
        assert err <= 1e-5, err


def test_msc_fuse_refusals(gpu):
    from excel_amd import ops
    plan = ops.RaggedPlan(SIZES, gpu)
    segs = [torch.randn(2 * len(SIZES), 5, 4, 4, device=gpu)]
    with pytest.raises(ValueError, match="label sizes differ"):
        ops.seg_msc_fuse_ragged(segs, [False], plan, want_labels=True, label_hw=[(h + 1, w) for h, w in SIZES])
    with pytest.raises(ValueError):
        ops.seg_msc_fuse_ragged(segs * 9, [False] * 9, plan)
    with pytest.raises(ValueError):
        ops.seg_msc_fuse_ragged([torch.randn(4, 5, 4, 4, device=gpu)], [False], plan)


@pytest.mark.parametrize("nc", [5, 21, 81])
def test_resize_argmax_matches_resize_then_argmax(gpu, nc):
    from excel_amd import ops
    src_hw = [(7, 10), (5, 2), (16, 1), (14, 26), (3, 3)]
    dst_hw = [(37, 50), (5, 2), (9, 3), (70, 131), (1, 7)]       # up, identity, down / mixed, up, mixed
    src, dst = ops.RaggedPlan(src_hw, gpu), ops.RaggedPlan(dst_hw, gpu)
    planes = torch.randn(nc * src.total_pix, generator=torch.Generator().manual_seed(nc)).to(gpu)
    lab = ops.seg_resize_argmax_ragged(planes, src, dst, nc)
    for b, (H, W) in enumerate(dst_hw):
        one = src.planes(planes, b, nc).contiguous()[None]
        ref = ops.argmax_label(ops.bilinear_resize(one, H, W))[0]
        assert torch.equal(dst.label(lab, b), ref), f"image {b}"
    with pytest.raises(ValueError):
        ops.seg_resize_argmax_ragged(planes, src, ops.RaggedPlan(dst_hw[:2], gpu), nc)


@pytest.mark.parametrize("nc", [5, 21, 81])
def test_softmax_resize(gpu, nc):
    from excel_amd import ops
    hw = [(7, 10), (13, 5), (9, 1)]
    targets = [(37, 50), (13, 5), (4, 3)]                       # up, identity (no resize), down
    plan = ops.RaggedPlan(hw, gpu)
    # logits of unit scale: the float32 bilinear blend (F.interpolate's arithmetic on float32 maps) then stays well inside the bound
    planes = torch.randn(nc * plan.total_pix, generator=torch.Generator().manual_seed(nc)).to(gpu)
    for b, (H, W) in enumerate(targets):
        prob = ops.seg_softmax_resize(planes, plan, b, nc, H, W)
        x = plan.planes(planes, b, nc).cpu().double()[None]
        if (H, W) != tuple(hw[b]):
            x = torch.nn.functional.interpolate(x, size=(H, W), mode="bilinear", align_corners=False)
        ref = torch.softmax(x[0], dim=0)
        got = prob.cpu().double()
        assert got.shape == (nc, H, W)
        assert (got - ref).abs().max().item() <= 1e-6
        assert (got.sum(0) - 1).abs().max().item() <= 1e-6


# ------------------------------------------------------------------ the model and the programs
NUM_CLASSES = 5


def _tiny_model(dec=None, mode="f32"):
    from oracle.vit import VitConfig, make_vit_weights
    from excel_amd.model import ExCEL_model, init_decoder_state_dict
    TINY = VitConfig(width=128, layers=8, heads=2, patch=16, out_dim=64, input_resolution=64, n_surgery=5)
    kw = dict(width=128, layers=8, heads=2, patch=16, output_dim=64, input_resolution=64)
    rs = np.random.RandomState(3)
    text = rs.standard_normal((9, 64)).astype(np.float32)
    text /= np.linalg.norm(text, axis=1, keepdims=True)
    if dec is None:
        dec = init_decoder_state_dict(num_classes=NUM_CLASSES, in_channels=128, embedding_dim=32, crop_size=96, seed=0, index=8)
    return ExCEL_model(clip_model="tiny", num_classes=NUM_CLASSES, img_size=64, mode="val", state_dict=make_vit_weights(TINY, seed=11),
                       vit_cfg=kw, text_attr=text.T.copy(), gemm_mode=mode, embedding_dim=32, in_channels=128, decoder_state_dict=dec)


@pytest.mark.parametrize("mode", ["f32", "bf16x3"])
def test_seg_logits_equals_forward(gpu, mode):
    model = _tiny_model(mode=mode)
    for S in (64, 48, 96):
        x = torch.randn(4, 3, S, S, generator=torch.Generator().manual_seed(S)).to(gpu)
        seg = model.seg_logits(x)
        assert torch.equal(seg, model(x)[0])


# tree: varied sizes (odd widths, one with W % 4 == 1), two grey JPEGs
TREE = [(37, 53, False), (41, 30, True), (25, 66, False), (50, 43, False), (33, 29, True)]


def _tree(tmp_path, coco=False):
    from PIL import Image
    rng = np.random.default_rng(7)
    root = tmp_path / ("COCO" if coco else "VOC")
    img_dir = root / "JPEGImages" / ("val" if coco else "")
    lab_dir = root / ("SegmentationClass" if coco else "SegmentationClassAug") / ("val" if coco else "")
    img_dir.mkdir(parents=True)
    lab_dir.mkdir(parents=True)
    onehot, names = {}, []
    for i, (h, w, grey) in enumerate(TREE):
        name = f"COCO_val2014_{i:012d}" if coco else f"2007_{i:06d}"
        # smooth images: the tiny head's logits then have structure, so labels are not all one class
        yy, xx = np.mgrid[0:h, 0:w]
        base = (127 + 100 * np.sin(xx / (3.0 + i)) * np.cos(yy / 4.0)).astype(np.float64)
        im = np.clip(base[..., None] + rng.integers(-30, 30, (h, w, 3)), 0, 255).astype(np.uint8)
        Image.fromarray(im[..., 0] if grey else im).save(img_dir / f"{name}.jpg", quality=90)
        lab = rng.integers(0, NUM_CLASSES, (h, w)).astype(np.uint8)
        lab[0, :] = 255
        Image.fromarray(lab, mode="L").save(lab_dir / f"{(name[13:] if coco else name)}.png")
        oh = np.zeros(NUM_CLASSES - 1, np.float32)
        oh[i % (NUM_CLASSES - 1)] = 1
        onehot[name] = oh
        names.append(name)
    lists = tmp_path / "lists"
    lists.mkdir(exist_ok=True)
    (lists / "val.txt").write_text("\n".join(names) + "\n")
    (lists / "test.txt").write_text("\n".join(names) + "\n")
    np.save(lists / "cls_labels_onehot.npy", onehot)
    return str(root), str(lists), names


def _args(mod, root, lists, ckpt, *extra):
    return mod.get_parser().parse_args(["--data_folder", root, "--test_data_folder", root, "--list_folder", lists, "--model_path", ckpt,
                                        "--num_classes", str(NUM_CLASSES), "--resize_size", "64", "--scales", "1.0,0.75,1.5",
                                        "--gemm_check", "false", "--num_workers", "2", *extra])


def _restate(model, dataset, i, variant, nc, scales=(1.0, 0.75, 1.5), resize_size=64):
    """The reference's per-image loop from the existing uniform library: -> (fused logits [1,nc,h,w], labels [H,W] u8)."""
    from excel_amd import ops
    from excel_amd.tools.infer_seg_voc import multi_scale_seg, seg_labels
    _, image, label, _ = dataset[i]
    inputs = ops.normalize_img_u8(torch.from_numpy(image)[None].cuda())
    H, W = label.shape
    if variant.fuse_factor is None:
        msc = multi_scale_seg(model, inputs, resize_size, scales)
    else:                                                              # COCO: every scale flip-averaged at (int(0.2h), int(0.2w))
        fh, fw = variant.fuse_size(H, W)
        todo = [1.0] + [s for s in scales if s != 1.0]
        msc = None
        for k, sc in enumerate(todo):
            S = resize_size if sc == 1.0 else int(resize_size * sc)
            x = ops.bilinear_resize(inputs, S, S)
            segs = model(torch.cat([x, x.flip(-1)], dim=0))[0]
            msc = ops.seg_scale_accumulate(segs, msc, fh, fw, flip_mean=True, init=(k == 0),
                                           scale=(1.0 / len(todo)) if k == len(todo) - 1 else 1.0)
    return msc, seg_labels(msc, (H, W))[0]


def _check_program(tmp_path, mod, variant, coco):
    from PIL import Image
    from excel_amd import ops
    from excel_amd.utils.dcrf import DenseCRF
    from excel_amd.tools.infer_seg_voc import CRF_PARAMS
    root, lists, names = _tree(tmp_path, coco=coco)
    ckpt = str(tmp_path / "run" / "checkpoints" / "model_iter_8.pth")
    model = _tiny_model()
    ds = variant.dataset(_args(mod, root, lists, ckpt), "val")
    nc = NUM_CLASSES
    ref_hist = torch.zeros((nc, nc), dtype=torch.int64, device="cuda")
    restated = []
    for i in range(len(ds)):
        msc, lab = _restate(model, ds, i, variant, nc)
        restated.append((msc, lab))
        ref_hist = ops.confusion_accumulate(torch.from_numpy(ds[i][2]).cuda(), lab, nc, ref_hist)
    times = {}
    for bs in (1, 3):
        t0 = time.time()
        res = mod.validate(_args(mod, root, lists, ckpt, "--batch_size", str(bs), "--crf_post", "false"), model=model)
        times[bs] = time.time() - t0
        assert torch.equal(res["hist"], ref_hist), f"batch {bs}"
        assert res["crf_score"] is None and res["images"] == len(names)
    print(f"\n{variant.name} program wall time: batch 1 {times[1]:.2f} s, batch 3 {times[3]:.2f} s")
    # --crf_post: PNGs at image size; CRF labels = DenseCRF on a torch softmax of the restated logits where its margin allows
    res = mod.validate(_args(mod, root, lists, ckpt, "--batch_size", "3", "--crf_post", "true"), model=model)
    assert torch.equal(res["hist"], ref_hist)
    d = res["dirs"]
    assert os.path.isfile(d["log"]) and "crf_seg_score" in open(d["log"]).read()
    assert not os.path.exists(os.path.join(d["segs"], "logits"))
    post = DenseCRF(**CRF_PARAMS)
    crf_hist = torch.zeros((nc, nc), dtype=torch.int64, device="cuda")
    for i, name in enumerate(names):
        _, image, label, _ = ds[i]
        H, W = label.shape
        png = np.asarray(Image.open(os.path.join(d["seg_preds"], name + ".png")))
        rgb = np.asarray(Image.open(os.path.join(d["seg_preds_rgb"], name + ".png")))
        assert png.shape == (H, W) and rgb.shape == (H, W, 3)
        msc = restated[i][0]
        if msc.shape[-2:] != (H, W):
            msc = ops.bilinear_resize(msc, H, W)
        q = post(torch.from_numpy(image).cuda(), torch.softmax(msc[0], dim=0)).cpu().numpy()
        top2 = np.sort(q, axis=0)[-2:]
        sure = (top2[1] - top2[0]) > 1e-4
        assert sure.mean() > 0.1
        assert np.array_equal(png[sure], q.argmax(0)[sure]), f"{name}: CRF labels differ where the CRF is decided"
        crf_hist = ops.confusion_accumulate(torch.from_numpy(label).cuda(), torch.from_numpy(png).cuda(), nc, crf_hist)
    assert torch.equal(res["hist_crf"], crf_hist)
    return root, lists, ckpt, model, ds, names, restated


def test_voc_program_end_to_end(gpu, tmp_path):
    from PIL import Image
    from excel_amd.tools import infer_seg_voc
    root, lists, ckpt, model, ds, names, restated = _check_program(tmp_path, infer_seg_voc, infer_seg_voc.VOC, coco=False)
    # --infer_set test: palette PNGs of the fused labels in the test-server layout, no scores
    res = infer_seg_voc.validate(_args(infer_seg_voc, root, lists, ckpt, "--infer_set", "test", "--batch_size", "2"), model=model)
    assert res["score"] is None and res["hist"] is None
    out = os.path.join(str(tmp_path), "run", "test", "test_model_iter_8_segs_no_crf", "results", "VOC2012", "Segmentation", "comp6_test_cls")
    assert res["dirs"]["test"] == out
    for i, name in enumerate(names):
        im = Image.open(os.path.join(out, name + ".png"))
        assert im.mode == "P" and np.array_equal(np.asarray(im), restated[i][1].cpu().numpy())


def test_coco_program_end_to_end(gpu, tmp_path):
    from excel_amd.tools import infer_seg_coco
    _check_program(tmp_path, infer_seg_coco, infer_seg_coco.COCO, coco=True)


def test_program_loads_checkpoints(gpu, tmp_path):
    """The program's own model: a CLIP checkpoint on disk + the decoder in train_voc's form and in the reference's DDP form."""
    from _clip_files import write_tiny_clip
    from excel_amd.model import ExCEL_model, init_decoder_state_dict
    from excel_amd.tools import infer_lam, infer_seg_voc
    clip_ckpt, bpe_path, _ = write_tiny_clip(tmp_path)
    dec = init_decoder_state_dict(num_classes=21, in_channels=128, embedding_dim=32, crop_size=64, seed=4, index=8)
    (tmp_path / "a" / "checkpoints").mkdir(parents=True)
    p_ours = str(tmp_path / "a" / "checkpoints" / "model_iter_5.pth")
    torch.save(dec, p_ours)
    ref_form = {"module." + k: v for k, v in dec.items()}
    ref_form["module.encoder.visual.positional_embedding"] = torch.zeros(17, 128)
    ref_form["module.encoder.visual.conv1.weight"] = torch.zeros(128, 3, 16, 16)
    p_ref = str(tmp_path / "ref_model.pth")
    torch.save(ref_form, p_ref)
    base = ["--model", clip_ckpt, "--bpe_path", bpe_path, "--embedding_dim", "32", "--in_channels", "128", "--resize_size", "64"]
    ns = infer_lam.get_parser().parse_args(["--model", clip_ckpt, "--bpe_path", bpe_path])
    direct = ExCEL_model(clip_model=clip_ckpt, embedding_dim=32, in_channels=128, num_classes=21, img_size=64, mode="val", device="cuda",
                         decoder_state_dict=dec, **infer_lam.resolve_model_inputs(ns))
    x = torch.randn(2, 3, 64, 64, generator=torch.Generator().manual_seed(1)).cuda()
    want = direct.seg_logits(x)
    for p in (p_ours, p_ref):
        m = infer_seg_voc.build_model(infer_seg_voc.get_parser().parse_args(base + ["--model_path", p]), torch.device("cuda"))
        assert torch.equal(m.seg_logits(x), want), p
