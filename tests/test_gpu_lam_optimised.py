"""GPU tests of the batched optimised-LAM regime (--training_free false on ragged batches): the grouped feature affinity, the mirrored
ragged network input, OptimisedLamPipeline against the per-image call sequence (tools/infer_lam.py:79-94) and the oracle, the
infer_lam harness on it, and a full-size step."""
import os

import numpy as np
import pytest

import oracle
from oracle.vit import VitConfig, make_vit_weights

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

TINY = VitConfig(width=128, layers=8, heads=2, patch=16, out_dim=64, input_resolution=64, n_surgery=5)
TINY_KW = dict(width=128, layers=8, heads=2, patch=16, output_dim=64, input_resolution=64)
RAGGED_HW = [(60, 80), (75, 50), (33, 47), (96, 96), (50, 64), (41, 30)]


def dev(a):
    return torch.as_tensor(np.ascontiguousarray(a)).cuda()


def host(t):
    return t.detach().cpu().numpy()


def maxabs(a, b):
    return float(np.max(np.abs(np.asarray(a, np.float64) - np.asarray(b, np.float64))))


@pytest.fixture(scope="module")
def gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import excel_amd.ops  # noqa: F401  (raises if libexcel_hip.so is missing: no fallback)
    return True


def _label_budget(pixels, gemm_mode):
    """Label pixels allowed to differ from the fp32 oracle (tests/test_gpu_pipeline.py's budget)."""
    if gemm_mode == "f32":
        return max(1, int(0.0005 * pixels))
    return max(5, int(np.ceil(0.001 * pixels)))


def _decoder_sd(g):
    sd = {"decoder_fts_fuse." + k[len("fuse."):]: g[k] for k in g.files if k.startswith("fuse.")}
    sd.update({"decoder." + k[len("dec."):]: g[k] for k in g.files if k.startswith("dec.")})
    return sd


def _ragged_samples(seed=5, num_fg=4):
    rs = np.random.RandomState(seed)
    imgs = [rs.randint(0, 256, (h, w, 3)).astype(np.uint8) for h, w in RAGGED_HW]
    gts = []
    for h, w in RAGGED_HW:
        gt = rs.randint(0, num_fg + 1, (h, w)).astype(np.uint8)
        gt[rs.rand(h, w) < 0.03] = 255
        gts.append(gt)
    cls = np.zeros((len(RAGGED_HW), num_fg), np.float32)
    for b in range(len(RAGGED_HW)):
        cls[b, rs.choice(num_fg, size=1 + b % 3, replace=False)] = 1
    return imgs, gts, cls


def _pack(arrs):
    return dev(np.concatenate([a.reshape(-1) for a in arrs]))


# ------------------------------------------------------------------ 1. grouped feature affinity
def _members(B, group, ms):
    return [[(j // ms) * group * ms + j % ms + m * ms for m in range(group)] for j in range(B // group)]


@pytest.mark.parametrize("C,g", [(37, 14), (32, 28)])
def test_grouped_affinity_bit_identical_to_per_group_calls(gpu, C, g):
    from excel_amd import ops
    B = 6
    rs = np.random.RandomState(C + g)
    f = rs.standard_normal((B, C, g, g)).astype(np.float32)
    f[:3] += 0.7                                   # different per-image means: a whole-batch mean is visibly different
    fd = dev(f)
    for mode, ref_fn in (("sigmoid", oracle.cam.attn_pred), ("mask_softmax", oracle.vit.ex_attention)):
        whole = host(ops.feature_affinity(fd, mode))
        for group, ms in ((1, 1), (2, B // 2), (2, 1), (3, 2)):
            got = host(ops.feature_affinity_grouped(fd, mode, group=group, member_stride=ms))
            for mem in _members(B, group, ms):
                alone = host(ops.feature_affinity(dev(f[mem]), mode))
                assert np.array_equal(got[mem], alone), (mode, group, ms, mem)           # the bit contract
                # the reference's batch = the group.  Mode 1 masks z < 0: on the 784-token grid a few entries of z sit within
                # round-off of 0 and may fall on the other side in the float64 oracle, which rescales their rows
                off_rows = (np.abs(got[mem] - ref_fn(f[mem])) > 1e-6).any(-1)
                assert off_rows.mean() < (0.01 if mode == "mask_softmax" and g > 14 else 1e-9), (mode, g, int(off_rows.sum()))
            assert not np.array_equal(got, whole)                                       # the test sees the whole-batch mean
    with pytest.raises(RuntimeError):
        ops.feature_affinity_grouped(fd, "sigmoid", group=4)                            # 6 images are not groups of 4


# ------------------------------------------------------------------ 2. mirrored ragged input
def test_mirrored_ragged_input(gpu):
    from excel_amd import ops
    imgs, _, _ = _ragged_samples()
    plan = ops.RaggedPlan(RAGGED_HW, "cuda")
    hwc = _pack(imgs)
    for S in (96, 448):
        one = ops.normalize_resize_u8_ragged(hwc, plan, S)
        two = ops.normalize_resize_u8_ragged_mirror(hwc, plan, S)
        B = plan.B
        assert tuple(two.shape) == (2 * B, 3, S, S)
        assert torch.equal(two[:B], one)
        assert torch.equal(two[B:], torch.flip(one, dims=[-1]))


# ------------------------------------------------------------------ 3. pipeline == per-image call sequence
def _tiny_decoder_model(golden, gemm_mode, fp16_weights=False, S=96):
    from excel_amd.model import ExCEL_model
    g = golden("decoder_tiny.npz")
    w = make_vit_weights(TINY, seed=int(g["seed_w"]))
    if fp16_weights:
        w = {k: (np.asarray(v, np.float32).astype(np.float16).astype(np.float32) if np.asarray(v).dtype == np.float32 else v) for k, v in w.items()}
    rs = np.random.RandomState(1)
    text = rs.standard_normal((9, 64)).astype(np.float32)
    text /= np.linalg.norm(text, axis=1, keepdims=True)
    model = ExCEL_model(clip_model="tiny", num_classes=5, img_size=S, mode="train", state_dict=w, vit_cfg=TINY_KW, text_attr=text.T.copy(),
                        gemm_mode=gemm_mode, embedding_dim=32, in_channels=128, decoder_state_dict=_decoder_sd(g))
    return model, w, text, {k: g[k] for k in g.files if k.startswith(("fuse.", "dec."))}


def _per_image(model, img_u8, cls_row, hw, S, par):
    """tools/infer_lam.py:345-356 with training_free=False for one image (batch 1)."""
    from excel_amd import ops
    from excel_amd.utils.affutils import refine_cams_with_aff, refine_cams_with_bkg_weclip
    from excel_amd.utils.camutils import cure_attr_map_flip
    x = ops.bilinear_resize(ops.normalize_img_u8(dev(img_u8[None])), S, S, align_corners=False)
    _, _, _, attn_weights, attn_pred = model(x, n_attn_out=6)
    attr = cure_attr_map_flip(model, x)
    refined, cls_lst = refine_cams_with_aff(attr[0], attn_weights[:, 0], dev(cls_row), size=(S, S), seg_attn=attn_pred[0][None], caa_thre=0.79)
    labels, normed = refine_cams_with_bkg_weclip(refined, x[0], cls_lst, par, hw)
    return x, labels[0], normed, attr[0]


def _oracle_optimised(x, cls_row, hw, wo, text, dw, F_):
    """The reference's optimised-LAM step for one image on the oracle (numpy), from the device's network input x [1,3,S,S]."""
    _, attn1, feats1 = oracle.vit.vit_forward(x, wo, TINY, aliased_feats=True)
    fts1 = oracle.decoder.segformer_fuse(feats1, dw)
    ap = oracle.cam.attn_pred(fts1)
    xc = np.concatenate([x, x[..., ::-1]], 0)
    _, _, feats_c = oracle.vit.vit_forward(xc, wo, TINY, aliased_feats=True)
    ex = oracle.decoder.segformer_fuse(feats_c, dw)
    m = oracle.cam.attr_maps_raw(xc, wo, TINY, text.T.copy(), F_, ex_feats=ex)[0]
    g = x.shape[-1] // 16
    lam = m.transpose(0, 2, 1).reshape(2, F_, g, g)
    lam = np.maximum(lam[:1], lam[1:][..., ::-1])
    lam = lam - lam.min(axis=(2, 3), keepdims=True)
    lam = (lam / (lam.max(axis=(2, 3), keepdims=True) + 1e-5)).reshape(1, F_, g * g).transpose(0, 2, 1)
    refined, cls_lst = oracle.aff.refine_cams_with_aff(lam[0], attn1[:, 0], cls_row, size=x.shape[-2:], caa_thre=0.79, seg_attn=ap[0][None])
    label, _ = oracle.aff.refine_cams_with_bkg_weclip(refined, x[0], cls_lst, oracle.par.PAR([1, 2, 4, 8, 12, 24], 20), hw)
    return label[0]


@pytest.mark.parametrize("gemm_mode", ["f32", "bf16x3", "f16x2"])
def test_pipeline_equals_per_image_path_and_oracle(gpu, golden, gemm_mode):
    """ONE ragged batch of 6 sizes through OptimisedLamPipeline.run_batch_ragged: labels, confusion matrix and cams equal the per-image
    call sequence BIT FOR BIT; labels agree with the oracle within the mode's label budget.  f16x2 runs on fp16-valued weights."""
    from excel_amd import ops
    from excel_amd.pipeline import OptimisedLamPipeline
    from excel_amd.utils.PAR import PAR
    S, F_ = 96, 4
    f16 = gemm_mode == "f16x2"
    model, w, text, dw = _tiny_decoder_model(golden, None if f16 else gemm_mode, fp16_weights=f16)
    assert model.encoder.visual.handle().gemm_mode() == gemm_mode
    imgs, gts, cls = _ragged_samples()
    plan = ops.RaggedPlan(RAGGED_HW, "cuda")
    pipe = OptimisedLamPipeline(model, num_classes=F_ + 1, smax=3)
    lab, inter = pipe.run_batch_ragged(_pack(imgs), plan, dev(cls), _pack(gts), S=S, return_intermediates=True)
    lab2 = pipe.run_batch_ragged(_pack(imgs), plan, dev(cls), None, S=S)                  # step buffers: the same labels
    assert torch.equal(lab, lab2)
    hist = host(pipe.hist)
    par = PAR(num_iter=20, dilations=[1, 2, 4, 8, 12, 24])
    wo = oracle.vit.reload_self_attn(w, TINY, S // 16, "train")
    ref_hist = np.zeros((F_ + 1, F_ + 1), np.int64)
    for b, (h, wd) in enumerate(RAGGED_HW):
        x, l1, normed, attr1 = _per_image(model, imgs[b], cls[b], (h, wd), S, par)
        assert torch.equal(inter["inputs"][b], x[0])
        assert torch.equal(inter["attr"][b], attr1), b
        mine = host(plan.label(lab, b))
        assert np.array_equal(mine, host(l1).astype(np.uint8)), (b, int((mine != host(l1)).sum()))
        k = int(cls[b].sum())
        assert torch.equal(plan.planes(inter["cams"], b, pipe.smax + 1)[:k + 1], normed), b
        ref_hist += oracle.evaluate.fast_hist(gts[b].flatten(), mine.flatten(), F_ + 1)
        r = _oracle_optimised(host(x), cls[b], (h, wd), wo, text, dw, F_)
        budget = _label_budget(r.size, "bf16x3" if f16 else gemm_mode)
        assert int((mine != r).sum()) <= budget, (b, int((mine != r).sum()), r.size)
    assert np.array_equal(hist, ref_hist)


def test_pipeline_refuses_a_model_without_decoder(gpu):
    from excel_amd.model import ExCEL_model
    from excel_amd.pipeline import OptimisedLamPipeline
    model = ExCEL_model(clip_model="tiny", num_classes=5, img_size=96, mode="train", state_dict=make_vit_weights(TINY, seed=11),
                        vit_cfg=TINY_KW, text_attr=np.eye(64, 9, dtype=np.float32))
    with pytest.raises(ValueError, match="decoder"):
        OptimisedLamPipeline(model, num_classes=5, smax=3)


# ------------------------------------------------------------------ 4. the harness
def _write_voc_tree(tmp_path, sizes, seed=3):
    from PIL import Image
    from excel_amd.utils import imutils
    root, lists = tmp_path / "VOC2012", tmp_path / "lists"
    (root / "JPEGImages").mkdir(parents=True)
    (root / "SegmentationClassAug").mkdir()
    lists.mkdir()
    rs = np.random.RandomState(seed)
    ids, onehot, npix = [], {}, 0
    for k, (h, w) in enumerate(sizes):
        name = f"2008_{k:06d}"
        ids.append(name)
        coarse = rs.randint(0, 256, (h // 8 + 2, w // 8 + 2, 3)).astype(np.uint8)
        Image.fromarray(np.repeat(np.repeat(coarse, 8, 0), 8, 1)[:h, :w]).save(root / "JPEGImages" / (name + ".jpg"), quality=90)
        lab = rs.randint(0, 21, (h, w)).astype(np.uint8)
        lab[:2] = 255
        npix += int((lab < 21).sum())
        im = Image.fromarray(lab, mode="P")
        im.putpalette(imutils.colormap().flatten().tolist())
        im.save(root / "SegmentationClassAug" / (name + ".png"))
        oh = np.zeros(20, np.float32)
        oh[[k % 20, (3 * k + 7) % 20]] = 1
        onehot[name] = oh
    (lists / "val.txt").write_text("\n".join(ids) + "\n")
    np.save(lists / "cls_labels_onehot.npy", onehot)
    return root, lists, ids, npix


def _save_head(path, **kw):
    from excel_amd.model.init_head import init_decoder_state_dict
    sd = init_decoder_state_dict(**kw)
    torch.save({"module." + k: v for k, v in sd.items()}, str(path))          # a DDP checkpoint: the prefixes are stripped
    return str(path)


def _files(d):
    return {f: open(os.path.join(d, f), "rb").read() for f in sorted(os.listdir(d))}


def test_infer_lam_optimised_on_disk_voc(gpu, tmp_path):
    """`infer_lam --data_folder ... --training_free false --model_path head.pth` at --batch_size 32 (40 images, 7 sizes: 2 ragged batches)
    runs OptimisedLamPipeline; its confusion matrix, --crf_post records and --save_cam files equal the --api_path true run's."""
    from _clip_files import write_tiny_clip
    from excel_amd.pipeline import OptimisedLamPipeline
    from excel_amd.tools import infer_lam
    from excel_amd.utils import imutils
    sizes = [(90 + 7 * (k % 7), 120 - 9 * (k % 5)) for k in range(40)]
    root, lists, ids, npix = _write_voc_tree(tmp_path, sizes)
    ckpt, bpe_path, _ = write_tiny_clip(tmp_path)
    head = _save_head(tmp_path / "head.pth", num_classes=21, in_channels=128, embedding_dim=32, index=8, layers=2, seed=3)
    common = ["--data_folder", str(root), "--list_folder", str(lists), "--infer_set", "val", "--resize_size", "128", "--model", ckpt,
              "--bpe_path", bpe_path, "--batch_size", "32", "--num_workers", "2", "--training_free", "false", "--model_path", head,
              "--in_channels", "128", "--embedding_dim", "32"]
    parse = infer_lam.get_parser().parse_args
    calls = []
    orig = OptimisedLamPipeline.run_batch_ragged

    def spy(self, *a, **k):
        calls.append(a[1].B)
        return orig(self, *a, **k)
    OptimisedLamPipeline.run_batch_ragged = spy
    try:
        logits, cs = tmp_path / "logits", tmp_path / "cs"
        score, total = infer_lam.validate(parse(common + ["--crf_post", "true", "--logits_dir", str(logits), "--save_cam", "true",
                                                          "--cs_cam_dir", str(cs)]))
    finally:
        OptimisedLamPipeline.run_batch_ragged = orig
    assert calls == [32, 8]
    assert int(host(total).sum()) == npix and 0.0 <= score["miou"] <= 1.0
    logits1, cs1 = tmp_path / "logits_api", tmp_path / "cs_api"
    _, total1 = infer_lam.validate(parse(common + ["--api_path", "true", "--crf_post", "true", "--logits_dir", str(logits1), "--save_cam", "true",
                                                   "--cs_cam_dir", str(cs1)]))
    assert np.array_equal(host(total), host(total1))
    for name in ids:
        lam, keys = imutils.load_logits(str(logits / (name + ".npy")))
        lam1, keys1 = imutils.load_logits(str(logits1 / (name + ".npy")))
        assert np.array_equal(lam, lam1) and list(keys) == list(keys1), name
    got = _files(cs)
    assert len(got) == 2 * len(ids) and got == _files(cs1)
    mx, mx1 = tmp_path / "mx", tmp_path / "mx_api"
    infer_lam.validate(parse(common + ["--save_cam", "true", "--save_cls_specific_cam", "false", "--cam_dir", str(mx)]))
    infer_lam.validate(parse(common + ["--save_cam", "true", "--save_cls_specific_cam", "false", "--cam_dir", str(mx1), "--api_path", "true"]))
    assert _files(mx) == _files(mx1) and len(_files(mx)) == len(ids)


def test_infer_lam_optimised_coco_config(gpu, tmp_path):
    """A COCO-config run (81 classes, seeded ViT-B/16-shaped tower, full-width head) on ragged synthetic batches: the batched regime's
    confusion matrix equals the per-image path's."""
    from excel_amd.tools import infer_lam
    head = _save_head(tmp_path / "head.pth", num_classes=81, in_channels=768, embedding_dim=256, index=12, seed=4)
    common = ["--synthetic", "6", "--ragged", "true", "--dataset_name", "ms_coco", "--num_classes", "81", "--num_attri", "224",
              "--resize_size", "128", "--batch_size", "4", "--num_workers", "2", "--gemm_check", "false", "--training_free", "false",
              "--model_path", head]
    parse = infer_lam.get_parser().parse_args
    score, total = infer_lam.validate(parse(common))
    assert int(host(total).sum()) > 0 and 0.0 <= score["miou"] <= 1.0
    _, total1 = infer_lam.validate(parse(common + ["--api_path", "true"]))
    assert np.array_equal(host(total), host(total1))


# ------------------------------------------------------------------ 5. full size
def test_full_size_batch32_ragged_448(gpu):
    """ViT-B/16-shaped seeded weights + a full-size seeded head, B = 32 ragged at 448: labels stay in each image's key set, and
    images 0 and 31 run alone give the same labels bit for bit."""
    from excel_amd import ops
    from excel_amd.model import ExCEL_model
    from excel_amd.model.init_head import init_decoder_state_dict
    from excel_amd.pipeline import OptimisedLamPipeline
    from excel_amd.tools import synthetic
    sd = synthetic.make_vit_state_dict(seed=0)
    model = ExCEL_model(clip_model="ExCEL_ViT-B/16", num_classes=21, img_size=448, mode="train", state_dict=sd,
                        text_features=synthetic.make_text_features(45), embedding_dim=256, in_channels=768,
                        decoder_state_dict=init_decoder_state_dict(seed=7))
    ds = synthetic.SyntheticSegDataset(32, num_classes=21, seed=9, ragged=True)
    samples = [ds[i] for i in range(32)]
    hw = [s[1].shape[:2] for s in samples]
    cls = np.stack([s[3] for s in samples]).astype(np.float32)
    pipe = OptimisedLamPipeline(model, num_classes=21, smax=ds.max_k())
    plan = ops.RaggedPlan(hw, "cuda")
    lab = pipe.run_batch_ragged(_pack([s[1] for s in samples]), plan, dev(cls), _pack([s[2] for s in samples]), S=448)
    torch.cuda.synchronize()
    assert int(host(pipe.hist).sum()) == sum(int((s[2] != 255).sum()) for s in samples)
    for b in range(32):
        keys = set([0] + [int(c) + 1 for c in np.flatnonzero(cls[b])])
        assert set(np.unique(host(plan.label(lab, b))).tolist()) <= keys, b
    for b in (0, 31):
        p1 = ops.RaggedPlan([hw[b]], "cuda")
        one = OptimisedLamPipeline(model, num_classes=21, smax=ds.max_k()).run_batch_ragged(_pack([samples[b][1]]), p1, dev(cls[b:b + 1]), S=448)
        assert torch.equal(one, plan.label(lab, b).reshape(-1)), b
