"""--save_cam on the GPU: excel_cam_overlay_ragged / excel_cam_overlay bit for bit against the numpy restatement of
tools/infer_lam.py:97-111 (tests/_cam_overlay_ref.py), from the pipeline's step buffers, on a busy side stream, and infer_lam end to end."""
import io
import os

import numpy as np
import pytest

from _cam_overlay_ref import overlays

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")


@pytest.fixture(scope="module")
def gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import excel_amd.ops  # noqa: F401
    return True


def _tables():
    from excel_amd.utils import imutils
    return imutils.jet_lut(), imutils.denormalize_roundtrip_table()


def _case(rs, sizes, ks, Cmax):
    """Decoded images + Cmax pitched planes per image: valid planes hold values around [0, 1] with the edge cases (0, 1, just below 1,
    negatives, > 1, NaN); pad columns and planes > k_b hold NaN / huge / negative sentinels."""
    from excel_amd import ops
    plan = ops.RaggedPlan(sizes, "cuda")
    imgs = rs.randint(0, 256, 3 * plan.total_label_pix).astype(np.uint8)
    cams = np.empty(Cmax * plan.total_pix, np.float32)
    sent = np.array([np.nan, 3e38, -3e38, 7.0, -1.0], np.float32)
    cams[:] = sent[np.arange(cams.size) % sent.size]
    special = np.array([0, 1, np.nextafter(np.float32(1), np.float32(0)), -0.25, 1.5, np.nan, 1 / 256, 0.5], np.float32)
    per_img = []
    for b, (H, W) in enumerate(sizes):
        Wp = (W + 3) // 4 * 4
        o = Cmax * int(plan.poff[b])
        view = cams[o:o + Cmax * H * Wp].reshape(Cmax, H, Wp)
        v = rs.uniform(-0.05, 1.05, (ks[b] + 1, H, W)).astype(np.float32)
        m = rs.rand(*v.shape) < 0.05
        v[m] = special[rs.randint(0, special.size, int(m.sum()))]
        view[:ks[b] + 1, :, :W] = v
        dec = imgs[3 * int(plan.loff[b]):3 * int(plan.loff[b + 1])].reshape(H, W, 3)
        per_img.append((dec, v))
    return plan, imgs, cams, per_img


SIZES = [(17, 5), (1, 70), (33, 1), (16, 64), (40, 131), (3, 3), (21, 66), (65, 13)]


@pytest.mark.parametrize("mode", ["max", "per_class"])
def test_ragged_kernel_bit_identical_to_the_reference(gpu, mode):
    from excel_amd import ops
    lut, rt = _tables()
    rs = np.random.RandomState(5)
    smax = 6
    ks = [0, 1, 2, 3, 4, 5, 6, 1]
    plan, imgs, cams, per_img = _case(rs, SIZES, ks, smax + 1)
    out, off = ops.cam_overlay_ragged(torch.from_numpy(imgs).cuda(), torch.from_numpy(cams).cuda(), plan, smax + 1, ks, mode)
    got = out.cpu().numpy()
    for b, (H, W) in enumerate(SIZES):
        want = overlays(per_img[b][0], per_img[b][1], mode, lut, rt)
        assert len(want) == (min(ks[b], 1) if mode == "max" else ks[b])
        for c, w in enumerate(want):
            g = got[int(off[b]) + 3 * c * H * W:][:3 * H * W].reshape(H, W, 3)
            assert np.array_equal(g, w), (mode, b, c, int((g != w).sum()))
    if mode == "per_class":
        assert out.numel() == 3 * sum(k * h * w for k, (h, w) in zip(ks, SIZES))


@pytest.mark.parametrize("mode", ["max", "per_class"])
def test_single_image_form_equals_the_reference(gpu, mode):
    from excel_amd import ops
    lut, rt = _tables()
    rs = np.random.RandomState(9)
    for (H, W), k in [((37, 29), 3), ((1, 1), 1), ((5, 130), 0)]:
        dec = rs.randint(0, 256, (H, W, 3)).astype(np.uint8)
        cams = rs.uniform(-0.1, 1.1, (k + 1, H, W)).astype(np.float32)
        cams.reshape(-1)[::7] = np.nan
        out = ops.cam_overlay(torch.from_numpy(dec).cuda(), torch.from_numpy(cams).cuda(), mode)
        want = overlays(dec, cams, mode, lut, rt)
        if mode == "max":
            assert (out is None) == (k == 0)
            if out is not None:
                assert np.array_equal(out.cpu().numpy(), want[0])
        else:
            assert tuple(out.shape) == (k, H, W, 3) and all(np.array_equal(out[c].cpu().numpy(), want[c]) for c in range(k))


def test_busy_side_stream_gives_the_same_bytes(gpu):
    from excel_amd import ops
    rs = np.random.RandomState(2)
    ks = [3, 1, 0, 6, 2, 2, 5, 4]
    plan, imgs, cams, _ = _case(rs, SIZES, ks, 7)
    im_d, cam_d = torch.from_numpy(imgs).cuda(), torch.from_numpy(cams).cuda()
    ref, _ = ops.cam_overlay_ragged(im_d, cam_d, plan, 7, ks, "per_class")
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    a = torch.randn(2048, 2048, device="cuda")
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(20):                       # keep the side stream busy ahead of the overlay
            a = a @ a * 1e-3
        out, _ = ops.cam_overlay_ragged(im_d, cam_d, plan, 7, ks, "per_class")
    torch.cuda.current_stream().wait_stream(side)
    assert torch.equal(out, ref)


def test_step_buffers_equal_return_intermediates(gpu):
    from excel_amd import ops
    from excel_amd.model import ExCEL_model
    from excel_amd.pipeline import TrainingFreePipeline
    from oracle.vit import VitConfig, make_vit_weights
    cfg = VitConfig(width=128, layers=8, heads=2, patch=16, out_dim=64, input_resolution=64, n_surgery=5)
    rs = np.random.RandomState(3)
    text = rs.standard_normal((9, 64)).astype(np.float32)
    text /= np.linalg.norm(text, axis=1, keepdims=True)
    model = ExCEL_model(clip_model="tiny", num_classes=5, img_size=96, mode="train", state_dict=make_vit_weights(cfg, seed=11),
                        text_attr=text.T.copy(), vit_cfg=dict(width=128, layers=8, heads=2, patch=16, output_dim=64, input_resolution=64),
                        device="cuda:0")
    sizes = [(50, 37), (96, 70), (23, 101)]
    plan = ops.RaggedPlan(sizes, "cuda")
    imgs = torch.from_numpy(rs.randint(0, 256, 3 * plan.total_label_pix).astype(np.uint8)).cuda()
    cls = np.zeros((3, 4), np.float32)
    cls[0, [1, 3]] = 1
    cls[1, 0] = 1
    ks = cls.sum(1).astype(int)
    pipe = TrainingFreePipeline(model, num_classes=5, smax=2)
    outs = {}
    for mode in ("max", "per_class"):
        pipe._bufs.clear()
        pipe.run_batch_ragged(imgs, plan, torch.from_numpy(cls).cuda(), S=96)
        a, off = ops.cam_overlay_ragged(imgs, pipe.last_cams, plan, 3, ks, mode)
        _, inter = pipe.run_batch_ragged(imgs, plan, torch.from_numpy(cls).cuda(), S=96, return_intermediates=True)
        b, _ = ops.cam_overlay_ragged(imgs, inter["cams"], plan, 3, ks, mode)
        for i, (h, w) in enumerate(sizes):              # the bytes of an image without a present class are not written (max mode)
            n = 3 * h * w * (min(int(ks[i]), 1) if mode == "max" else int(ks[i]))
            assert torch.equal(a[int(off[i]):int(off[i]) + n], b[int(off[i]):int(off[i]) + n]), (mode, i)
        outs[mode] = a
    assert outs["per_class"].numel() == 3 * sum(int(k) * h * w for k, (h, w) in zip(ks, sizes))


def _jpeg(a):
    from PIL import Image
    buf = io.BytesIO()
    Image.fromarray(a).save(buf, format="JPEG", quality=75)
    return buf.getvalue()


def _files(d):
    return {f: open(os.path.join(d, f), "rb").read() for f in sorted(os.listdir(d))}


def test_infer_lam_writes_the_reference_files(gpu, tmp_path):
    """--save_cam on a tiny on-disk VOC tree: the expected names and counts, every file = Pillow's quality-75 encoding of the restated
    overlay of the run's own CAM records, the ragged and --api_path runs write identical files, the scores do not change."""
    from PIL import Image
    from _clip_files import write_tiny_clip
    from excel_amd.tools import infer_lam, synthetic
    from excel_amd.utils import imutils
    root, lists = tmp_path / "VOC2012", tmp_path / "lists"
    ids, _ = synthetic.write_voc_tree(str(root), str(lists), 9, seed=4, split="val")
    ckpt, bpe_path, _ = write_tiny_clip(tmp_path)
    common = ["--data_folder", str(root), "--list_folder", str(lists), "--infer_set", "val", "--resize_size", "128", "--model", ckpt,
              "--bpe_path", bpe_path, "--batch_size", "4", "--num_workers", "2"]
    parse = infer_lam.get_parser().parse_args
    _, plain = infer_lam.validate(parse(common))
    cs, mx = tmp_path / "cs", tmp_path / "mx"
    _, t1 = infer_lam.validate(parse(common + ["--save_cam", "true", "--cs_cam_dir", str(cs), "--crf_post", "true",
                                               "--logits_dir", str(tmp_path / "logits")]))
    assert torch.equal(plain.cpu(), t1.cpu())
    _, t2 = infer_lam.validate(parse(common + ["--save_cam", "true", "--save_cls_specific_cam", "false", "--cam_dir", str(mx)]))
    assert torch.equal(plain.cpu(), t2.cpu())
    lut, rt = _tables()
    onehot = np.load(lists / "cls_labels_onehot.npy", allow_pickle=True).item()
    want_cs, want_mx = {}, {}
    for name in ids:
        lam, keys = imutils.load_logits(str(tmp_path / "logits" / (name + ".npy")))
        assert list(keys) == list(np.flatnonzero(onehot[name]))
        dec = np.asarray(Image.open(root / "JPEGImages" / (name + ".jpg")).convert("RGB"))
        for c, a in zip(keys, overlays(dec, lam, "per_class", lut, rt)):
            want_cs[f"{name}_{infer_lam.VOC_CLASSES[int(c) + 1]}.jpg"] = _jpeg(a)
        for a in overlays(dec, lam, "max", lut, rt):
            want_mx[name + ".jpg"] = _jpeg(a)
    got_cs, got_mx = _files(cs), _files(mx)
    assert sorted(got_cs) == sorted(want_cs) and len(got_cs) == int(sum(onehot[n].sum() for n in ids))
    assert got_cs == want_cs and got_mx == want_mx
    # the per-image path writes the same files through the single-image form
    _, t3 = infer_lam.validate(parse(common + ["--save_cam", "true", "--cs_cam_dir", str(tmp_path / "cs_api"), "--api_path", "true"]))
    assert torch.equal(plain.cpu(), t3.cpu())
    assert _files(tmp_path / "cs_api") == got_cs


def test_infer_lam_coco_config_uses_coco_class_names(gpu, tmp_path):
    from excel_amd.datasets import coco
    from excel_amd.tools import infer_lam, synthetic
    cs = tmp_path / "cs"
    common = ["--synthetic", "6", "--ragged", "true", "--dataset_name", "ms_coco", "--num_classes", "81", "--num_attri", "224", "--resize_size", "128",
              "--batch_size", "4", "--num_workers", "2", "--gemm_check", "false"]
    parse = infer_lam.get_parser().parse_args
    _, plain = infer_lam.validate(parse(common))
    _, t = infer_lam.validate(parse(common + ["--save_cam", "true", "--cs_cam_dir", str(cs)]))
    assert torch.equal(plain.cpu(), t.cpu())
    ds = synthetic.SyntheticSegDataset(6, num_classes=81, seed=1234, ragged=True)
    want = sorted(f"{ds[i][0]}_{coco.class_list[int(c) + 1]}.jpg" for i in range(6) for c in np.flatnonzero(ds[i][3]))
    assert sorted(os.listdir(cs)) == want
    assert any(int(c) >= 20 for i in range(6) for c in np.flatnonzero(ds[i][3]))     # names past the VOC list
