"""The batched DenseCRF stage on the device: excel_dcrf_inference_ragged and excel_seg_softmax_resize_ragged against the per-image
entries (bit for bit: marginals, labels, unaries), independence of the grouping and of the batch neighbours, the numpy oracle, and the
VOC / COCO evaluation programs with --crf_batched true against false (files and histograms equal)."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

# one image narrower than 4 pixels (and one of width 1), widths that are not multiples of 4, one that is
SIZES = [(37, 50), (23, 3), (30, 41), (16, 64), (9, 1), (25, 66)]
VOC_SET = (10, 3, 1, 4, 67, 3)            # tools/infer_seg_voc.CRF_PARAMS as (iters, pos_w, pos_xy_std, bi_w, bi_xy_std, bi_rgb_std)
DCRF_SET = (10, 3, 3, 10, 80, 13)         # utils/dcrf.crf_inference (t=10, scale_factor=1)


@pytest.fixture(scope="module")
def gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from excel_amd import _lib
    _lib.lib()
    return torch.device("cuda")


def _image(rs, H, W):
    """A smooth half and a noisy half, like test_dcrf_vs_oracle's."""
    img = (rs.rand(H, W, 3) * 255).astype(np.uint8)
    img[:, : W // 2] = (img[:, : W // 2] * 0.15 + 140).astype(np.uint8)
    return img


def _prob(rs, C, H, W):
    p = rs.rand(C, H, W).astype(np.float32) ** 2 + 1e-3
    return p / p.sum(0, keepdims=True)


def _batch(sizes, C, seed):
    rs = np.random.RandomState(seed)
    return [_image(rs, H, W) for H, W in sizes], [_prob(rs, C, H, W) for H, W in sizes]


def _pack(imgs, probs, dev):
    images = torch.from_numpy(np.concatenate([i.reshape(-1) for i in imgs])).to(dev)
    unary = torch.from_numpy(np.concatenate([p.reshape(-1) for p in probs])).to(dev)
    return images, unary


def _alone(img, prob, params, dev):
    """The per-image chain: ops.dcrf_inference + ops.argmax_label."""
    from excel_amd import ops
    q = ops.dcrf_inference(torch.from_numpy(img).to(dev), torch.from_numpy(prob).to(dev), *params)
    return q, ops.argmax_label(q[None])[0]


def _split(plan, labels, q, C):
    out = []
    for b in range(plan.B):
        H, W = int(plan.hw[b, 0]), int(plan.hw[b, 1])
        lo = int(plan.loff[b])
        out.append((q[C * lo:C * (lo + H * W)].view(C, H, W), labels[lo:lo + H * W].view(H, W)))
    return out


@pytest.mark.parametrize("iters", [0, 10])
@pytest.mark.parametrize("params", [VOC_SET, DCRF_SET], ids=["voc", "dcrf"])
@pytest.mark.parametrize("C", [5, 21, 81])
def test_group_has_the_bits_of_every_image_alone(gpu, C, params, iters):
    from excel_amd import ops
    params = (iters,) + params[1:]
    imgs, probs = _batch(SIZES, C, seed=C + iters)
    plan = ops.RaggedPlan(SIZES, gpu)
    images, unary = _pack(imgs, probs, gpu)
    labels, q = ops.dcrf_inference_ragged(images, plan, unary, C, *params, want_labels=True, want_q=True)
    labels_only, none = ops.dcrf_inference_ragged(images, plan, unary, C, *params, want_labels=True, want_q=False)
    assert none is None and torch.equal(labels_only, labels)
    for b, (qb, lb) in enumerate(_split(plan, labels, q, C)):
        q_ref, l_ref = _alone(imgs[b], probs[b], params, gpu)
        assert np.array_equal(qb.cpu().numpy(), q_ref.cpu().numpy()), f"image {b} {SIZES[b]}: Q differs from excel_dcrf_inference"
        assert np.array_equal(lb.cpu().numpy(), l_ref.cpu().numpy()), f"image {b} {SIZES[b]}: labels differ from excel_argmax_label"


def test_energies_and_ties(gpu):
    """Unary energies instead of probabilities (utils/dcrf.crf_inference_label's form), with constant planes: exact ties in Q, which
    the arg-max must break like excel_argmax_label (first maximum)."""
    from excel_amd import ops
    from excel_amd.utils.dcrf import unary_from_labels
    C = 4
    rs = np.random.RandomState(5)
    imgs = [_image(rs, H, W) for H, W in SIZES]
    ens = [unary_from_labels(rs.randint(0, C, (H, W)), C, 0.7, zero_unsure=False).reshape(C, H, W) for H, W in SIZES]
    for e in ens:
        e[:, : e.shape[1] // 2] = 1.25                      # all classes equal on the top half: ties
    plan = ops.RaggedPlan(SIZES, gpu)
    images, unary = _pack(imgs, ens, gpu)
    for iters in (0, 10):
        params = (iters, 3, 3, 10, 50, 5)
        labels, q = ops.dcrf_inference_ragged(images, plan, unary, C, *params, is_energy=True, want_labels=True, want_q=True)
        ties = 0
        for b, (qb, lb) in enumerate(_split(plan, labels, q, C)):
            q_ref = ops.dcrf_inference(torch.from_numpy(imgs[b]).to(gpu), torch.from_numpy(ens[b]).to(gpu), *params, is_energy=True)
            assert np.array_equal(qb.cpu().numpy(), q_ref.cpu().numpy())
            assert np.array_equal(lb.cpu().numpy(), ops.argmax_label(q_ref[None])[0].cpu().numpy())
            top2 = np.sort(q_ref.cpu().numpy(), axis=0)[-2:]
            ties += int((top2[0] == top2[1]).sum())
        if iters == 0:
            assert ties > 0


def test_one_image_against_the_oracle(gpu):
    """Image 0 of a group against the numpy restatement, at test_dcrf_vs_oracle's tolerance (1e-3)."""
    import oracle
    from excel_amd import ops
    C = 5
    imgs, probs = _batch(SIZES, C, seed=77)
    plan = ops.RaggedPlan(SIZES, gpu)
    images, unary = _pack(imgs, probs, gpu)
    for params in (VOC_SET, DCRF_SET):
        _, q = ops.dcrf_inference_ragged(images, plan, unary, C, *params, want_labels=False, want_q=True)
        H, W = SIZES[0]
        got = q[:C * H * W].view(C, H, W).cpu().numpy()
        ref = oracle.dcrf.dense_crf_2d(imgs[0], oracle.dcrf.unary_from_softmax(probs[0]), *params)
        err = float(np.abs(got - ref).max())
        print(f"\nmax |Q - oracle| = {err:.3e}")
        assert err < 1e-3


@pytest.mark.parametrize("C", [5, 21])
def test_grouping_changes_nothing(gpu, C):
    from excel_amd import ops
    imgs, probs = _batch(SIZES, C, seed=3 * C)
    plan = ops.RaggedPlan(SIZES, gpu)
    images, unary = _pack(imgs, probs, gpu)
    ws = lambda hw: ops.dcrf_ragged_workspace_bytes(hw, C)
    whole = ws(SIZES)
    pairs = max(ws(SIZES[b:b + 2]) for b in range(len(SIZES) - 1))
    budgets = {"ones": 1, "pairs": pairs, "whole": whole}
    shapes = {k: ops.dcrf_groups(SIZES, C, v) for k, v in budgets.items()}
    assert shapes["ones"] == [(b, b + 1) for b in range(len(SIZES))]
    assert shapes["whole"] == [(0, len(SIZES))]
    assert 1 < len(shapes["pairs"]) < len(SIZES) and max(e - s for s, e in shapes["pairs"]) >= 2
    ref = ops.dcrf_inference_ragged(images, plan, unary, C, *VOC_SET, want_labels=True, want_q=True)
    for k, v in budgets.items():
        got = ops.dcrf_inference_ragged(images, plan, unary, C, *VOC_SET, want_labels=True, want_q=True, budget_bytes=v)
        assert torch.equal(got[0], ref[0]) and torch.equal(got[1], ref[1]), k


def test_images_do_not_see_their_neighbours(gpu):
    from excel_amd import ops
    C = 7
    imgs, probs = _batch(SIZES, C, seed=11)
    other_i, other_p = _batch(SIZES, C, seed=12)
    a = 2                                                               # the image under test: (30, 41)
    # the same image twice in one batch, between different neighbours
    order = [0, a, 3, 1, a, 5]
    sizes = [SIZES[k] for k in order]
    plan = ops.RaggedPlan(sizes, gpu)
    images, unary = _pack([imgs[k] for k in order], [probs[k] for k in order], gpu)
    labels, q = ops.dcrf_inference_ragged(images, plan, unary, C, *VOC_SET, want_labels=True, want_q=True)
    parts = _split(plan, labels, q, C)
    assert torch.equal(parts[1][0], parts[4][0]) and torch.equal(parts[1][1], parts[4][1])
    # the neighbours replaced by other images of the same sizes (same layout, other content), and by other sizes
    images2, unary2 = _pack([imgs[k] if k == a else other_i[k] for k in order], [probs[k] if k == a else other_p[k] for k in order], gpu)
    labels2, q2 = ops.dcrf_inference_ragged(images2, plan, unary2, C, *VOC_SET, want_labels=True, want_q=True)
    parts2 = _split(plan, labels2, q2, C)
    assert torch.equal(parts2[1][0], parts[1][0]) and torch.equal(parts2[4][1], parts[1][1])
    assert not torch.equal(parts2[0][0], parts[0][0])
    order3 = [4, 4, a, 0]
    plan3 = ops.RaggedPlan([SIZES[k] for k in order3], gpu)
    images3, unary3 = _pack([other_i[k] if k != a else imgs[k] for k in order3], [other_p[k] if k != a else probs[k] for k in order3], gpu)
    labels3, q3 = ops.dcrf_inference_ragged(images3, plan3, unary3, C, *VOC_SET, want_labels=True, want_q=True)
    parts3 = _split(plan3, labels3, q3, C)
    assert torch.equal(parts3[2][0], parts[1][0]) and torch.equal(parts3[2][1], parts[1][1])


def test_refusals(gpu):
    from excel_amd import ops
    C = 3
    imgs, probs = _batch(SIZES, C, seed=1)
    plan = ops.RaggedPlan(SIZES, gpu)
    images, unary = _pack(imgs, probs, gpu)
    with pytest.raises(ValueError):
        ops.dcrf_inference_ragged(images, plan, unary, C, *VOC_SET, want_labels=False, want_q=False)
    with pytest.raises(ValueError):
        ops.dcrf_inference_ragged(images[:-3], plan, unary, C, *VOC_SET)
    with pytest.raises(ValueError):
        ops.dcrf_inference_ragged(images, plan, unary[:-1], C, *VOC_SET)
    with pytest.raises(RuntimeError, match="positive"):
        ops.dcrf_inference_ragged(images, plan, unary, C, 10, 3, 0.0, 4, 67, 3)


@pytest.mark.parametrize("nc", [5, 21, 81])
@pytest.mark.parametrize("flavour", ["voc", "coco"])
def test_ragged_unary_matches_per_image(gpu, nc, flavour):
    """excel_seg_softmax_resize_ragged against excel_seg_softmax_resize per image: at the same size (VOC) and from the 0.2x fuse sizes
    (COCO, tools/infer_seg_coco.py:63-64, :144-145)."""
    from excel_amd import ops
    dst_hw = [(37, 50), (23, 7), (30, 41), (16, 64), (50, 5), (25, 66)]
    src_hw = dst_hw if flavour == "voc" else [(int(0.2 * h), int(0.2 * w)) for h, w in dst_hw]
    assert min(min(s) for s in src_hw) >= 1
    src, dst = ops.RaggedPlan(src_hw, gpu), ops.RaggedPlan(dst_hw, gpu)
    planes = (torch.randn(nc * src.total_pix, generator=torch.Generator().manual_seed(nc)) * 3).to(gpu)
    prob = ops.seg_softmax_resize_ragged(planes, src, dst, nc)
    assert prob.numel() == nc * dst.total_label_pix
    for b, (H, W) in enumerate(dst_hw):
        ref = ops.seg_softmax_resize(planes, src, b, nc, H, W)
        lo = nc * int(dst.loff[b])
        assert torch.equal(prob[lo:lo + nc * H * W].view(nc, H, W), ref), f"image {b}"
    with pytest.raises(ValueError):
        ops.seg_softmax_resize_ragged(planes, src, ops.RaggedPlan(dst_hw[:2], gpu), nc)


# ------------------------------------------------------------------ the programs
def _read_dir(d, names, mode=None):
    from PIL import Image
    assert sorted(os.listdir(d)) == sorted(n + ".png" for n in names), d
    out = {}
    for n in names:
        im = Image.open(os.path.join(d, n + ".png"))
        if mode is not None:
            assert im.mode == mode
        out[n] = np.asarray(im).copy()
    return out


def _same_files(a, b, what):
    assert a.keys() == b.keys()
    for n in a:
        assert a[n].shape == b[n].shape and np.array_equal(a[n], b[n]), f"{what}: {n}"


def _check_programs(tmp_path, mod, coco):
    from excel_amd import ops
    import test_gpu_seg_eval as E
    root, lists, names = E._tree(tmp_path, coco=coco)
    assert len(names) % 3 != 0                                         # batch size 3 leaves an uneven tail
    ckpt = str(tmp_path / "run" / "checkpoints" / "model_iter_8.pth")
    model = E._tiny_model()
    nc = E.NUM_CLASSES

    def base_args(*extra):
        return E._args(mod, root, lists, ckpt, *extra)

    def validate(*extra):
        res = mod.validate(base_args(*extra, "--crf_post", "true"), model=model)
        d = res["dirs"]
        return {"hist": res["hist"], "hist_crf": res["hist_crf"], "seg_preds": _read_dir(d["seg_preds"], names, "L"),
                "seg_preds_rgb": _read_dir(d["seg_preds_rgb"], names, "RGB"), "images": res["images"]}

    # a workspace budget that cuts the first batch of three into sub-groups
    hw = [(h, w) for h, w, _ in E.TREE[:3]]
    budget = ops.dcrf_ragged_workspace_bytes(hw[:2], nc) + 4096
    assert ops.dcrf_groups(hw, nc, budget) == [(0, 2), (2, 3)]
    runs = {("false", 1): validate("--batch_size", "1", "--crf_batched", "false")}
    runs[("false", 3)] = validate("--batch_size", "3", "--crf_batched", "false")
    runs[("true", 1)] = validate("--batch_size", "1", "--crf_batched", "true")
    runs[("true", 3)] = validate("--batch_size", "3")                  # the default is the batched stage
    runs[("groups", 3)] = validate("--batch_size", "3", "--crf_batched", "true", "--crf_ws_gb", repr(budget / 2 ** 30))
    ref = runs[("false", 1)]
    assert ref["images"] == len(names) and int(ref["hist_crf"].sum()) > 0
    for key, r in runs.items():
        assert torch.equal(r["hist"], ref["hist"]), key
        assert torch.equal(r["hist_crf"], ref["hist_crf"]), key
        _same_files(r["seg_preds"], ref["seg_preds"], f"{key} seg_preds")
        _same_files(r["seg_preds_rgb"], ref["seg_preds_rgb"], f"{key} seg_preds_rgb")
    return base_args, model, names


def test_voc_program_batched_equals_per_image(gpu, tmp_path):
    from excel_amd.tools import infer_seg_voc
    base_args, model, names = _check_programs(tmp_path, infer_seg_voc, coco=False)
    # --infer_set test with the CRF: the test-server files come from the CRF labels
    got = {}
    for flag in ("false", "true"):
        res = infer_seg_voc.validate(base_args("--infer_set", "test", "--batch_size", "3", "--crf_post", "true", "--crf_batched", flag), model=model)
        assert res["score"] is None and res["hist_crf"] is None
        assert res["dirs"]["test"].endswith(os.path.join("test_model_iter_8_segs_crf", "results", "VOC2012", "Segmentation", "comp6_test_cls"))
        got[flag] = (_read_dir(res["dirs"]["test"], names, "P"), _read_dir(res["dirs"]["seg_preds"], names, "L"))
    _same_files(got["true"][0], got["false"][0], "comp6_test_cls")
    _same_files(got["true"][1], got["false"][1], "test seg_preds")
    _same_files(got["true"][0], got["true"][1], "comp6_test_cls holds the CRF labels")


def test_coco_program_batched_equals_per_image(gpu, tmp_path):
    from excel_amd.tools import infer_seg_coco
    assert infer_seg_coco.get_parser().parse_args([]).crf_batched is True
    _check_programs(tmp_path, infer_seg_coco, coco=True)
