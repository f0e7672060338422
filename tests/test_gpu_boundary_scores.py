"""Boundary scores on the GPU: excel_boundary_scores (boundary.hip) against the literal erosion judge of _boundary_ref.py, integer for
integer, at every size around the kernel's tile, radii below, at and beyond the tile and the image, every class count, alignment and
addressing mode; then --boundary_scores of infer_lam, infer_seg_voc and eval_labels end to end against the label PNGs the runs wrote."""
import ctypes as C
import os

import numpy as np
import pytest

import _boundary_ref as R

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")


@pytest.fixture(scope="module")
def gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import excel_amd.ops  # noqa: F401
    return True


def _dev(a):
    return torch.from_numpy(np.array(a)).cuda()                 # a copy: the shared cases are read-only


def _at_offset(arr, off):
    """A device copy of `arr` that starts `off` bytes behind a 16-byte boundary"""
    base = torch.zeros(arr.size + 32, dtype=torch.uint8, device="cuda")
    assert base.data_ptr() % 16 == 0
    view = base[off:off + arr.size]
    view.copy_(torch.from_numpy(np.array(arr).reshape(-1)))
    return view


def test_the_case_table_is_sized_from_this_build(gpu):
    from excel_amd import ops
    assert tuple(ops.BOUNDARY_TILE) == R.TILE and ops.boundary_max_radius() == R.MAX_RADIUS >= 64


@pytest.mark.parametrize("case", R.case_table(), ids=[c[0] for c in R.case_table()])
def test_uniform_maps_against_the_erosion_judge(gpu, case):
    """Two uniform images per launch: the case and the case with its maps swapped (rows 0 and 1 swap).  A radius that covers the image
    makes every pixel a band pixel: the counts are ops.image_scores'."""
    from excel_amd import ops
    _, h, w, nc, d, seed = case
    g, p, ref = R.case(h, w, nc, d, seed)
    gd, pd = _dev(np.stack([g, p])), _dev(np.stack([p, g]))
    got = ops.boundary_scores(gd, pd, nc, d)
    assert got.dtype == torch.int32 and tuple(got.shape) == (2, 3, nc)
    got = got.cpu().numpy()
    print(case[0], "band", ref.sum(1), "got", got[0].sum(1))
    assert np.array_equal(got[0], ref) and np.array_equal(got[1], ref[[1, 0, 2]])
    if d >= max(h, w):
        assert torch.equal(ops.image_scores(gd.view(2, -1), pd.view(2, -1), nc).cpu(), torch.from_numpy(got))


@pytest.mark.parametrize("offs", [(0, 0), (3, 3), (1, 2)])
@pytest.mark.parametrize("hw", [(R.TILE[0] + 1, R.TILE[1] + 1), (2 * R.TILE[0] + 3, 2 * R.TILE[1] + 5)])
def test_alignment_of_both_maps(gpu, offs, hw):
    from excel_amd import ops
    nc = 21
    for d in (2, R.TILE[0] + 1):
        g, p, ref = R.case(hw[0], hw[1], nc, d, 77 + d)
        gd, pd = _at_offset(g, offs[0]), _at_offset(p, offs[1])
        assert gd.data_ptr() % 16 == offs[0] and pd.data_ptr() % 16 == offs[1]
        got = ops.boundary_scores(gd.view(1, *hw), pd.view(1, *hw), nc, d)
        assert np.array_equal(got.cpu().numpy()[0], ref)


def _ragged(repeat, nc=21):
    """Every size of the table, `repeat` times, image b with the (b mod 7)-th radius of the table (shifted per round) -> sizes, radii,
    gts, preds, judge counts [B,3,nc]"""
    sizes = R.sizes(*R.TILE) * repeat
    rad = R.radii(R.TILE[0], R.TILE[1], R.MAX_RADIUS)
    ds = [rad[(b + b // len(R.sizes(*R.TILE))) % len(rad)] for b in range(len(sizes))]
    cases = [R.case(h, w, nc, d, 31 + b % 11) for b, ((h, w), d) in enumerate(zip(sizes, ds))]
    return sizes, ds, [c[0] for c in cases], [c[1] for c in cases], np.stack([c[2] for c in cases])


@pytest.mark.parametrize("repeat", [1, 8])
@pytest.mark.parametrize("skip_kind", ["none", "zeros", "mix"])
def test_ragged_batches_a_radius_per_image_and_skip(gpu, repeat, skip_kind):
    from excel_amd import ops
    nc = 21
    sizes, ds, gs, ps, want = _ragged(repeat)
    assert len(set(ds)) == len(R.radii(R.TILE[0], R.TILE[1], R.MAX_RADIUS)), "every radius of the table occurs"
    B = len(sizes)
    plan = ops.RaggedPlan(sizes, "cuda")
    gd, pd = _dev(np.concatenate([g.reshape(-1) for g in gs])), _dev(np.concatenate([p.reshape(-1) for p in ps]))
    skip_h = {"none": None, "zeros": np.zeros(B, np.int32), "mix": (np.arange(B) % 3 == 1).astype(np.int32) * 7}[skip_kind]
    skip = None if skip_h is None else _dev(skip_h)
    want = want.copy()
    if skip_h is not None:
        want[skip_h != 0] = 0
    got = ops.boundary_scores(gd, pd, nc, ds, skip=skip, plan=plan)                     # a host sequence, uploaded by the op
    assert np.array_equal(got.cpu().numpy(), want)
    got = ops.boundary_scores(gd, pd, nc, _dev(np.asarray(ds, np.int32)), skip=skip, plan=plan)   # a device tensor, bound = the build's
    assert np.array_equal(got.cpu().numpy(), want)


def test_refused_radii_are_marked_not_clamped(gpu):
    """Radius 0 and a radius beyond max_radius: all 3 * nc entries of those images are -1 and every other image is right - with the bound
    the caller gives (17 < 18) and with the build's."""
    from excel_amd import ops
    nc = 21
    sizes = R.sizes(*R.TILE)
    for bound, ds in ((17, [2, 0, 17, 18, 1, 16, 15]), (None, [R.MAX_RADIUS, R.MAX_RADIUS + 1, 2, 0, 17, -3, 1])):
        cases = [R.case(h, w, nc, max(d, 1), 5) for (h, w), d in zip(sizes, ds)]
        bad = [b for b, d in enumerate(ds) if d < 1 or d > (bound or R.MAX_RADIUS)]
        assert len(bad) >= 2
        want = np.stack([c[2] for c in cases])
        want[bad] = -1
        plan = ops.RaggedPlan(sizes, "cuda")
        gd, pd = _dev(np.concatenate([c[0].reshape(-1) for c in cases])), _dev(np.concatenate([c[1].reshape(-1) for c in cases]))
        got = ops.boundary_scores(gd, pd, nc, _dev(np.asarray(ds, np.int32)), plan=plan, max_radius=bound).cpu().numpy()
        assert np.array_equal(got, want)
    # uniform addressing: the same marking
    g, p, ref = R.case(35, 133, nc, 2, 9)
    got = ops.boundary_scores(_dev(np.stack([g, g, g])), _dev(np.stack([p, p, p])), nc, _dev(np.asarray([0, 2, R.MAX_RADIUS + 1], np.int32))).cpu().numpy()
    assert (got[0] == -1).all() and (got[2] == -1).all() and np.array_equal(got[1], ref)


def test_host_radii_beyond_the_build_are_refused_by_name(gpu):
    from excel_amd import ops
    g = torch.zeros((2, 5, 9), dtype=torch.uint8, device="cuda")
    with pytest.raises(ValueError, match=r"image 1 \(5 x 9\) has radius 73"):
        ops.boundary_scores(g, g, 21, [3, R.MAX_RADIUS + 1])
    with pytest.raises(ValueError, match=r"image 0 \(5 x 9\) has radius 0"):
        ops.boundary_scores(g, g, 21, 0)
    plan = ops.RaggedPlan([(5, 9), (3, 15)], "cuda")
    with pytest.raises(ValueError, match=r"image 1 \(3 x 15\) has radius 99"):
        ops.boundary_scores(g.view(-1), g.view(-1), 21, [1, 99], plan=plan)
    with pytest.raises(ValueError, match="3 radii for 2 images"):
        ops.boundary_scores(g, g, 21, [1, 2, 3])
    for nc in (0, 257):
        with pytest.raises(ValueError, match="num_classes"):
            ops.boundary_scores(g, g, nc, 2)


def test_poisoned_out_buffer_is_fully_overwritten(gpu):
    from excel_amd import ops
    nc = 21
    sizes, ds, gs, ps, want = _ragged(1)
    plan = ops.RaggedPlan(sizes, "cuda")
    out = torch.full((len(sizes) * 3 * nc,), -0x5A5A5A5B, dtype=torch.int32, device="cuda")
    skip = _dev(np.asarray([0, 1, 0, 0, 1, 0, 0], np.int32))
    got = ops.boundary_scores(_dev(np.concatenate([g.reshape(-1) for g in gs])), _dev(np.concatenate([p.reshape(-1) for p in ps])), nc, ds,
                              skip=skip, plan=plan, out=out)
    assert got.data_ptr() == out.data_ptr()
    want = want.copy()
    want[[1, 4]] = 0
    assert np.array_equal(out.view(-1, 3, nc).cpu().numpy(), want)


def test_bad_arguments_are_refused_before_any_launch(gpu):
    from excel_amd import ops
    g = torch.zeros((2, 2, 4), dtype=torch.uint8, device="cuda")
    poison = torch.full((2 * 3 * 256 + 1,), 77, dtype=torch.int32, device="cuda")
    rad = torch.ones(3, dtype=torch.int32, device="cuda")
    plan = ops.RaggedPlan([(2, 4), (2, 4)], "cuda")
    lib = ops.lib()
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    gp, cp, rp = C.c_void_p(g.data_ptr()), C.c_void_p(poison.data_ptr()), C.c_void_p(rad.data_ptr())
    info, tab = C.byref(plan.info), C.c_void_p(plan.table.data_ptr())
    odd = lambda t: C.c_void_p(t.data_ptr() + 2)
    top = ops.boundary_max_radius()
    for args, word in (((None, gp, 2, 2, 4, None, None, None, 2, None, 21, cp, st), "null argument"),
                       ((gp, None, 2, 2, 4, None, None, None, 2, None, 21, cp, st), "null argument"),
                       ((gp, gp, 2, 2, 4, None, None, None, 2, None, 21, None, st), "null argument"),
                       ((gp, gp, 0, 2, 4, None, None, None, 2, None, 21, cp, st), "B = 0"),
                       ((gp, gp, 65536, 2, 4, None, None, None, 2, None, 21, cp, st), "B = 65536"),
                       ((gp, gp, 2, 2, 4, None, None, None, 2, None, 0, cp, st), "num_classes"),
                       ((gp, gp, 2, 2, 4, None, None, None, 2, None, 257, cp, st), "num_classes"),
                       ((gp, gp, 2, 0, 4, None, None, None, 2, None, 21, cp, st), "H >= 1 and W >= 1"),
                       ((gp, gp, 2, 2, 0, None, None, None, 2, None, 21, cp, st), "H >= 1 and W >= 1"),
                       ((gp, gp, 3, 0, 0, tab, info, None, 2, None, 21, cp, st), "plan holds 2 images, B = 3"),
                       ((gp, gp, 2, 0, 0, tab, None, None, 2, None, 21, cp, st), "plan holds -1 images"),
                       ((gp, gp, 2, 2, 4, None, None, None, 0, None, 21, cp, st), "max_radius"),
                       ((gp, gp, 2, 2, 4, None, None, rp, top + 1, None, 21, cp, st), "max_radius"),
                       ((gp, gp, 2, 2, 4, None, None, None, 2, None, 21, odd(poison), st), "4-byte aligned"),
                       ((gp, gp, 2, 2, 4, None, None, None, 2, odd(rad), 21, cp, st), "4-byte aligned"),
                       ((gp, gp, 2, 2, 4, None, None, odd(rad), 2, None, 21, cp, st), "4-byte aligned")):
        assert lib.excel_boundary_scores(*args) != 0, word
        assert word in lib.excel_last_error().decode(), lib.excel_last_error()
    torch.cuda.synchronize()
    assert bool((poison == 77).all()), "a refused call wrote to counts"


def test_score_ticket_carries_the_boundary_twin(gpu):
    """ScoreTicket.launch with boundary=: the set and its "<set>_bd" twin from the same arrays, radii by the host rule; without it the
    ticket is what it was."""
    from excel_amd import ops
    from excel_amd.pipeline import ScoreTicket
    from excel_amd.utils.image_scores import boundary_radius, counts_numpy
    nc = 21
    sizes = [(35, 133), (17, 65), (16, 64)]
    cases = [R.case(h, w, nc, boundary_radius(h, w), 3) for h, w in sizes]
    assert [boundary_radius(h, w) for h, w in sizes] == [3, 1, 1]
    plan = ops.RaggedPlan(sizes, "cuda")
    gd, pd = _dev(np.concatenate([c[0].reshape(-1) for c in cases])), _dev(np.concatenate([c[1].reshape(-1) for c in cases]))
    c = ScoreTicket().launch("main", gd, pd, nc, plan=plan).counts()
    assert sorted(c) == ["main"]
    c = ScoreTicket().launch("main", gd, pd, nc, plan=plan, boundary=dict(ratio=0.02, px=0)).counts()
    assert sorted(c) == ["main", "main_bd"]
    assert np.array_equal(c["main"], np.stack([counts_numpy(x[0], x[1], nc) for x in cases]))
    assert np.array_equal(c["main_bd"], np.stack([x[2] for x in cases]))
    fixed = [R.case(h, w, nc, 2, 3) for h, w in sizes]                       # a fixed pixel radius, uniform addressing (B = 1)
    c = ScoreTicket().launch("crf", _dev(fixed[0][0][None]), _dev(fixed[0][1][None]), nc, boundary=dict(px=2)).counts()
    assert np.array_equal(c["crf_bd"][0], fixed[0][2])


# ------------------------------------------------------------------ the programs: --boundary_scores end to end
def _png_bcounts(ids, gt_of, png_dir, nc, boundary=None):
    """The judge over the PNGs a run wrote, each image at the radius of the host rule"""
    from PIL import Image
    from excel_amd.utils.image_scores import boundary_radius
    out = []
    for n in ids:
        gt = gt_of(n)
        out.append(R.judge_counts(gt, np.asarray(Image.open(os.path.join(str(png_dir), n + ".png"))), nc, boundary_radius(*gt.shape, **(boundary or {}))))
    return np.stack(out)


def test_infer_lam_boundary_scores_on_disk_voc(gpu, tmp_path, monkeypatch, caplog):
    """The tree of test_gpu_image_scores.py: 6 ragged images at batch 4.  bcounts_main is the judge over the PNGs the same run wrote;
    --api_path true gives the same arrays; --conf_label adds the conf set; eval_labels over the written PNGs reproduces the counts;
    the logged table is boundary_scores_from_counts of the npz; the flag alone writes no file; without it the files are today's."""
    import csv
    import json
    import logging
    from PIL import Image
    from _clip_files import write_tiny_clip
    from excel_amd.tools import eval_labels, infer_lam, synthetic
    from excel_amd.utils import image_scores
    from excel_amd.utils.evaluate import boundary_scores_from_counts
    root, lists = tmp_path / "VOC2012", tmp_path / "lists"
    ids, _ = synthetic.write_voc_tree(str(root), str(lists), 6, seed=4, split="val")
    ckpt, bpe_path, _ = write_tiny_clip(tmp_path)
    common = ["--data_folder", str(root), "--list_folder", str(lists), "--infer_set", "val", "--resize_size", "128", "--model", ckpt,
              "--bpe_path", bpe_path, "--batch_size", "4", "--num_workers", "2", "--save_label", "true"]
    parse = infer_lam.get_parser().parse_args
    monkeypatch.chdir(tmp_path)
    gt_of = lambda n: np.asarray(Image.open(root / "SegmentationClassAug" / (n + ".png")))
    bd = ["--boundary_scores", "true"]

    out0 = str(tmp_path / "scores" / "plain.csv")
    _, t0 = infer_lam.validate(parse(common + ["--label_dir", str(tmp_path / "l0"), "--per_image_scores", out0]))
    z0 = np.load(out0 + ".npz")
    assert sorted(z0.files) == ["counts_main", "hw", "names"], "flag off: no new array"
    with open(out0, newline="") as f:
        head0 = next(csv.reader(f))
    assert not [c for c in head0 if "biou" in c or c == "radius"], "flag off: no new column"

    out1, js = str(tmp_path / "scores" / "batched.csv"), str(tmp_path / "run.json")
    with caplog.at_level(logging.INFO):
        _, t1 = infer_lam.validate(parse(common + bd + ["--label_dir", str(tmp_path / "l1"), "--per_image_scores", out1, "--json_out", js]))
    assert torch.equal(t0.cpu(), t1.cpu()), "the flag changes no score"
    z1 = np.load(out1 + ".npz")
    assert sorted(z1.files) == ["bcounts_main", "counts_main", "hw", "names", "radius"] and list(z1["names"]) == ids
    assert np.array_equal(z1["counts_main"], z0["counts_main"])
    assert np.array_equal(z1["radius"], [image_scores.boundary_radius(*gt_of(n).shape) for n in ids])
    want = _png_bcounts(ids, gt_of, tmp_path / "l1", 21)
    print("bcounts_main sums", z1["bcounts_main"].sum((0, 2)), "judge", want.sum((0, 2)), "region", z1["counts_main"].sum((0, 2)))
    assert np.array_equal(z1["bcounts_main"], want)
    # (the tree's ground truth is per-pixel noise, all band; the labels are coherent)
    assert 0 < want[:, 1].sum() < z1["counts_main"][:, 1].sum(), "a predicted band that is neither empty nor everything"
    score = boundary_scores_from_counts(z1["bcounts_main"])
    assert "boundary_score of the labels" in caplog.text and image_scores.boundary_table(score, infer_lam.VOC_CLASSES) in caplog.text
    with open(js) as f:
        block = json.load(f)["boundary"]
    assert block["ratio"] == 0.02 and block["px"] == 0 and block["sets"]["main"]["band_pixels"] == [int(x) for x in score["band_pixels"]]
    with open(out1, newline="") as f:
        rows = list(csv.reader(f))
    assert rows[0] == head0 + ["radius", "biou"] and [int(r[-2]) for r in rows[1:]] == z1["radius"].tolist()

    # the flag alone: tables in the log, no file
    before = sorted(os.listdir(tmp_path / "scores"))
    _, t1b = infer_lam.validate(parse(common + bd + ["--label_dir", str(tmp_path / "l1b")]))
    assert sorted(os.listdir(tmp_path / "scores")) == before and torch.equal(t1b.cpu(), t1.cpu())
    assert np.array_equal(infer_lam.validate.last_image_scores["bcounts"]["main"], z1["bcounts_main"])

    # eval_labels over the directory the run wrote
    oute = str(tmp_path / "scores" / "eval.csv")
    res = eval_labels.validate(eval_labels.get_parser().parse_args(
        ["--pred_dir", str(tmp_path / "l1"), "--data_folder", str(root), "--list_folder", str(lists), "--infer_set", "val", "--num_workers", "2",
         "--batch_size", "4", "--per_image_scores", oute] + bd))
    ze = np.load(oute + ".npz")
    assert np.array_equal(ze["bcounts_main"], z1["bcounts_main"]) and np.array_equal(ze["radius"], z1["radius"])
    assert np.array_equal(res["image_scores"]["bcounts"]["main"], z1["bcounts_main"])

    # the per-image path: the op with B = 1 per image, a fixed pixel radius
    px = bd + ["--boundary_px", "3"]
    out2, out2b = str(tmp_path / "scores" / "api.csv"), str(tmp_path / "scores" / "px.csv")
    infer_lam.validate(parse(common + px + ["--label_dir", str(tmp_path / "l2"), "--per_image_scores", out2, "--api_path", "true"]))
    infer_lam.validate(parse(common + px + ["--label_dir", str(tmp_path / "l2b"), "--per_image_scores", out2b]))
    z2, z2b = np.load(out2 + ".npz"), np.load(out2b + ".npz")
    assert np.array_equal(z2["bcounts_main"], _png_bcounts(ids, gt_of, tmp_path / "l2", 21, dict(px=3))) and (z2["radius"] == 3).all()
    assert np.array_equal(z2["counts_main"], z2b["counts_main"]), "precondition: the two paths label these images alike"
    assert np.array_equal(z2["bcounts_main"], z2b["bcounts_main"]) and np.array_equal(z2["radius"], z2b["radius"])

    out3 = str(tmp_path / "scores" / "conf.csv")
    infer_lam.validate(parse(common + bd + ["--label_dir", str(tmp_path / "l3"), "--per_image_scores", out3, "--conf_label", "true",
                                            "--conf_label_dir", str(tmp_path / "c3")]))
    z3 = np.load(out3 + ".npz")
    assert sorted(z3.files) == ["bcounts_conf", "bcounts_main", "counts_conf", "counts_main", "hw", "names", "radius"]
    assert np.array_equal(z3["bcounts_main"], z1["bcounts_main"])
    assert np.array_equal(z3["bcounts_conf"], _png_bcounts(ids, gt_of, tmp_path / "c3", 21))
    with open(out3, newline="") as f:
        assert next(csv.reader(f))[-3:] == ["radius", "biou", "conf_biou"]


def test_infer_lam_crf_inline_and_uniform_synthetic_sets(gpu, tmp_path, monkeypatch):
    from PIL import Image
    from _clip_files import write_tiny_clip
    from excel_amd.tools import infer_lam, synthetic
    root, lists = tmp_path / "VOC2012", tmp_path / "lists"
    ids, _ = synthetic.write_voc_tree(str(root), str(lists), 5, seed=4, split="val")
    ckpt, bpe_path, _ = write_tiny_clip(tmp_path)
    monkeypatch.chdir(tmp_path)
    out = str(tmp_path / "crf.csv")
    infer_lam.validate(infer_lam.get_parser().parse_args(
        ["--data_folder", str(root), "--list_folder", str(lists), "--infer_set", "val", "--resize_size", "128", "--model", ckpt, "--bpe_path", bpe_path,
         "--batch_size", "4", "--num_workers", "2", "--crf_post", "true", "--crf_inline", "true", "--crf_label_dir", str(tmp_path / "crf"),
         "--per_image_scores", out, "--boundary_scores", "true"]))
    gt_of = lambda n: np.asarray(Image.open(root / "SegmentationClassAug" / (n + ".png")))
    z = np.load(out + ".npz")
    assert sorted(z.files) == ["bcounts_crf", "bcounts_main", "counts_crf", "counts_main", "hw", "names", "radius"]
    assert np.array_equal(z["bcounts_crf"], _png_bcounts(ids, gt_of, tmp_path / "crf", 21))
    # the uniform synthetic loop (run_batch: [B,H,W] maps, one radius for all)
    out = str(tmp_path / "u.csv")
    d = tmp_path / "labels"
    infer_lam.validate(infer_lam.get_parser().parse_args(["--synthetic", "6", "--resize_size", "128", "--model", ckpt, "--bpe_path", bpe_path,
                                                          "--batch_size", "4", "--per_image_scores", out, "--save_label", "true",
                                                          "--label_dir", str(d), "--boundary_scores", "true"]))
    ds = synthetic.SyntheticSegDataset(6, (128, 128), num_classes=21, seed=1234)
    gts = {ds[i][0]: ds[i][2] for i in range(6)}
    z = np.load(out + ".npz")
    assert (z["radius"] == 4).all()                              # 0.02 * 128 * sqrt(2) = 3.62
    assert np.array_equal(z["bcounts_main"], _png_bcounts(list(z["names"]), gts.__getitem__, d, 21))


def test_infer_seg_voc_raw_and_crf_sets(gpu, tmp_path):
    """The tiny head of test_gpu_seg_eval.py: the raw set is the judge over the labels of the per-image chain, the CRF set over the PNGs
    the run wrote; the summed tables are boundary_scores_from_counts of the npz."""
    import test_gpu_seg_eval as se
    from PIL import Image
    from excel_amd.tools import infer_seg_voc
    from excel_amd.utils import image_scores
    root, lists, names = se._tree(tmp_path)
    ckpt = str(tmp_path / "run" / "checkpoints" / "model_iter_8.pth")
    model = se._tiny_model()
    nc = se.NUM_CLASSES
    out = str(tmp_path / "seg.csv")
    res = infer_seg_voc.validate(se._args(infer_seg_voc, root, lists, ckpt, "--batch_size", "3", "--crf_post", "true", "--per_image_scores", out,
                                          "--boundary_scores", "true"), model=model)
    ds = infer_seg_voc.VOC.dataset(se._args(infer_seg_voc, root, lists, ckpt), "val")
    z = np.load(out + ".npz")
    assert sorted(z.files) == ["bcounts_crf", "bcounts_main", "counts_crf", "counts_main", "hw", "names", "radius"] and list(z["names"]) == names
    rad = [image_scores.boundary_radius(*ds[i][2].shape) for i in range(len(ds))]
    raw = np.stack([R.judge_counts(ds[i][2], se._restate(model, ds, i, infer_seg_voc.VOC, nc)[1].cpu().numpy(), nc, rad[i]) for i in range(len(ds))])
    crf = np.stack([R.judge_counts(ds[i][2], np.asarray(Image.open(os.path.join(res["dirs"]["seg_preds"], n + ".png"))), nc, rad[i])
                    for i, n in enumerate(names)])
    assert np.array_equal(z["radius"], rad) and np.array_equal(z["bcounts_main"], raw) and np.array_equal(z["bcounts_crf"], crf)
    summary = image_scores.boundary_summary(res["image_scores"])
    assert np.array_equal(summary["main"]["band_pixels"], raw[:, 0].sum(0)) and np.array_equal(summary["crf"]["band_pixels"], crf[:, 0].sum(0))
    # image by image (--crf_batched false): the op with B = 1, the same table; and the flag alone writes nothing
    res2 = infer_seg_voc.validate(se._args(infer_seg_voc, root, lists, ckpt, "--batch_size", "2", "--crf_post", "true", "--crf_batched", "false",
                                           "--boundary_scores", "true"), model=model)
    assert np.array_equal(res2["image_scores"]["bcounts"]["main"], raw) and res2["image_scores"]["bcounts"]["crf"].shape == crf.shape
