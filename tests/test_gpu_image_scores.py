"""Per-image scores on the GPU: excel_image_scores (confusion.hip) against numpy, integer for integer, at every size, class count, label
value, alignment and addressing mode the kernel has a path for; then --per_image_scores of infer_lam and infer_seg_voc end to end
against the label PNGs the same run wrote."""
import ctypes as C
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

RAGGED_SIZES = [(1, 1), (3, 5), (16, 16), (17, 23), (70, 65)]


@pytest.fixture(scope="module")
def gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import excel_amd.ops  # noqa: F401
    return True


def _ref(gt, pred, nc):
    """gt / pred: lists of flat uint8 arrays (one per image) -> int32 [B,3,nc]"""
    out = np.zeros((len(gt), 3, nc), np.int64)
    for b, (g, p) in enumerate(zip(gt, pred)):
        g, p = g.astype(np.int64), p.astype(np.int64)
        m = (g < nc) & (p < nc)
        out[b, 0] = np.bincount(g[m], minlength=nc)
        out[b, 1] = np.bincount(p[m], minlength=nc)
        out[b, 2] = np.bincount(g[m & (g == p)], minlength=nc)
    return out.astype(np.int32)


def _maps(rs, n, nc):
    """n label pairs with runs (coherent maps) and every kind of value: classes, 255, values in [nc, 255), a pred of 255"""
    def one():
        v = rs.randint(0, nc, size=n)
        run = np.repeat(rs.randint(0, nc, size=n // 7 + 1), 7)[:n]
        v = np.where(rs.rand(n) < 0.6, run, v)
        return v
    g, p = one(), one()
    p = np.where(rs.rand(n) < 0.5, g, p)
    g = np.where(rs.rand(n) < 0.05, 255, g)
    p = np.where(rs.rand(n) < 0.05, 255, p)
    if nc < 255:
        g = np.where(rs.rand(n) < 0.03, rs.randint(nc, 255, size=n), g)
        p = np.where(rs.rand(n) < 0.03, rs.randint(nc, 255, size=n), p)
    return g.astype(np.uint8), p.astype(np.uint8)


def _at_offset(arr, off):
    """A device copy of `arr` that starts `off` bytes behind a 16-byte boundary"""
    base = torch.zeros(arr.size + 32, dtype=torch.uint8, device="cuda")
    assert base.data_ptr() % 16 == 0
    view = base[off:off + arr.size]
    view.copy_(torch.from_numpy(arr))
    return view


@pytest.mark.parametrize("per_image", [1, 15, 16, 17, 4096, 4101])
@pytest.mark.parametrize("nc", [1, 2, 21, 81, 91, 256])
def test_uniform_sizes_and_class_counts(gpu, per_image, nc):
    from excel_amd import ops
    rs = np.random.RandomState(per_image * 7 + nc)
    g, p = _maps(rs, 3 * per_image, nc)
    got = ops.image_scores(torch.from_numpy(g).cuda().view(3, per_image), torch.from_numpy(p).cuda().view(3, per_image), nc)
    assert got.dtype == torch.int32 and tuple(got.shape) == (3, 3, nc)
    want = _ref(list(g.reshape(3, -1)), list(p.reshape(3, -1)), nc)
    assert torch.equal(got.cpu(), torch.from_numpy(want))


@pytest.mark.parametrize("offs", [(0, 0), (3, 3), (1, 2), (5, 0)])
@pytest.mark.parametrize("per_image", [2, 17, 4101])
def test_alignment_of_both_maps(gpu, offs, per_image):
    """(0,0) / (3,3): the maps share their 16-byte phase (scalar head, 16-byte body); (1,2) / (5,0): they do not (byte path).  per_image
    = 2 at offset 3 is an image shorter than its head."""
    from excel_amd import ops
    nc = 21
    rs = np.random.RandomState(per_image + offs[0] * 16 + offs[1])
    g, p = _maps(rs, 3 * per_image, nc)
    gd, pd = _at_offset(g, offs[0]), _at_offset(p, offs[1])
    assert gd.data_ptr() % 16 == offs[0] and pd.data_ptr() % 16 == offs[1]
    got = ops.image_scores(gd.view(3, per_image), pd.view(3, per_image), nc)
    assert torch.equal(got.cpu(), torch.from_numpy(_ref(list(g.reshape(3, -1)), list(p.reshape(3, -1)), nc)))


def _hist_ref(gs, ps, nc):
    """gs / ps: lists of flat uint8 arrays (one per image) -> int64 [nc,nc], the confusion matrix over the pixels with g < nc and p < nc"""
    h = np.zeros(nc * nc, np.int64)
    for g, p in zip(gs, ps):
        g, p = g.astype(np.int32), p.astype(np.int32)
        m = (g < nc) & (p < nc)
        h += np.bincount(nc * g[m] + p[m], minlength=nc * nc)
    return h.reshape(nc, nc)


SWEEP_RAGGED = [(5, 7), (16, 64), (17, 65), (1, 1)]


@pytest.mark.parametrize("offs", [(0, 0), (3, 3), (1, 2), (5, 0)])
@pytest.mark.parametrize("layout", [1, 15, 16, 17, 4101, "ragged"])
@pytest.mark.parametrize("nc", [21, 151])
def test_the_three_entries_agree_on_the_same_arrays(gpu, offs, layout, nc):
    """confusion_accumulate, confusion_accumulate_masked and image_scores run one sweep: on the same slices - a shared 16-byte phase or
    none (the scalar-only path), uniform B = 3 images of `layout` pixels or one ragged plan, a whole matrix in LDS (21) or bands (151) -
    the masked matrix with an all-zero skip is the plain one bit for bit and numpy's, the margins of image_scores are that matrix's,
    and a skipped image is dropped by both per-image entries, exactly."""
    from excel_amd import ops
    from excel_amd.utils.evaluate import hist_margins
    if layout == "ragged":
        plan, pix = ops.RaggedPlan(SWEEP_RAGGED, "cuda"), [h * w for h, w in SWEEP_RAGGED]
    else:
        plan, pix = None, [layout] * 3
    B = len(pix)
    rs = np.random.RandomState(sum(pix) * 31 + offs[0] * 16 + offs[1] + nc)
    g, p = _maps(rs, sum(pix), nc)
    cuts = np.cumsum(pix)[:-1]
    gs, ps = np.split(g, cuts), np.split(p, cuts)
    gd, pd = _at_offset(g, offs[0]), _at_offset(p, offs[1])
    assert gd.data_ptr() % 16 == offs[0] and pd.data_ptr() % 16 == offs[1]
    if plan is None:
        gd, pd = gd.view(B, -1), pd.view(B, -1)
    zeros = torch.zeros(B, dtype=torch.int32, device="cuda")
    plain = ops.confusion_accumulate(gd, pd, nc)
    masked = ops.confusion_accumulate_masked(gd, pd, nc, zeros, plan=plan)
    assert plain.dtype == masked.dtype == torch.int64 and torch.equal(masked, plain)
    assert np.array_equal(plain.cpu().numpy(), _hist_ref(gs, ps, nc))
    counts = ops.image_scores(gd, pd, nc, skip=zeros, plan=plan).cpu().numpy()
    assert np.array_equal(counts, _ref(gs, ps, nc))
    rows, cols, diag = hist_margins(counts)
    hist = plain.cpu().numpy()
    assert np.array_equal(rows, hist.sum(1)) and np.array_equal(cols, hist.sum(0)) and np.array_equal(diag, np.diagonal(hist))
    # image 1 skipped
    skip = torch.tensor([0, 5] + [0] * (B - 2), dtype=torch.int32, device="cuda")
    kept = [b for b in range(B) if b != 1]
    masked = ops.confusion_accumulate_masked(gd, pd, nc, skip, plan=plan).cpu().numpy()
    assert np.array_equal(masked, _hist_ref([gs[b] for b in kept], [ps[b] for b in kept], nc))
    counts = ops.image_scores(gd, pd, nc, skip=skip, plan=plan).cpu().numpy()
    want = _ref(gs, ps, nc)
    want[1] = 0
    assert np.array_equal(counts, want)


def _noise(rs, n, nc):
    """n label pairs, cheap to draw: uniform over the classes, 255 and (nc < 255) one value in [nc, 255)"""
    def one():
        v = rs.randint(0, nc + 2, size=n).astype(np.uint8)
        v[v == nc + 1] = 255
        return v
    return one(), one()


def test_two_rounds_of_the_stride_loop_per_image(gpu):
    """700 uniform images of 3 * 4096 + 5 pixels: the chunk rule gives 2048 // 700 = 2 chunks per image where the image has 4 groups of
    4096 pixels, so every workgroup of the masked confusion and of image_scores goes round its stride loop twice."""
    from excel_amd import ops
    B, per_image, nc = 700, 3 * 4096 + 5, 21
    rs = np.random.RandomState(700)
    g, p = _noise(rs, B * per_image, nc)
    gs, ps = list(g.reshape(B, -1)), list(p.reshape(B, -1))
    gd, pd = torch.from_numpy(g).cuda().view(B, per_image), torch.from_numpy(p).cuda().view(B, per_image)
    skip_h = np.zeros(B, np.int32)
    skip_h[[3, 698]] = 1
    skip = torch.from_numpy(skip_h).cuda()
    kept = np.nonzero(skip_h == 0)[0]
    hist = ops.confusion_accumulate_masked(gd, pd, nc, skip).cpu().numpy()
    assert np.array_equal(hist, _hist_ref([gs[b] for b in kept], [ps[b] for b in kept], nc))
    want = _ref(gs, ps, nc)
    want[skip_h != 0] = 0
    assert np.array_equal(ops.image_scores(gd, pd, nc, skip=skip).cpu().numpy(), want)


def test_two_rounds_of_the_stride_loop_of_the_plain_entry(gpu):
    """2048 * 4096 * 2 + 5 pixels in one range: the grid stops at 2048 chunks, so every workgroup makes two rounds and chunk 0 a third."""
    from excel_amd import ops
    n, nc = 2048 * 4096 * 2 + 5, 21
    g, p = _noise(np.random.RandomState(2048), n, nc)
    hist = ops.confusion_accumulate(torch.from_numpy(g).cuda(), torch.from_numpy(p).cuda(), nc).cpu().numpy()
    assert np.array_equal(hist, _hist_ref([g], [p], nc))


def _ragged_case(sizes, nc, seed):
    rs = np.random.RandomState(seed)
    gs, ps = zip(*[_maps(rs, h * w, nc) for h, w in sizes])
    return list(gs), list(ps)


@pytest.mark.parametrize("repeat", [1, 8])
@pytest.mark.parametrize("skip_kind", ["none", "zeros", "mix"])
def test_ragged_batches_skip_and_the_confusion_margins(gpu, repeat, skip_kind):
    """The 5 sizes (odd loff_b for most images) and 40 such images in one batch; skip = None, all zero, a mix; the margins equal those of
    the confusion kernels on the same arrays."""
    from excel_amd import ops
    from excel_amd.utils.evaluate import hist_margins
    nc = 21
    sizes = RAGGED_SIZES * repeat
    B = len(sizes)
    gs, ps = _ragged_case(sizes, nc, 5 + repeat)
    plan = ops.RaggedPlan(sizes, "cuda")
    gd, pd = torch.from_numpy(np.concatenate(gs)).cuda(), torch.from_numpy(np.concatenate(ps)).cuda()
    skip_h = {"none": None, "zeros": np.zeros(B, np.int32), "mix": (np.arange(B) % 3 == 1).astype(np.int32) * 7}[skip_kind]
    skip = None if skip_h is None else torch.from_numpy(skip_h).cuda()
    got = ops.image_scores(gd, pd, nc, skip=skip, plan=plan)
    want = _ref(gs, ps, nc)
    if skip_h is not None:
        want[skip_h != 0] = 0
    assert torch.equal(got.cpu(), torch.from_numpy(want))
    if skip_h is not None:
        assert not got.cpu().numpy()[skip_h != 0].any(), "skipped rows are zero"
        hist = ops.confusion_accumulate_masked(gd, pd, nc, skip, plan=plan).cpu().numpy()
    else:
        hist = ops.confusion_accumulate(gd, pd, nc).cpu().numpy()
    rows, cols, diag = hist_margins(got.cpu().numpy())
    assert np.array_equal(rows, hist.sum(1)) and np.array_equal(cols, hist.sum(0)) and np.array_equal(diag, np.diagonal(hist))


def test_uniform_skip_and_margins_at_wide_vocabularies(gpu):
    from excel_amd import ops
    from excel_amd.utils.evaluate import hist_margins
    for nc in (91, 256):                                      # the banded arm of the confusion kernels
        rs = np.random.RandomState(nc)
        g, p = _maps(rs, 4 * 1000, nc)
        gd, pd = torch.from_numpy(g).cuda().view(4, 1000), torch.from_numpy(p).cuda().view(4, 1000)
        skip = torch.tensor([0, 3, 0, 0], dtype=torch.int32, device="cuda")
        got = ops.image_scores(gd, pd, nc, skip=skip).cpu().numpy()
        want = _ref(list(g.reshape(4, -1)), list(p.reshape(4, -1)), nc)
        want[1] = 0
        assert np.array_equal(got, want)
        hist = ops.confusion_accumulate_masked(gd, pd, nc, skip).cpu().numpy()
        rows, cols, diag = hist_margins(got)
        assert np.array_equal(rows, hist.sum(1)) and np.array_equal(cols, hist.sum(0)) and np.array_equal(diag, np.diagonal(hist))


def test_poisoned_out_buffer_is_fully_overwritten(gpu):
    from excel_amd import ops
    nc = 21
    gs, ps = _ragged_case(RAGGED_SIZES, nc, 3)
    plan = ops.RaggedPlan(RAGGED_SIZES, "cuda")
    out = torch.full((len(RAGGED_SIZES) * 3 * nc,), -0x5A5A5A5B, dtype=torch.int32, device="cuda")
    skip = torch.tensor([0, 1, 0, 0, 1], dtype=torch.int32, device="cuda")
    got = ops.image_scores(torch.from_numpy(np.concatenate(gs)).cuda(), torch.from_numpy(np.concatenate(ps)).cuda(), nc, skip=skip,
                           plan=plan, out=out)
    assert got.data_ptr() == out.data_ptr()
    want = _ref(gs, ps, nc)
    want[[1, 4]] = 0
    assert torch.equal(out.view(-1, 3, nc).cpu(), torch.from_numpy(want))


def test_bad_arguments_are_refused_before_any_launch(gpu):
    from excel_amd import ops
    g = torch.zeros((2, 8), dtype=torch.uint8, device="cuda")
    poison = torch.full((2 * 3 * 256,), 77, dtype=torch.int32, device="cuda")
    for nc in (0, 257):
        with pytest.raises(ValueError, match="num_classes"):
            ops.image_scores(g, g, nc)
    with pytest.raises(ValueError, match="B = 0"):
        ops.image_scores(g[:0], g[:0], 21)
    plan = ops.RaggedPlan([(2, 4), (2, 4)], "cuda")
    with pytest.raises(ValueError, match="skip holds 3 flags for 2 images"):
        ops.image_scores(g, g, 21, skip=torch.zeros(3, dtype=torch.int32, device="cuda"), plan=plan)
    # the C entry itself: the same refusals, by name, with nothing written
    lib = ops.lib()
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    gp, cp = C.c_void_p(g.data_ptr()), C.c_void_p(poison.data_ptr())
    info = C.byref(plan.info)
    tab = C.c_void_p(plan.table.data_ptr())
    for args, word in (((gp, gp, 2, 8, None, None, None, 0, cp, st), "num_classes"), ((gp, gp, 2, 8, None, None, None, 257, cp, st), "num_classes"),
                       ((gp, gp, 0, 8, None, None, None, 21, cp, st), "B = 0"), ((gp, gp, 3, 8, tab, info, None, 21, cp, st), "plan holds 2 images, B = 3"),
                       ((gp, gp, 2, 0, None, None, None, 21, cp, st), "per_image")):
        assert lib.excel_image_scores(*args) != 0
        assert word in lib.excel_last_error().decode(), lib.excel_last_error()
    torch.cuda.synchronize()
    assert bool((poison == 77).all()), "a refused call wrote to counts"


def test_score_ticket_of_a_step(gpu):
    """ScoreTicket.launch on a side stream behind a busy kernel: ready() does not block, counts() waits and returns the step's parts."""
    from excel_amd import ops
    from excel_amd.pipeline import ScoreTicket
    nc = 21
    gs, ps = _ragged_case(RAGGED_SIZES, nc, 9)
    plan = ops.RaggedPlan(RAGGED_SIZES, "cuda")
    gd, pd = torch.from_numpy(np.concatenate(gs)).cuda(), torch.from_numpy(np.concatenate(ps)).cuda()
    t = ScoreTicket()
    assert t.ready() and t.counts() == {}
    t.launch("main", gd, pd, nc, plan=plan).launch("conf", gd, torch.full_like(pd, 255), nc, plan=plan)
    assert isinstance(t.ready(), bool)
    c = t.counts()
    assert sorted(c) == ["conf", "main"]
    assert np.array_equal(c["main"], _ref(gs, ps, nc)) and not c["conf"].any()


# ------------------------------------------------------------------ the programs: --per_image_scores end to end
def _png_counts(ids, gt_of, png_dir, nc):
    from PIL import Image
    from excel_amd.utils.image_scores import counts_numpy
    return np.stack([counts_numpy(gt_of(n), np.asarray(Image.open(os.path.join(str(png_dir), n + ".png"))), nc) for n in ids])


def _margins_equal(counts, hist):
    from excel_amd.utils.evaluate import hist_margins
    rows, cols, diag = hist_margins(counts)
    h = hist.cpu().numpy() if torch.is_tensor(hist) else np.asarray(hist)
    return np.array_equal(rows, h.sum(1)) and np.array_equal(cols, h.sum(0)) and np.array_equal(diag, np.diagonal(h))


def test_infer_lam_per_image_scores_on_disk_voc(gpu, tmp_path, monkeypatch):
    """6 ragged images at batch 4 (two steps, a tail): the npz counts are numpy's counts over the PNGs the same run wrote and the data
    set's ground truth, their margins the run's own matrix; --api_path true gives the same npz; --conf_label adds the conf set, over the
    conf PNGs; without the flag no file appears and the matrix is the same."""
    import csv
    from PIL import Image
    from _clip_files import write_tiny_clip
    from excel_amd.tools import infer_lam, synthetic
    root, lists = tmp_path / "VOC2012", tmp_path / "lists"
    ids, _ = synthetic.write_voc_tree(str(root), str(lists), 6, seed=4, split="val")
    ckpt, bpe_path, _ = write_tiny_clip(tmp_path)
    common = ["--data_folder", str(root), "--list_folder", str(lists), "--infer_set", "val", "--resize_size", "128", "--model", ckpt,
              "--bpe_path", bpe_path, "--batch_size", "4", "--num_workers", "2", "--save_label", "true"]
    parse = infer_lam.get_parser().parse_args
    monkeypatch.chdir(tmp_path)
    gt_of = lambda n: np.asarray(Image.open(root / "SegmentationClassAug" / (n + ".png")))
    _, plain = infer_lam.validate(parse(common + ["--label_dir", str(tmp_path / "l0")]))
    assert infer_lam.validate.last_image_scores is None

    out1 = str(tmp_path / "scores" / "batched.csv")
    _, t1 = infer_lam.validate(parse(common + ["--label_dir", str(tmp_path / "l1"), "--per_image_scores", out1, "--per_image_worst", "3"]))
    assert torch.equal(plain.cpu(), t1.cpu()), "the flag changes no score"
    z1 = np.load(out1 + ".npz")
    assert sorted(z1.files) == ["counts_main", "hw", "names"] and list(z1["names"]) == ids
    assert z1["counts_main"].dtype == np.int64 and np.array_equal(z1["hw"], [gt_of(n).shape for n in ids])
    assert np.array_equal(z1["counts_main"], _png_counts(ids, gt_of, tmp_path / "l1", 21))
    assert _margins_equal(z1["counts_main"], t1)
    with open(out1, newline="") as f:
        rows = list(csv.reader(f))
    assert [r[0] for r in rows[1:]] == ids and rows[0][:7] == ["name", "height", "width", "scored", "pacc", "miou", "present"]
    assert len(rows[0]) == 7 + 21 and rows[0][7] == "iou_" + infer_lam.VOC_CLASSES[0]

    # eval_labels over the directory the run wrote: the same table from the files (one ragged plan per batch of 4)
    from excel_amd.tools import eval_labels
    oute = str(tmp_path / "scores" / "eval.csv")
    res = eval_labels.validate(eval_labels.get_parser().parse_args(
        ["--pred_dir", str(tmp_path / "l1"), "--data_folder", str(root), "--list_folder", str(lists), "--infer_set", "val", "--num_workers", "2",
         "--batch_size", "4", "--per_image_scores", oute]))
    ze = np.load(oute + ".npz")
    assert list(ze["names"]) == ids and np.array_equal(ze["counts_main"], z1["counts_main"]) and np.array_equal(ze["hw"], z1["hw"])
    assert np.array_equal(res["image_scores"]["counts"]["main"], z1["counts_main"])

    out2 = str(tmp_path / "scores" / "api.csv")
    _, t2 = infer_lam.validate(parse(common + ["--label_dir", str(tmp_path / "l2"), "--per_image_scores", out2, "--api_path", "true"]))
    z2 = np.load(out2 + ".npz")
    assert np.array_equal(z2["counts_main"], _png_counts(ids, gt_of, tmp_path / "l2", 21)) and _margins_equal(z2["counts_main"], t2)
    assert list(z2["names"]) == ids and np.array_equal(z2["hw"], z1["hw"])

    out3 = str(tmp_path / "scores" / "conf.csv")
    _, t3 = infer_lam.validate(parse(common + ["--label_dir", str(tmp_path / "l3"), "--per_image_scores", out3, "--conf_label", "true",
                                               "--conf_label_dir", str(tmp_path / "c3")]))
    z3 = np.load(out3 + ".npz")
    assert sorted(z3.files) == ["counts_conf", "counts_main", "hw", "names"]
    assert np.array_equal(z3["counts_main"], z1["counts_main"])
    assert np.array_equal(z3["counts_conf"], _png_counts(ids, gt_of, tmp_path / "c3", 21))
    assert _margins_equal(z3["counts_conf"], infer_lam.validate.last_conf[1])
    with open(out3, newline="") as f:
        assert next(csv.reader(f))[-3:] == ["conf_pacc", "conf_miou", "conf_scored"]


def test_infer_lam_api_path_gives_the_batched_npz(gpu, tmp_path, monkeypatch):
    """The per-image path calls the op with B = 1 per image; on the same images its table is the batched loop's."""
    from _clip_files import write_tiny_clip
    from excel_amd.tools import infer_lam, synthetic
    root, lists = tmp_path / "VOC2012", tmp_path / "lists"
    synthetic.write_voc_tree(str(root), str(lists), 6, seed=4, split="val")
    ckpt, bpe_path, _ = write_tiny_clip(tmp_path)
    common = ["--data_folder", str(root), "--list_folder", str(lists), "--infer_set", "val", "--resize_size", "128", "--model", ckpt,
              "--bpe_path", bpe_path, "--batch_size", "4", "--num_workers", "2"]
    parse = infer_lam.get_parser().parse_args
    monkeypatch.chdir(tmp_path)
    a, b = str(tmp_path / "a.csv"), str(tmp_path / "b.csv")
    _, ta = infer_lam.validate(parse(common + ["--per_image_scores", a]))
    _, tb = infer_lam.validate(parse(common + ["--per_image_scores", b, "--api_path", "true"]))
    za, zb = np.load(a + ".npz"), np.load(b + ".npz")
    assert torch.equal(ta.cpu(), tb.cpu()), "precondition: the two paths label these images alike"
    assert np.array_equal(za["counts_main"], zb["counts_main"]) and list(za["names"]) == list(zb["names"])


def test_infer_lam_uniform_synthetic_loop(gpu, tmp_path):
    from _clip_files import write_tiny_clip
    from excel_amd.tools import infer_lam, synthetic
    ckpt, bpe_path, _ = write_tiny_clip(tmp_path)
    out = str(tmp_path / "u.csv")
    d = tmp_path / "labels"
    _, t = infer_lam.validate(infer_lam.get_parser().parse_args(["--synthetic", "6", "--resize_size", "128", "--model", ckpt, "--bpe_path", bpe_path,
                                                                 "--batch_size", "4", "--per_image_scores", out, "--save_label", "true",
                                                                 "--label_dir", str(d)]))
    ds = synthetic.SyntheticSegDataset(6, (128, 128), num_classes=21, seed=1234)
    gts = {ds[i][0]: ds[i][2] for i in range(6)}
    z = np.load(out + ".npz")
    assert list(z["names"]) == [ds[i][0] for i in range(6)]
    assert np.array_equal(z["counts_main"], _png_counts(list(z["names"]), gts.__getitem__, d, 21)) and _margins_equal(z["counts_main"], t)


def test_infer_lam_crf_inline_set(gpu, tmp_path, monkeypatch):
    from PIL import Image
    from _clip_files import write_tiny_clip
    from excel_amd.tools import infer_lam, synthetic
    root, lists = tmp_path / "VOC2012", tmp_path / "lists"
    ids, _ = synthetic.write_voc_tree(str(root), str(lists), 5, seed=4, split="val")
    ckpt, bpe_path, _ = write_tiny_clip(tmp_path)
    monkeypatch.chdir(tmp_path)
    out = str(tmp_path / "crf.csv")
    _, t = infer_lam.validate(infer_lam.get_parser().parse_args(
        ["--data_folder", str(root), "--list_folder", str(lists), "--infer_set", "val", "--resize_size", "128", "--model", ckpt, "--bpe_path", bpe_path,
         "--batch_size", "4", "--num_workers", "2", "--crf_post", "true", "--crf_inline", "true", "--crf_label_dir", str(tmp_path / "crf"),
         "--per_image_scores", out]))
    gt_of = lambda n: np.asarray(Image.open(root / "SegmentationClassAug" / (n + ".png")))
    z = np.load(out + ".npz")
    assert sorted(z.files) == ["counts_crf", "counts_main", "hw", "names"]
    assert np.array_equal(z["counts_crf"], _png_counts(ids, gt_of, tmp_path / "crf", 21))
    assert _margins_equal(z["counts_crf"], infer_lam.validate.last_crf[1]) and _margins_equal(z["counts_main"], t)


def test_infer_lam_guarded_rerun_replaces_the_flagged_rows(gpu, golden, tmp_path):
    """The overflow case of test_gpu_overflow_guard.py: the first pass leaves the flagged images' rows zero (skip), the exact-fp32
    second pass replaces them - every row is numpy's count over the composed labels."""
    import test_gpu_overflow_guard as og
    from excel_amd.tools import infer_lam
    from excel_amd.utils.image_scores import counts_numpy
    c = og._case("tf", "f16x3", golden)
    nc = og.NFG + 1
    pipe = c["mk"]("skip")
    pipe.image_scores = True
    out = str(tmp_path / "g.csv")
    args = infer_lam.get_parser().parse_args(["--num_classes", str(nc), "--resize_size", str(og.S6), "--batch_size", str(og.B6), "--num_workers", "2",
                                              "--overflow_guard", "rerun", "--per_image_scores", out])
    _, total = infer_lam.validate(args, dataset=og._SixSet(c), pipe=pipe)
    assert infer_lam.validate.last_guard["rerun"] == len(c["flagged"]) >= 1
    z = np.load(out + ".npz")
    want = np.stack([counts_numpy(c["gts"][b], c["composed"][b], nc) for b in range(og.B6)])
    assert list(z["names"]) == [f"g{b:03d}" for b in range(og.B6)]
    assert np.array_equal(z["counts_main"], want) and _margins_equal(z["counts_main"], total)
    assert all(z["counts_main"][b].any() for b in c["flagged"])
    # the first pass on its own: the flagged rows are zero
    from excel_amd import ops
    skip = c["mk"]("skip")
    skip.image_scores = True
    B = og.B6
    plan = ops.RaggedPlan([(og.S6, og.S6)] * B, "cuda")
    skip.run_batch_ragged(og.dev(np.concatenate([u.reshape(-1) for u in c["imgs"]])), plan, og.dev(c["cls"]),
                          og.dev(np.concatenate([g.reshape(-1) for g in c["gts"]])), S=og.S6)
    first = skip.last_score_ticket.counts()["main"]
    assert not first[c["flagged"]].any() and _margins_equal(first, skip.hist)
    with pytest.raises(ValueError, match="built without image_scores=True"):
        infer_lam.validate(args, dataset=og._SixSet(c), pipe=c["mk"]("skip"))


def test_validation_pipeline_ticket_holds_main_and_seg(gpu, golden):
    import test_gpu_overflow_guard as og
    from excel_amd import ops
    from excel_amd.pipeline import ValidationPipeline
    c = og._case("opt", "f16x3", golden)
    nc = og.NFG + 1
    h = c["model"].encoder.visual.handle()
    h.set_gemm_mode("f32")
    try:
        which = [3, 4, 5]
        plan = ops.RaggedPlan([(og.S6, og.S6)] * 3, "cuda")
        hwc = og.dev(np.concatenate([c["imgs"][b].reshape(-1) for b in which]))
        gt = og.dev(np.concatenate([c["gts"][b].reshape(-1) for b in which]))
        off = ValidationPipeline(c["model"], num_classes=nc, smax=og.NFG)
        off.run_batch_ragged(hwc, plan, og.dev(c["cls"][which]), gt, S=og.S6)
        assert off.last_score_ticket is None
        on = ValidationPipeline(c["model"], num_classes=nc, smax=og.NFG, image_scores=True)
        on.run_batch_ragged(hwc, plan, og.dev(c["cls"][which]), gt, S=og.S6)
        got = on.last_score_ticket.counts()
        assert sorted(got) == ["main", "seg"] and got["main"].shape == (3, 3, nc)
        assert torch.equal(on.hist, off.hist) and torch.equal(on.hist_seg, off.hist_seg)
        assert _margins_equal(got["main"], on.hist) and _margins_equal(got["seg"], on.hist_seg)
    finally:
        h.set_gemm_mode(c["mode"])


def test_infer_seg_voc_raw_and_crf_sets(gpu, tmp_path):
    """The tiny head of test_gpu_seg_eval.py: the raw set is numpy's count over the labels of the per-image chain (what the program's
    matrix is checked against there), the CRF set over the PNGs the run wrote."""
    import test_gpu_seg_eval as se
    from PIL import Image
    from excel_amd.tools import infer_seg_voc
    from excel_amd.utils.image_scores import counts_numpy
    root, lists, names = se._tree(tmp_path)
    ckpt = str(tmp_path / "run" / "checkpoints" / "model_iter_8.pth")
    model = se._tiny_model()
    nc = se.NUM_CLASSES
    out = str(tmp_path / "seg.csv")
    res = infer_seg_voc.validate(se._args(infer_seg_voc, root, lists, ckpt, "--batch_size", "3", "--crf_post", "true", "--per_image_scores", out),
                                 model=model)
    ds = infer_seg_voc.VOC.dataset(se._args(infer_seg_voc, root, lists, ckpt), "val")
    z = np.load(out + ".npz")
    assert sorted(z.files) == ["counts_crf", "counts_main", "hw", "names"] and list(z["names"]) == names
    raw = np.stack([counts_numpy(ds[i][2], se._restate(model, ds, i, infer_seg_voc.VOC, nc)[1].cpu().numpy(), nc) for i in range(len(ds))])
    crf = np.stack([counts_numpy(ds[i][2], np.asarray(Image.open(os.path.join(res["dirs"]["seg_preds"], n + ".png"))), nc)
                    for i, n in enumerate(names)])
    assert np.array_equal(z["counts_main"], raw) and np.array_equal(z["counts_crf"], crf)
    assert _margins_equal(z["counts_main"], res["hist"]) and _margins_equal(z["counts_crf"], res["hist_crf"])
    # image by image (--crf_batched false): the op with B = 1, the same table
    out2 = str(tmp_path / "seg1.csv")
    infer_seg_voc.validate(se._args(infer_seg_voc, root, lists, ckpt, "--batch_size", "2", "--crf_post", "true", "--crf_batched", "false",
                                    "--per_image_scores", out2), model=model)
    z2 = np.load(out2 + ".npz")
    assert np.array_equal(z2["counts_main"], raw) and np.array_equal(z2["counts_crf"].sum(0)[0], z["counts_crf"].sum(0)[0])
