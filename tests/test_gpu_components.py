"""Connected components and the small-region filter on the GPU: excel_label_components / excel_filter_small_regions (components.hip)
against the plain two-pass judge of tests/_components_ref.py, integer for integer - the root of a component is canonical (its first
pixel in raster order), so there is no tolerance and no relabelling -, at sizes around the 64 x 16 tile, on patterns that stress the
seams and the corner rule, in uniform and ragged batches, at misaligned addresses, into poisoned outputs; the filter's rules; the
refusals; the stream contract."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _components_ref as R  # noqa: E402
import _streams as St  # noqa: E402

TH, TW = R.TILE


@pytest.fixture(scope="module")
def gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import excel_amd.ops  # noqa: F401
    return True


def _dev(a):
    return torch.from_numpy(np.array(a)).cuda()


def _poisoned(n, dtype):
    """n elements whose every byte is 0xFF"""
    return torch.full((n * torch.empty((), dtype=dtype).element_size(),), 0xFF, dtype=torch.uint8, device="cuda").view(dtype)


def _ragged(maps):
    from excel_amd import ops
    plan = ops.RaggedPlan([m.shape for m in maps], "cuda")
    return plan, _dev(np.concatenate([m.reshape(-1) for m in maps]))


def _split(flat, maps):
    out, o = [], 0
    flat = flat.cpu().numpy()
    for m in maps:
        out.append(flat[o:o + m.size].reshape(m.shape))
        o += m.size
    return out


def test_the_tile_is_the_judges(gpu):
    from excel_amd.utils import components as cc
    assert tuple(cc.COMPONENTS_TILE) == R.TILE


@pytest.mark.parametrize("connectivity", [4, 8])
@pytest.mark.parametrize("pattern", sorted(R.PATTERNS))
def test_every_size_in_one_ragged_batch(gpu, pattern, connectivity):
    """All sizes of the table as one ragged launch, into outputs whose every byte was 0xFF; a second run gives identical bits."""
    from excel_amd.utils import components as cc
    cases = [R.judged(pattern, s, connectivity) for s in R.SIZES]
    maps = [c[0] for c in cases]
    plan, lab = _ragged(maps)
    comp, area = _poisoned(lab.numel(), torch.int32), _poisoned(lab.numel(), torch.int32)
    cc.label_components(lab, plan=plan, connectivity=connectivity, out=(comp, area))
    again = cc.label_components(lab, plan=plan, connectivity=connectivity)
    torch.cuda.synchronize()
    for (m, want_c, want_a), got_c, got_a in zip(cases, _split(comp, maps), _split(area, maps)):
        assert np.array_equal(got_c, want_c), f"comp of {pattern} {m.shape} at {connectivity}"
        assert np.array_equal(got_a, want_a), f"area of {pattern} {m.shape} at {connectivity}"
    assert torch.equal(again[0], comp) and torch.equal(again[1], area), "two runs differ"


def test_what_the_patterns_are_for(gpu):
    """The judge's own answers on the patterns: they exercise what they are named after (a check of the cases, not of the kernels)."""
    big = (3 * TH, 3 * TW)
    assert len(np.unique(R.judged("constant", big, 4)[1])) == 1
    assert len(np.unique(R.judged("checkerboard", big, 4)[1])) == big[0] * big[1]
    assert len(np.unique(R.judged("checkerboard", big, 8)[1])) == 2
    m, comp, _ = R.judged("serpentine", big, 4)
    assert len(np.unique(comp[m == 1])) == 1
    m, comp, _ = R.judged("comb", big, 4)
    assert len(np.unique(comp[m == 5])) == 1
    m, comp, _ = R.judged("u_shape", big, 4)
    assert len(np.unique(comp[m == 9])) == 1 and m[1, TW - 1] == 9 and m[2, TW - 1] == 0 and m[2, TW + 3] == 9
    for conn, n in ((4, 2), (8, 1)):
        m, comp, _ = R.judged("corner_diagonals", big, conn)
        assert m[TH - 1, TW - 1] == m[TH, TW] == 11 and len(np.unique(comp[m == 11])) == n and len(np.unique(comp[m == 12])) == n


@pytest.mark.parametrize("connectivity", [4, 8])
def test_uniform_batch(gpu, connectivity):
    from excel_amd.utils import components as cc
    size = (2 * TH + 3, 2 * TW + 5)
    cases = [R.judged(p, size, connectivity) for p in ("blobs", "random21")]
    lab = _dev(np.stack([c[0] for c in cases]))
    comp, area = cc.label_components(lab, connectivity=connectivity)
    assert comp.shape == lab.shape and comp.dtype == torch.int32
    for b, (_, want_c, want_a) in enumerate(cases):
        assert np.array_equal(comp[b].cpu().numpy(), want_c) and np.array_equal(area[b].cpu().numpy(), want_a)


def test_nothing_connects_across_images(gpu):
    """Constant maps of ONE value back to back - 1 x 1, one row, several tiles, 1 x 1 again: the last pixel of every image equals the
    first pixel of the next, and every image is still one component of its own, rooted at its own pixel 0."""
    from excel_amd.utils import components as cc
    maps = [np.full(s, 4, np.uint8) for s in ((1, 1), (1, TW + 9), (2 * TH + 1, TW + 3), (1, 1), (TH + 2, 1))]
    plan, lab = _ragged(maps)
    for conn in (4, 8):
        comp, area = cc.label_components(lab, plan=plan, connectivity=conn)
        for m, c, a in zip(maps, _split(comp, maps), _split(area, maps)):
            assert (c == 0).all() and (a == m.size).all(), (m.shape, conn)


@pytest.mark.parametrize("offset", [0, 1, 3])
def test_maps_that_start_at_any_byte(gpu, offset):
    """The maps start `offset` bytes behind a 16-byte boundary: a uniform batch whose rows are whole 16-byte segments (the wide loads
    at offset 0, the byte path otherwise) and a ragged one."""
    from excel_amd.utils import components as cc
    size = (TH + 3, 2 * TW)
    cases = [R.judged(p, size, 8) for p in ("blobs", "random2")]
    host = np.stack([c[0] for c in cases])
    buf = torch.zeros(host.size + 64, dtype=torch.uint8, device="cuda")
    assert buf.data_ptr() % 16 == 0
    lab = buf[offset:offset + host.size].view(host.shape)
    lab.copy_(_dev(host))
    comp, area = cc.label_components(lab, connectivity=8)
    cleaned, counts = cc.filter_small_regions(lab, comp, area, 6, 21)
    assert lab.data_ptr() % 16 == offset
    for b, (m, want_c, want_a) in enumerate(cases):
        assert np.array_equal(comp[b].cpu().numpy(), want_c) and np.array_equal(area[b].cpu().numpy(), want_a)
        want, want_n = R.clean(m, 6, 21, 8)
        assert np.array_equal(cleaned[b].cpu().numpy(), want) and counts[b].tolist() == want_n.tolist()
    rag = [R.judged("blobs", s, 8) for s in ((TH + 1, TW + 1), (5, 7), (TH, TW))]
    maps = [c[0] for c in rag]
    plan, flat = _ragged(maps)
    buf2 = torch.zeros(flat.numel() + 64, dtype=torch.uint8, device="cuda")
    lab2 = buf2[offset:offset + flat.numel()]
    lab2.copy_(flat)
    comp, area = cc.label_components(lab2, plan=plan, connectivity=8)
    for (m, want_c, want_a), c, a in zip(rag, _split(comp, maps), _split(area, maps)):
        assert np.array_equal(c, want_c) and np.array_equal(a, want_a)


# ------------------------------------------------------------------ the filter
def _filter_maps():
    rs = np.random.RandomState(5)
    maps = [R.PATTERNS["blobs"](2 * TH + 3, 2 * TW + 5), R.PATTERNS["random21"](TH + 1, TW - 1), np.full((1, 1), 3, np.uint8),
            R.PATTERNS["random2"](1, TW + 7), R.PATTERNS["blobs"](TH, TW)]
    maps[1] = maps[1].copy()
    maps[1][rs.rand(*maps[1].shape) < 0.1] = 30                # a value >= num_classes that is not 255
    return maps


@pytest.mark.parametrize("connectivity", [4, 8])
def test_filter_rules_and_counts(gpu, connectivity):
    from excel_amd.utils import components as cc
    maps = _filter_maps()
    plan, lab = _ragged(maps)
    comp, area = cc.label_components(lab, plan=plan, connectivity=connectivity)
    # min_area 1 removes nothing
    cleaned, counts = cc.filter_small_regions(lab, comp, area, 1, 21, plan=plan)
    assert torch.equal(cleaned, lab) and (counts[:, 1:] == 0).all()
    assert counts[:, 0].tolist() == [int(R.clean(m, 1, 21, connectivity)[1][0]) for m in maps]
    # per-image thresholds in one launch, a host sequence and a device tensor; outputs whose every byte was 0xFF
    thr = [7, 3, 1, 2, 2 ** 20]                                 # the last one is above the image's area: every class pixel goes
    for arg in (thr, _dev(np.asarray(thr, np.int32))):
        out = (_poisoned(lab.numel(), torch.uint8), _poisoned(3 * len(maps), torch.int32))
        cleaned, counts = cc.filter_small_regions(lab, comp, area, arg, 21, plan=plan, out=out)
        for b, (m, got) in enumerate(zip(maps, _split(cleaned, maps))):
            want, want_n = R.clean(m, thr[b], 21, connectivity)
            assert np.array_equal(got, want), (b, m.shape)
            assert counts[b].tolist() == want_n.tolist(), (b, counts[b].tolist(), want_n)
    last = _split(cleaned, maps)[-1]
    assert (last[maps[-1] < 21] == 255).all() and int(counts[-1, 0]) == int(counts[-1, 1]) > 0
    # values >= num_classes are untouched and uncounted: with num_classes = 1 only the background's regions exist
    cleaned, counts = cc.filter_small_regions(lab, comp, area, 2 ** 20, 1, plan=plan)
    for b, (m, got) in enumerate(zip(maps, _split(cleaned, maps))):
        assert np.array_equal(got[m >= 1], m[m >= 1]) and (got[m == 0] == 255).all()
        want_n = R.clean(m, 2 ** 20, 1, connectivity)[1]
        assert counts[b].tolist() == want_n.tolist() and int(counts[b, 2]) == int((m == 0).sum())


def test_a_region_of_exactly_min_area_stays(gpu):
    from excel_amd.utils import components as cc
    m = np.zeros((TH + 2, TW + 2), np.uint8)
    m[2, 3:8] = 1                                              # 5 pixels
    m[TH, TW - 2:TW + 2] = 2                                   # 4 pixels, across the vertical seam
    m[TH - 1:TH + 1, 10] = 255                                 # an ignore region of 2 pixels: never removed, never counted
    lab = _dev(m[None])
    comp, area = cc.label_components(lab, connectivity=4)
    cleaned, counts = cc.filter_small_regions(lab, comp, area, 5, 21)
    got = cleaned[0].cpu().numpy()
    assert (got[2, 3:8] == 1).all() and (got[TH, TW - 2:TW + 2] == 255).all() and (got[m == 0] == 0).all()
    assert counts.tolist() == [[3, 1, 4]]
    cleaned, counts = cc.filter_small_regions(lab, comp, area, 6, 21)
    assert (cleaned[0].cpu().numpy()[m > 0] == 255).all() and counts.tolist() == [[3, 2, 9]]


def test_a_threshold_below_one_is_refused_per_image(gpu):
    from excel_amd.utils import components as cc
    maps = _filter_maps()[:3]
    plan, lab = _ragged(maps)
    comp, area = cc.label_components(lab, plan=plan)
    cleaned, counts = cc.filter_small_regions(lab, comp, area, _dev(np.asarray([4, 0, -3], np.int32)), 21, plan=plan)
    got = _split(cleaned, maps)
    want, want_n = R.clean(maps[0], 4, 21, 8)
    assert np.array_equal(got[0], want) and counts[0].tolist() == want_n.tolist()
    assert np.array_equal(got[1], maps[1]) and np.array_equal(got[2], maps[2]), "a refused image's map is copied unchanged"
    assert counts[1].tolist() == [-1, -1, -1] and counts[2].tolist() == [-1, -1, -1]
    with pytest.raises(ValueError, match="image 1 has min_area 0"):
        cc.filter_small_regions(lab, comp, area, [4, 0, 2], 21, plan=plan)
    with pytest.raises(ValueError, match="integer >= 1"):
        cc.filter_small_regions(lab, comp, area, 0, 21, plan=plan)


def test_bad_arguments_are_refused_before_any_launch(gpu):
    from excel_amd import ops
    plan = ops.RaggedPlan([(2, 4), (3, 5)], "cuda")
    n = plan.total_label_pix
    lab = torch.zeros(n + 8, dtype=torch.uint8, device="cuda")
    comp = torch.full((n + 8,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    area = torch.full((n + 8,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    out = torch.full((n + 8,), 0x5A, dtype=torch.uint8, device="cuda")
    counts = torch.full((16,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    lib = ops.lib()
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    lp, cp, ap, op, np_ = (C.c_void_p(t.data_ptr()) for t in (lab, comp, area, out, counts))
    info, tab = C.byref(plan.info), C.c_void_p(plan.table.data_ptr())
    off = lambda t, k: C.c_void_p(t.data_ptr() + k)
    big = plan.info.__class__.from_buffer_copy(plan.info)
    big.total_label_pix = 2 ** 31
    for args, word in (((None, 2, 0, 0, tab, info, 8, cp, ap, st), "null argument"),
                       ((lp, 2, 0, 0, tab, info, 8, None, ap, st), "null argument"),
                       ((lp, 2, 0, 0, tab, info, 8, cp, None, st), "null argument"),
                       ((lp, 2, 0, 0, tab, info, 6, cp, ap, st), "connectivity must be 4 or 8 (got 6)"),
                       ((lp, 0, 2, 4, None, None, 8, cp, ap, st), "1 <= B <= 65535 (B = 0)"),
                       ((lp, 65536, 1, 1, None, None, 8, cp, ap, st), "1 <= B <= 65535 (B = 65536)"),
                       ((lp, 3, 0, 0, tab, info, 8, cp, ap, st), "the plan holds 2 images, B = 3"),
                       ((lp, 2, 0, 0, tab, None, 8, cp, ap, st), "the plan holds -1 images"),
                       ((lp, 2, 0, 0, tab, C.byref(big), 8, cp, ap, st), "outside [1, 2^31)"),
                       ((lp, 1, 0, 4, None, None, 8, cp, ap, st), "H >= 1 and W >= 1"),
                       ((lp, 1, 65536, 32768, None, None, 8, cp, ap, st), "too large an image"),
                       ((lp, 2, 0, 0, tab, info, 8, off(comp, 2), ap, st), "4-byte aligned"),
                       ((lp, 2, 0, 0, tab, info, 8, cp, off(area, 1), st), "4-byte aligned")):
        assert lib.excel_label_components(*args) == -1, word
        assert word in lib.excel_last_error().decode(), (word, lib.excel_last_error())
    for args, word in (((None, cp, ap, 2, 0, 0, tab, info, None, 4, 21, op, np_, st), "null argument"),
                       ((lp, None, ap, 2, 0, 0, tab, info, None, 4, 21, op, np_, st), "null argument"),
                       ((lp, cp, None, 2, 0, 0, tab, info, None, 4, 21, op, np_, st), "null argument"),
                       ((lp, cp, ap, 2, 0, 0, tab, info, None, 4, 21, None, np_, st), "null argument"),
                       ((lp, cp, ap, 2, 0, 0, tab, info, None, 4, 21, op, None, st), "null argument"),
                       ((lp, cp, ap, 2, 0, 0, tab, info, None, 4, 0, op, np_, st), "num_classes"),
                       ((lp, cp, ap, 2, 0, 0, tab, info, None, 4, 257, op, np_, st), "num_classes"),
                       ((lp, cp, ap, 0, 2, 4, None, None, None, 4, 21, op, np_, st), "1 <= B <= 65535"),
                       ((lp, cp, ap, 2, 0, 0, tab, info, None, 4, 21, lp, np_, st), "out overlaps labels"),
                       ((lp, cp, ap, 2, 0, 0, tab, info, None, 4, 21, off(lab, n - 1), np_, st), "out overlaps labels"),
                       ((lp, cp, ap, 2, 0, 0, tab, info, None, 4, 21, op, off(counts, 2), st), "4-byte aligned"),
                       ((lp, cp, ap, 2, 0, 0, tab, info, off(counts, 1), 4, 21, op, np_, st), "4-byte aligned")):
        assert lib.excel_filter_small_regions(*args) == -1, word
        assert word in lib.excel_last_error().decode(), (word, lib.excel_last_error())
    torch.cuda.synchronize()
    for t, v in ((comp, 0x5A5A5A5A), (area, 0x5A5A5A5A), (counts, 0x5A5A5A5A), (out, 0x5A)):
        assert bool((t == v).all()), "a refused call wrote to its outputs"
    # the wrapper's own checks
    from excel_amd.utils import components as cc
    with pytest.raises(ValueError, match="must be 4 or 8"):
        cc.label_components(lab[:n], plan=plan, connectivity=6)
    with pytest.raises(ValueError, match="the plan holds 23"):
        cc.label_components(lab, plan=plan)
    with pytest.raises(ValueError, match=r"uniform maps must be \[B,H,W\]"):
        cc.label_components(lab)
    with pytest.raises(RuntimeError, match="out overlaps labels"):
        cc.filter_small_regions(lab[:n], comp[:n], area[:n], 2, 21, plan=plan, out=(lab[:n], counts[:6]))


# ------------------------------------------------------------------ the stream contract (tests/_streams.py, by import)
@pytest.fixture(scope="module")
def t_link(gpu):
    t = St.time_link()
    print(f"\n[components streams] one chain link: {t * 1e6:.0f} us")
    assert t > 0
    return t


@pytest.fixture(scope="module")
def stream_case(gpu):
    """fn() -> both ops' outputs from uninitialised memory on the current stream, and the reference on the idle default stream."""
    from excel_amd.utils import components as cc
    maps = [R.PATTERNS[p](h, w) for p, (h, w) in (("blobs", (120, 200)), ("constant", (75, 333)), ("random21", (17, 65)), ("blobs", (200, 120))) * 4]
    plan, lab = _ragged(maps)
    thr = _dev(np.asarray([5, 2, 3, 9] * 4, np.int32))
    torch.cuda.synchronize()

    def fn():
        comp, area = cc.label_components(lab, plan=plan, connectivity=8)
        cleaned, counts = cc.filter_small_regions(lab, comp, area, thr, 21, plan=plan)
        return dict(comp=comp, area=area, cleaned=cleaned, counts=counts)
    return fn, St.reference(fn)


@pytest.mark.parametrize("arrangement", ["behind", "beside"])
def test_the_ops_stay_on_their_callers_stream(gpu, stream_case, t_link, arrangement):
    fn, ref = stream_case
    links = St.links_for(ref.t_case, t_link)
    run = (St.run_behind if arrangement == "behind" else St.run_beside)(fn, links)
    print(f"\n[components streams] {arrangement}: t_case {ref.t_case * 1e3:.2f} ms, {run.links} links, side-stream run {run.host_s * 1e3:.2f} ms, "
          f"default stream busy afterwards: {run.busy}")
    assert int(ref.tree["counts"][:, 1].sum()) > 0
    if arrangement == "behind":
        St.assert_matches(ref.tree, run.final, None, "queued behind a busy chain on its own stream")
        return
    St.assert_matches(ref.tree, run.early, None, "(a) beside a busy default stream, read when the side stream was done")
    St.assert_matches(ref.tree, run.final, None, "(b) beside a busy default stream, read after the device had drained")
    assert run.busy, "(c) " + St.busy_message(run, ref.t_case, t_link)


# ------------------------------------------------------------------ the pipeline and the programs
@pytest.fixture(scope="module")
def program(gpu, tmp_path_factory):
    """infer_lam.validate on a synthetic VOC tree (6 ragged images at batch 4: two steps) with the tiny checkpoint: once plain, once with
    --clean_min_region 32 and every output the flag has.  The model of the second run serves the pipeline test."""
    import json
    import logging
    from _clip_files import write_tiny_clip
    from excel_amd.tools import infer_lam, synthetic
    tmp = tmp_path_factory.mktemp("components")
    root, lists = tmp / "VOC2012", tmp / "lists"
    synthetic.write_voc_tree(str(root), str(lists), 6, seed=4, split="val")
    ckpt, bpe_path, _ = write_tiny_clip(tmp)
    common = ["--data_folder", str(root), "--list_folder", str(lists), "--infer_set", "val", "--resize_size", "128", "--model", ckpt,
              "--bpe_path", bpe_path, "--batch_size", "4", "--num_workers", "2", "--save_label", "true"]
    parse = infer_lam.get_parser().parse_args
    lines = []

    class Capture(logging.Handler):
        def emit(self, record):
            lines.append(record.getMessage())
    cap = Capture(logging.INFO)
    cwd = os.getcwd()
    os.chdir(tmp)
    logging.getLogger().addHandler(cap)
    level = logging.getLogger().level
    logging.getLogger().setLevel(logging.INFO)
    try:
        _, plain = infer_lam.validate(parse(common + ["--label_dir", str(tmp / "plain")]))
        assert infer_lam.validate.last_clean is None and not any("clean" in x for x in lines)
        js, table = str(tmp / "run.json"), str(tmp / "rows.csv")
        _, cleaned = infer_lam.validate(parse(common + ["--label_dir", str(tmp / "labels"), "--clean_min_region", "32", "--clean_label_dir",
                                                        str(tmp / "clean"), "--json_out", js, "--per_image_scores", table]))
        with open(js) as f:
            record = json.load(f)
    finally:
        logging.getLogger().removeHandler(cap)
        logging.getLogger().setLevel(level)
        os.chdir(cwd)
    with open(lists / "val.txt") as f:
        names = [x.split()[0] for x in f.read().split("\n") if x.strip()]
    return dict(common=common, tmp=tmp, root=root, lists=lists, names=names, plain=plain.cpu().numpy(), cleaned=cleaned.cpu().numpy(), record=record, table=table,
                log="\n".join(lines), last=infer_lam.validate.last_clean, model=infer_lam.validate.last_model)


def _png(path):
    from PIL import Image
    return np.asarray(Image.open(path))


def _hist(g, p, nc=21):
    g, p = g.reshape(-1).astype(np.int64), p.reshape(-1).astype(np.int64)
    m = (g < nc) & (p < nc)
    return np.bincount(nc * g[m] + p[m], minlength=nc * nc).reshape(nc, nc)


def test_infer_lam_clean_min_region(gpu, program):
    import csv
    from excel_amd.tools import infer_lam
    from excel_amd.utils import components as cc
    from excel_amd.utils.evaluate import scores_from_hist
    p = program
    assert np.array_equal(p["plain"], p["cleaned"]), "the flag changes no score of the plain labels"
    hist, rows = np.zeros((21, 21), np.int64), []
    for n in p["names"]:
        lab = _png(p["tmp"] / "labels" / f"{n}.png")
        assert open(p["tmp"] / "labels" / f"{n}.png", "rb").read() == open(p["tmp"] / "plain" / f"{n}.png", "rb").read(), "same bytes without the flag"
        want, cnt = cc.clean_numpy(lab, 32, 21, 8)
        assert np.array_equal(_png(p["tmp"] / "clean" / f"{n}.png"), want), n
        hist += _hist(_png(p["root"] / "SegmentationClassAug" / f"{n}.png"), want)
        rows.append(cnt.tolist())
    last = p["last"]
    print("regions, removed, pixels per image:", rows)
    assert last["names"] == p["names"] and last["counts"].tolist() == rows
    assert np.array_equal(last["hist"].cpu().numpy(), hist), "clean_label_score is `evaluate` on the cleaned files"
    want_score = scores_from_hist(torch.from_numpy(hist))
    assert last["score"]["miou"] == want_score["miou"] and last["score"]["pAcc"] == want_score["pAcc"]
    assert last["coverage"] == hist.sum() / p["plain"].sum()
    assert "clean_label_score (--clean_min_region 32, connectivity 8):" in p["log"]
    assert infer_lam.format_scores_table(want_score, infer_lam.VOC_CLASSES) in p["log"]
    assert cc.format_clean_summary(cc.region_stats(np.asarray(rows)), last["coverage"]) in p["log"]
    assert p["record"]["clean"] == cc.clean_json(32, 8, cc.region_stats(np.asarray(rows)), want_score, last["coverage"])
    with open(p["table"]) as f:
        table = list(csv.reader(f))
    assert table[0][-6:] == ["clean_pacc", "clean_miou", "clean_scored", "regions", "regions_removed", "pixels_removed"]
    assert [r[0] for r in table[1:]] == p["names"] and [[int(v) for v in r[-3:]] for r in table[1:]] == rows
    npz = np.load(p["table"] + ".npz")
    assert np.array_equal(npz["counts_clean"].sum(0), np.stack([hist.sum(1), hist.sum(0), np.diag(hist)])) and npz["regions"].tolist() == rows


def test_infer_lam_unlabeled_writes_the_cleaned_maps(gpu, program, monkeypatch):
    """--unlabeled true: nothing is scored, the cleaned maps are the output - the same files the labelled run wrote."""
    from excel_amd.tools import infer_lam
    p = program
    monkeypatch.chdir(p["tmp"])
    parse = infer_lam.get_parser().parse_args
    score, total = infer_lam.validate(parse(p["common"] + ["--unlabeled", "true", "--label_dir", str(p["tmp"] / "u_labels"), "--clean_min_region", "32",
                                                           "--clean_label_dir", str(p["tmp"] / "u_clean")]))
    last = infer_lam.validate.last_clean
    assert score is None and int(total.sum()) == 0 and last["score"] is None and last["coverage"] is None
    assert last["names"] == p["names"] and last["counts"].tolist() == p["last"]["counts"].tolist()
    for n in p["names"]:
        assert np.array_equal(_png(p["tmp"] / "u_clean" / f"{n}.png"), _png(p["tmp"] / "clean" / f"{n}.png")), n
    with pytest.raises(ValueError, match="give --clean_label_dir"):
        infer_lam.validate(parse(p["common"] + ["--unlabeled", "true", "--clean_min_region", "32"]))


def test_pipeline_clean_with_the_guards_skip_flags(gpu, program):
    """clean= on the ragged step: the cleaned maps, the counts, the kept pixels' matrix and the ticket's "clean" set, with and without
    the guard (the tiny model overflows nothing: the flags are zero, the results equal the unguarded ones)."""
    from excel_amd import ops
    from excel_amd.pipeline import TrainingFreePipeline
    from excel_amd.utils import components as cc
    model = program["model"]
    rs = np.random.RandomState(41)
    sizes = [(40, 151), (17, 65), (64, 96), (33, 70)]
    images = _dev(np.concatenate([rs.randint(0, 256, (h, w, 3)).astype(np.uint8).reshape(-1) for h, w in sizes]))
    gts_h = [rs.randint(0, 21, (h, w)).astype(np.uint8) for h, w in sizes]
    gts = _dev(np.concatenate([g.reshape(-1) for g in gts_h]))
    cls = np.zeros((4, 20), np.float32)
    for b, k in enumerate([1, 3, 2, 3]):
        cls[b, rs.choice(20, size=k, replace=False)] = 1
    cls = _dev(cls)
    plan = ops.RaggedPlan(sizes, "cuda")
    got = {}
    for guard in (None, "skip", "observe"):
        for value in (6, 0.01):
            p = TrainingFreePipeline(model, num_classes=21, smax=3, guard=guard, image_scores=True, clean=dict(min_region=value, connectivity=4))
            labels = p.run_batch_ragged(images, plan, cls, gts, S=128)
            maps = [np.empty(s, np.uint8) for s in sizes]
            lab_h, clean_h = _split(labels, maps), _split(p.last_clean_labels, maps)
            hist = np.zeros((21, 21), np.int64)
            for b, (m, g) in enumerate(zip(lab_h, gts_h)):
                want, cnt = R.clean(m, cc.min_area_rule(value, *m.shape), 21, 4)
                assert np.array_equal(clean_h[b], want) and p.last_clean_counts[b].tolist() == cnt.tolist(), (guard, value, b)
                hist += _hist(g, want)
            assert np.array_equal(p.hist_clean.cpu().numpy(), hist) and p.hist_clean.dtype == torch.int64
            counts = p.last_score_ticket.counts()
            assert np.array_equal(counts["clean"].sum(0), np.stack([hist.sum(1), hist.sum(0), np.diag(hist)]))
            got[(guard, value)] = (labels.cpu().numpy(), hist)
            p.reset()
            assert p.hist_clean is None
    for value in (6, 0.01):
        for guard in ("skip", "observe"):
            assert np.array_equal(got[(None, value)][0], got[(guard, value)][0]) and np.array_equal(got[(None, value)][1], got[(guard, value)][1])
    # the default step leaves nothing behind, and the other entry points refuse the option
    plain = TrainingFreePipeline(model, num_classes=21, smax=3)
    assert torch.equal(plain.run_batch_ragged(images, plan, cls, gts, S=128), _dev(got[(None, 6)][0]))
    assert plain.last_clean_labels is None and plain.last_clean_counts is None and plain.hist_clean is None
    p = TrainingFreePipeline(model, num_classes=21, smax=3, clean=dict(min_region=6))
    for fn in (p.run_batch, p.run_batch_split, p.run_batch_overlapped):
        with pytest.raises(ValueError, match="has no label cleaning"):
            fn(torch.zeros(2, 3, 128, 128, device="cuda"), cls[:2])


def test_eval_labels_on_the_device_equals_its_numpy_path(gpu, program, monkeypatch):
    from excel_amd.tools import eval_labels
    p = program
    base = ["--pred_dir", str(p["tmp"] / "labels"), "--data_folder", str(p["root"]), "--list_folder", str(p["lists"]), "--infer_set", "val",
            "--num_workers", "2", "--batch_size", "4", "--clean_min_region", "0.002", "--clean_connectivity", "4"]
    parse = eval_labels.get_parser().parse_args
    dev = eval_labels.validate(parse(base + ["--clean_label_dir", str(p["tmp"] / "ev_dev")]))
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    host = eval_labels.validate(parse(base + ["--clean_label_dir", str(p["tmp"] / "ev_host")]))
    assert np.array_equal(dev["hist"].numpy(), host["hist"].numpy())
    assert np.array_equal(dev["clean"]["hist"].numpy(), host["clean"]["hist"].numpy())
    assert dev["clean"]["counts"].tolist() == host["clean"]["counts"].tolist() and dev["clean"]["coverage"] == host["clean"]["coverage"]
    for n in p["names"]:
        assert np.array_equal(_png(p["tmp"] / "ev_dev" / f"{n}.png"), _png(p["tmp"] / "ev_host" / f"{n}.png")), n


def test_infer_lam_guarded_rerun_cleans_the_second_pass(gpu, golden, tmp_path):
    """The overflow case of test_gpu_overflow_guard.py with --overflow_guard rerun: a flagged image's cleaned map, counts row and PNG come
    from its exact-fp32 second pass - every image's outputs are clean_numpy of the composed labels, and the kept pixels are counted once."""
    import test_gpu_overflow_guard as og
    from excel_amd.tools import infer_lam
    from excel_amd.utils import components as cc
    c = og._case("tf", "f16x3", golden)
    nc = og.NFG + 1
    pipe = c["mk"]("skip")
    pipe.clean = dict(min_region=6, connectivity=8)
    args = infer_lam.get_parser().parse_args(["--num_classes", str(nc), "--resize_size", str(og.S6), "--batch_size", str(og.B6), "--num_workers", "2",
                                              "--overflow_guard", "rerun", "--clean_min_region", "6", "--clean_label_dir", str(tmp_path / "clean")])
    infer_lam.validate(args, dataset=og._SixSet(c), pipe=pipe)
    assert infer_lam.validate.last_guard["rerun"] == len(c["flagged"]) >= 1
    last = infer_lam.validate.last_clean
    hist = np.zeros((nc, nc), np.int64)
    for b in range(og.B6):
        want, cnt = cc.clean_numpy(c["composed"][b], 6, nc, 8)
        assert np.array_equal(_png(tmp_path / "clean" / f"g{b:03d}.png"), want), b
        assert last["counts"][b].tolist() == cnt.tolist(), b
        hist += _hist(c["gts"][b], want, nc)
    assert np.array_equal(last["hist"].cpu().numpy(), hist)
