"""The nearest-label fill on the GPU: excel_fill_nearest_label (fill.hip) against the brute-force judge of tests/_fill_ref.py, integer
for integer - squared distances and a raster-order tie rule make the result canonical, so there is no tolerance and no pixel is left
out -, at sizes around the tile and the row pass's stride, in ragged and uniform batches, at misaligned addresses, into poisoned
outputs; the ties and the radius edge by hand; the refusals; the stream contract; the pipeline step and infer_lam end to end."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _fill_ref as R  # noqa: E402
import _streams as St  # noqa: E402


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


def test_the_stride_is_the_judges(gpu):
    from excel_amd.utils import label_fill as lf
    assert lf.FILL_ROW_THREADS == R.T


@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("pattern", sorted(R.PATTERNS))
def test_every_size_in_one_ragged_batch(gpu, pattern, masked):
    """All sizes of the table as one ragged launch, into outputs whose every byte was 0xFF; a second run gives identical bits."""
    from excel_amd.utils import label_fill as lf
    cases = [R.want(pattern, s, masked) for s in R.SIZES]
    maps = [c[0] for c in cases]
    plan, lab = _ragged(maps)
    mask = _ragged([c[1] for c in cases])[1] if masked else None
    out = (_poisoned(lab.numel(), torch.uint8), _poisoned(lab.numel(), torch.int32), _poisoned(3 * len(maps), torch.int32))
    filled, dist2, counts = lf.fill_nearest_label(lab, R.NC, plan=plan, mask=mask, out=out)
    again = lf.fill_nearest_label(lab, R.NC, plan=plan, mask=mask)
    torch.cuda.synchronize()
    for b, ((m, _, want_o, want_d, want_n), got_o, got_d) in enumerate(zip(cases, _split(filled, maps), _split(dist2, maps))):
        assert np.array_equal(got_o, want_o), f"out of {pattern} {m.shape}"
        assert np.array_equal(got_d, want_d), f"dist2 of {pattern} {m.shape}"
        assert counts[b].tolist() == want_n.tolist(), f"counts of {pattern} {m.shape}: {counts[b].tolist()} {want_n.tolist()}"
    assert all(torch.equal(a, b) for a, b in zip(again, (filled, dist2, counts))), "two runs differ"


@pytest.mark.parametrize("radius", [1, 2, 5])
def test_every_size_within_a_radius(gpu, radius):
    from excel_amd.utils import label_fill as lf
    for pattern in ("random21", "sparse_seeds", "passthrough"):
        cases = [R.want(pattern, s, False, radius * radius) for s in R.SIZES]
        maps = [c[0] for c in cases]
        plan, lab = _ragged(maps)
        filled, dist2, counts = lf.fill_nearest_label(lab, R.NC, plan=plan, radius=radius)
        for b, ((m, _, want_o, want_d, want_n), got_o, got_d) in enumerate(zip(cases, _split(filled, maps), _split(dist2, maps))):
            assert np.array_equal(got_o, want_o) and np.array_equal(got_d, want_d), (pattern, m.shape, radius)
            assert counts[b].tolist() == want_n.tolist(), (pattern, m.shape, radius)


@pytest.mark.parametrize("masked", [False, True])
def test_uniform_batch(gpu, masked):
    from excel_amd.utils import label_fill as lf
    size = (2 * 16 + 3, 2 * 64 + 5)
    cases = [R.want(p, size, masked) for p in ("random21", "sparse_seeds")]
    lab = _dev(np.stack([c[0] for c in cases]))
    mask = _dev(np.stack([c[1] for c in cases])) if masked else None
    filled, dist2, counts = lf.fill_nearest_label(lab, R.NC, mask=mask)
    assert filled.shape == lab.shape and filled.dtype == torch.uint8 and dist2.shape == lab.shape and dist2.dtype == torch.int32
    for b, (_, _, want_o, want_d, want_n) in enumerate(cases):
        assert np.array_equal(filled[b].cpu().numpy(), want_o) and np.array_equal(dist2[b].cpu().numpy(), want_d)
        assert counts[b].tolist() == want_n.tolist()
    assert int(counts[:, 1].sum()) > 0


def test_ties_go_to_the_first_seed_in_raster_order(gpu):
    from excel_amd.utils import label_fill as lf
    cases = R.tie_cases()
    maps = [c[1] for c in cases]
    plan, lab = _ragged(maps)
    filled, dist2, _ = lf.fill_nearest_label(lab, R.NC, plan=plan)
    for (name, m, (y, x), value, d2), got_o, got_d in zip(cases, _split(filled, maps), _split(dist2, maps)):
        assert int(got_o[y, x]) == value and int(got_d[y, x]) == d2, (name, int(got_o[y, x]), int(got_d[y, x]))
        want_o, want_d, _ = R.fill(m)
        assert np.array_equal(got_o, want_o) and np.array_equal(got_d, want_d), name


def test_the_radius_includes_its_edge(gpu):
    """One seed at the origin, radius 5: the hole at (3,4) lies at d2 = 25 and is filled, the hole at (4,4), d2 = 32, stays."""
    from excel_amd.utils import label_fill as lf
    m = np.full((6, 6), 255, np.uint8)
    m[0, 0] = 9
    filled, dist2, counts = lf.fill_nearest_label(_dev(m[None]), R.NC, radius=5)
    o, d = filled[0].cpu().numpy(), dist2[0].cpu().numpy()
    assert o[3, 4] == 9 and d[3, 4] == 25 and o[4, 3] == 9 and d[4, 3] == 25 and o[4, 4] == 255 and d[4, 4] == -1 and o[0, 5] == 9 and d[0, 5] == 25
    want_o, want_d, want_n = R.fill(m, max_dist2=25)
    assert np.array_equal(o, want_o) and np.array_equal(d, want_d) and counts[0].tolist() == want_n.tolist() and int(counts[0, 2]) == 25


def test_nothing_reaches_across_images(gpu):
    """All-hole images of 1 x 1 and 3 x 70 between all-seed neighbours of one value: they stay 255 and report nothing filled."""
    from excel_amd.utils import label_fill as lf
    maps = [np.full((2, 5), 4, np.uint8), np.full((1, 1), 255, np.uint8), np.full((1, 66), 4, np.uint8), np.full((3, 70), 255, np.uint8),
            np.full((17, 3), 4, np.uint8)]
    plan, lab = _ragged(maps)
    filled, dist2, counts = lf.fill_nearest_label(lab, R.NC, plan=plan)
    assert torch.equal(filled, lab)
    for b, (m, d) in enumerate(zip(maps, _split(dist2, maps))):
        hole = m[0, 0] == 255
        assert (d == (-1 if hole else 0)).all() and counts[b].tolist() == [m.size if hole else 0, 0, 0], (b, counts[b].tolist())


@pytest.mark.parametrize("offset", [0, 1, 3])
def test_maps_that_start_at_any_byte(gpu, offset):
    from excel_amd.utils import label_fill as lf
    cases = [R.want("random21", s, True) for s in ((17, 63), (1, 65), (16, 64))]
    maps = [c[0] for c in cases]
    plan, flat = _ragged(maps)
    mflat = _ragged([c[1] for c in cases])[1]
    bufs = [torch.zeros(flat.numel() + 64, dtype=torch.uint8, device="cuda") for _ in range(3)]
    lab, mask, out = (b[offset:offset + flat.numel()] for b in bufs)
    lab.copy_(flat)
    mask.copy_(mflat)
    assert lab.data_ptr() % 16 == offset and out.data_ptr() % 16 == offset
    filled, dist2, counts = lf.fill_nearest_label(lab, R.NC, plan=plan, mask=mask, out=(out, torch.empty(flat.numel(), dtype=torch.int32, device="cuda"),
                                                                                   torch.empty(9, dtype=torch.int32, device="cuda")))
    assert filled.data_ptr() == out.data_ptr()
    for b, ((m, _, want_o, want_d, want_n), got_o, got_d) in enumerate(zip(cases, _split(filled, maps), _split(dist2, maps))):
        assert np.array_equal(got_o, want_o) and np.array_equal(got_d, want_d) and counts[b].tolist() == want_n.tolist(), (offset, m.shape)
    assert bool((bufs[2][:offset] == 0).all()) and bool((bufs[2][offset + flat.numel():] == 0).all()), "a write outside the maps"


def test_bad_arguments_are_refused_before_any_launch(gpu):
    from excel_amd import ops
    from excel_amd.utils import label_fill as lf
    plan = ops.RaggedPlan([(2, 4), (3, 5)], "cuda")
    n = plan.total_label_pix
    lab = torch.full((n + 8,), 255, dtype=torch.uint8, device="cuda")
    mask = torch.zeros(n + 8, dtype=torch.uint8, device="cuda")
    out = torch.full((2 * n + 8,), 0x5A, dtype=torch.uint8, device="cuda")
    dist2 = torch.full((n + 8,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    counts = torch.full((16,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    lib = ops.lib()
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    lp, mp, op, dp, cp = (C.c_void_p(t.data_ptr()) for t in (lab, mask, out, dist2, counts))
    info, tab = C.byref(plan.info), C.c_void_p(plan.table.data_ptr())
    off = lambda t, k: C.c_void_p(t.data_ptr() + k)
    big = plan.info.__class__.from_buffer_copy(plan.info)
    big.total_label_pix = 2 ** 31
    M = 2 ** 31 - 1
    for args, word in (((None, mp, 2, 0, 0, tab, info, 21, M, op, dp, cp, st), "null argument"),
                       ((lp, mp, 2, 0, 0, tab, info, 21, M, None, dp, cp, st), "null argument"),
                       ((lp, mp, 2, 0, 0, tab, info, 21, M, op, None, cp, st), "null argument"),
                       ((lp, mp, 2, 0, 0, tab, info, 21, M, op, dp, None, st), "null argument"),
                       ((lp, None, 2, 0, 0, tab, info, 21, M, lp, dp, cp, st), "out overlaps labels"),
                       ((lp, None, 2, 0, 0, tab, info, 21, M, off(lab, n - 1), dp, cp, st), "out overlaps labels"),
                       ((lp, mp, 2, 0, 0, tab, info, 21, M, mp, dp, cp, st), "out overlaps mask"),
                       ((lp, mp, 2, 0, 0, tab, info, 21, M, off(mask, n - 1), dp, cp, st), "out overlaps mask"),
                       ((lp, mp, 2, 0, 0, tab, info, 0, M, op, dp, cp, st), "num_classes"),
                       ((lp, mp, 2, 0, 0, tab, info, 256, M, op, dp, cp, st), "num_classes"),
                       ((lp, mp, 2, 0, 0, tab, info, 21, 0, op, dp, cp, st), "max_dist2 >= 1 (got 0)"),
                       ((lp, mp, 2, 0, 0, tab, info, 21, -4, op, dp, cp, st), "max_dist2 >= 1 (got -4)"),
                       ((lp, mp, 0, 2, 4, None, None, 21, M, op, dp, cp, st), "1 <= B <= 65535 (B = 0)"),
                       ((lp, mp, 65536, 1, 1, None, None, 21, M, op, dp, cp, st), "1 <= B <= 65535 (B = 65536)"),
                       ((lp, mp, 3, 0, 0, tab, info, 21, M, op, dp, cp, st), "the plan holds 2 images, B = 3"),
                       ((lp, mp, 1, 8193, 1, None, None, 21, M, op, dp, cp, st), "beyond 8192 pixels a side"),
                       ((lp, mp, 1, 1, 8193, None, None, 21, M, op, dp, cp, st), "beyond 8192 pixels a side"),
                       ((lp, mp, 1, 0, 4, None, None, 21, M, op, dp, cp, st), "H >= 1 and W >= 1"),
                       ((lp, mp, 2, 0, 0, tab, C.byref(big), 21, M, op, dp, cp, st), "outside [1, 2^31)"),
                       ((lp, mp, 64, 8192, 8192, None, None, 21, M, op, dp, cp, st), "outside [1, 2^31)"),
                       ((lp, mp, 2, 0, 0, tab, info, 21, M, op, off(dist2, 2), cp, st), "4-byte aligned"),
                       ((lp, mp, 2, 0, 0, tab, info, 21, M, op, dp, off(counts, 1), st), "4-byte aligned")):
        assert lib.excel_fill_nearest_label(*args) == -1, word
        assert word in lib.excel_last_error().decode(), (word, lib.excel_last_error())
    torch.cuda.synchronize()
    for t, v in ((out, 0x5A), (dist2, 0x5A5A5A5A), (counts, 0x5A5A5A5A)):
        assert bool((t == v).all()), "a refused call wrote to its outputs"
    # the wrapper's own checks
    for kw, word in ((dict(radius=0), "fill_ignore"), (dict(radius=2.5), "fill_ignore"), (dict(radius="far"), "fill_ignore"),
                     (dict(radius=True), "fill_ignore"), (dict(mask=mask[:n].int()), "mask must hold"), (dict(mask=mask), "mask must hold")):
        with pytest.raises(ValueError, match=word):
            lf.fill_nearest_label(lab[:n], 21, plan=plan, **kw)
    with pytest.raises(ValueError, match=r"outside \[1, 255\]"):
        lf.fill_nearest_label(lab[:n], 256, plan=plan)
    with pytest.raises(ValueError, match="the plan holds 23"):
        lf.fill_nearest_label(lab, 21, plan=plan)
    with pytest.raises(ValueError, match=r"uniform maps must be \[B,H,W\]"):
        lf.fill_nearest_label(lab, 21)
    with pytest.raises(ValueError, match="labels must be uint8"):
        lf.fill_nearest_label(lab[:n].int(), 21, plan=plan)
    with pytest.raises(ValueError, match="beyond 8192 pixels a side"):
        lf.fill_nearest_label(torch.zeros((1, 1, 8193), dtype=torch.uint8, device="cuda"), 21)
    with pytest.raises(RuntimeError, match="out overlaps labels"):
        lf.fill_nearest_label(lab[:n], 21, plan=plan, out=(lab[:n], dist2[:n], counts[:6]))
    filled, d2, cnt = lf.fill_nearest_label(lab[:n], 21, plan=plan, radius="inf")       # all holes, no seed: accepted, nothing filled
    assert torch.equal(filled, lab[:n]) and bool((d2 == -1).all()) and cnt.tolist() == [[8, 0, 0], [15, 0, 0]]


# ------------------------------------------------------------------ the stream contract (tests/_streams.py, by import)
@pytest.fixture(scope="module")
def t_link(gpu):
    t = St.time_link()
    print(f"\n[fill streams] one chain link: {t * 1e6:.0f} us")
    assert t > 0
    return t


@pytest.fixture(scope="module")
def stream_case(gpu):
    """fn() -> the op's outputs from uninitialised memory on the current stream, and the reference on the idle default stream."""
    from excel_amd.utils import label_fill as lf
    maps = [R.PATTERNS[p](h, w) for p, (h, w) in (("random21", (120, 200)), ("passthrough", (75, 333)), ("random21", (17, 65)), ("random21", (200, 120))) * 4]
    plan, lab = _ragged(maps)
    mask = _ragged([R.mask_of(*m.shape) for m in maps])[1]
    torch.cuda.synchronize()

    def fn():
        filled, dist2, counts = lf.fill_nearest_label(lab, R.NC, plan=plan, mask=mask, radius=9)
        return dict(filled=filled, dist2=dist2, counts=counts)
    return fn, St.reference(fn)


@pytest.mark.parametrize("arrangement", ["behind", "beside"])
def test_the_op_stays_on_its_callers_stream(gpu, stream_case, t_link, arrangement):
    fn, ref = stream_case
    links = St.links_for(ref.t_case, t_link)
    run = (St.run_behind if arrangement == "behind" else St.run_beside)(fn, links)
    print(f"\n[fill streams] {arrangement}: t_case {ref.t_case * 1e3:.2f} ms, {run.links} links, side-stream run {run.host_s * 1e3:.2f} ms, "
          f"default stream busy afterwards: {run.busy}")
    assert int(ref.tree["counts"][:, 1].sum()) > 0
    if arrangement == "behind":
        St.assert_matches(ref.tree, run.final, None, "queued behind a busy chain on its own stream")
        return
    St.assert_matches(ref.tree, run.early, None, "(a) beside a busy default stream, read when the side stream was done")
    St.assert_matches(ref.tree, run.final, None, "(b) beside a busy default stream, read after the device had drained")
    assert run.busy, "(c) " + St.busy_message(run, ref.t_case, t_link)


# ------------------------------------------------------------------ the pipeline and the program
def _png(path):
    from PIL import Image
    return np.asarray(Image.open(path))


def _hist(g, p, nc=21):
    g, p = g.reshape(-1).astype(np.int64), p.reshape(-1).astype(np.int64)
    m = (g < nc) & (p < nc)
    return np.bincount(nc * g[m] + p[m], minlength=nc * nc).reshape(nc, nc)


@pytest.fixture(scope="module")
def program(gpu, tmp_path_factory):
    """infer_lam.validate on the synthetic ragged set (6 images at batch 4: two steps) with the tiny checkpoint, --clean_min_region 8
    --fill_ignore inf and every output the flags have.  The model of the run serves the pipeline test."""
    import json
    import logging
    from _clip_files import write_tiny_clip
    from excel_amd.tools import infer_lam
    tmp = tmp_path_factory.mktemp("fill")
    ckpt, bpe_path, _ = write_tiny_clip(tmp)
    js, table = str(tmp / "run.json"), str(tmp / "rows.csv")
    argv = ["--synthetic", "6", "--ragged", "true", "--resize_size", "96", "--model", ckpt, "--bpe_path", bpe_path, "--batch_size", "4",
            "--num_workers", "2", "--gemm_check", "false", "--save_label", "true", "--label_dir", str(tmp / "labels"), "--clean_min_region", "8",
            "--clean_label_dir", str(tmp / "clean"), "--fill_ignore", "inf", "--fill_label_dir", str(tmp / "fill"), "--json_out", js,
            "--per_image_scores", table]
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
        _, total = infer_lam.validate(infer_lam.get_parser().parse_args(argv))
        with open(js) as f:
            record = json.load(f)
    finally:
        logging.getLogger().removeHandler(cap)
        logging.getLogger().setLevel(level)
        os.chdir(cwd)
    return dict(tmp=tmp, total=total.cpu().numpy(), record=record, table=table, log="\n".join(lines), last=infer_lam.validate.last_fill,
                clean=infer_lam.validate.last_clean, model=infer_lam.validate.last_model)


def test_infer_lam_fill_ignore(gpu, program):
    import csv
    from excel_amd.tools import infer_lam, synthetic
    from excel_amd.utils import label_fill as lf
    from excel_amd.utils.evaluate import scores_from_hist
    p = program
    ds = synthetic.SyntheticSegDataset(6, num_classes=21, seed=1234, ragged=True)
    hist, rows, names = np.zeros((21, 21), np.int64), [], []
    for i in range(6):
        name, gt = ds[i][0], ds[i][2]
        main, cleaned = _png(p["tmp"] / "labels" / f"{name}.png"), _png(p["tmp"] / "clean" / f"{name}.png")
        want, _, cnt = R.fill(cleaned, 21, mask=main)
        assert np.array_equal(_png(p["tmp"] / "fill" / f"{name}.png"), want), name
        hist += _hist(np.asarray(gt), want)
        rows.append(cnt.tolist())
        names.append(name)
    last = p["last"]
    print("holes, filled, largest d2 per image:", rows)
    assert sum(r[1] for r in rows) > 0, "the case fills nothing"
    assert last["names"] == names and last["counts"].tolist() == rows and last["radius"] is None
    assert np.array_equal(last["hist"].cpu().numpy(), hist), "fill_label_score is `evaluate` on the filled files"
    want_score = scores_from_hist(torch.from_numpy(hist))
    assert last["score"]["miou"] == want_score["miou"] and last["coverage"] == hist.sum() / p["total"].sum()
    assert last["coverage"] >= p["clean"]["coverage"]
    stats = lf.fill_stats(np.asarray(rows))
    assert "fill_label_score (--fill_ignore inf):" in p["log"] and infer_lam.format_scores_table(want_score, infer_lam.VOC_CLASSES) in p["log"]
    assert lf.format_fill_summary(stats, last["coverage"]) in p["log"]
    assert p["record"]["fill"] == lf.fill_json(None, stats, want_score, last["coverage"]) and p["record"]["fill"]["filled"] == stats["filled"]
    with open(p["table"]) as f:
        table = list(csv.reader(f))
    assert table[0][-3:] == ["holes", "filled", "max_fill_dist"] and "fill_miou" in table[0] and "clean_miou" in table[0]
    assert [r[0] for r in table[1:]] == names and [[int(r[-3]), int(r[-2])] for r in table[1:]] == [r[:2] for r in rows]
    npz = np.load(p["table"] + ".npz")
    assert npz["fills"].tolist() == rows and np.array_equal(npz["counts_fill"].sum(0), np.stack([hist.sum(1), hist.sum(0), np.diag(hist)]))


def test_pipeline_fill_step(gpu, program):
    """clean= and fill= on the ragged step: the filled maps are the judge's answer on last_clean_labels with the main labels as mask,
    hist_fill is the host confusion of those maps, and the main and clean outputs equal those of a pipeline built without fill."""
    from excel_amd import ops
    from excel_amd.pipeline import TrainingFreePipeline
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
    maps = [np.empty(s, np.uint8) for s in sizes]
    clean = dict(min_region=6, connectivity=4)
    plain = TrainingFreePipeline(model, num_classes=21, smax=3, image_scores=True, clean=clean)
    plain_labels = plain.run_batch_ragged(images, plan, cls, gts, S=96)
    assert plain.last_fill_labels is None and plain.last_fill_counts is None and plain.last_fill_dist2 is None and plain.hist_fill is None
    assert "fill" not in plain.last_score_ticket.counts()
    for radius in (None, 2):
        p = TrainingFreePipeline(model, num_classes=21, smax=3, image_scores=True, clean=clean, fill=dict(radius=radius))
        labels = p.run_batch_ragged(images, plan, cls, gts, S=96)
        assert torch.equal(labels, plain_labels) and torch.equal(p.last_clean_labels, plain.last_clean_labels)
        assert torch.equal(p.last_clean_counts, plain.last_clean_counts) and torch.equal(p.hist, plain.hist) and torch.equal(p.hist_clean, plain.hist_clean)
        hist = np.zeros((21, 21), np.int64)
        for b, (main, cleaned, got, got_d, g) in enumerate(zip(_split(labels, maps), _split(p.last_clean_labels, maps), _split(p.last_fill_labels, maps),
                                                               _split(p.last_fill_dist2, maps), gts_h)):
            want, want_d, cnt = R.fill(cleaned, 21, mask=main, max_dist2=None if radius is None else radius * radius)
            assert np.array_equal(got, want) and np.array_equal(got_d, want_d) and p.last_fill_counts[b].tolist() == cnt.tolist(), (radius, b)
            hist += _hist(g, want)
        assert int(p.last_fill_counts[:, 1].sum()) > 0, "the case fills nothing"
        assert np.array_equal(p.hist_fill.cpu().numpy(), hist) and p.hist_fill.dtype == torch.int64
        assert np.array_equal(p.last_score_ticket.counts()["fill"].sum(0), np.stack([hist.sum(1), hist.sum(0), np.diag(hist)]))
        p.reset()
        assert p.hist_fill is None
    with pytest.raises(ValueError, match="fill needs clean"):
        TrainingFreePipeline(model, num_classes=21, smax=3, fill=dict(radius=None))
    p = TrainingFreePipeline(model, num_classes=21, smax=3, clean=clean, fill=dict(radius=3))
    for fn in (p.run_batch, p.run_batch_split, p.run_batch_overlapped):
        with pytest.raises(ValueError, match="has no label cleaning"):
            fn(torch.zeros(2, 3, 96, 96, device="cuda"), cls[:2])


def test_eval_labels_on_the_device_equals_its_numpy_path(gpu, program, monkeypatch):
    from excel_amd.tools import eval_labels, synthetic
    from PIL import Image
    p = program
    ds = synthetic.SyntheticSegDataset(6, num_classes=21, seed=1234, ragged=True)
    root, lists = p["tmp"] / "VOC", p["tmp"] / "lists"
    (root / "SegmentationClassAug").mkdir(parents=True, exist_ok=True)
    lists.mkdir(exist_ok=True)
    names = [ds[i][0] for i in range(6)]
    for i, n in enumerate(names):
        Image.fromarray(np.asarray(ds[i][2], np.uint8)).save(root / "SegmentationClassAug" / f"{n}.png")
    (lists / "val.txt").write_text("\n".join(names) + "\n")
    parse = eval_labels.get_parser().parse_args
    for tag, extra in (("plain", []), ("cleaned", ["--clean_min_region", "12", "--clean_connectivity", "4"])):
        base = ["--pred_dir", str(p["tmp"] / "clean"), "--data_folder", str(root), "--list_folder", str(lists), "--infer_set", "val",
                "--num_workers", "2", "--batch_size", "4", "--fill_ignore", "3"] + extra
        with monkeypatch.context() as mp:
            dev = eval_labels.validate(parse(base + ["--fill_label_dir", str(p["tmp"] / f"ev_dev_{tag}")]))
            mp.setattr(torch.cuda, "is_available", lambda: False)
            host = eval_labels.validate(parse(base + ["--fill_label_dir", str(p["tmp"] / f"ev_host_{tag}")]))
        assert np.array_equal(dev["fill"]["hist"].numpy(), host["fill"]["hist"].numpy()) and dev["fill"]["counts"].tolist() == host["fill"]["counts"].tolist()
        assert dev["fill"]["coverage"] == host["fill"]["coverage"] and int(dev["fill"]["counts"][:, 1].sum()) > 0
        for n in names:
            assert np.array_equal(_png(p["tmp"] / f"ev_dev_{tag}" / f"{n}.png"), _png(p["tmp"] / f"ev_host_{tag}" / f"{n}.png")), (tag, n)
