"""Boundary scores, host side (no GPU): the erosion judge against scipy, the production numpy path against the judge on the whole case
table, non-vacuity of that table, the radius rule, the data-set arithmetic, flags and refusals of the four programs, the header and
the bindings, the pipelines' off switch, the files with and without the flag, and eval_labels' CPU path end to end."""
import csv
import inspect
import os
import re

import numpy as np
import pytest

import _boundary_ref as R

torch = pytest.importorskip("torch")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "boundary_scores")
NC = 6


def test_judge_is_scipy_binary_erosion():
    ndi = pytest.importorskip("scipy.ndimage")
    st = np.ones((3, 3), bool)
    for name, h, w, nc, d, seed in R.case_table()[::3]:
        g, _, _ = R.case(h, w, nc, d, seed)
        for c in np.unique(g)[:3]:
            m = g == c
            want = m & ~ndi.binary_erosion(m, structure=st, iterations=d, border_value=0)
            assert np.array_equal(R.mask_to_boundary(m, d), want), (name, int(c))


def test_numpy_path_equals_the_judge_on_the_whole_case_table():
    from excel_amd.utils.image_scores import boundary_counts_numpy, counts_numpy
    table = R.case_table()
    assert len({(h, w) for _, h, w, _, _, _ in table}) == 7 and {nc for _, _, _, nc, _, _ in table} == {1, 21, 256}
    for name, h, w, nc, d, seed in table:
        g, p, ref = R.case(h, w, nc, d, seed)
        got = boundary_counts_numpy(g, p, nc, d)
        assert got.dtype == np.int64 and np.array_equal(got, ref), name
        if d >= max(h, w):                                    # the window always leaves the image: every valid pixel is a band pixel
            assert np.array_equal(ref, counts_numpy(g, p, nc)), name


def test_case_table_is_not_vacuous():
    """Wherever the image is large enough for an interior (min(H,W) > 4d+2) both maps have a class with 0 < band < area; the table
    also holds a 255 in both maps and a value in [nc, 255) where nc allows."""
    seen = 0
    for name, h, w, nc, d, seed in R.case_table():
        g, p, ref = R.case(h, w, nc, d, seed)
        if h * w >= 8:
            assert (g == 255).any() and (p == 255).any(), name
            if nc < 255:
                assert ((g >= nc) & (g < 255)).any(), name
        if min(h, w) > 4 * d + 2:
            seen += 1
            for m in (g, p):
                assert any(0 < band < area for band, area in (R.judge_band(m, c, d) for c in range(nc))), name
            assert 0 < ref[2].sum() < ref[0].sum(), name
    assert seen >= 8


def test_radius_rule_is_pinned():
    from excel_amd.utils.image_scores import boundary_radius
    assert boundary_radius(375, 500) == 12 and boundary_radius(448, 448) == 13 and boundary_radius(1, 1) == 1
    assert boundary_radius(300, 400) == 10
    assert boundary_radius(75, 100) == 2, "0.02 * 125 = 2.5: Python's round goes to the even neighbour"
    assert boundary_radius(375, 500, px=5) == 5 and boundary_radius(1, 1, ratio=0.5, px=3) == 3
    assert boundary_radius(375, 500, ratio=0.1) == 62 and boundary_radius(375, 500, ratio=0.02, px=0) == 12


def test_equal_maps_give_three_equal_rows():
    from excel_amd.utils.image_scores import boundary_counts_numpy
    for name, h, w, nc, d, seed in R.case_table()[::5]:
        g, p, _ = R.case(h, w, nc, d, seed)
        for m in (g, p):
            c = boundary_counts_numpy(m, m, nc, d)
            assert np.array_equal(c[0], c[1]) and np.array_equal(c[0], c[2]), name
            assert np.array_equal(c, R.judge_counts(m, m, nc, d)), name


def test_dataset_scores_are_the_formula_on_the_summed_counts():
    from excel_amd.utils.evaluate import boundary_scores_from_counts
    rs = np.random.RandomState(4)
    inter = rs.randint(0, 50, (5, NC))
    counts = np.stack([inter + rs.randint(0, 30, (5, NC)), inter + rs.randint(0, 30, (5, NC)), inter], 1)
    counts[:, :, 2] = 0                                        # a class in no band at all
    counts[:, 0, 3], counts[:, 2, 3] = 0, 0                    # a class with a predicted band only: IoU 0, not in the mean
    s = boundary_scores_from_counts(counts)
    tot = counts.sum(0).astype(np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        want = tot[2] / (tot[0] + tot[1] - tot[2])
    assert np.allclose(s["biou"], want, rtol=0, atol=0, equal_nan=True) and np.isnan(s["biou"][2]) and s["biou"][3] == 0.0
    assert s["mbiou"] == pytest.approx(np.mean(want[[0, 1, 4, 5]]), abs=1e-15)
    assert s["band_pixels"].dtype == np.int64 and np.array_equal(s["band_pixels"], counts[:, 0].sum(0))
    assert np.isnan(boundary_scores_from_counts(np.zeros((2, 3, NC), np.int32))["mbiou"])
    with pytest.raises(ValueError, match=r"\[N,3,nc\]"):
        boundary_scores_from_counts(np.zeros((3, NC)))


def test_flags_defaults_and_refusals_of_the_four_programs(tmp_path):
    from excel_amd.tools import eval_labels, infer_lam, infer_seg_coco, infer_seg_voc
    from excel_amd.utils import image_scores
    for prog in (infer_lam, infer_seg_voc, infer_seg_coco, eval_labels):
        extra = ["--pred_dir", "x", "--data_folder", "x", "--list_folder", "x"] if prog is eval_labels else []
        a = prog.get_parser().parse_args(extra)
        assert a.boundary_scores is False and a.boundary_ratio == 0.02 and a.boundary_px == 0
        assert image_scores.boundary_of(a) is None and not image_scores.wanted(a)
        a = prog.get_parser().parse_args(extra + ["--boundary_scores", "true", "--boundary_ratio", "0.05", "--boundary_px", "3"])
        assert image_scores.boundary_of(a) == dict(ratio=0.05, px=3) and image_scores.wanted(a)
    lam = lambda *more: infer_lam.get_parser().parse_args(["--boundary_scores", "true", *more])
    seg = lambda prog, *more: prog.get_parser().parse_args(["--boundary_scores", "true", *more])
    with pytest.raises(ValueError, match="--boundary_scores needs ground truth: --unlabeled true"):
        infer_lam.validate(lam("--unlabeled", "true", "--data_folder", str(tmp_path), "--save_label", "true"))
    for prog in (infer_seg_voc, infer_seg_coco):
        with pytest.raises(ValueError, match="--boundary_scores needs ground truth: --infer_set test is a test split"):
            prog.validate(seg(prog, "--infer_set", "test", "--test_data_folder", str(tmp_path)))
    ev = lambda *more: eval_labels.get_parser().parse_args(["--pred_dir", "x", "--data_folder", "x", "--list_folder", "x",
                                                            "--boundary_scores", "true", *more])
    for ratio in ("0", "-0.1", "1.5"):
        for run in (lambda: infer_lam.validate(lam("--boundary_ratio", ratio, "--synthetic", "2")),
                    lambda: infer_seg_voc.validate(seg(infer_seg_voc, "--boundary_ratio", ratio)),
                    lambda: infer_seg_coco.validate(seg(infer_seg_coco, "--boundary_ratio", ratio)),
                    lambda: eval_labels.validate(ev("--boundary_ratio", ratio))):
            with pytest.raises(ValueError, match=r"--boundary_ratio .* must be in \(0, 1\]"):
                run()
    for run in (lambda: infer_lam.validate(lam("--boundary_px", "-1", "--synthetic", "2")),
                lambda: infer_seg_voc.validate(seg(infer_seg_voc, "--boundary_px", "-1")),
                lambda: eval_labels.validate(ev("--boundary_px", "-1"))):
        with pytest.raises(ValueError, match="--boundary_px -1 must not be negative"):
            run()
    with pytest.raises(ValueError, match="--boundary_px 73 is beyond the largest radius"):
        eval_labels.validate(ev("--boundary_px", "73"))
    assert image_scores.boundary_of(eval_labels.get_parser().parse_args(
        ["--pred_dir", "x", "--data_folder", "x", "--list_folder", "x", "--boundary_ratio", "7"])) is None, "flag off: nothing is checked"


def test_header_and_bindings_agree_and_no_workspace_query_is_added():
    from excel_amd import _lib, ops
    with open(os.path.join(ROOT, "include", "excel_hip.h")) as f:
        header = f.read()
    decl = re.search(r"int excel_boundary_scores\(([^;]*)\);", header).group(1)
    nargs = len([a for a in re.sub(r"/\*.*?\*/", "", decl, flags=re.S).split(",") if a.strip()])
    ret, args = _lib.SIGNATURES["excel_boundary_scores"]
    assert nargs == len(args) == 13
    assert re.search(r"int excel_boundary_max_radius\(void\);", header) and _lib.SIGNATURES["excel_boundary_max_radius"][1] == []
    assert "boundary scores" in header
    assert not [s for s in list(_lib.SIGNATURES) + re.findall(r"\bexcel_\w+", header) if "boundary" in s and "workspace_bytes" in s]
    assert list(inspect.signature(ops.boundary_scores).parameters)[:7] == ["gt_u8", "pred_u8", "num_classes", "radius", "skip", "plan", "out"]
    assert not re.search(r"_ws\(|workspace", inspect.getsource(ops.boundary_scores))
    assert tuple(ops.BOUNDARY_TILE) == R.TILE
    from excel_amd import build
    assert "boundary.hip" in build.SOURCES and "boundary_scores_kernel" in build.NO_SCRATCH
    assert build.NO_SCRATCH_EXPECTED["boundary"] == "boundary_scores_kernel"


def test_pipelines_take_boundary_and_never_launch_without_it(monkeypatch):
    from excel_amd import ops, pipeline
    calls = []
    monkeypatch.setattr(ops, "boundary_scores", lambda *a, **k: calls.append("bd") or torch.zeros((2, 3, NC), dtype=torch.int32))
    monkeypatch.setattr(ops, "image_scores", lambda *a, **k: calls.append("img") or torch.zeros((2, 3, NC), dtype=torch.int32))
    monkeypatch.setattr(pipeline.ScoreTicket, "launch", _launch_without_events(pipeline.ScoreTicket.launch))
    monkeypatch.setattr(pipeline.TrainingFreePipeline, "_buf",                       # the real one is keyed by the launch stream
                        lambda self, name, numel, dtype=torch.float32, device=None: torch.empty(int(numel), dtype=dtype))
    for cls in (pipeline.TrainingFreePipeline, pipeline.OptimisedLamPipeline, pipeline.ValidationPipeline):
        assert inspect.signature(cls.__init__).parameters["boundary"].default is None
    with pytest.raises(ValueError, match="needs image_scores=True"):
        pipeline.TrainingFreePipeline(model=None, boundary=dict(ratio=0.02, px=0))
    with pytest.raises(ValueError, match="unknown keys"):
        pipeline.TrainingFreePipeline(model=None, image_scores=True, boundary=dict(radius=3))
    with pytest.raises(ValueError, match="must be in"):
        pipeline.TrainingFreePipeline(model=None, image_scores=True, boundary=dict(ratio=2.0))
    g = torch.zeros((2, 4, 5), dtype=torch.uint8)
    off = pipeline.TrainingFreePipeline(model=None, num_classes=NC, image_scores=True)
    assert off.boundary is None
    off.last_score_ticket = pipeline.ScoreTicket()
    off._image_scores("main", g, g)
    assert calls == ["img"] and sorted(off.last_score_ticket._parts) == ["main"]
    on = pipeline.TrainingFreePipeline(model=None, num_classes=NC, image_scores=True, boundary=dict(px=2))
    assert on.boundary == dict(ratio=0.02, px=2)
    on.last_score_ticket = pipeline.ScoreTicket()
    on._image_scores("main", g, g)
    assert calls == ["img", "img", "bd"] and sorted(on.last_score_ticket._parts) == ["main", "main_bd"]
    for name in ("run_batch_split", "run_batch_overlapped"):                      # the paths that refuse image scores refuse these too
        with pytest.raises(ValueError, match="no per-image scores"):
            getattr(on, name)(None, None)


def _launch_without_events(launch):
    """ScoreTicket.launch on a machine without a GPU: pinned memory and events are replaced, the calls to ops stay."""
    def run(self, *a, **k):
        import unittest.mock as mock
        empty = torch.empty
        with mock.patch.object(torch, "empty", lambda *s, **kw: empty(*s, **{x: v for x, v in kw.items() if x != "pin_memory"})), \
                mock.patch.object(torch.cuda, "Event", lambda: mock.Mock()):
            return launch(self, *a, **k)
    return run


def _tables(boundary):
    """A deterministic two-set log of four images, with or without boundary counts -> merged"""
    from excel_amd.utils.image_scores import ImageScoreLog, boundary_counts_numpy, boundary_radius, counts_numpy
    log = ImageScoreLog(NC, ("main", "crf"), boundary=boundary)
    for i, (h, w) in enumerate([(9, 14), (30, 41), (5, 5), (17, 65)]):
        g, p = R.block_maps(h, w, NC, 2, 50 + i)
        if i == 2:
            g = np.full_like(g, 255)                           # an image without a scored pixel
        for s, pr in (("main", p), ("crf", g)):
            log.put(3 - i, f"img{3 - i:02d}", (h, w), s, counts_numpy(g, pr, NC))
            if boundary is not None:
                log.put(3 - i, f"img{3 - i:02d}", (h, w), s + "_bd", boundary_counts_numpy(g, pr, NC, boundary_radius(h, w, **log.boundary)))
    return log.merged()


CATS = ["background", "a", "b", "c", "d", "e"]


def test_files_without_the_flag_are_those_of_the_writer_before_it(tmp_path):
    """golden/boundary_scores/plain.csv was written by utils/image_scores.write_files as it was before boundary scores existed, from this
    very table: the CSV is the same bytes, the npz holds the same arrays under the same names."""
    from excel_amd.utils import image_scores
    merged = _tables(None)
    assert sorted(merged) == ["counts", "hw", "index", "names"]
    path = str(tmp_path / "plain.csv")
    image_scores.write_files(path, merged, CATS)
    with open(path, "rb") as f, open(os.path.join(GOLDEN, "plain.csv"), "rb") as g:
        assert f.read() == g.read()
    z = np.load(path + ".npz")
    assert sorted(z.files) == ["counts_crf", "counts_main", "hw", "names"]
    want = np.load(os.path.join(GOLDEN, "plain_counts.npy"))
    assert np.array_equal(np.stack([z["counts_main"], z["counts_crf"]]), want) and z["counts_main"].dtype == np.int64


def test_files_with_the_flag_gain_columns_and_arrays(tmp_path):
    from excel_amd.utils import image_scores
    from excel_amd.utils.evaluate import image_score_rows
    plain, merged = _tables(None), _tables(dict(ratio=0.02, px=0))
    assert merged["radius"].tolist() == [image_scores.boundary_radius(h, w) for h, w in merged["hw"]]
    path, ppath = str(tmp_path / "bd.csv"), str(tmp_path / "plain.csv")
    image_scores.write_files(path, merged, CATS)
    image_scores.write_files(ppath, plain, CATS)
    with open(path, newline="") as f, open(ppath, newline="") as g:
        rows, prow = list(csv.reader(f)), list(csv.reader(g))
    assert rows[0] == prow[0] + ["radius", "biou", "crf_biou"]
    bd = image_score_rows(merged["bcounts"]["main"])
    for i, (r, q) in enumerate(zip(rows[1:], prow[1:])):
        assert r[:len(q)] == q and int(r[-3]) == merged["radius"][i]
        assert np.allclose(float(r[-2]), bd["miou"][i], atol=1e-6, equal_nan=True)
        assert r[-1] == ("nan" if r[0] == "img01" else "1.000000")          # the crf set is gt against gt; img01 has no scored pixel
    z = np.load(path + ".npz")
    assert sorted(z.files) == ["bcounts_crf", "bcounts_main", "counts_crf", "counts_main", "hw", "names", "radius"]
    assert z["bcounts_main"].dtype == np.int64 and np.array_equal(z["bcounts_main"], merged["bcounts"]["main"])
    assert z["radius"].dtype == np.int32 and np.array_equal(z["counts_main"], plain["counts"]["main"])
    summary = image_scores.boundary_summary(merged)
    assert sorted(summary) == ["crf", "main"] and summary["crf"]["mbiou"] == 1.0 and 0 < summary["main"]["mbiou"] < 1
    text = image_scores.boundary_table(summary["main"], CATS)
    assert text.splitlines()[0].split() == ["class", "bIoU", "band_pixels"] and [ln.split()[0] for ln in text.splitlines()[1:]] == CATS + ["mean"]
    assert image_scores.boundary_summary(plain) == {}
    js = image_scores.boundary_json(merged, dict(ratio=0.02, px=0))
    assert js["sets"]["main"]["mbiou"] == summary["main"]["mbiou"] and js["radius_max"] == int(merged["radius"].max())


def test_a_missing_boundary_twin_is_an_error():
    from excel_amd.utils.image_scores import ImageScoreLog
    log = ImageScoreLog(NC, ("main",), boundary=dict(px=2))
    log.put(0, "x", (2, 2), "main", np.zeros((3, NC)))
    with pytest.raises(RuntimeError, match=r"'x' has no counts for \['main_bd'\]"):
        log.merged()
    with pytest.raises(ValueError, match="not recorded"):
        ImageScoreLog(NC, ("main",)).put(0, "x", (2, 2), "main_bd", np.zeros((3, NC)))


def test_eval_labels_on_the_cpu_end_to_end(tmp_path, monkeypatch, caplog):
    """eval_labels without a GPU on a tiny on-disk tree: bcounts_main is the judge's count of every image at the radius of the host
    rule, the logged table is boundary_scores_from_counts of the npz; without --per_image_scores no file appears and the table is the
    same; an image whose radius is beyond the build's maximum stops the run."""
    import logging
    from PIL import Image
    from excel_amd.tools import eval_labels, synthetic
    from excel_amd.utils import image_scores
    from excel_amd.utils.evaluate import boundary_scores_from_counts
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    root, lists, pred = tmp_path / "VOC2012", tmp_path / "lists", tmp_path / "pred"
    ids, _ = synthetic.write_voc_tree(str(root), str(lists), 4, seed=2, split="val")
    os.makedirs(pred)
    want = []
    for n in ids:
        gt = np.asarray(Image.open(root / "SegmentationClassAug" / (n + ".png")))
        pr = np.roll(np.where(gt == 255, 0, gt), (2, 3), (0, 1)).astype(np.uint8)
        Image.fromarray(pr).save(pred / (n + ".png"))
        want.append(R.judge_counts(gt, pr, 21, image_scores.boundary_radius(*gt.shape)))
    want = np.stack(want)
    base = ["--pred_dir", str(pred), "--data_folder", str(root), "--list_folder", str(lists), "--infer_set", "val", "--num_workers", "2",
            "--batch_size", "3"]
    out = str(tmp_path / "scores.csv")
    with caplog.at_level(logging.INFO):
        res = eval_labels.validate(eval_labels.get_parser().parse_args(base + ["--boundary_scores", "true", "--per_image_scores", out]))
    z = np.load(out + ".npz")
    assert list(z["names"]) == ids and np.array_equal(z["bcounts_main"], want) and want[:, 2].sum() > 0
    assert np.array_equal(z["radius"], [image_scores.boundary_radius(h, w) for h, w in z["hw"]])
    score = boundary_scores_from_counts(z["bcounts_main"])
    assert "boundary_score of the labels" in caplog.text and image_scores.boundary_table(score, eval_labels.VOC_CLASSES) in caplog.text
    assert np.array_equal(res["image_scores"]["bcounts"]["main"], want)
    before = sorted(os.listdir(tmp_path))
    caplog.clear()
    with caplog.at_level(logging.INFO):
        res2 = eval_labels.validate(eval_labels.get_parser().parse_args(base + ["--boundary_scores", "true", "--boundary_px", "2"]))
    assert sorted(os.listdir(tmp_path)) == before and "boundary_score of the labels" in caplog.text
    assert np.array_equal(res2["image_scores"]["bcounts"]["main"],
                          np.stack([R.judge_counts(np.asarray(Image.open(root / "SegmentationClassAug" / (n + ".png"))),
                                                   np.asarray(Image.open(pred / (n + ".png"))), 21, 2) for n in ids]))
    plain = eval_labels.validate(eval_labels.get_parser().parse_args(base))
    assert "image_scores" not in plain and np.array_equal(plain["hist"].numpy(), res["hist"].numpy())
    with pytest.raises(ValueError, match=r"has radius \d+, beyond the largest this build accepts \(72\)"):
        eval_labels.validate(eval_labels.get_parser().parse_args(base + ["--boundary_scores", "true", "--boundary_ratio", "1.0"]))
