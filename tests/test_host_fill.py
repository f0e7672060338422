"""The nearest-label fill without a GPU: the numpy restatement against the brute-force judge, the ties and the radius edge by hand, the
C ABI, the flags of infer_lam and eval_labels with their refusals, the pipelines' option, and eval_labels --fill_ignore end to end on
its numpy path."""
import os
import re
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _fill_ref as R  # noqa: E402

from excel_amd.utils import label_fill as lf  # noqa: E402


# ------------------------------------------------------------------ the restatement and the judge
def test_the_size_table_is_placed_around_the_row_stride():
    assert lf.FILL_ROW_THREADS == R.T
    assert {(3, R.T - 1), (2, R.T), (3, R.T + 1), (33, 2 * R.T + 1), (1, 1), (1, 2), (2, 2), (5, 1), (1, 65), (17, 63), (16, 64)} == set(R.SIZES)
    assert max(h * w for h, w in R.SIZES) < 2 * 10 ** 4


@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("pattern", sorted(R.PATTERNS))
def test_the_numpy_restatement_equals_the_judge(pattern, masked):
    for size in R.SIZES:
        m, k, want_o, want_d, want_n = R.want(pattern, size, masked)
        out, dist2, counts = lf.fill_numpy(m, R.NC, mask=k)
        assert out.dtype == np.uint8 and dist2.dtype == np.int32
        assert np.array_equal(out, want_o) and np.array_equal(dist2, want_d), (pattern, size)
        assert counts.tolist() == want_n.tolist(), (pattern, size, counts, want_n)
        hole = (m == 255) if k is None else (m == 255) & (k != 255)
        assert counts[0] == hole.sum() and counts[1] == (hole & (out != 255)).sum() and np.array_equal(out[~hole], m[~hole])
        assert counts[2] == (dist2[hole].max() if counts[1] else 0)


@pytest.mark.parametrize("radius", [1, 2, 5, "inf"])
@pytest.mark.parametrize("pattern", sorted(R.PATTERNS))
def test_the_numpy_restatement_within_a_radius(pattern, radius):
    for size in R.SIZES:
        m, _, want_o, want_d, want_n = R.want(pattern, size, False, None if radius == "inf" else radius * radius)
        out, dist2, counts = lf.fill_numpy(m, R.NC, radius=radius)
        assert np.array_equal(out, want_o) and np.array_equal(dist2, want_d) and counts.tolist() == want_n.tolist(), (pattern, size, radius)


def test_what_the_patterns_are_for():
    big = (33, 2 * R.T + 1)
    assert 0.25 < (R.random21(*big) == 255).mean() < 0.35
    assert 0 < (R.sparse_seeds(*big) < R.NC).mean() < 0.02
    assert (R.no_seed(*big) == 255).all() and (R.no_hole(*big) < R.NC).all()
    assert (R.one_seed_corner(*big) < R.NC).sum() == 1
    assert set(np.nonzero(R.seeds_in_one_column(*big) < R.NC)[1]) == {big[1] // 2}
    assert set(np.nonzero(R.seeds_in_one_row(*big) < R.NC)[0]) == {big[0] // 2}
    m = R.passthrough(*big)
    out, dist2, _ = R.fill(m)
    assert (m == 200).sum() > 0 and (out[m == 200] == 200).all() and (dist2[m == 200] == -1).all() and (out[m == 255] < R.NC).all()
    # a 200 directly between a hole and its nearest seed does not block
    m = np.asarray([[255, 200, 4]], np.uint8)
    assert R.fill(m)[0].tolist() == [[4, 200, 4]] and lf.fill_numpy(m, R.NC)[0].tolist() == [[4, 200, 4]]


def test_ties_go_to_the_first_seed_in_raster_order():
    names = []
    for name, m, (y, x), value, d2 in R.tie_cases():
        for who, (out, dist2, _) in (("judge", R.fill(m)), ("numpy", lf.fill_numpy(m, R.NC))):
            assert int(out[y, x]) == value and int(dist2[y, x]) == d2, (name, who, int(out[y, x]), int(dist2[y, x]))
        names.append(name)
    assert names == ["row", "column", "row_against_column", "column_against_row"]


def test_the_radius_includes_its_edge():
    m = np.full((6, 6), 255, np.uint8)
    m[0, 0] = 9
    out, dist2, counts = lf.fill_numpy(m, R.NC, radius=5)
    assert out[3, 4] == 9 and dist2[3, 4] == 25 and out[4, 4] == 255 and dist2[4, 4] == -1
    want_o, want_d, want_n = R.fill(m, max_dist2=25)
    assert np.array_equal(out, want_o) and np.array_equal(dist2, want_d) and counts.tolist() == want_n.tolist() and counts[2] == 25
    assert lf.radius_rule(None) == lf.radius_rule("inf") == 2 ** 31 - 1 and lf.radius_rule(5) == 25 and lf.radius_rule(np.int64(1)) == 1
    assert lf.radius_rule(10 ** 6) == 2 ** 31 - 1
    for bad in (0, -1, 2.5, 5.0, True, "5", "far", float("inf"), [3]):
        with pytest.raises(ValueError, match="fill_ignore"):
            lf.radius_rule(bad)
    for bad in (np.zeros((0, 3), np.uint8), np.zeros(5, np.uint8)):
        with pytest.raises(ValueError, match="non-empty"):
            lf.fill_numpy(bad, R.NC)
    with pytest.raises(ValueError, match=r"outside \[1, 255\]"):
        lf.fill_numpy(m, 256)
    with pytest.raises(ValueError, match="the mask is"):
        lf.fill_numpy(m, R.NC, mask=m[:3])


def test_the_report_helpers():
    rows = np.asarray([[10, 8, 25], [0, 0, 0], [-1, -1, -1], [4, 4, 2]])
    stats = lf.fill_stats(rows)
    assert stats == dict(images=3, holes=14, filled=12, max_dist2=25)
    line = lf.format_fill_summary(stats, 0.99)
    assert "\n" not in line and "holes: 14" in line and "filled: 12" in line and "5.00 px" in line and "99.000 %" in line
    assert "coverage" not in lf.format_fill_summary(stats)
    assert lf.fill_json(None, stats)["radius"] == "inf" and lf.fill_json(3, stats, dict(miou=0.5, pAcc=0.75), 0.9) == dict(
        radius=3, images=3, holes=14, filled=12, max_dist2=25, max_dist=5.0, miou=0.5, pAcc=0.75, coverage=0.9)
    assert lf.fill_stats(np.zeros((0, 3)))["max_dist2"] == 0


# ------------------------------------------------------------------ the C ABI
def test_header_and_ctypes_agree_and_no_size_query_exists():
    import ctypes as C
    from excel_amd import _lib, build
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "excel_hip.h")).read(), flags=re.S)
    name = "excel_fill_nearest_label"
    m = re.search(r"\bint\s+" + name + r"\s*\((.*?)\)\s*;", src, flags=re.S)
    assert m, f"{name} is not declared in include/excel_hip.h"
    params = [" ".join(p.split()) for p in m.group(1).split(",")]
    res, argtypes = _lib.SIGNATURES[name]
    assert res is C.c_int and len(argtypes) == len(params) == 13, (len(argtypes), params)
    for p, t in zip(params, argtypes):
        if "excel_ragged_info" in p:
            assert t is C.POINTER(_lib.RaggedInfo), p
        elif "*" in p:
            assert re.match(r"(const )?(uint8_t|int32_t|void)\* ?\w+$", p) and t is C.c_void_p, p
        else:
            assert p.startswith("int ") and t is C.c_int, p
    assert [p.split()[-1].lstrip("*") for p in params] == ["labels", "mask", "B", "H", "W", "table", "info", "num_classes", "max_dist2", "out", "dist2",
                                                           "counts", "stream"]
    names = set(re.findall(r"\b(excel_[a-z0-9_]+)\s*\(", src)) | set(_lib.SIGNATURES)
    assert not [n for n in names if "fill" in n and "workspace_bytes" in n]
    if os.path.exists(_lib.LIB_PATH):
        handle = C.CDLL(_lib.LIB_PATH)
        assert hasattr(handle, name) and not hasattr(handle, name + "_workspace_bytes")
    assert "fill.hip" in build.SOURCES and "fill.hip" not in build.SPLIT_SOURCES and build.NO_SCRATCH_EXPECTED["fill"] in ("fill_col_kernel", "fill_row_kernel")
    assert "fill_col_kernel" in build.NO_SCRATCH and "fill_row_kernel" in build.NO_SCRATCH
    text = open(os.path.join(ROOT, "excel_amd", "csrc", "fill.hip")).read()
    assert re.search(r"#define FILL_ROW_THREADS\s+%d\b" % lf.FILL_ROW_THREADS, text) and re.search(r"#define FILL_MAX_SIDE\s+%d\b" % lf.FILL_MAX_SIDE, text)


# ------------------------------------------------------------------ flags and refusals, before anything is built
def test_infer_lam_flags_and_refusals():
    from excel_amd.tools import infer_lam
    parse = infer_lam.get_parser().parse_args
    off = parse([])
    assert off.fill_ignore is None and off.fill_label_dir is None and lf.resolve(off) is None
    assert lf.resolve(parse(["--clean_min_region", "8", "--fill_ignore", "inf"])) == dict(radius=None, label_dir=None)
    assert lf.resolve(parse(["--clean_min_region", "8", "--fill_ignore", "3", "--fill_label_dir", "d"])) == dict(radius=3, label_dir="d")
    for argv, word in ((["--fill_label_dir", "d"], "needs --fill_ignore"),
                       (["--clean_min_region", "8", "--fill_ignore", "0"], "--fill_ignore"), (["--clean_min_region", "8", "--fill_ignore", "-2"], "--fill_ignore"),
                       (["--clean_min_region", "8", "--fill_ignore", "2.5"], "--fill_ignore"), (["--clean_min_region", "8", "--fill_ignore", "far"], "--fill_ignore"),
                       (["--fill_ignore", "inf"], "needs --clean_min_region"),
                       (["--clean_min_region", "8", "--fill_ignore", "inf", "--unlabeled", "true", "--clean_label_dir", "c"], "give --fill_label_dir")):
        with pytest.raises(ValueError, match=word):
            lf.resolve(parse(argv))
        with pytest.raises(ValueError, match=word):                 # validate refuses it before it builds a model or touches a device
            infer_lam.validate(parse(argv + ["--synthetic", "2"]))
    api = parse(["--fill_ignore", "inf", "--api_path", "true"])
    api.clean_min_region = "8"                                      # (the cleaning refuses the pair itself; the fill's own refusal stands behind it)
    with pytest.raises(ValueError, match="--fill_ignore runs on the batched loop"):
        lf.resolve(api)
    with pytest.raises(ValueError, match="--api_path true"):
        infer_lam.validate(parse(["--clean_min_region", "8", "--fill_ignore", "inf", "--api_path", "true", "--synthetic", "2"]))
    ok = parse(["--clean_min_region", "8", "--fill_ignore", "inf", "--unlabeled", "true", "--clean_label_dir", "c", "--fill_label_dir", "d"])
    assert lf.resolve(ok)["label_dir"] == "d"
    doc = infer_lam.__doc__
    assert "--fill_ignore" in doc and "--fill_label_dir" in doc


def test_eval_labels_flags_and_refusals():
    from excel_amd.tools import eval_labels
    base = ["--pred_dir", "p", "--data_folder", "d", "--list_folder", "l"]
    parse = eval_labels.get_parser().parse_args
    assert lf.resolve(parse(base), program="eval_labels") is None
    assert lf.resolve(parse(base + ["--fill_ignore", "inf"]), program="eval_labels") == dict(radius=None, label_dir=None)      # no cleaning needed here
    assert lf.resolve(parse(base + ["--fill_ignore", "7", "--fill_label_dir", "x"]), program="eval_labels") == dict(radius=7, label_dir="x")
    for argv, word in ((["--fill_ignore", "0"], "--fill_ignore"), (["--fill_ignore", "1.5"], "--fill_ignore"), (["--fill_ignore", "near"], "--fill_ignore"),
                       (["--fill_label_dir", "x"], "needs --fill_ignore")):
        with pytest.raises(ValueError, match=word):
            eval_labels.validate(parse(base + argv))                 # before the list file is opened


def test_the_pipelines_check_the_option():
    import inspect
    from excel_amd import pipeline
    clean = dict(min_region=3, connectivity=8)
    assert pipeline._check_fill(None, None) is None and pipeline._check_fill(None, clean) is None
    assert pipeline._check_fill(dict(radius=None), clean) == dict(radius=None) and pipeline._check_fill(dict(), clean) == dict(radius=None)
    assert pipeline._check_fill(dict(radius="inf"), clean) == dict(radius=None) and pipeline._check_fill(dict(radius=4), clean) == dict(radius=4)
    for bad in (dict(radius=0), dict(radius=1.5), dict(radius=3, mask=1), 3):
        with pytest.raises(ValueError):
            pipeline._check_fill(bad, clean)
    with pytest.raises(ValueError, match="fill needs clean"):
        pipeline._check_fill(dict(radius=None), None)
    for cls in (pipeline.TrainingFreePipeline, pipeline.OptimisedLamPipeline, pipeline.ValidationPipeline):
        assert inspect.signature(cls.__init__).parameters["fill"].default is None


# ------------------------------------------------------------------ eval_labels end to end on the CPU
def _hist(g, p, nc=21):
    g, p = g.reshape(-1).astype(np.int64), p.reshape(-1).astype(np.int64)
    m = (g < nc) & (p < nc)
    return np.bincount(nc * g[m] + p[m], minlength=nc * nc).reshape(nc, nc)


def test_eval_labels_fills_scores_and_writes(tmp_path, monkeypatch, caplog):
    import logging
    from PIL import Image
    from excel_amd.tools import eval_labels
    from excel_amd.utils import components as cc
    from excel_amd.utils.evaluate import scores_from_hist
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)   # the numpy path, whatever the machine
    root, lists, preds = tmp_path / "VOC", tmp_path / "lists", tmp_path / "pred"
    (root / "SegmentationClassAug").mkdir(parents=True)
    lists.mkdir()
    preds.mkdir()
    names, maps, gts = [], [], []
    for i, (h, w) in enumerate([(9, 13), (20, 31), (17, 66)]):
        rs = np.random.RandomState(90 + i)
        n = f"im{i}"
        y, x = np.mgrid[:h, :w]
        pred = (1 + (x * 3 // w) + 3 * (y * 2 // h)).astype(np.uint8)                 # six blocks of classes
        sp = rs.rand(h, w) < 0.08
        pred[sp] = rs.randint(0, 21, int(sp.sum())).astype(np.uint8)                  # speckle for the cleaning to remove
        pred[rs.rand(h, w) < 0.05] = 255                                             # ignore pixels the predictions already have
        gt = (1 + (x * 3 // w) + 3 * (y * 2 // h)).astype(np.uint8)
        gt[rs.rand(h, w) < 0.05] = 255
        Image.fromarray(pred).save(preds / f"{n}.png")
        Image.fromarray(gt).save(root / "SegmentationClassAug" / f"{n}.png")
        names.append(n), maps.append(pred), gts.append(gt)
    (lists / "val.txt").write_text("\n".join(names) + "\n")
    base = ["--pred_dir", str(preds), "--data_folder", str(root), "--list_folder", str(lists), "--infer_set", "val", "--num_workers", "2",
            "--batch_size", "2"]
    parse = eval_labels.get_parser().parse_args
    plain = eval_labels.validate(parse(base))
    assert "fill" not in plain and "clean" not in plain
    only_clean = eval_labels.validate(parse(base + ["--clean_min_region", "3"]))
    assert "fill" not in only_clean
    # without the cleaning: every 255 of the predictions is a hole
    with caplog.at_level(logging.INFO):
        out = eval_labels.validate(parse(base + ["--fill_ignore", "inf", "--fill_label_dir", str(tmp_path / "f1")]))
    assert np.array_equal(out["hist"].numpy(), plain["hist"].numpy()) and "clean" not in out, "the first table is unchanged"
    hist, rows = np.zeros((21, 21), np.int64), []
    for n, m, g in zip(names, maps, gts):
        want, _, cnt = R.fill(m, 21)
        got = Image.open(tmp_path / "f1" / f"{n}.png")
        assert got.mode == "P" and np.array_equal(np.asarray(got), want) and (want != 255).all(), n
        hist += _hist(g, want)
        rows.append(cnt.tolist())
    f = out["fill"]
    assert np.array_equal(f["hist"].numpy(), hist) and f["counts"].tolist() == rows and f["radius"] is None
    assert f["score"]["miou"] == scores_from_hist(torch.from_numpy(hist))["miou"] and f["stats"] == lf.fill_stats(np.asarray(rows))
    assert f["coverage"] == hist.sum() / plain["hist"].numpy().sum() > 1, "every ignore pixel of the predictions is labelled now"
    assert "fill_label_score of" in caplog.text and lf.format_fill_summary(f["stats"], f["coverage"]) in caplog.text
    # behind the cleaning, within a radius: only what the cleaning removed, the predictions' own 255 stay
    out = eval_labels.validate(parse(base + ["--clean_min_region", "3", "--clean_connectivity", "4", "--fill_ignore", "2", "--fill_label_dir", str(tmp_path / "f2"),
                                             "--clean_label_dir", str(tmp_path / "c2")]))
    hist, rows = np.zeros((21, 21), np.int64), []
    for n, m, g in zip(names, maps, gts):
        cleaned = cc.clean_numpy(m, 3, 21, 4)[0]
        assert np.array_equal(np.asarray(Image.open(tmp_path / "c2" / f"{n}.png")), cleaned)
        want, _, cnt = R.fill(cleaned, 21, mask=m, max_dist2=4)
        assert np.array_equal(np.asarray(Image.open(tmp_path / "f2" / f"{n}.png")), want), n
        assert (want[m == 255] == 255).all() and cnt[0] == ((cleaned == 255) & (m != 255)).sum()
        hist += _hist(g, want)
        rows.append(cnt.tolist())
    f = out["fill"]
    assert np.array_equal(f["hist"].numpy(), hist) and f["counts"].tolist() == rows and f["radius"] == 2 and sum(r[1] for r in rows) > 0
    assert out["clean"]["coverage"] <= f["coverage"] <= 1
