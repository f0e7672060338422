"""Connected-component cleaning without a GPU: the judge of the GPU tests against scipy, the numpy restatement against the judge, the
threshold rule, the C ABI, the flags of infer_lam and eval_labels with their refusals, the shape of the log / JSON / CSV with and
without the flag (a stub pipeline on CPU tensors), and eval_labels --clean_min_region end to end on its numpy path."""
import csv
import json
import logging
import os
import re
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _components_ref as R  # noqa: E402

from excel_amd.utils import components as cc  # noqa: E402

SMALL = [(1, 1), (1, 9), (7, 1), (5, 6), (12, 17)]


# ------------------------------------------------------------------ the judge and the restatement
@pytest.mark.parametrize("connectivity", [4, 8])
def test_the_judge_agrees_with_scipy(connectivity):
    ndi = pytest.importorskip("scipy.ndimage")
    structure = np.ones((3, 3), int) if connectivity == 8 else np.asarray([[0, 1, 0], [1, 1, 1], [0, 1, 0]])
    for pattern in ("blobs", "random2", "random21", "checkerboard", "serpentine", "corner_diagonals"):
        for size in SMALL + [(R.TH + 1, R.TW + 1)]:
            m = R.PATTERNS[pattern](*size)
            comp, area = R.components(m, connectivity)
            want_c, want_a = np.zeros(m.shape, np.int64), np.zeros(m.shape, np.int64)
            lin = np.arange(m.size).reshape(m.shape)
            for v in np.unique(m):                                   # per value; the canonical root = the minimum linear index per label
                lab, n = ndi.label(m == v, structure=structure)
                for k in range(1, n + 1):
                    sel = lab == k
                    want_c[sel] = lin[sel].min()
                    want_a[sel] = sel.sum()
            assert np.array_equal(comp, want_c) and np.array_equal(area, want_a), (pattern, size, connectivity)


@pytest.mark.parametrize("connectivity", [4, 8])
def test_the_numpy_restatement_equals_the_judge(connectivity):
    for pattern in sorted(R.PATTERNS):
        for size in SMALL + [(R.TH + 1, R.TW + 1), (2 * R.TH + 3, 2 * R.TW + 5)]:
            m, comp, area = R.judged(pattern, size, connectivity)
            got_c, got_a = cc.components_numpy(m, connectivity)
            assert got_c.dtype == np.int32 and np.array_equal(got_c, comp) and np.array_equal(got_a, area), (pattern, size)
            for thr in (1, 2, 5, 10 ** 6):
                out, n = cc.clean_numpy(m, thr, 21, connectivity)
                want, want_n = R.clean(m, thr, 21, connectivity)
                assert np.array_equal(out, want) and n.tolist() == want_n.tolist(), (pattern, size, thr)
    m = R.PATTERNS["random21"](9, 11)
    out, n = cc.clean_numpy(m, 1, 21)
    assert np.array_equal(out, m) and n[1] == n[2] == 0, "min_area 1 removes nothing"
    with pytest.raises(ValueError, match="integer >= 1"):
        cc.clean_numpy(m, 0, 21)


def test_min_area_rule():
    assert cc.min_area_rule(1, 375, 500) == 1 and cc.min_area_rule(64, 375, 500) == 64 and cc.min_area_rule(64.0, 3, 3) == 64
    assert cc.min_area_rule(0.001, 375, 500) == 188                 # 187.5: Python's round goes to the even integer
    assert cc.min_area_rule(0.5, 1, 5) == 2 and cc.min_area_rule(0.5, 1, 7) == 4      # 2.5 -> 2, 3.5 -> 4
    assert cc.min_area_rule(0.001, 5, 5) == 1                       # never below one pixel
    for bad in (0, 0.0, -1, -0.5, 1.5, 64.5, float("nan"), float("inf"), "64", None, True):
        with pytest.raises(ValueError, match="clean_min_region"):
            cc.min_area_rule(bad, 375, 500)
    assert isinstance(cc.min_area_rule(0.25, 10, 10), int)


# ------------------------------------------------------------------ the C ABI
def test_header_and_ctypes_agree_and_no_size_query_exists():
    import ctypes as C
    from excel_amd import _lib
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "excel_hip.h")).read(), flags=re.S)
    for name in ("excel_label_components", "excel_filter_small_regions"):
        m = re.search(r"\bint\s+" + name + r"\s*\((.*?)\)\s*;", src, flags=re.S)
        assert m, f"{name} is not declared in include/excel_hip.h"
        params = [p.strip() for p in m.group(1).split(",")]
        res, argtypes = _lib.SIGNATURES[name]
        assert res is C.c_int and len(argtypes) == len(params), (name, len(argtypes), params)
        for p, t in zip(params, argtypes):
            if "excel_ragged_info" in p:
                assert t is C.POINTER(_lib.RaggedInfo), p
            elif "*" in p:
                assert t is C.c_void_p, p
            else:
                assert p.startswith("int ") and t is C.c_int, p
    names = set(re.findall(r"\b(excel_[a-z0-9_]+)\s*\(", src)) | set(_lib.SIGNATURES)
    bad = [n for n in names if ("components" in n or "regions" in n) and "workspace_bytes" in n]
    assert not bad, bad
    if os.path.exists(_lib.LIB_PATH):
        handle = C.CDLL(_lib.LIB_PATH)
        assert hasattr(handle, "excel_label_components") and hasattr(handle, "excel_filter_small_regions")
    assert tuple(cc.COMPONENTS_TILE) == R.TILE
    from excel_amd import build
    assert "components.hip" in build.SOURCES and build.NO_SCRATCH_EXPECTED["components"] == "cc_tile_kernel"
    for k in ("cc_tile_kernel", "cc_merge_kernel", "cc_flatten_kernel", "cc_broadcast_kernel", "cc_filter_kernel"):
        assert k in build.NO_SCRATCH


# ------------------------------------------------------------------ flags and refusals, before anything is built
def test_infer_lam_flags_and_refusals():
    from excel_amd.tools import infer_lam
    parse = infer_lam.get_parser().parse_args
    off = parse([])
    assert off.clean_min_region is None and off.clean_connectivity == 8 and off.clean_label_dir is None and cc.resolve(off) is None
    assert cc.resolve(parse(["--clean_min_region", "32"])) == dict(min_region=32, connectivity=8, label_dir=None)
    got = cc.resolve(parse(["--clean_min_region", "0.001", "--clean_connectivity", "4", "--clean_label_dir", "d"]))
    assert got == dict(min_region=0.001, connectivity=4, label_dir="d")
    for argv, word in ((["--clean_min_region", "0"], "clean_min_region"), (["--clean_min_region", "-3"], "clean_min_region"),
                       (["--clean_min_region", "1.5"], "has to be an integer"), (["--clean_min_region", "many"], "is not a number"),
                       (["--clean_min_region", "8", "--clean_connectivity", "6"], "must be 4 or 8"),
                       (["--clean_label_dir", "d"], "needs --clean_min_region"), (["--clean_connectivity", "4"], "needs --clean_min_region"),
                       (["--clean_min_region", "8", "--api_path", "true"], "--api_path true"),
                       (["--clean_min_region", "8", "--unlabeled", "true", "--save_label", "true"], "give --clean_label_dir")):
        with pytest.raises(ValueError, match=word):
            cc.resolve(parse(argv))
        with pytest.raises(ValueError, match=word):                 # validate refuses it before it builds a model or touches a device
            infer_lam.validate(parse(argv + ["--synthetic", "2"]))
    ok = parse(["--clean_min_region", "8", "--unlabeled", "true", "--clean_label_dir", "d"])
    assert cc.resolve(ok)["label_dir"] == "d"
    # uniform batches have no ragged step
    with pytest.raises(ValueError, match="runs behind the ragged step"):
        infer_lam.build_validation(args=parse(["--clean_min_region", "8", "--synthetic", "2"]), device="cpu", pipe=_StubPipe(None))


def test_eval_labels_flags_and_refusals():
    from excel_amd.tools import eval_labels
    base = ["--pred_dir", "p", "--data_folder", "d", "--list_folder", "l"]
    parse = eval_labels.get_parser().parse_args
    assert cc.resolve(parse(base), program="eval_labels") is None
    assert cc.resolve(parse(base + ["--clean_min_region", "0.01"]), program="eval_labels")["min_region"] == 0.01
    for argv, word in ((["--clean_min_region", "0"], "clean_min_region"), (["--clean_min_region", "2.5"], "has to be an integer"),
                       (["--clean_min_region", "4", "--clean_connectivity", "5"], "must be 4 or 8"),
                       (["--clean_label_dir", "x"], "needs --clean_min_region")):
        with pytest.raises(ValueError, match=word):
            eval_labels.validate(parse(base + argv))                 # before the list file is opened


def test_the_pipelines_check_and_refuse_the_option():
    from excel_amd import pipeline
    assert pipeline._check_clean(None) is None
    assert pipeline._check_clean(dict(min_region=32)) == dict(min_region=32, connectivity=8)
    assert pipeline._check_clean(dict(min_region=0.01, connectivity=4)) == dict(min_region=0.01, connectivity=4)
    for bad in (dict(), dict(min_region=0), dict(min_region=3, connectivity=6), dict(min_region=3, radius=1), 32):
        with pytest.raises(ValueError):
            pipeline._check_clean(bad)
    p = object.__new__(pipeline.TrainingFreePipeline)
    p.clean = dict(min_region=3, connectivity=8)
    for what in ("run_batch", "run_batch_split", "run_batch_overlapped"):
        with pytest.raises(ValueError, match=what + " has no label cleaning"):
            p._no_clean(what)
    import inspect
    for cls in (pipeline.TrainingFreePipeline, pipeline.OptimisedLamPipeline, pipeline.ValidationPipeline):
        assert inspect.signature(cls.__init__).parameters["clean"].default is None
    for fn in ("run_batch", "run_batch_split", "run_batch_overlapped"):
        assert f'self._no_clean("{fn}")' in inspect.getsource(getattr(pipeline.TrainingFreePipeline, fn))


# ------------------------------------------------------------------ the report: a stub pipeline on CPU tensors
class _TinyRaggedSet:
    """(name, image u8 [h,w,3], label u8 [h,w], cls f32 [20]) with a different size per sample; the image's first channel is a blob map."""
    def __init__(self, n):
        self.n = n

    def __len__(self):
        return self.n

    def max_k(self):
        return 2

    def __getitem__(self, i):
        rs = np.random.RandomState(700 + i)
        h, w = 9 + i % 7, 11 + (3 * i) % 5
        gt = R.PATTERNS["blobs"](h, w) % 21
        gt[rs.rand(h, w) < 0.1] = 255
        img = rs.randint(0, 256, (h, w, 3)).astype(np.uint8)
        img[..., 0] = R.PATTERNS["blobs"](h + 1, w)[:h] % 21
        cls = np.zeros(20, np.float32)
        cls[i % 20] = 1
        return f"s{i:03d}", img, gt, cls


class _Ticket:
    def __init__(self, parts):
        self.parts = parts

    def ready(self):
        return True

    def counts(self):
        return self.parts


class _StubPipe:
    """Stands in for TrainingFreePipeline: labels = the images' first channel; with `clean` it cleans them with clean_numpy and leaves
    what the real step leaves (last_clean_labels, last_clean_counts, hist_clean, the "clean" set of the ticket)."""
    device, smax, image_scores, boundary, guard = "cpu", 2, True, None, None

    def __init__(self, clean):
        self.clean, self.hist, self.hist_clean = clean, None, None

    def run_batch_ragged(self, images, plan, cls, gts, S=448, return_intermediates=False):
        from excel_amd.utils.image_scores import counts_numpy
        pred = images.view(-1, 3)[:, 0].contiguous().numpy()
        g = gts.numpy()
        parts, maps, rows, mains = {}, [], [], []
        for b in range(plan.B):
            h, w = (int(x) for x in plan.hw[b])
            sl = slice(int(plan.loff[b]), int(plan.loff[b + 1]))
            mains.append(counts_numpy(g[sl], pred[sl], 21))
            if self.clean is not None:
                out, n = cc.clean_numpy(pred[sl].reshape(h, w), cc.min_area_rule(self.clean["min_region"], h, w), 21, self.clean["connectivity"])
                maps.append(out.reshape(-1))
                rows.append(n)
        parts["main"] = np.stack(mains)
        self.hist += torch.from_numpy(_hist(g, pred))
        if self.clean is not None:
            cleaned = np.concatenate(maps)
            self.last_clean_labels, self.last_clean_counts = torch.from_numpy(cleaned), torch.from_numpy(np.stack(rows).astype(np.int32))
            self.hist_clean += torch.from_numpy(_hist(g, cleaned))
            parts["clean"] = np.stack([counts_numpy(g[int(plan.loff[b]):int(plan.loff[b + 1])], cleaned[int(plan.loff[b]):int(plan.loff[b + 1])], 21)
                                       for b in range(plan.B)])
        self.last_score_ticket = _Ticket(parts)
        return torch.from_numpy(pred)


def _hist(g, p, nc=21):
    g, p = g.astype(np.int64), p.astype(np.int64)
    m = (g < nc) & (p < nc)
    return np.bincount(nc * g[m] + p[m], minlength=nc * nc).reshape(nc, nc)


class _Capture(logging.Handler):
    def __init__(self):
        super().__init__(logging.INFO)
        self.lines = []

    def emit(self, record):
        self.lines.append(record.getMessage())


def _run_infer_lam(tmp_path, tag, extra, clean):
    from excel_amd.tools import infer_lam
    js, table = str(tmp_path / f"{tag}.json"), str(tmp_path / f"{tag}.csv")
    args = infer_lam.get_parser().parse_args(["--batch_size", "4", "--num_workers", "0", "--json_out", js, "--per_image_scores", table] + extra)
    cap = _Capture()
    root = logging.getLogger()
    root.addHandler(cap)
    level = root.level
    root.setLevel(logging.INFO)
    try:
        score, total = infer_lam.validate(args, dataset=_TinyRaggedSet(10), pipe=_StubPipe(clean))
    finally:
        root.removeHandler(cap)
        root.setLevel(level)
    with open(js) as f:
        record = json.load(f)
    with open(table) as f:
        rows = list(csv.reader(f))
    return dict(score=score, total=total.numpy(), record=record, rows=rows, log="\n".join(cap.lines), last=infer_lam.validate.last_clean,
                npz=dict(np.load(table + ".npz")), raw=open(table, "rb").read())


def test_the_report_with_and_without_the_flag(tmp_path):
    from excel_amd.tools import infer_lam
    from excel_amd.utils.evaluate import scores_from_hist
    off = _run_infer_lam(tmp_path, "off", [], None)
    assert off["last"] is None and "clean" not in off["record"] and "clean" not in off["log"]
    assert not any("clean" in c or "regions" in c for c in off["rows"][0]) and not any("clean" in k or "regions" in k for k in off["npz"])
    on = _run_infer_lam(tmp_path, "on", ["--clean_min_region", "4", "--clean_connectivity", "4"], dict(min_region=4, connectivity=4))
    assert np.array_equal(on["total"], off["total"]), "the flag changes no score of the plain labels"
    head = on["rows"][0]
    assert head[:len(off["rows"][0])] == off["rows"][0], "the columns of a plain table come first, unchanged"
    assert head[len(off["rows"][0]):] == ["clean_pacc", "clean_miou", "clean_scored", "regions", "regions_removed", "pixels_removed"]
    for a, b in zip(on["rows"][1:], off["rows"][1:]):
        assert a[:len(b)] == b
    # the judge, image by image
    ds, want_rows, hist_clean = _TinyRaggedSet(10), [], np.zeros((21, 21), np.int64)
    for i in range(10):
        _, img, gt, _ = ds[i]
        out, n = R.clean(img[..., 0], 4, 21, 4)
        want_rows.append(n.tolist())
        hist_clean += _hist(gt.reshape(-1), out.reshape(-1))
    last = on["last"]
    assert last["counts"].tolist() == want_rows and np.array_equal(last["hist"].numpy(), hist_clean)
    assert [[int(v) for v in r[-3:]] for r in on["rows"][1:]] == want_rows and on["npz"]["regions"].tolist() == want_rows
    assert np.array_equal(on["npz"]["counts_clean"].sum(0), np.stack([hist_clean.sum(1), hist_clean.sum(0), np.diag(hist_clean)]))
    want_score = scores_from_hist(torch.from_numpy(hist_clean))
    assert last["score"]["miou"] == want_score["miou"]
    cover = hist_clean.sum() / on["total"].sum()
    assert 0 < cover < 1 and last["coverage"] == cover
    block = on["record"]["clean"]
    stats = cc.region_stats(np.asarray(want_rows))
    assert block == cc.clean_json(4, 4, stats, want_score, cover) and block["min_region"] == 4 and block["connectivity"] == 4
    assert block["miou"] == want_score["miou"] and block["pixels_removed"] == int(np.asarray(want_rows)[:, 2].sum()) > 0
    assert "clean_label_score (--clean_min_region 4, connectivity 4):" in on["log"]
    assert infer_lam.format_scores_table(want_score, infer_lam.VOC_CLASSES) in on["log"]
    assert cc.format_clean_summary(stats, cover) in on["log"] and "clean coverage" in on["log"] and "clean regions per image" in on["log"]
    # a fraction of every image's own area
    frac = _run_infer_lam(tmp_path, "frac", ["--clean_min_region", "0.03"], dict(min_region=0.03, connectivity=8))
    want = [R.clean(ds[i][1][..., 0], cc.min_area_rule(0.03, *ds[i][1].shape[:2]), 21, 8)[1].tolist() for i in range(10)]
    assert frac["last"]["counts"].tolist() == want and frac["record"]["clean"]["min_region"] == 0.03
    # a pipeline built with another option than the flags ask for is refused
    with pytest.raises(ValueError, match="the supplied pipeline was built with clean="):
        _run_infer_lam(tmp_path, "bad", ["--clean_min_region", "5"], dict(min_region=4, connectivity=8))


# ------------------------------------------------------------------ eval_labels end to end on the CPU
def test_eval_labels_cleans_scores_and_writes(tmp_path, monkeypatch):
    from PIL import Image
    from excel_amd.tools import eval_labels
    from excel_amd.utils.evaluate import scores_from_hist
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)   # the numpy path, whatever the machine
    root, lists, preds, outd = tmp_path / "VOC", tmp_path / "lists", tmp_path / "pred", tmp_path / "clean"
    (root / "SegmentationClassAug").mkdir(parents=True)
    lists.mkdir()
    preds.mkdir()
    names, maps, gts = [], [], []
    for i, (h, w) in enumerate([(9, 13), (20, 31), (1, 7), (R.TH + 1, R.TW + 2)]):
        n = f"im{i}"
        pred = R.PATTERNS["blobs"](h, w)
        gt = R.PATTERNS["blobs"](h + 2, w)[2:].copy()
        Image.fromarray(pred).save(preds / f"{n}.png")
        Image.fromarray(gt).save(root / "SegmentationClassAug" / f"{n}.png")
        names.append(n), maps.append(pred), gts.append(gt)
    (lists / "val.txt").write_text("\n".join(names) + "\n")
    base = ["--pred_dir", str(preds), "--data_folder", str(root), "--list_folder", str(lists), "--infer_set", "val", "--num_workers", "2",
            "--batch_size", "3"]
    plain = eval_labels.validate(eval_labels.get_parser().parse_args(base))
    assert "clean" not in plain
    out = eval_labels.validate(eval_labels.get_parser().parse_args(base + ["--clean_min_region", "6", "--clean_label_dir", str(outd)]))
    assert np.array_equal(out["hist"].numpy(), plain["hist"].numpy()), "the first table is unchanged"
    hist, rows = np.zeros((21, 21), np.int64), []
    for n, m, g in zip(names, maps, gts):
        want, cnt = cc.clean_numpy(m, 6, 21, 8)
        judged, cnt2 = R.clean(m, 6, 21, 8)
        assert np.array_equal(want, judged) and cnt.tolist() == cnt2.tolist()
        got = Image.open(outd / f"{n}.png")
        assert got.mode == "P" and np.array_equal(np.asarray(got), want), n
        hist += _hist(g.reshape(-1), want.reshape(-1))
        rows.append(cnt.tolist())
    c = out["clean"]
    assert np.array_equal(c["hist"].numpy(), hist) and c["counts"].tolist() == rows
    assert c["score"]["miou"] == scores_from_hist(torch.from_numpy(hist))["miou"]
    assert c["coverage"] == hist.sum() / plain["hist"].numpy().sum() and c["stats"]["pixels_removed"] == int(np.asarray(rows)[:, 2].sum()) > 0
    # a fraction: every image its own threshold
    frac = eval_labels.validate(eval_labels.get_parser().parse_args(base + ["--clean_min_region", "0.02", "--clean_connectivity", "4"]))
    want = [cc.clean_numpy(m, cc.min_area_rule(0.02, *m.shape), 21, 4)[1].tolist() for m in maps]
    assert frac["clean"]["counts"].tolist() == want
