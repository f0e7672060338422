"""utils/label_stages.py, the one table of the label stages (snap, clean, fill, margin): that it agrees with what it describes - the
score sets, the programs' flags, the pipelines' keywords - and that infer_lam and eval_labels, with every stage on at once, write what
the stages' judges (tests/_snap_ref.py, _components_ref.py, _fill_ref.py) say, in the orders the table states.  No GPU: infer_lam runs
a stub pipeline on CPU tensors (the pattern of test_host_components.py), eval_labels its numpy path.

`validate.last_<name>` of the all-stages run is compared with a run of that stage's flags plus those of the stages in front of it in
the chain (snap for clean; snap and clean for fill): a stage works on the maps of the one in front of it, so a run without that one
cleans or fills other maps."""
import ast
import csv
import inspect
import json
import logging
import os
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _components_ref as RC  # noqa: E402
import _fill_ref as RF  # noqa: E402
import _snap_ref as RS  # noqa: E402
from test_host_components import _Capture, _hist, _Ticket, _TinyRaggedSet  # noqa: E402

from excel_amd.utils import components as cc  # noqa: E402
from excel_amd.utils import label_fill as lf  # noqa: E402
from excel_amd.utils import label_stages as ls  # noqa: E402
from excel_amd.utils import margin as mg  # noqa: E402
from excel_amd.utils import superpixels as sx  # noqa: E402

NC = 21
SNAP = dict(step=4, compactness=10, iters=5, min_share=0.0)
CLEAN = dict(min_region=3, connectivity=4)
FILL = dict(radius=2)
MARGIN_MIN = 0.4
FLAGS = {"snap": ["--snap_superpixels", "4"], "clean": ["--clean_min_region", "3", "--clean_connectivity", "4"], "fill": ["--fill_ignore", "2"],
         "margin": ["--margin_min", "0.4"]}
IN_FRONT = {"snap": (), "clean": ("snap",), "fill": ("snap", "clean"), "margin": ()}     # what a stage's input depends on


# ------------------------------------------------------------------ the table against what it describes
def test_the_table_agrees_with_the_sets_the_flags_and_the_pipelines():
    from excel_amd import pipeline
    from excel_amd.tools import eval_labels, infer_lam
    from excel_amd.utils import image_scores
    assert set(ls.STAGES) == {"snap", "clean", "fill", "margin"} and all(s.name == name for name, s in ls.STAGES.items())
    flags_lam = {o for a in infer_lam.get_parser()._actions for o in a.option_strings}
    flags_eval = {o for a in eval_labels.get_parser()._actions for o in a.option_strings}
    for name, stage in ls.STAGES.items():
        assert name in image_scores.SETS and name in image_scores.BOUNDARY_SET_NAMES
        flags = {stage.flag, f"--{name}_label_dir"}
        assert stage.flag.startswith(f"--{name}_") and flags <= flags_lam
        assert flags <= flags_eval or name == "margin"
        for cls in (pipeline.TrainingFreePipeline, pipeline.OptimisedLamPipeline, pipeline.ValidationPipeline):
            assert inspect.signature(cls.__init__).parameters[stage.kwarg].default is None
    assert ls.STAGES["margin"].rows is None
    with_rows = sorted(name for name, s in ls.STAGES.items() if s.rows is not None)
    for order, covers in ((ls.CHAIN_ORDER, with_rows), (ls.ROW_SET_ORDER, with_rows), (ls.EVAL_LABELS_ORDER, with_rows),
                          (ls.INFER_LAM_ORDER, sorted(ls.STAGES)), (ls.INFER_LAM_JSON_ORDER, sorted(ls.STAGES))):
        assert sorted(order) == covers, order
    assert ls.INFER_LAM_ORDER == ("clean", "fill", "snap", "margin")         # the order in which the ranks gather
    assert [r.key for r in ls.ROW_SETS] == ["regions", "fills", "snaps"] and all(len(r.heads) == 3 for r in ls.ROW_SETS)
    for mod in (ls, cc, lf, mg, sx):                                          # the table is host only: nothing it loads imports torch
        top = [n for n in ast.parse(inspect.getsource(mod)).body if isinstance(n, (ast.Import, ast.ImportFrom))]
        loaded = [a.name for n in top if isinstance(n, ast.Import) for a in n.names] + [n.module or "" for n in top if isinstance(n, ast.ImportFrom)]
        assert not any(m.split(".")[0] == "torch" for m in loaded), mod.__name__


# ------------------------------------------------------------------ infer_lam: a stub pipeline with every stage, on CPU tensors
def _margin_of(img):
    """The stub's arg-max margin of every pixel: the image's second channel over 255."""
    return img[..., 1].astype(np.float64) / 255.0


class _StubPipe:
    """Stands in for TrainingFreePipeline: labels = the images' first channel.  With the options it is built with it runs the stages'
    numpy restatements in the chain's order and leaves what the real step leaves: last_<name>_labels, last_<name>_counts, hist_<name>
    and the stage's set in the step's ticket."""
    device, smax, image_scores, boundary, guard = "cpu", 2, True, None, None
    margin_sweep = margin_totals = margin_kept = None

    def __init__(self, snap=None, clean=None, fill=None, margin_min=None):
        self.snap, self.clean, self.fill, self.margin_min, self.hist = snap, clean, fill, margin_min, None

    def run_batch_ragged(self, images, plan, cls, gts, S=448, return_intermediates=False):
        from excel_amd.utils.image_scores import counts_numpy
        g, maps, rows = gts.numpy(), {}, {}
        for b in range(plan.B):
            h, w = (int(x) for x in plan.hw[b])
            img = images[3 * int(plan.loff[b]):3 * int(plan.loff[b + 1])].view(h, w, 3).numpy()
            chain = main = np.ascontiguousarray(img[..., 0])
            done = {"main": (main, None)}
            if self.snap is not None:
                _, _, chain, n = sx.snap_batch_numpy([img], [chain], self.snap["step"], NC, self.snap["compactness"], self.snap["iters"],
                                                     self.snap["min_share"])[0]
                done["snap"] = (chain, n)
            if self.clean is not None:
                snapped = chain
                chain, n = cc.clean_numpy(chain, cc.min_area_rule(self.clean["min_region"], h, w), NC, self.clean["connectivity"])
                done["clean"] = (chain, n)
                if self.fill is not None:
                    filled, _, n = lf.fill_numpy(chain, NC, mask=snapped, radius=self.fill["radius"])
                    done["fill"] = (filled, n)
            if self.margin_min is not None:
                done["margin"] = (np.where(_margin_of(img) >= self.margin_min, main, 255).astype(np.uint8), None)
            for name, (m, n) in done.items():
                maps.setdefault(name, []).append(m.reshape(-1))
                rows.setdefault(name, []).append(n)
        parts = {}
        for name, flat in maps.items():
            flat = np.concatenate(flat)
            into = "hist" if name == "main" else "hist_" + name
            setattr(self, into, getattr(self, into) + torch.from_numpy(_hist(g, flat)))
            parts[name] = np.stack([counts_numpy(g[int(plan.loff[b]):int(plan.loff[b + 1])], flat[int(plan.loff[b]):int(plan.loff[b + 1])], NC)
                                    for b in range(plan.B)])
            if name != "main":
                setattr(self, f"last_{name}_labels", torch.from_numpy(flat))
                if rows[name][0] is not None:
                    setattr(self, f"last_{name}_counts", torch.from_numpy(np.stack(rows[name]).astype(np.int32)))
        self.last_score_ticket = _Ticket(parts)
        return torch.from_numpy(np.concatenate(maps["main"]))


class _HostSaver:
    """Stands in for infer_lam._LabelSaver, whose PNG encoder runs on the device: the same entry, the files written on the host."""

    def __init__(self, args, directory=None):
        self.dir = directory
        os.makedirs(self.dir, exist_ok=True)

    def ragged(self, names, plan, labels_flat):
        from excel_amd.tools.eval_labels import _save_index_png
        for b, n in enumerate(names):
            h, w = (int(x) for x in plan.hw[b])
            _save_index_png(os.path.join(self.dir, str(n) + ".png"), labels_flat[int(plan.loff[b]):int(plan.loff[b + 1])].view(h, w).numpy())

    def barrier(self):
        pass

    close = barrier


def run_infer_lam(tmp_path, tag, on):
    """infer_lam.validate over 10 images at batch 4 with the stages `on`, a label directory for each -> what it left"""
    from excel_amd.tools import infer_lam
    js, table = str(tmp_path / f"{tag}.json"), str(tmp_path / f"{tag}.csv")
    argv = ["--batch_size", "4", "--num_workers", "0", "--json_out", js, "--per_image_scores", table]
    for name in on:
        argv += FLAGS[name] + [f"--{name}_label_dir", str(tmp_path / f"{tag}_{name}")]
    pipe = _StubPipe(**{"snap": SNAP if "snap" in on else None, "clean": CLEAN if "clean" in on else None, "fill": FILL if "fill" in on else None,
                        "margin_min": MARGIN_MIN if "margin" in on else None})
    cap, root = _Capture(), logging.getLogger()
    root.addHandler(cap)
    level, saver = root.level, infer_lam._LabelSaver
    root.setLevel(logging.INFO)
    infer_lam._LabelSaver = _HostSaver
    try:
        infer_lam.validate(infer_lam.get_parser().parse_args(argv), dataset=_TinyRaggedSet(10), pipe=pipe)
    finally:
        infer_lam._LabelSaver = saver
        root.removeHandler(cap)
        root.setLevel(level)
    with open(js) as f:
        record = json.load(f)
    with open(table) as f:
        rows = list(csv.reader(f))
    return dict(dir=tmp_path, tag=tag, record=record, rows=rows, log=cap.lines, npz=dict(np.load(table + ".npz")), last={name: getattr(infer_lam.validate, "last_" + name) for name in ls.STAGES})


def _same(a, b):
    if isinstance(a, dict):
        return isinstance(b, dict) and sorted(a) == sorted(b) and all(_same(a[k], b[k]) for k in a)
    if isinstance(a, (list, tuple)):
        return isinstance(b, (list, tuple)) and len(a) == len(b) and all(_same(x, y) for x, y in zip(a, b))
    if torch.is_tensor(a):
        return torch.is_tensor(b) and torch.equal(a, b)
    if isinstance(a, (np.ndarray, float, np.floating)):
        return type(a) is type(b) and np.array_equal(np.asarray(a), np.asarray(b), equal_nan=True)
    return type(a) is type(b) and a == b


@pytest.fixture(scope="module")
def all_on(tmp_path_factory):
    return run_infer_lam(tmp_path_factory.mktemp("stages"), "all", ("snap", "clean", "fill", "margin"))


def test_infer_lam_with_every_stage_writes_what_the_judges_say(all_on):
    from PIL import Image
    from excel_amd.tools import infer_lam
    from excel_amd.utils import image_scores
    from excel_amd.utils.evaluate import scores_from_hist
    head = all_on["rows"][0]
    sets = [s for s in image_scores.SETS if s in ("clean", "fill", "snap", "margin")]
    tail = [f"{s}_{k}" for s in sets for k in ("pacc", "miou", "scored")] + ["regions", "regions_removed", "pixels_removed", "holes", "filled",
                                                                             "max_fill_dist", "superpixels", "snapped", "pixels_changed"]
    assert head[-len(tail):] == tail and head[-len(tail) - 1].startswith("iou_")
    assert {"regions", "fills", "snaps"} <= set(all_on["npz"]) and all("counts_" + s in all_on["npz"] for s in sets)
    # the judges, image by image, in the chain's order
    ds = _TinyRaggedSet(10)
    hists = {name: np.zeros((NC, NC), np.int64) for name in ("main",) + tuple(ls.STAGES)}
    rows = {"snap": [], "clean": [], "fill": []}
    for i in range(10):
        _, img, gt, _ = ds[i]
        main = img[..., 0]
        sp, _, _ = RS.slic(img, SNAP["step"], SNAP["compactness"], SNAP["iters"])
        snapped, n_snap = RS.snap(main, sp, NC, 0)
        cleaned, n_clean = RC.clean(snapped, CLEAN["min_region"], NC, CLEAN["connectivity"])
        filled, _, n_fill = RF.fill(cleaned, NC, mask=snapped, max_dist2=FILL["radius"] ** 2)
        cut = np.where(_margin_of(img) >= MARGIN_MIN, main, 255)
        for name, m in (("main", main), ("snap", snapped), ("clean", cleaned), ("fill", filled), ("margin", cut)):
            hists[name] += _hist(gt.reshape(-1), np.asarray(m).reshape(-1))
            if name != "main":
                got = Image.open(all_on["dir"] / f"{all_on['tag']}_{name}" / f"s{i:03d}.png")
                assert got.mode == "P" and np.array_equal(np.asarray(got), m), (name, i)
        for name, n in (("snap", n_snap), ("clean", n_clean), ("fill", n_fill)):
            rows[name].append([int(v) for v in n])
    assert sum(r[2] for r in rows["snap"]) > 0 and sum(r[2] for r in rows["clean"]) > 0 and sum(r[1] for r in rows["fill"]) > 0, "every stage does something"
    assert 0 < hists["margin"].sum() < hists["main"].sum()
    score = {name: scores_from_hist(torch.from_numpy(h)) for name, h in hists.items()}
    cover = {name: h.sum() / hists["main"].sum() for name, h in hists.items()}
    pixels = sum(ds[i][1].shape[0] * ds[i][1].shape[1] for i in range(10))
    record = all_on["record"]
    assert [k for k in record if k in ls.STAGES] == ["margin", "clean", "fill", "snap"]
    assert record["margin"] == mg.margin_min_json(MARGIN_MIN, score["margin"], cover["margin"])
    assert record["clean"] == cc.clean_json(3, 4, cc.region_stats(np.asarray(rows["clean"])), score["clean"], cover["clean"])
    assert record["fill"] == lf.fill_json(2, lf.fill_stats(np.asarray(rows["fill"])), score["fill"], cover["fill"])
    assert record["snap"] == sx.snap_json(SNAP, sx.snap_stats(np.asarray(rows["snap"]), pixels), score["snap"], cover["snap"])
    for name, key in (("clean", "regions"), ("fill", "fills"), ("snap", "snaps")):
        assert all_on["npz"][key].tolist() == rows[name] and all_on["last"][name]["counts"].tolist() == rows[name]
    assert [r[-9:-6] for r in all_on["rows"][1:]] == [[str(v) for v in r] for r in rows["clean"]]
    assert [r[-6:-3] for r in all_on["rows"][1:]] == [[str(r[0]), str(r[1]), f"{np.sqrt(r[2]):.6f}"] for r in rows["fill"]]
    assert [r[-3:] for r in all_on["rows"][1:]] == [[str(v) for v in r] for r in rows["snap"]]
    # the log: the titles in the report's order, each with its table, its summary and its directory
    titles = ["clean_label_score (--clean_min_region 3, connectivity 4):", "fill_label_score (--fill_ignore 2):",
              "snap_label_score (--snap_superpixels 4, compactness 10, 5 iterations, min share 0):", "margin_label_score (--margin_min 0.4):"]
    at = [all_on["log"].index(t) for t in titles]
    assert at == sorted(at)
    for j, (name, noun) in enumerate((("clean", "cleaned"), ("fill", "filled"), ("snap", "snapped"), ("margin", "margin"))):
        assert all_on["log"][at[j] + 1] == "\n" + infer_lam.format_scores_table(score[name], infer_lam.VOC_CLASSES)
        assert all_on["log"][at[j] + 3].startswith(f"{noun} label maps -> ")
    assert all_on["log"][at[0] + 2] == cc.format_clean_summary(cc.region_stats(np.asarray(rows["clean"])), cover["clean"])
    assert all_on["log"][at[1] + 2] == lf.format_fill_summary(lf.fill_stats(np.asarray(rows["fill"])), cover["fill"])
    assert all_on["log"][at[2] + 2] == sx.format_snap_summary(sx.snap_stats(np.asarray(rows["snap"]), pixels), cover["snap"])
    assert all_on["log"][at[3] + 2] == f"margin coverage (kept pixels over labelled pixels): {cover['margin'] * 100:.3f} %"


@pytest.mark.parametrize("name", ["snap", "clean", "fill", "margin"])
def test_a_stage_reports_the_same_with_the_others_on(tmp_path, all_on, name):
    alone = run_infer_lam(tmp_path, name, IN_FRONT[name] + (name,))
    assert alone["last"][name] is not None and _same(all_on["last"][name], alone["last"][name])
    assert all(alone["last"][other] is None for other in ls.STAGES if other not in IN_FRONT[name] + (name,))
    assert alone["record"][name] == all_on["record"][name]


# ------------------------------------------------------------------ eval_labels: the three stages at once, the numpy path
def run_eval_labels(tmp_path, monkeypatch):
    """eval_labels.validate over four images (one of them 1 x 7) with snap, clean and fill on -> (what it returned, its log, the inputs)"""
    from PIL import Image
    from excel_amd.tools import eval_labels
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)   # the numpy path, whatever the machine
    root, lists, preds = tmp_path / "VOC", tmp_path / "lists", tmp_path / "pred"
    (root / "SegmentationClassAug").mkdir(parents=True)
    (root / "JPEGImages").mkdir()
    lists.mkdir()
    preds.mkdir()
    names, maps, imgs = [], [], []
    for i, (h, w) in enumerate([(9, 13), (20, 31), (1, 7), (RC.TILE[0] + 1, RC.TILE[1] + 2)]):
        img, truth, noisy = RS.scene(h, w, seed=40 + i, shift=1, speckle=0.1)
        n = f"im{i}"
        Image.fromarray(img).save(root / "JPEGImages" / f"{n}.jpg", quality=95)
        Image.fromarray(noisy).save(preds / f"{n}.png")
        Image.fromarray(truth).save(root / "SegmentationClassAug" / f"{n}.png")
        names.append(n), maps.append(noisy)
        imgs.append(np.asarray(Image.open(root / "JPEGImages" / f"{n}.jpg").convert("RGB")))
    (lists / "val.txt").write_text("\n".join(names) + "\n")
    argv = ["--pred_dir", str(preds), "--data_folder", str(root), "--list_folder", str(lists), "--infer_set", "val", "--num_workers", "2",
            "--batch_size", "3", "--snap_superpixels", "4", "--clean_min_region", "3", "--clean_connectivity", "4", "--fill_ignore", "2"]
    for name in ("snap", "clean", "fill"):
        argv += [f"--{name}_label_dir", str(tmp_path / name)]
    cap, root_log = _Capture(), logging.getLogger()
    root_log.addHandler(cap)
    level = root_log.level
    root_log.setLevel(logging.INFO)
    try:
        out = eval_labels.validate(eval_labels.get_parser().parse_args(argv))
    finally:
        root_log.removeHandler(cap)
        root_log.setLevel(level)
    return out, cap.lines, names, maps, imgs


def test_eval_labels_with_every_stage_is_the_chain_by_hand(tmp_path, monkeypatch):
    from PIL import Image
    out, log, names, maps, imgs = run_eval_labels(tmp_path, monkeypatch)
    snapped = [d[2] for d in sx.snap_batch_numpy(imgs, maps, 4, NC, 10, 5, 0.0)]
    changed = 0
    for n, m, s in zip(names, maps, snapped):
        cleaned = cc.clean_numpy(s, 3, NC, 4)[0]
        filled = lf.fill_numpy(cleaned, NC, mask=s, radius=2)[0]
        changed += int((s != m).sum()) + int((cleaned != s).sum()) + int((filled != cleaned).sum())
        for name, want in (("snap", s), ("clean", cleaned), ("fill", filled)):
            got = Image.open(tmp_path / name / f"{n}.png")
            assert got.mode == "P" and np.array_equal(np.asarray(got), want), (name, n)
    assert changed > 0
    assert [k for k in out if k in ls.STAGES] == ["snap", "clean", "fill"]
    at = [next(i for i, line in enumerate(log) if line.startswith(f"{name}_label_score of ")) for name in ("snap", "clean", "fill")]
    assert at == sorted(at)
    assert [log[i + 3].split(" label maps -> ")[0] for i in at] == ["snapped", "cleaned", "filled"]
