"""Background-scale sweep, host side (no GPU): the scales and their refusals, the numpy restatement of excel_bkg_sweep_ragged on a
hand-worked case, scores_from_totals against scores_from_hist, the registration of the kernel (header, ctypes, build lists), the flags of
infer_lam and its report through a stub pipeline."""
import json
import logging
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAN = float("nan")


# ------------------------------------------------------------------ the scales
@pytest.mark.parametrize("seq, word", [
    ([], "1..16 scales, got 0"),
    ([0.1 * (i + 1) for i in range(17)], "1..16 scales, got 17"),
    ([0.5, NAN], "scale nan"),
    ([0.5, float("inf")], "scale inf"),
    ([0.0, 1.0], "scale 0.0 must be a finite number > 0"),
    ([-1.0], "scale -1.0"),
    ([0.5, 1.0, 1.0], "scale 1.0 follows 1.0"),
    ([0.5, 2.0, 1.5], "scale 1.5 follows 2.0"),
    ([1.0, 1.0 + 1e-12], "strictly increasing"),           # equal once they are float32, which is what the kernel compares with
    ([1e-50], "outside the float32 range"),
    (["x"], "must be numbers"),
])
def test_check_scales_refusals_name_the_value(seq, word):
    from excel_amd.utils.bkg_sweep import check_scales
    with pytest.raises(ValueError, match=re.escape(word)):
        check_scales(seq)


def test_check_and_parse_scales():
    from excel_amd.utils import bkg_sweep as bs
    assert bs.check_scales([0.5, 1, 2]) == (0.5, 1.0, 2.0) and bs.check_scales(np.float32([0.25])) == (0.25,)
    assert len(bs.check_scales([0.1 * (i + 1) for i in range(16)])) == 16
    assert bs.parse_scales(None) is None and bs.parse_scales("") is None and bs.parse_scales("  ") is None
    assert bs.parse_scales("0.5,0.7, 0.85,1.0,1.2,1.5,2.0") == (0.5, 0.7, 0.85, 1.0, 1.2, 1.5, 2.0)
    with pytest.raises(ValueError, match="'a' is not a number"):
        bs.parse_scales("0.5,a")
    with pytest.raises(ValueError, match="scale 0.5 follows 1.0"):
        bs.parse_scales("1.0,0.5")
    assert bs.check_scale(2) == 2.0
    with pytest.raises(ValueError, match="scale 0.0"):
        bs.check_scale(0)


# ------------------------------------------------------------------ the numpy restatement on a hand-worked case
def _hand_case():
    """Two 2 x 3 images (row pitch 4), Cmax = 3.  Image 0 has three channels and class list [4, 9] (keys 5 and 10); image 1 has the
    background alone.  Pad columns and image 1's unused planes hold NaN."""
    b0 = [[0.5, 0.25, 1.0], [0.0, 0.5, 0.125]]
    p1 = [[0.5, 0.5, 0.25], [0.25, 0.125, 0.125]]
    p2 = [[0.25, 0.5, 0.5], [0.25, 1.0, 0.0]]
    planes = np.full((2, 3, 2, 4), NAN, np.float32)
    planes[0, :, :, :3] = np.float32([b0, p1, p2])
    planes[1, 0, :, :3] = 0.75
    gts = np.uint8([[[0, 5, 255], [5, 10, 0]], [[0, 0, 3], [255, 30, 1]]])
    return planes.reshape(-1), [(2, 3), (2, 3)], np.int32([3, 1]), np.int32([[4, 9], [7, 7]]), gts.reshape(-1)


def test_sweep_reference_on_a_hand_worked_image():
    """F = [[.5,.5,.5],[.25,1,.125]], first maximum ci = [[1,1,2],[1,2,1]] (two ties between the planes), keys [[5,5,10],[5,10,5]].
    a = 0.5: only (0,2) is background, by the tie .5 >= .5;  a = 1: (0,0), (0,2), (1,2) - two ties;  a = 2: all but (1,0), whose b0 is 0.
    gt 255 at (0,2) of image 0 and (1,0) of image 1, gt 30 >= nc at (1,1) of image 1: three pixels never count."""
    from excel_amd.utils.bkg_sweep import sweep_reference
    planes, hw, nchan, cls_idx, gts = _hand_case()
    nc = 21
    totals, labels = sweep_reference(planes, hw, 3, (0.5, 1.0, 2.0), nchan=nchan, cls_idx=cls_idx, gts=gts, num_classes=nc, label_sel=1)
    assert labels.dtype == np.uint8 and labels.tolist() == [0, 5, 0, 5, 10, 0] + [0] * 6
    want = np.zeros((3, 3, nc), np.int64)
    want[:, 0, [0, 5, 10]] = [2, 2, 1]                               # image 0's ground truth, the same at every scale
    want[0, 1, [5, 10]], want[0, 2, [5, 10]] = [4, 1], [2, 1]
    want[1, 1, [0, 5, 10]], want[1, 2, [0, 5, 10]] = [2, 2, 1], [2, 2, 1]
    want[2, 1, [0, 5]], want[2, 2, [0, 5]] = [4, 1], [2, 1]
    want[:, 0, [0, 3, 1]] += [2, 1, 1]                               # image 1: background alone, four counted pixels
    want[:, 1, 0] += 4
    want[:, 2, 0] += 2
    assert np.array_equal(totals, want)
    for sel, lab0 in ((0, [5, 5, 0, 5, 10, 5]), (2, [0, 0, 0, 5, 0, 0])):
        assert sweep_reference(planes, hw, 3, (0.5, 1.0, 2.0), nchan=nchan, cls_idx=cls_idx, label_sel=sel)[1].tolist() == lab0 + [0] * 6
    # without a class list the key is the plane index; skip drops an image; totals are added to
    t2, lab = sweep_reference(planes, hw, 3, (1.0,), nchan=nchan, gts=gts, num_classes=nc, skip=[0, 9], totals=want[1:2], label_sel=0)
    assert lab.tolist() == [0, 1, 0, 1, 2, 0] + [0] * 6
    only0 = np.zeros((1, 3, nc), np.int64)
    only0[0, 0, [0, 5, 10]] = [2, 2, 1]
    only0[0, 1, [0, 1, 2]] = [2, 2, 1]
    only0[0, 2, 0] = 2
    assert np.array_equal(t2, want[1:2] + only0)
    assert sweep_reference(planes, hw, 3, (1.0,), nchan=nchan, label_sel=0)[0] is None
    assert sweep_reference(planes, hw, 3, (1.0,), nchan=nchan, gts=gts, num_classes=nc)[1] is None


def _random_batch(rs, sizes, Cmax, nc, grid=8):
    """Planes on a coarse grid (multiples of 1/grid in [0, 2]) so that exact ties are frequent; pad columns NaN."""
    planes, gts = [], []
    for h, w in sizes:
        wp = (w + 3) // 4 * 4
        p = np.full((Cmax, h, wp), NAN, np.float32)
        p[:, :, :w] = rs.randint(0, 2 * grid + 1, (Cmax, h, w)).astype(np.float32) / grid
        planes.append(p.reshape(-1))
        gts.append(rs.randint(0, nc, h * w).astype(np.uint8))
    return np.concatenate(planes), np.concatenate(gts)


def test_background_area_is_monotone_in_the_scale_on_non_negative_planes():
    from excel_amd.utils.bkg_sweep import sweep_reference
    rs = np.random.RandomState(3)
    sizes = [(9, 13), (5, 4), (1, 1)]
    planes, gts = _random_batch(rs, sizes, 5, 21)
    scales = (0.25, 0.5, 0.75, 1.0, 1.5, 2.0, 4.0, 8.0)
    totals, _ = sweep_reference(planes, sizes, 5, scales, nchan=np.int32([5, 3, 2]), gts=gts, num_classes=21)
    bkg = totals[:, 1, 0]
    assert (np.diff(bkg) >= 0).all() and bkg[0] < bkg[-1]
    assert (totals[:, 0] == totals[0, 0]).all() and (totals[:, 1].sum(1) == totals[0, 0].sum()).all()      # every pixel counts at every scale
    fg = totals[:, 1, 1:].sum(1)
    assert (np.diff(fg) <= 0).all()


@pytest.mark.parametrize("nc", [21, 81])
def test_scores_from_totals_equal_scores_from_hist(nc):
    """Random label pairs, some classes absent from the ground truth, some never predicted: every key of scores_from_hist, NaNs included."""
    from excel_amd.utils.bkg_sweep import scores_from_totals
    from excel_amd.utils.evaluate import scores_from_hist
    rs = np.random.RandomState(nc)
    hists = []
    for _ in range(3):
        present, predicted = rs.permutation(nc)[:nc // 2 + 1], rs.permutation(nc)[:nc // 2 + 3]
        g, p = present[rs.randint(0, len(present), 20000)], predicted[rs.randint(0, len(predicted), 20000)]
        p = np.where(rs.rand(20000) < 0.6, g, p)
        hists.append(np.bincount(nc * g + p, minlength=nc * nc).reshape(nc, nc))
    totals = np.stack([np.stack([h.sum(1), h.sum(0), np.diag(h)]) for h in hists])
    got = scores_from_totals(totals)
    assert len(got) == 3
    for h, s in zip(hists, got):
        want = scores_from_hist(h)
        assert sorted(s) == sorted(want) == sorted(["pAcc", "mAcc", "miou", "iou", "confusion", "precision", "recall"])
        for k in ("pAcc", "mAcc", "miou"):
            assert s[k] == want[k], k
        for k in ("iou", "confusion", "precision", "recall"):
            assert list(s[k]) == list(want[k]) == list(range(nc))
            assert np.array_equal(np.array(list(s[k].values())), np.array(list(want[k].values())), equal_nan=True), k
    assert any(np.isnan(list(s["iou"].values())).any() for s in got), "the cases hold classes that are in neither map"
    assert scores_from_totals(torch.from_numpy(totals))[1]["miou"] == got[1]["miou"]
    with pytest.raises(ValueError, match=r"\[K,3,nc\]"):
        scores_from_totals(totals[0])


def test_best_scale_and_the_table():
    from excel_amd.utils import bkg_sweep as bs

    def sc(miou, bkg=0.5):
        return {"pAcc": 0.9, "mAcc": 0.8, "miou": miou, "iou": {0: bkg, 1: 0.25, 2: 0.75, 3: NAN}, "confusion": {}, "precision": {},
                "recall": {0: 1.0, 1: 0.5, 2: 0.5, 3: NAN}}
    scales = (0.5, 0.85, 1.2, 2.0)
    assert bs.best_scale([sc(0.1), sc(0.3), sc(0.2), sc(0.25)], scales) == (1, 0.85)
    assert bs.best_scale([sc(0.3), sc(0.3), sc(0.3), sc(0.1)], scales) == (1, 0.85)            # a tie: |0.85 - 1| < |1.2 - 1| < |0.5 - 1|
    assert bs.best_scale([sc(0.3), sc(0.2), sc(0.3), sc(0.3)], scales) == (2, 1.2)
    assert bs.best_scale([sc(NAN), sc(0.0)], (0.5, 2.0)) == (1, 2.0)
    table = bs.format_sweep_table([sc(0.1), sc(0.3, bkg=0.625), sc(0.2), sc(0.25)], scales, ["_background_", "a", "b", "c"])
    rows = [[c.strip() for c in ln.strip("|").split("|")] for ln in table.splitlines() if ln.startswith("|")]
    assert rows[0] == ["bkg_scale", "pAcc", "mIoU", "IoU _background_", "mIoU foreground", ""]
    assert [r[0] for r in rows[1:]] == ["0.5", "0.85", "1.2", "2"] and [r[-1] for r in rows[1:]] == ["", "*", "", ""]
    assert rows[2][1:5] == ["90.000", "30.000", "62.500", "50.000"]                             # foreground: the classes with ground truth
    block = bs.sweep_json([sc(0.1), sc(NAN)], (0.5, 1.0))
    assert block == {"scales": [0.5, 1.0], "miou": [0.1, None], "best_scale": 0.5} and json.dumps(block)


# ------------------------------------------------------------------ registration
def test_the_entry_is_declared_bound_and_built_without_scratch_or_workspace():
    from excel_amd import _lib, build
    header = open(os.path.join(ROOT, "include", "excel_hip.h")).read()
    m = re.search(r"int excel_bkg_sweep_ragged\((.*?)\);", header, re.S)
    assert m, "include/excel_hip.h declares excel_bkg_sweep_ragged"
    params = [p.strip() for p in re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S).split(",")]
    assert [p.split()[-1].lstrip("*") for p in params] == ["planes", "nchan", "cls_idx", "gt", "table", "info", "Smax", "Cmax", "scales", "K", "skip",
                                                          "num_classes", "totals", "label_sel", "labels_u8", "stream"]
    ret, args = _lib.SIGNATURES["excel_bkg_sweep_ragged"]
    assert ret is _lib.c_i and len(args) == len(params) == 16
    assert [i for i, a in enumerate(args) if a is _lib.c_i] == [6, 7, 9, 11, 13]
    assert "background-scale sweep" in header and "ADDED to" in m.group(1)
    assert "bkgsweep.hip" in build.SOURCES and os.path.exists(os.path.join(build.CSRC, "bkgsweep.hip"))
    assert "bkg_sweep_kernel" in build.NO_SCRATCH and build.NO_SCRATCH_EXPECTED["bkgsweep"] == "bkg_sweep_kernel"
    assert "bkgsweep.hip" not in build.SPLIT_SOURCES
    src = open(os.path.join(build.CSRC, "bkgsweep.hip")).read()
    assert re.search(r"void bkg_sweep_kernel\(", src) and "__fmul_rn" in src
    names = list(_lib.SIGNATURES) + re.findall(r"\bexcel_\w+", header) + re.findall(r"\bexcel_\w+", src)
    assert not [s for s in names if "bkg" in s and "workspace_bytes" in s]


def test_the_binding_lives_outside_ops():
    """ops.py's stream callers are pinned by tests/_stream_cases.py; the sweep has its own stream test (test_gpu_bkg_sweep.py)."""
    from excel_amd import ops
    from excel_amd.utils import bkg_sweep
    assert not hasattr(ops, "bkg_sweep_ragged") and "excel_bkg_sweep_ragged" not in open(ops.__file__).read()
    assert callable(bkg_sweep.sweep_ragged)


# ------------------------------------------------------------------ the program
def test_parser_defaults_and_refusals():
    from excel_amd.tools import infer_lam
    from excel_amd.utils import bkg_sweep
    parse = infer_lam.get_parser().parse_args
    a = parse([])
    assert a.bkg_sweep is None and a.bkg_scale == 1.0
    assert bkg_sweep.resolve(a) == (None, 1.0)
    a = parse(["--bkg_sweep", "0.5,1.0,2.0", "--bkg_scale", "1.5"])
    assert bkg_sweep.resolve(a) == ((0.5, 1.0, 2.0), 1.5)
    for flags, word in ((["--bkg_sweep", "0.5,1.0", "--unlabeled", "true"], "--bkg_sweep scores the labels against ground truth: --unlabeled true"),
                        (["--bkg_sweep", "0.5,1.0", "--api_path", "true"], "--bkg_sweep runs on the batched loop: --api_path true"),
                        (["--bkg_scale", "1.5", "--api_path", "true"], "--bkg_scale runs on the batched loop: --api_path true"),
                        (["--bkg_scale", "0"], "--bkg_scale: bkg_sweep: scale 0.0"),
                        (["--bkg_sweep", "1.0,0.5"], "scale 0.5 follows 1.0")):
        with pytest.raises(ValueError, match=re.escape(word)):
            bkg_sweep.resolve(parse(flags))
        with pytest.raises(ValueError, match=re.escape(word)):          # the program stops there, before it builds anything
            infer_lam.validate(parse(flags))


class _Set:
    """Six small ragged samples (tests/test_host_cpu.py's stub set, a size of its own)"""
    has_cls_labels = True

    def __len__(self):
        return 6

    def max_k(self):
        return 2

    def __getitem__(self, i):
        rs = np.random.RandomState(900 + i)
        h, w = 5 + i % 4, 4 + (3 * i) % 5
        gt = rs.randint(0, 21, (h, w)).astype(np.uint8)
        gt[rs.rand(h, w) < 0.1] = 255
        cls = np.zeros(20, np.float32)
        cls[i % 20] = 1
        return f"s{i:03d}", rs.randint(0, 256, (h, w, 3)).astype(np.uint8), gt, cls


class _SweepStub:
    """A pipeline on CPU tensors: label = first image byte mod 21 where it exceeds a threshold that grows with the scale, else 0 -
    so the background grows with the scale, like the real one."""
    device, smax = "cpu", 2

    def __init__(self, bkg_sweep=None, bkg_scale=1.0):
        self.hist, self.bkg_sweep, self.bkg_scale, self.sweep_totals = None, bkg_sweep, bkg_scale, None

    @staticmethod
    def labels(images, scale):
        v = images.view(-1, 3)[:, 0].to(torch.int64).numpy()
        return np.where(v >= 64 * scale, v % 21, 0)

    def run_batch_ragged(self, images, plan, cls, gts, S=448, return_intermediates=False):
        g = gts.numpy().astype(np.int64)
        for j, s in enumerate((self.bkg_scale,) + tuple(self.bkg_sweep or ())):
            p = self.labels(images, s)
            ok = g < 21
            if j == 0:
                self.hist += torch.from_numpy(np.bincount(21 * g[ok] + p[ok], minlength=441).reshape(21, 21))
            else:
                rows = np.stack([np.bincount(g[ok], minlength=21), np.bincount(p[ok], minlength=21), np.bincount(g[ok & (g == p)], minlength=21)])
                self.sweep_totals[j - 1] += torch.from_numpy(rows)
        return torch.from_numpy(self.labels(images, self.bkg_scale).astype(np.uint8))


def test_validate_reports_the_sweep(tmp_path, caplog):
    """infer_lam.validate through a stub pipeline: the totals the loop hands to the pipeline come back summed, scored, logged as a table
    and written to --json_out; the matrix is the one of a run without the flag; a pipeline built for other scales is refused."""
    from excel_amd.tools import infer_lam
    from excel_amd.utils import bkg_sweep
    from excel_amd.utils.evaluate import scores_from_hist
    parse = infer_lam.get_parser().parse_args
    common = ["--batch_size", "4", "--num_workers", "0"]
    _, plain = infer_lam.validate(parse(common), dataset=_Set(), pipe=_SweepStub())
    assert infer_lam.validate.last_bkg_sweep is None
    scales = (0.5, 1.0, 2.0)
    js = str(tmp_path / "run.json")
    with caplog.at_level(logging.INFO):
        score, total = infer_lam.validate(parse(common + ["--bkg_sweep", "0.5,1.0,2.0", "--json_out", js]), dataset=_Set(), pipe=_SweepStub(scales))
    assert torch.equal(total, plain), "the flag changes no score"
    rep = infer_lam.validate.last_bkg_sweep
    assert rep["scales"] == scales and tuple(rep["totals"].shape) == (3, 3, 21) and rep["totals"].dtype == torch.int64
    t = rep["totals"].numpy()
    assert np.array_equal(t[1], np.stack([plain.numpy().sum(1), plain.numpy().sum(0), np.diag(plain.numpy())]))
    assert (np.diff(t[:, 1, 0]) > 0).all()
    want = scores_from_hist(plain)
    assert rep["scores"][1]["miou"] == want["miou"] and rep["scores"][1]["pAcc"] == want["pAcc"]
    assert "bkg_sweep_score:" in caplog.text and bkg_sweep.format_sweep_table(rep["scores"], scales, infer_lam.VOC_CLASSES) in caplog.text
    assert f"bkg_sweep best scale {rep['best_scale']:g}" in caplog.text
    with open(js) as f:
        block = json.load(f)["bkg_sweep"]
    assert block == bkg_sweep.sweep_json(rep["scores"], scales) and block["scales"] == [0.5, 1.0, 2.0] and block["miou"][1] == want["miou"]
    # --bkg_scale: the labels of that scale are what the run scores
    _, at2 = infer_lam.validate(parse(common + ["--bkg_scale", "2.0"]), dataset=_Set(), pipe=_SweepStub(None, 2.0))
    assert np.array_equal(np.stack([at2.numpy().sum(1), at2.numpy().sum(0), np.diag(at2.numpy())]), t[2])
    with pytest.raises(ValueError, match=re.escape("--bkg_sweep: the supplied pipeline was built with bkg_sweep=(0.5, 1.0)")):
        infer_lam.validate(parse(common + ["--bkg_sweep", "0.5,1.0,2.0"]), dataset=_Set(), pipe=_SweepStub((0.5, 1.0)))
    with pytest.raises(ValueError, match=re.escape("--bkg_scale: the supplied pipeline was built with bkg_scale=1.0")):
        infer_lam.validate(parse(common + ["--bkg_scale", "2.0"]), dataset=_Set(), pipe=_SweepStub())


def test_the_uniform_loop_and_the_other_entry_points_refuse():
    from excel_amd.pipeline import TrainingFreePipeline
    from excel_amd.tools import infer_lam
    with pytest.raises(ValueError, match=re.escape("--bkg_sweep runs behind the ragged step: ragged batches")):
        infer_lam.build_validation(args=infer_lam.get_parser().parse_args(["--bkg_sweep", "0.5,1.0"]), device="cpu", pipe=_SweepStub((0.5, 1.0)))
    with pytest.raises(ValueError, match=re.escape("--bkg_scale runs behind the ragged step")):
        infer_lam.build_validation(args=infer_lam.get_parser().parse_args(["--bkg_scale", "0.5"]), device="cpu", pipe=_SweepStub(None, 0.5))
    p = TrainingFreePipeline(None)
    assert p.bkg_sweep is None and p.bkg_scale == 1.0 and p.sweep_totals is None
    x = torch.zeros(1, 3, 32, 32)
    for kw, word in ((dict(bkg_sweep=(0.5, 1.0)), "bkg_sweep=(0.5, 1.0)"), (dict(bkg_scale=0.5), "bkg_scale=0.5")):
        p = TrainingFreePipeline(None, **kw)
        for name in ("run_batch", "run_batch_split", "run_batch_overlapped"):
            with pytest.raises(ValueError, match=re.escape(f"{name} has no background s") + ".*" + re.escape(word)):
                getattr(p, name)(x, None)
    with pytest.raises(ValueError, match="scale 1.0 follows 1.0"):
        TrainingFreePipeline(None, bkg_sweep=(1.0, 1.0))
    with pytest.raises(ValueError, match="scale -1.0"):
        TrainingFreePipeline(None, bkg_scale=-1.0)
    p = TrainingFreePipeline(None, bkg_sweep=[0.5, 1], bkg_scale=2)
    assert p.bkg_sweep == (0.5, 1.0) and p.bkg_scale == 2.0 and p.sweep_totals is None
