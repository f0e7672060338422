"""Host side of the DenseCRF stage for LAMs on ragged batches (excel_dcrf_lam_ragged): the C ABI declares and exports the entries, the
parser knows the flags, the workspace (a host function of the sizes and class counts) grows with the class counts and stays within its
documented bound of the uniform entry's, ops.dcrf_lam_groups cuts a batch into consecutive runs within a budget, and infer_lam's main
loop hands every ragged batch - its own plan and host class counts - to ops.dcrf_lam_ragged without writing a record.  No device."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["excel_dcrf_lam_ragged_workspace_bytes", "excel_dcrf_lam_ragged"]
SIZES = [(375, 500), (500, 333), (37, 53), (480, 640), (1, 1), (16, 3), (480, 640), (333, 500), (12, 12)]
NCHAN = [2, 3, 2, 5, 1, 2, 2, 4, 3]


def _ws(hw, nchan):
    from excel_amd import ops
    return ops.dcrf_lam_ragged_workspace_bytes(hw, nchan)


def test_new_entries_declared_exported_and_bound():
    from excel_amd import _lib, ops
    src = open(os.path.join(ROOT, "include", "excel_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    handle = ctypes.CDLL(_lib.LIB_PATH)
    for n in NEW:
        assert re.search(r"\b%s\s*\(" % n, src), f"{n} is not declared in include/excel_hip.h"
        assert hasattr(handle, n), f"{n} is not exported"
        assert n in _lib.SIGNATURES
    _lib.lib()
    for f in ("dcrf_lam_ragged_workspace_bytes", "dcrf_lam_groups", "dcrf_lam_ragged"):
        assert callable(getattr(ops, f))


def test_parser_defaults():
    from excel_amd.tools import infer_lam
    a = infer_lam.get_parser().parse_args([])
    assert a.crf_inline is False and a.crf_ws_gb == 16 and a.crf_label_dir is None
    a = infer_lam.get_parser().parse_args(["--crf_inline", "true", "--crf_ws_gb", "0.5", "--crf_label_dir", "x"])
    assert a.crf_inline is True and a.crf_ws_gb == 0.5 and a.crf_label_dir == "x"
    # the stage runs inline only when both flags are set, and never on a test split
    a.crf_post, a.infer_set = True, "val"
    assert infer_lam.crf_inline_wanted(a)
    a.infer_set = "test"
    assert not infer_lam.crf_inline_wanted(a)
    a.infer_set, a.crf_post = "val", False
    assert not infer_lam.crf_inline_wanted(a)
    assert infer_lam.CRF_PARAMS == dict(iter_max=10, pos_w=3, pos_xy_std=1, bi_w=4, bi_xy_std=67, bi_rgb_std=3)     # tools/infer_lam.py:191-198


def test_workspace_grows_with_the_class_counts_and_is_bounded():
    from excel_amd import ops
    # the largest count of the group sets the rows' stride: the workspace grows with it, and with every image
    got = [_ws(SIZES, [c] * len(SIZES)) for c in (1, 2, 3, 5, 21)]
    assert all(a < b for a, b in zip(got, got[1:])), got
    assert _ws(SIZES, [1] * 8 + [5]) == _ws(SIZES, [5] * 9) > _ws(SIZES, [4] * 9)
    more = [_ws(SIZES[:k], NCHAN[:k]) for k in range(1, len(SIZES) + 1)]
    assert all(a <= b for a, b in zip(more, more[1:])) and more[0] < more[-1]
    # uniform counts: the uniform entry's workspace plus one int32 per lattice vertex (3 + 6 per pixel), two arrays rounded up to 256 bytes
    for hw in (SIZES, SIZES[2:3], [(1, 1)]):
        n = sum(h * w for h, w in hw)
        for c in (1, 3, 21):
            uni = ops.dcrf_ragged_workspace_bytes(hw, c)
            lam = _ws(hw, [c] * len(hw))
            assert uni < lam <= uni + 4 * 9 * n + 2 * 255, (hw, c)


def test_workspace_refusals():
    with pytest.raises(RuntimeError, match="classes"):
        _ws(SIZES[:2], [2, 0])
    with pytest.raises(RuntimeError, match="32-bit"):
        _ws([(40000, 40000)], [2])
    with pytest.raises(RuntimeError):
        _ws([(0, 5)], [2])
    with pytest.raises(ValueError):
        _ws(SIZES[:2], [2])


def _check_runs(runs, sizes, nchan, budget):
    assert [s for s, _ in runs] == [0] + [e for _, e in runs[:-1]] and runs[-1][1] == len(sizes)     # every image once, in order
    assert all(e > s for s, e in runs)
    for s, e in runs:
        if e - s > 1:
            assert _ws(sizes[s:e], nchan[s:e]) <= budget                                              # the budget is honoured
        if e < len(sizes) and _ws(sizes[s:e], nchan[s:e]) <= budget:
            assert _ws(sizes[s:e + 1], nchan[s:e + 1]) > budget, "the run stopped although the next image fits"


def test_dcrf_lam_groups():
    from excel_amd import ops
    one = [_ws([s], [c]) for s, c in zip(SIZES, NCHAN)]
    whole = _ws(SIZES, NCHAN)
    assert ops.dcrf_lam_groups(SIZES, NCHAN, whole) == [(0, len(SIZES))]
    assert ops.dcrf_lam_groups(SIZES, NCHAN, 1) == [(b, b + 1) for b in range(len(SIZES))]
    for budget in (max(one), 2 * max(one), max(one) + min(one), whole // 2, whole - 1):
        runs = ops.dcrf_lam_groups(SIZES, NCHAN, budget)
        _check_runs(runs, SIZES, NCHAN, budget)
        assert runs == ops.dcrf_lam_groups(list(SIZES), list(NCHAN), budget) and len(runs) > 1
    # the image with 5 classes at 480 x 640 is over this budget: a run of its own, its neighbours still group
    small = one[3] - 1
    runs = ops.dcrf_lam_groups(SIZES, NCHAN, small)
    _check_runs(runs, SIZES, NCHAN, small)
    assert (3, 4) in runs and any(e - s > 1 for s, e in runs)
    # the class counts matter: the same sizes with fewer classes make fewer groups
    assert len(ops.dcrf_lam_groups(SIZES, [1] * 9, whole // 2)) <= len(ops.dcrf_lam_groups(SIZES, [5] * 9, whole // 2))
    assert len(ops.dcrf_lam_groups(SIZES, [1] * 9, whole // 3)) < len(ops.dcrf_lam_groups(SIZES, [21] * 9, whole // 3))
    assert ops.dcrf_lam_groups([(5, 5)], [2], 1) == [(0, 1)]
    assert ops.dcrf_lam_groups([], [], 1) == []


# ------------------------------------------------------------------ the main loop's control flow
class _TinyRaggedSet:
    """(name, image u8 [h,w,3], label u8 [h,w], cls f32 [20]) with a different size and 1..3 present classes per sample."""
    def __init__(self, n):
        self.n = n

    def __len__(self):
        return self.n

    def max_k(self):
        return 3

    def __getitem__(self, i):
        rs = np.random.RandomState(700 + i)
        h, w = 5 + i % 7, 4 + (3 * i) % 5
        gt = rs.randint(0, 21, (h, w)).astype(np.uint8)
        gt[rs.rand(h, w) < 0.1] = 255
        cls = np.zeros(20, np.float32)
        cls[[(i + 7 * j) % 20 for j in range(1 + i % 3)]] = 1
        return f"s{i:03d}", rs.randint(0, 256, (h, w, 3)).astype(np.uint8), gt, cls


class _StubPipe:
    """Stands in for TrainingFreePipeline: labels = a function of the image bytes; the step leaves cams / class counts behind."""
    device, smax = "cpu", 3

    def __init__(self):
        self.hist, self.steps = None, []

    def run_batch_ragged(self, images, plan, cls, gts, S=448, return_intermediates=False):
        assert not return_intermediates, "the inline CRF stage needs no copies of the intermediates"
        self.last_cams = torch.zeros((self.smax + 1) * plan.total_pix)
        k = (cls != 0).sum(1).to(torch.int32)
        self.last_nchan = k + 1
        self.last_cls_idx = torch.zeros((plan.B, self.smax), dtype=torch.int32)
        self.steps.append(plan)
        return (images.view(-1, 3)[:, 0] % 21).to(torch.uint8)


def test_main_loop_runs_the_stage_once_per_batch_without_records(monkeypatch, tmp_path):
    from excel_amd import ops
    from excel_amd.tools import infer_lam
    from excel_amd.utils import imutils
    for k in ("WORLD_SIZE", "RANK", "LOCAL_WORLD_SIZE"):
        monkeypatch.delenv(k, raising=False)
    n, calls = 12, []

    def fake_crf(images_u8, plan, cams, Cmax, nchan, nchan_host, cls_idx, iters, pos_w, pos_xy_std, bi_w, bi_xy_std, bi_rgb_std,
                 want_labels=True, want_q=False, budget_bytes=None):
        calls.append(dict(plan=plan, cams=cams, Cmax=Cmax, nchan=nchan, host=np.asarray(nchan_host).copy(), cls_idx=cls_idx,
                          params=(iters, pos_w, pos_xy_std, bi_w, bi_xy_std, bi_rgb_std), want=(want_labels, want_q), budget=budget_bytes))
        assert images_u8.numel() == 3 * plan.total_label_pix
        return (images_u8.view(-1, 3)[:, 1] % 21).to(torch.uint8), None

    def fake_confusion(gt, pred, nc, hist=None):
        g, p = gt.view(-1).to(torch.int64), pred.view(-1).to(torch.int64)
        keep = g < nc
        hist += torch.bincount(nc * g[keep] + p[keep], minlength=nc * nc).view(nc, nc)
        return hist

    def no_records(*a, **k):
        raise AssertionError("save_logits called on the inline path")

    monkeypatch.setattr(ops, "dcrf_lam_ragged", fake_crf)
    monkeypatch.setattr(ops, "confusion_accumulate", fake_confusion)
    monkeypatch.setattr(imutils, "save_logits", no_records)
    monkeypatch.setattr(infer_lam, "crf_proc", lambda *a, **k: pytest.fail("crf_proc ran on the inline path"))
    logits = tmp_path / "logits"
    pipe = _StubPipe()
    args = infer_lam.get_parser().parse_args(["--batch_size", "5", "--num_workers", "0", "--crf_post", "true", "--crf_inline", "true",
                                              "--crf_ws_gb", "0.25", "--logits_dir", str(logits)])
    infer_lam.validate(args, dataset=_TinyRaggedSet(n), pipe=pipe)
    ds = _TinyRaggedSet(n)
    assert [c["plan"].B for c in calls] == [5, 5, 2]
    for c, step, s0 in zip(calls, pipe.steps, (0, 5, 10)):
        idx = range(s0, min(s0 + 5, n))
        assert c["plan"] is step                                               # the batch's own plan
        assert [tuple(x) for x in c["plan"].hw] == [ds[i][1].shape[:2] for i in idx]
        assert c["host"].dtype == np.int32 and list(c["host"]) == [1 + int(ds[i][3].sum()) for i in idx]       # k + 1 from the one-hot rows
        assert c["Cmax"] == pipe.smax + 1 and c["cams"].numel() == c["Cmax"] * c["plan"].total_pix
        assert c["params"] == (10, 3, 1, 4, 67, 3) and c["want"] == (True, False) and c["budget"] == 2 ** 28
        assert c["nchan"].dtype == torch.int32 and list(c["nchan"]) == list(c["host"])
    assert not logits.exists()
    # the stage's labels were scored against the batch's ground truth and gathered like the main histogram
    import oracle
    ref = sum(oracle.evaluate.fast_hist(ds[i][2].flatten(), ds[i][1].reshape(-1, 3)[:, 1].astype(np.int64) % 21, 21) for i in range(n))
    score, total = infer_lam.validate.last_crf
    assert np.array_equal(total.numpy(), ref) and 0.0 <= score["miou"] <= 1.0
    # without --crf_inline the loop asks for the record path's copies instead
    args = infer_lam.get_parser().parse_args(["--batch_size", "5", "--num_workers", "0", "--crf_post", "true", "--logits_dir", str(logits)])
    with pytest.raises(AssertionError, match="no copies"):
        infer_lam.validate(args, dataset=_TinyRaggedSet(n), pipe=_StubPipe())
    assert len(calls) == 3


def test_a_second_run_reports_nothing_of_the_first(monkeypatch):
    """validate twice in one process: with the inline CRF stage and the confident labels, then with neither - what the second call
    leaves in validate.last_* / build_validation.last_* is its own (None for the stages it did not run)."""
    import test_host_overflow_guard as G
    from excel_amd import ops
    from excel_amd.tools import infer_lam
    for k in ("WORLD_SIZE", "RANK", "LOCAL_WORLD_SIZE"):
        monkeypatch.delenv(k, raising=False)

    class ConfPipe(_StubPipe):
        def run_batch_ragged(self, images, plan, cls, gts, S=448, return_intermediates=False, conf=None):
            labels = super().run_batch_ragged(images, plan, cls, gts, S=S, return_intermediates=return_intermediates)
            return labels, labels

    G._FakeLabelSaver.log = []
    monkeypatch.setattr(infer_lam, "_LabelSaver", G._FakeLabelSaver)
    monkeypatch.setattr(ops, "dcrf_lam_ragged", lambda images_u8, plan, *a, **k: ((images_u8.view(-1, 3)[:, 1] % 21).to(torch.uint8), None))
    monkeypatch.setattr(ops, "confusion_accumulate", lambda gt, pred, nc, hist=None: hist)
    flags = ["--batch_size", "5", "--num_workers", "0"]
    first = infer_lam.get_parser().parse_args(flags + ["--crf_post", "true", "--crf_inline", "true", "--conf_label", "true"])
    infer_lam.validate(first, dataset=_TinyRaggedSet(7), pipe=ConfPipe())
    assert infer_lam.validate.last_crf is not None and infer_lam.validate.last_conf is not None
    assert infer_lam.build_validation.last_crf_hist is not None and infer_lam.build_validation.last_conf_hist is not None
    infer_lam.validate(infer_lam.get_parser().parse_args(flags), dataset=_TinyRaggedSet(7), pipe=_StubPipe())
    assert infer_lam.validate.last_crf is None and infer_lam.validate.last_conf is None
    assert infer_lam.build_validation.last_crf_hist is None and infer_lam.build_validation.last_conf_hist is None


def test_gpu_tests_use_the_programs_parameter_set():
    import test_gpu_dcrf_lam as G
    from excel_amd.tools.infer_lam import CRF_PARAMS as P
    assert G.LAM_SET == (P["pos_w"], P["pos_xy_std"], P["bi_w"], P["bi_xy_std"], P["bi_rgb_std"]) and P["iter_max"] == 10
