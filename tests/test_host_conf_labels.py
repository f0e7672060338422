"""Host side of the two-threshold pseudo labels (include/excel_hip.h, "confident labels"): the float64 numpy restatement
(tests/_conf_ref.py) is pinned to the fixture minted from the reference's refine_cams_with_bkg_v2 (tests/golden/conf_labels.npz,
tests/golden/make_conf_golden.py), the C ABI declares and exports the two entries, the parser knows the flags and refuses a bad pair
of thresholds before a model is built, and the half plan refuses an image too small to halve by name.  No device."""
import ctypes
import os
import re

import numpy as np
import pytest

import _conf_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["excel_conf_planes_ragged", "excel_conf_merge_ragged"]


@pytest.fixture(scope="module")
def fixture(golden):
    z = golden("conf_labels.npz")
    return {k: z[k] for k in z.files}


def test_fixture_holds_arrays_only_and_covers_the_cases(fixture):
    high, low, ignore, ds, num_iter, _ = fixture["meta"]
    assert (high, low, ignore, ds, num_iter) == (0.7, 0.25, 255, 2, 10)
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "conf_labels.npz")) < 1 << 20
    for c, hw in enumerate([(50, 66), (33, 47)]):
        assert fixture[f"img_{c}"].shape == (2, 3) + hw and fixture[f"cams_{c}"].shape == (2, 5) + hw
        assert fixture[f"cls_{c}"].sum(1).tolist() == [3, 1]
        assert 0.0 <= fixture[f"cams_{c}"].min() and fixture[f"cams_{c}"].max() <= 1.0
        y0, y1, x0, x1 = fixture[f"box_{c}"][0]
        assert 0 < y0 < y1 < hw[0] and 0 < x0 < x1 < hw[1], "the box of image 0 cuts both axes on both sides"
        for b in range(2):
            lab = fixture[f"lab_{c}"][b]
            keys = set(np.flatnonzero(fixture[f"cls_{c}"][b]) + 1)
            assert set(np.unique(lab)) <= keys | {0, 255} and (lab == 255).any() and (lab != 255).any()
            # the reference's own float32 and float64 labels inside the gate of tests/test_gpu_many_classes.py, with room
            for tag in ("", "_box"):
                assert (fixture[f"lab{tag}_{c}"][b] == fixture[f"lab64{tag}_{c}"][b]).mean() >= 0.9995


@pytest.mark.parametrize("c", [0, 1])
def test_restatement_matches_the_reference(fixture, c):
    """planes within 1e-6 of the reference's float32 planes (their own rounding is ~6e-8); PAR outputs within test_par_golden's 1e-4; labels EQUAL to the reference's float64 labels, with and without img_box."""
    high, low, ignore, ds, num_iter, _ = fixture["meta"]
    img, cams, cls, box = (fixture[f"{n}_{c}"] for n in ("img", "cams", "cls", "box"))
    for b in range(img.shape[0]):
        lab, ph, pl, qh, ql = R.conf_labels_ref(img[b], cams[b], cls[b], high, low, int(ignore), None, int(ds), int(num_iter))
        planes, par = fixture[f"planes_{c}_{b}"], fixture[f"par_{c}_{b}"]
        e_planes = max(np.abs(ph - planes[0]).max(), np.abs(pl - planes[1]).max())
        e_par = max(np.abs(qh - par[0]).max(), np.abs(ql - par[1]).max())
        print(f"\n[conf-ref] case {c} image {b}: planes {e_planes:.2e}, PAR {e_par:.2e}")
        assert ph.shape == planes[0].shape and e_planes < 1e-6
        assert e_par < 1e-4
        assert np.array_equal(lab, fixture[f"lab64_{c}"][b])
        keys = np.concatenate([[0], np.flatnonzero(cls[b]) + 1])
        boxed = R.merge_ref(qh, ql, keys, cams.shape[-2:], int(ignore), box[b])
        assert np.array_equal(boxed, fixture[f"lab64_box_{c}"][b])
        y0, y1, x0, x1 = box[b]
        outside = np.ones(boxed.shape, bool)
        outside[y0:y1, x0:x1] = False
        assert (boxed[outside] == ignore).all()


def test_new_entries_declared_exported_and_bound():
    from excel_amd import _lib, build, ops
    assert "conf.hip" in build.SOURCES
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "excel_hip.h")).read(), flags=re.S)
    handle = ctypes.CDLL(_lib.LIB_PATH)
    for n in NEW:
        assert re.search(r"\b%s\s*\(" % n, src), f"{n} is not declared in include/excel_hip.h"
        assert hasattr(handle, n), f"{n} is not exported"
        assert n in _lib.SIGNATURES
    for f in ("conf_half_plan", "conf_planes_ragged", "conf_merge_ragged"):
        assert callable(getattr(ops, f))


def test_parser_defaults():
    from excel_amd.tools import infer_lam
    a = infer_lam.get_parser().parse_args([])
    assert a.conf_label is False and a.conf_label_dir is None
    assert (a.conf_high_thre, a.conf_low_thre) == (0.7, 0.25)          # the reference's --high_thre / --low_thre defaults
    assert infer_lam.resolve_conf(a) is None
    a = infer_lam.get_parser().parse_args(["--conf_label", "true", "--conf_label_dir", "x"])
    assert infer_lam.resolve_conf(a) == (0.7, 0.25) and a.conf_label_dir == "x"
    d = infer_lam.conf_label_output_dir(None, "train")
    assert d.endswith("_conf_label") and d != infer_lam.label_output_dir(None, "train")


@pytest.mark.parametrize("flags, named", [
    (["--conf_high_thre", "0.3", "--conf_low_thre", "0.3"], "0.3"),       # low_thre >= high_thre
    (["--conf_high_thre", "0.2", "--conf_low_thre", "0.6"], "0.6"),
    (["--conf_high_thre", "1.0"], "1.0"),                                  # outside (0, 1)
    (["--conf_low_thre", "0.0"], "0.0"),
    (["--conf_low_thre", "-0.25"], "-0.25"),
    (["--conf_high_thre", "1.5"], "1.5"),
])
def test_bad_thresholds_are_refused_before_a_model_is_built(flags, named, monkeypatch):
    from excel_amd.tools import infer_lam
    from excel_amd.model import model_excel

    def no_model(*a, **k):
        raise AssertionError("a model was built before the thresholds were checked")
    monkeypatch.setattr(model_excel, "ExCEL_model", no_model)
    monkeypatch.setattr("torch.cuda.set_device", no_model)
    args = infer_lam.get_parser().parse_args(["--conf_label", "true", "--synthetic", "2"] + flags)
    with pytest.raises(ValueError, match=re.escape(named)):
        infer_lam.validate(args)
    # without --conf_label the two values are not read
    infer_lam.resolve_conf(infer_lam.get_parser().parse_args(flags))


def test_check_conf():
    from excel_amd.pipeline import check_conf
    assert check_conf(None) is None and check_conf((0.7, 0.25)) == (0.7, 0.25) and check_conf(["0.5", 0.1]) == (0.5, 0.1)
    for bad in [(0.25, 0.7), (0.5, 0.5), (1.0, 0.5), (0.5, 0.0), (float("nan"), 0.2)]:
        with pytest.raises(ValueError):
            check_conf(bad)


def test_half_plan_refuses_an_empty_half_by_name():
    from excel_amd import ops
    plan = ops.RaggedPlan([(33, 50), (64, 47), (17, 96), (2, 3)], None)
    half = ops.conf_half_plan(plan)
    assert half.hw.tolist() == [[16, 25], [32, 23], [8, 48], [1, 1]] and half.B == 4
    assert ops.conf_half_plan(plan, 1).hw.tolist() == plan.hw.tolist()
    with pytest.raises(ValueError, match="2008_000001.*1 x 7"):
        ops.conf_half_plan(ops.RaggedPlan([(8, 8), (1, 7)], None), names=["2007_000032", "2008_000001"])
    with pytest.raises(ValueError, match="image 0"):
        ops.conf_half_plan(ops.RaggedPlan([(5, 1)], None))


# ------------------------------------------------------------------ the program's control flow, through the overflow guard's stub
def test_conf_labels_go_through_the_guard_rerun_and_the_one_gather(monkeypatch, caplog):
    """--conf_label on the batched loop with --overflow_guard rerun, driven by a stub pipeline on CPU tensors: every step is asked for
    conf=(high, low) and handed a half plan, the confident labels of a step go to their own writer, flagged images stay out of
    hist_conf in the first pass and run once more through the same consumer behind the barrier (files overwritten by name), and
    validate reports the second table and the coverage from the gathered matrix."""
    import logging
    import torch
    import oracle
    import test_host_overflow_guard as G
    from excel_amd.tools import infer_lam

    class Stub(G._GuardStub):
        hist_conf = None

        def run_batch_ragged(self, images, plan, cls, gts, S=448, return_intermediates=False, conf=None):
            assert conf == (0.6, 0.2) and plan.conf_half.hw.tolist() == (plan.hw // 2).tolist()
            labels = super().run_batch_ragged(images, plan, cls, gts, S=S)
            kept = torch.where(labels % 2 == 0, labels, torch.full_like(labels, 255))       # odd labels fall into the band
            flags = self._ticket._flags
            for b in range(plan.B):
                if not (self.guard == "skip" and flags[b]):
                    lo, hi = int(plan.loff[b]), int(plan.loff[b + 1])
                    g, k = gts.numpy()[lo:hi], kept.numpy()[lo:hi]
                    self.hist_conf += torch.from_numpy(oracle.evaluate.fast_hist(g[k < 21], k[k < 21].astype(np.int64), 21))
            return labels, kept

    class Saver(G._FakeLabelSaver):
        def __init__(self, args, directory=None):
            self.tag = "conf" if directory == "conf_dir" else "main"

        def ragged(self, names, plan, labels_flat):
            self.log.append(("write", self.tag, tuple(str(n) for n in names), int((labels_flat == 255).sum())))

    n, log = 8, []
    ds = G._IndexedSet(n)
    Saver.log = log
    monkeypatch.setattr(infer_lam, "_LabelSaver", Saver)
    pipe = Stub("skip", bad_fast={1, 6}, log=log)
    args = G._args("--overflow_guard", "rerun", "--save_label", "true", "--conf_label", "true", "--conf_label_dir", "conf_dir",
                   "--conf_high_thre", "0.6", "--conf_low_thre", "0.2")
    with caplog.at_level(logging.INFO):
        _, total = infer_lam.validate(args, dataset=ds, pipe=pipe)
    writes = [e for e in log if e[0] == "write"]
    assert [e[1:3] for e in writes if e[1] == "conf"] == [("conf", ("s000", "s001", "s002")), ("conf", ("s003", "s004", "s005")),
                                                          ("conf", ("s006", "s007")), ("conf", ("s001", "s006"))]
    assert [e[2] for e in writes if e[1] == "main"] == [e[2] for e in writes if e[1] == "conf"]
    assert any(e[3] > 0 for e in writes if e[1] == "conf") and all(e[3] == 0 for e in writes if e[1] == "main")
    assert sum(1 for e in log if e == ("barrier",)) == 2 and sum(1 for e in log if e == ("close",)) == 2      # both writers
    ref = np.zeros((21, 21), np.int64)
    for i in range(n):
        _, img, gt, _ = ds[i]
        pred = img.reshape(-1, 3)[:, 0].astype(np.int64) % 21
        keep = pred % 2 == 0
        ref += oracle.evaluate.fast_hist(gt.flatten()[keep], pred[keep], 21)
    conf_score, conf_total, coverage = infer_lam.validate.last_conf
    assert np.array_equal(conf_total.numpy(), ref) and 0 < ref.sum() < int(total.sum())
    assert coverage == ref.sum() / float(total.sum())
    assert "conf_label_score:" in caplog.text and "conf_label coverage" in caplog.text
    # the flag off: the stub of the overflow guard's own tests (no conf= parameter) is driven exactly as before
    plain = G._GuardStub(None)
    infer_lam.validate(G._args(), dataset=ds, pipe=plain)
    assert infer_lam.validate.last_conf is None


def test_a_writer_that_fails_on_close_is_raised_before_any_score_and_every_writer_is_closed_once(monkeypatch, caplog):
    import logging
    import test_host_overflow_guard as G
    from excel_amd.tools import infer_lam

    class Stub(G._GuardStub):
        hist_conf = None

        def run_batch_ragged(self, images, plan, cls, gts, S=448, return_intermediates=False, conf=None):
            labels = super().run_batch_ragged(images, plan, cls, gts, S=S)
            return labels, labels

    class Saver(G._FakeLabelSaver):
        def __init__(self, args, directory=None):
            self.tag = "conf" if directory == "conf_dir" else "main"

        def close(self):
            self.log.append(("close", self.tag))
            raise OSError(f"disk full ({self.tag})")

    Saver.log = log = []
    monkeypatch.setattr(infer_lam, "_LabelSaver", Saver)
    args = G._args("--save_label", "true", "--conf_label", "true", "--conf_label_dir", "conf_dir")
    with caplog.at_level(logging.INFO), pytest.raises(OSError, match="disk full"):
        infer_lam.validate(args, dataset=G._IndexedSet(5), pipe=Stub(None))
    assert sum(1 for e in log if e[0] == "write") == 4                                  # the loop ran through: 2 steps, both writers
    assert sorted(e for e in log if e[0] == "close") == [("close", "conf"), ("close", "main")]
    assert "LAM_score" not in caplog.text and "mIoU" not in caplog.text and "conf_label_score" not in caplog.text


def test_conf_label_needs_the_ragged_step():
    from excel_amd.tools import infer_lam
    args = infer_lam.get_parser().parse_args(["--conf_label", "true", "--synthetic", "4"])
    args.ragged_batches = False

    class P:
        smax, guard, model, device = 2, None, None, "cpu"
    with pytest.raises(ValueError, match="--conf_label"):
        infer_lam.build_validation(None, None, None, np.arange(4), "cpu", args, pipe=P())
