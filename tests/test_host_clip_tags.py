"""Host-side tests of the predicted image tags (tools/infer_lam --tags clip, --unlabeled, --save_tags): the float64 restatement of
excel_clip_tags and its case table, the flags and what they refuse, the pipeline constructors, the tag metrics, the image-only data
set, the tags file, and the batched loop's control flow through a stub pipeline on CPU tensors - alone and with two ranks on gloo."""
import ast
import inspect
import os
import socket
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _clip_tags_ref as R  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------ the reference itself
def test_reference_ties_go_to_the_lower_index():
    rs = np.random.RandomState(0)
    text = rs.standard_normal((6, 16))
    text[3] = text[1]                                    # two identical rows: identical scores
    x = (text[1] + 0.05 * rs.standard_normal(16))[None]  # ... and they are the best two
    onehot, s = R.clip_tags_ref(x, text, 6, 10.0, 0.0, 1)
    assert s[0, 1] == s[0, 3] == s[0].max()
    assert onehot[0].tolist() == [0, 1, 0, 0, 0, 0]      # kmax = 1 cuts between them: the lower index stays
    onehot2, _ = R.clip_tags_ref(x, text, 6, 10.0, 0.0, 2)
    assert onehot2[0].tolist() == [0, 1, 0, 1, 0, 0]
    assert R.margin(s, 0.0, 1) > 1e-3                     # the exact tie is no margin violation


def test_reference_top1_always_kept_and_kmax_caps():
    rs = np.random.RandomState(1)
    x, text = rs.standard_normal((5, 32)), rs.standard_normal((12, 32))
    for thre in (0.0, 0.3, 1.0):
        for kmax in (1, 3, 8):
            onehot, s = R.clip_tags_ref(x, text, 8, 100.0, thre, kmax)
            k = onehot.sum(1)
            assert (k >= 1).all() and (k <= kmax).all()
            assert (onehot[np.arange(5), s.argmax(1)] == 1).all()
            if thre == 0.0:
                assert (k == kmax).all()                 # thre = 0: exactly the kmax best
                for b in range(5):
                    assert set(np.flatnonzero(onehot[b])) == set(np.argsort(-s[b], kind="stable")[:kmax])
            if thre == 1.0:
                assert (k == 1).all()                    # thre = 1: only a score equal to the best passes
    # background rows compete: the same foreground rows with more prompts get less mass
    _, s_all = R.clip_tags_ref(x, text, 8, 100.0, 0.2, 3)
    _, s_fg = R.clip_tags_ref(x, text[:8], 8, 100.0, 0.2, 3)
    assert (s_all <= s_fg + 1e-15).all() and np.allclose(s_fg.sum(1), 1.0)


def test_reference_nonfinite_row_gives_class_zero():
    rs = np.random.RandomState(2)
    x, text = rs.standard_normal((3, 16)), rs.standard_normal((7, 16))
    x[1, 5] = np.inf
    onehot, s = R.clip_tags_ref(x, text, 4, 100.0, 0.2, 2)
    assert onehot[1].tolist() == [1, 0, 0, 0] and np.isnan(s[1]).all()
    assert np.isfinite(s[[0, 2]]).all() and (onehot[[0, 2]].sum(1) >= 1).all()
    x[1] = 0                                              # a zero row has no direction either
    onehot, s = R.clip_tags_ref(x, text, 4, 100.0, 0.2, 2)
    assert onehot[1].tolist() == [1, 0, 0, 0] and np.isnan(s[1]).all()
    assert R.score_error(s, s) == 0.0


@pytest.mark.parametrize("name", sorted(R.CASES))
def test_case_margins_make_exact_comparison_legitimate(name):
    """Every case of the table decides each class at a relative distance of at least 1e-3 from a boundary in float64 - four orders of
    magnitude above a float32 evaluation's score error - so a float32 kernel must reproduce the one-hot rows exactly."""
    x, text, F, scale, thre, kmax = R.make_case(name)
    onehot, s = R.clip_tags_ref(x, text, F, scale, thre, kmax)
    m = R.margin(s, thre, kmax)
    onehot32, s32 = R.clip_tags_ref(x, text, F, scale, thre, kmax, dtype=np.float32)
    err = R.score_error(s32, s)
    print(f"{name}: margin {m:.4g}, float32 numpy score error {err:.3g}, bound {R.score_bound(scale, x.shape[1]):.3g}")
    assert m >= R.MIN_MARGIN
    assert err <= 1e-6 and err <= R.score_bound(scale, x.shape[1])
    assert np.array_equal(onehot32, onehot)
    assert (onehot.sum(1) >= 1).all() and (onehot.sum(1) <= kmax).all()


# ------------------------------------------------------------------ the C ABI and the op, as far as a host can see them
def test_entry_is_declared_bound_and_built():
    from excel_amd import _lib, build, ops
    hdr = open(os.path.join(ROOT, "include", "excel_hip.h")).read()
    assert "int excel_clip_tags(const float* x_cls, long long stride, const float* text, int B, int C, int T, int F, float scale" in hdr
    assert "clip_surgery_model.py:442-446" in hdr
    res, args = _lib.SIGNATURES["excel_clip_tags"]
    assert res is _lib.c_i and len(args) == 13 and args[1] is _lib.c_ll and args[7] is args[8] is _lib.C.c_float
    assert "tag.hip" in build.SOURCES and build.NO_SCRATCH_EXPECTED["tag"] in build.NO_SCRATCH
    assert _lib.lib().excel_abi_version() >= 6
    # no workspace: nothing for the scratch-contract table to cover
    fn = next(n for n in ast.parse(inspect.getsource(ops)).body if isinstance(n, ast.FunctionDef) and n.name == "clip_tags")
    assert "ws" not in [a.arg for a in fn.args.args + fn.args.kwonlyargs]
    called = {c.func.id for c in ast.walk(fn) if isinstance(c, ast.Call) and isinstance(c.func, ast.Name)}
    assert "_ws" not in called
    assert [a.arg for a in fn.args.args] == ["x", "text_rows", "num_fg", "scale", "thre", "kmax", "want_scores"]
    assert [ast.literal_eval(d) for d in fn.args.defaults] == [100.0, 0.2, 6, True]


def test_entry_refuses_bad_arguments_before_any_launch():
    """EXCEL_ERR_ARG comes from host-side checks: no device is needed to see them (the pointers are never dereferenced)."""
    from excel_amd import _lib
    lib = _lib.lib()
    ok = dict(x=0x1000, stride=512, text=0x2000, B=2, C=512, T=45, F=20, scale=100.0, thre=0.2, kmax=6, onehot=0x3000, scores=0x4000)

    def call(**kw):
        a = dict(ok, **kw)
        return lib.excel_clip_tags(a["x"], a["stride"], a["text"], a["B"], a["C"], a["T"], a["F"], a["scale"], a["thre"], a["kmax"],
                                   a["onehot"], a["scores"], None)
    for bad in (dict(F=0), dict(F=46), dict(T=513, F=20), dict(T=512, F=255, kmax=6), dict(C=510, stride=512), dict(C=1028, stride=1028),
                dict(stride=508), dict(stride=514), dict(x=0x1004), dict(text=0x2008), dict(kmax=0), dict(kmax=21), dict(thre=-0.1),
                dict(thre=1.5), dict(scale=0.0), dict(scale=-1.0), dict(B=0), dict(onehot=None), dict(x=None), dict(thre=float("nan"))):
        assert call(**bad) == -1, bad
        assert b"clip_tags" in lib.excel_last_error()


# ------------------------------------------------------------------ flags
def _args(*extra):
    from excel_amd.tools import infer_lam
    return infer_lam.get_parser().parse_args(["--batch_size", "3", "--num_workers", "0", "--backend", "gloo"] + list(extra))


def test_flag_defaults_live_in_the_parser():
    from types import SimpleNamespace
    from excel_amd.tools import infer_lam
    a = infer_lam.get_parser().parse_args([])
    assert (a.tags, a.tag_thre, a.tag_max, a.tag_scale, a.save_tags, a.unlabeled) == ("labels", 0.2, 6, 100.0, None, False)
    b = infer_lam.flag_defaults(SimpleNamespace())
    assert (b.tags, b.tag_thre, b.tag_max, b.tag_scale, b.save_tags, b.unlabeled) == ("labels", 0.2, 6, 100.0, None, False)
    with pytest.raises(SystemExit):
        infer_lam.get_parser().parse_args(["--tags", "guess"])


def test_resolve_tags():
    from excel_amd.tools.infer_lam import resolve_tags
    assert resolve_tags(_args()) is None
    assert resolve_tags(_args("--tags", "labels", "--tag_max", "999", "--tag_thre", "7")) is None      # unread without --tags clip
    assert resolve_tags(_args("--tags", "clip")) == dict(thre=0.2, kmax=6, scale=100.0)
    assert resolve_tags(_args("--tags", "clip", "--tag_thre", "0", "--tag_max", "20", "--tag_scale", "50")) == dict(thre=0.0, kmax=20, scale=50.0)
    assert resolve_tags(_args("--tags", "clip", "--tag_thre", "1", "--tag_max", "1")) == dict(thre=1.0, kmax=1, scale=100.0)
    assert resolve_tags(_args("--tags", "clip", "--cam_flip", "true", "--cam_scales", "1.0,0.5", "--conf_label", "true", "--save_label", "true",
                              "--overflow_guard", "rerun")) is not None
    ok = _args("--unlabeled", "true", "--data_folder", "/nowhere", "--list_folder", "/nowhere", "--tags", "clip", "--save_tags", "/nowhere/t.npy")
    assert resolve_tags(ok) == dict(thre=0.2, kmax=6, scale=100.0)
    assert resolve_tags(_args("--unlabeled", "true", "--data_folder", "/nowhere", "--list_folder", "/nowhere", "--save_label", "true")) is None
    assert resolve_tags(_args("--unlabeled", "true", "--conf_label", "true"), have_dataset=True) is None


REFUSED = [
    (("--tags", "clip", "--training_free", "false"), "--training_free"),
    (("--tags", "clip", "--api_path", "true"), "--api_path"),
    (("--tags", "clip", "--save_cam", "true"), "--save_cam"),
    (("--tags", "clip", "--crf_post", "true"), "--crf_post"),
    (("--tags", "clip", "--crf_inline", "true"), "--crf_inline"),
    (("--tags", "clip", "--tag_max", "0"), "--tag_max"),
    (("--tags", "clip", "--tag_max", "21"), "--tag_max"),
    (("--tags", "clip", "--num_classes", "5", "--tag_max", "5"), "--tag_max"),
    (("--tags", "clip", "--tag_thre", "-0.01"), "--tag_thre"),
    (("--tags", "clip", "--tag_thre", "1.01"), "--tag_thre"),
    (("--tags", "clip", "--tag_scale", "0"), "--tag_scale"),
    (("--unlabeled", "true", "--save_label", "true"), "--synthetic"),
    (("--unlabeled", "true", "--data_folder", "/nowhere", "--save_label", "true"), "--list_folder"),
    (("--unlabeled", "true", "--data_folder", "/nowhere", "--list_folder", "/nowhere", "--save_label", "true", "--crf_post", "true"), "--crf_post"),
    (("--unlabeled", "true", "--data_folder", "/nowhere", "--list_folder", "/nowhere", "--save_label", "true", "--api_path", "true"), "--api_path"),
    (("--unlabeled", "true", "--data_folder", "/nowhere", "--list_folder", "/nowhere"), "--save_tags"),
    (("--save_tags", "/nowhere/t.npy"), "--tags clip"),
]


@pytest.mark.parametrize("flags,named", REFUSED, ids=[" ".join(f) for f, _ in REFUSED])
def test_validate_refuses_before_a_device_or_a_model_is_touched(monkeypatch, flags, named):
    from excel_amd.model import model_excel
    from excel_amd.tools import infer_lam

    def never(*a, **k):
        raise AssertionError("touched before the flags were checked")
    monkeypatch.setattr(model_excel, "ExCEL_model", never)
    monkeypatch.setattr(torch.cuda, "set_device", never)
    monkeypatch.setattr(infer_lam.dist, "init_process_group", never)
    with pytest.raises(ValueError) as e:
        infer_lam.validate(_args(*flags))
    assert named in str(e.value), str(e.value)
    if "--save_cam" in flags or "--crf_post" in flags and "--tags" in flags:
        assert "--save_tags" in str(e.value) and "--tags labels" in str(e.value)          # the two-run route is named


def test_tags_labels_leaves_validate_as_it_was(monkeypatch):
    """The default resolves to no tagger, and the flags that only --tags clip reads change nothing: the same steps, the same matrix."""
    from excel_amd.tools import infer_lam
    ds = _TagSet(7)
    runs = []
    for extra in ((), ("--tags", "labels", "--tag_max", "3", "--tag_thre", "0.9")):
        pipe = _TagStub()
        _, total = infer_lam.validate(_args("--overflow_guard", "off", *extra), dataset=ds, pipe=pipe)
        assert pipe.ticket_looks == 0 and infer_lam.validate.last_tags is None and infer_lam.build_validation.last_tags is None
        runs.append((pipe.log, total.numpy()))
    assert runs[0][0] == runs[1][0] and np.array_equal(runs[0][1], runs[1][1]) and runs[0][1].sum() > 0
    # the present-class check of the labelled path is still there
    with pytest.raises(RuntimeError, match="present classes"):
        infer_lam.validate(_args("--overflow_guard", "off"), dataset=_TagSet(7, k=3), pipe=_TagStub())


# ------------------------------------------------------------------ pipeline constructors
def test_pipeline_constructors_validate_the_tagger():
    from excel_amd import pipeline as P
    p = P.TrainingFreePipeline(None, smax=4, tagger=dict(thre=0.3, kmax=4, scale=50.0))
    assert p.tagger == dict(thre=0.3, kmax=4, scale=50.0) and p.last_tags is None and p.last_tag_ticket is None
    assert P.TrainingFreePipeline(None, smax=4, tagger={}).tagger == dict(thre=0.2, kmax=4, scale=100.0)
    assert P.TrainingFreePipeline(None).tagger is None
    for bad in (dict(kmax=5), dict(kmax=3), dict(thre=-0.1, kmax=4), dict(thre=1.1, kmax=4), dict(scale=0.0, kmax=4), dict(kmax=4, top=1), "clip"):
        with pytest.raises(ValueError, match="tagger"):
            P.TrainingFreePipeline(None, smax=4, tagger=bad)
    with pytest.raises(ValueError, match="tagger"):
        P.TrainingFreePipeline(None, num_classes=5, smax=6, tagger=dict(kmax=6))        # more tags than foreground classes
    for cls in (P.OptimisedLamPipeline, P.ValidationPipeline):
        with pytest.raises(ValueError, match="tagger"):
            cls(None, tagger=dict(kmax=6))
    x = torch.zeros(2, 3, 32, 32)
    for name in ("run_batch_split", "run_batch_overlapped"):
        with pytest.raises(ValueError, match="tagger"):
            getattr(p, name)(x, None)


def test_run_batch_signatures_did_not_change():
    from excel_amd.pipeline import TrainingFreePipeline as T
    assert list(inspect.signature(T.run_batch).parameters) == ["self", "inputs", "cls_labels", "gts", "label_hw", "return_intermediates"]
    assert list(inspect.signature(T.run_batch_ragged).parameters) == ["self", "hwc_packed", "plan", "cls_labels", "gts_packed", "S",
                                                                      "return_intermediates", "conf"]


# ------------------------------------------------------------------ metrics
def test_multilabel_score_matches_sklearn():
    metrics = pytest.importorskip("sklearn.metrics")
    from excel_amd.utils.evaluate import multilabel_score
    rs = np.random.RandomState(3)
    rows = [(rs.rand(20) < 0.2, rs.rand(20) < 0.2) for _ in range(40)]
    rows += [(np.zeros(20, bool), np.zeros(20, bool)), (np.zeros(20, bool), rows[0][1]), (rows[1][0], np.zeros(20, bool)), (rows[2][0], rows[2][0])]
    for t, p in rows:
        want = metrics.f1_score(t.astype(int), p.astype(int), zero_division=0)
        assert multilabel_score(t.astype(np.float32), p.astype(np.float32)) == pytest.approx(want, abs=1e-15)


def test_multilabel_score_by_hand():
    from excel_amd.utils.evaluate import multilabel_score
    assert multilabel_score([1, 1, 0, 0], [1, 0, 1, 0]) == 0.5           # TP 1, FP 1, FN 1
    assert multilabel_score([0, 0, 0], [0, 0, 0]) == 0.0
    assert multilabel_score([1, 0, 1], [1, 0, 1]) == 1.0
    assert multilabel_score([0, 0, 1], [1, 1, 0]) == 0.0


def test_tag_score_arithmetic_on_a_hand_made_example():
    from excel_amd.tools.infer_lam import format_scores_table, tag_report
    rows = {"a": [1, 0, 0], "b": [1, 1, 0], "c": [0, 1, 0], "d": [1, 0, 0], "e": [0, 0, 1]}
    truth = {"a": [1, 0, 0], "b": [1, 0, 0], "c": [1, 1, 0], "d": [0, 0, 0]}            # "e" has no labels: counted, not scored
    rep = tag_report({k: np.asarray(v, np.float32) for k, v in rows.items()}, {k: np.asarray(v, np.float32) for k, v in truth.items()}, 3)
    assert rep["images"] == 5 and rep["scored"] == 4 and rep["tags_per_image"] == [0, 4, 1]
    assert rep["per_class_counts"] == [[2, 1, 1], [1, 1, 0], [0, 0, 0]]                  # (TP, FP, FN) per class
    assert rep["counts"] == {"tp": 3, "fp": 2, "fn": 1, "tn": 6} and sum(rep["counts"].values()) == 4 * 3
    sc = rep["score"]
    assert list(sc["precision"].values()) == [2 / 3, 0.5, 0.0] and list(sc["recall"].values()) == [2 / 3, 1.0, 0.0]
    assert list(sc["f1"].values()) == pytest.approx([2 / 3, 2 / 3, 0.0])
    assert sc["micro"] == pytest.approx({"precision": 3 / 5, "recall": 3 / 4, "f1": 6 / 9})
    assert rep["image_f1"] == pytest.approx((1.0 + 2 / 3 + 2 / 3 + 0.0) / 4)
    tab = format_scores_table(sc, ["x", "y", "z"], metric_names=("precision", "recall", "f1"))
    assert "f1" in tab.splitlines()[1] and "| y " in tab and "average_metrics" in tab
    empty = tag_report({}, {}, 3)
    assert empty["images"] == 0 and empty["score"] is None and empty["tags_per_image"] == []
    nolab = tag_report({"a": np.asarray([1, 1, 0], np.float32)}, {}, 3)
    assert nolab["tags_per_image"] == [0, 0, 1] and nolab["scored"] == 0 and nolab["counts"] is None


# ------------------------------------------------------------------ data and file format
def _image_tree(root, names, with_labels=None):
    from PIL import Image
    os.makedirs(os.path.join(root, "JPEGImages"))
    os.makedirs(os.path.join(root, "lists"))
    rs = np.random.RandomState(5)
    for i, n in enumerate(names):
        arr = rs.randint(0, 256, (20 + 3 * i, 17 + 2 * i, 3)).astype(np.uint8)
        (Image.fromarray(arr) if i != 1 else Image.fromarray(arr[..., 0])).save(os.path.join(root, "JPEGImages", n + ".jpg"))
    with open(os.path.join(root, "lists", "train.txt"), "w") as f:
        f.write("\n".join(names) + "\n")
    if with_labels is not None:
        np.save(os.path.join(root, "lists", "cls_labels_onehot.npy"), with_labels, allow_pickle=True)
    return os.path.join(root, "lists")


def test_image_list_dataset(tmp_path):
    from excel_amd.datasets.images import ImageListDataset
    from excel_amd.datasets.loader import pack_samples
    names = ["im_a", "im_b", "im_c"]
    lists = _image_tree(str(tmp_path), names)
    ds = ImageListDataset(str(tmp_path), lists, split="train", num_fg=7)
    assert len(ds) == 3 and ds.max_k() == 1 and ds.has_cls_labels is False
    for i, n in enumerate(names):
        name, img, lab, cls = ds[i]
        assert name == n and lab is None and img.dtype == np.uint8 and img.shape == (20 + 3 * i, 17 + 2 * i, 3)     # (im_b: a grey JPEG)
        assert cls.dtype == np.float32 and cls.shape == (7,) and not cls.any()
    rb = pack_samples([ds[i] for i in range(3)])
    assert rb.labels is None and rb.hw.tolist() == [[20, 17], [23, 19], [26, 21]]
    assert not os.path.exists(os.path.join(str(tmp_path), "SegmentationClassAug"))
    labels = {n: np.eye(7, dtype=np.float32)[i] + np.eye(7, dtype=np.float32)[6] * (i == 2) for i, n in enumerate(names)}
    ds = ImageListDataset(str(tmp_path), lists, split="train", num_fg=7, label_list=labels)
    assert ds.max_k() == 2 and ds.has_cls_labels and np.array_equal(ds[2][3], labels["im_c"]) and ds[2][2] is None
    with pytest.raises(KeyError, match="im_c"):
        ImageListDataset(str(tmp_path), lists, split="train", num_fg=7, label_list={n: labels[n] for n in names[:2]})
    with pytest.raises(ValueError, match="foreground"):
        ImageListDataset(str(tmp_path), lists, split="train", num_fg=9, label_list=labels)


def test_save_tags_round_trip(tmp_path):
    from excel_amd.datasets.voc import load_cls_label_list
    from excel_amd.tools.infer_lam import save_tags_file
    rows = {"b": np.asarray([0, 1, 1], np.float64), "a": np.asarray([1, 0, 0], np.float32)}
    path = os.path.join(str(tmp_path), "lists", "cls_labels_onehot.npy")
    save_tags_file(path, rows)
    save_tags_file(path, rows)                                                            # overwrites in one step
    back = load_cls_label_list(os.path.dirname(path))
    assert sorted(back) == ["a", "b"] and all(v.dtype == np.float32 and v.shape == (3,) for v in back.values())
    assert back["b"].tolist() == [0, 1, 1] and os.listdir(os.path.dirname(path)) == ["cls_labels_onehot.npy"]


def test_voc_dataset_takes_optional_image_level_labels(tmp_path):
    from PIL import Image
    from excel_amd.datasets import voc
    lists = _image_tree(str(tmp_path), ["v0", "v1"])
    os.makedirs(os.path.join(str(tmp_path), "SegmentationClassAug"))
    for i, n in enumerate(["v0", "v1"]):
        Image.fromarray(np.zeros((20 + 3 * i, 17 + 2 * i), np.uint8)).save(os.path.join(str(tmp_path), "SegmentationClassAug", n + ".png"))
    with pytest.raises(FileNotFoundError):
        voc.VOC12SegDataset(str(tmp_path), lists, split="train", stage="val")
    ds = voc.VOC12SegDataset(str(tmp_path), lists, split="train", stage="val", cls_labels_optional=True, num_fg=5)
    assert ds.has_cls_labels is False and ds[1][3].shape == (5,) and ds[1][2].shape == (23, 19)
    np.save(os.path.join(lists, "cls_labels_onehot.npy"), {"v0": np.eye(5, dtype=np.float32)[0], "v1": np.eye(5, dtype=np.float32)[3]}, allow_pickle=True)
    ds = voc.VOC12SegDataset(str(tmp_path), lists, split="train", stage="val", cls_labels_optional=True, num_fg=5)
    assert ds.has_cls_labels and ds[1][3].tolist() == [0, 0, 0, 1, 0]


def test_coco_dataset_takes_optional_image_level_labels(tmp_path):
    from PIL import Image
    from excel_amd.datasets import coco
    root, lists = tmp_path / "COCO", tmp_path / "lists"
    for d in ("JPEGImages/val", "SegmentationClass/val"):
        (root / d).mkdir(parents=True)
    lists.mkdir()
    name = "COCO_val2014_000000000042"
    Image.fromarray(np.zeros((18, 22, 3), np.uint8)).save(root / "JPEGImages/val" / (name + ".jpg"))
    Image.fromarray(np.zeros((18, 22), np.uint8)).save(root / "SegmentationClass/val" / "000000000042.png")
    (lists / "val.txt").write_text(name + "\n")
    with pytest.raises(FileNotFoundError):
        coco.CocoSegDataset(str(root), str(lists), split="val", stage="val")
    ds = coco.CocoSegDataset(str(root), str(lists), split="val", stage="val", cls_labels_optional=True)
    assert ds.has_cls_labels is False and ds[0][3].shape == (80,) and not ds[0][3].any() and ds[0][2].shape == (18, 22)
    oh = np.zeros(80, np.float32)
    oh[[0, 79]] = 1
    np.save(lists / "cls_labels_onehot.npy", {name: oh})
    ds = coco.CocoSegDataset(str(root), str(lists), split="val", stage="val", cls_labels_optional=True)
    assert ds.has_cls_labels and np.array_equal(ds[0][3], oh)


# ------------------------------------------------------------------ the control flow, through a stub
F_STUB = 20


class _TagSet:
    """(name, image u8 [h,w,3], label u8 [h,w] or None, cls f32 [20]); byte 0 of an image is its data set index."""

    def __init__(self, n, labelled=True, has_cls=True, k=1):
        self.n, self.labelled, self.has_cls_labels, self.k = n, labelled, has_cls, k

    def __len__(self):
        return self.n

    def max_k(self):
        return 2

    def __getitem__(self, i):
        i = int(i)
        rs = np.random.RandomState(700 + i)
        h, w = 5 + i % 7, 4 + (3 * i) % 5
        img = rs.randint(0, 256, (h, w, 3)).astype(np.uint8)
        img[0, 0, 0] = i
        gt = rs.randint(0, 21, (h, w)).astype(np.uint8) if self.labelled else None
        cls = np.zeros(F_STUB, np.float32)
        if self.has_cls_labels:
            cls[[(i + j) % F_STUB for j in range(self.k)]] = 1
        return f"t{i:03d}", img, gt, cls


def _stub_tags(i, mode="fast"):
    """what the stub 'predicts' for image i: its own class, and for odd i a second one; image 4 in the fast mode: the NaN row's class 0"""
    row = np.zeros(F_STUB, np.float32)
    if i == 4 and mode == "fast":
        row[0] = 1
        return row
    row[i % F_STUB] = 1
    if i % 2:
        row[(i + 5) % F_STUB] = 1
    return row


class _TagTicket:
    def __init__(self, onehot, log, not_ready_polls):
        self._onehot, self._log, self._wait = onehot, log, not_ready_polls

    def ready(self):
        self._log.append(("tag_poll",))
        if self._wait > 0:
            self._wait -= 1
            return False
        return True

    def tags(self):
        self._log.append(("tag_read", self._onehot.shape[0]))
        return self._onehot, np.zeros_like(self._onehot)


class _GuardTicket:
    def __init__(self, flags):
        self._flags = np.asarray(flags, np.int32)

    def ready(self):
        return True

    def flags(self):
        return self._flags


class _TagStub:
    """Stands in for a pipeline with a tagger: records its steps (and what it was given as cls / gts), leaves a tag ticket that says
    "not ready" on its first poll, and with a guard flags image 4 in the fast mode."""
    device, smax = "cpu", 2

    def __init__(self, guard=None):
        import contextlib
        self.guard, self.mode, self.hist, self.log = guard, "fast", None, []
        self.ticket_looks = 0
        self._ticket = self.last_guard = None
        self._ctx = contextlib

    @property
    def last_tag_ticket(self):
        self.ticket_looks += 1
        return self._ticket

    def exact_mode(self):
        stub = self

        @self._ctx.contextmanager
        def cm():
            stub.mode = "exact"
            try:
                yield stub
            finally:
                stub.mode = "fast"
        return cm()

    def run_batch_ragged(self, images, plan, cls, gts, S=448, return_intermediates=False):
        px = images.view(-1, 3).numpy()
        idx = [int(px[int(plan.loff[b]), 0]) for b in range(plan.B)]
        self.log.append(("step", self.mode, tuple(idx), gts is None))
        self._ticket = _TagTicket(np.stack([_stub_tags(i, self.mode) for i in idx]), self.log, not_ready_polls=1)
        if self.guard is not None:
            self.last_guard = _GuardTicket([1 if (i == 4 and self.mode == "fast") else 0 for i in idx])
        if gts is not None:
            self.hist += torch.eye(self.hist.shape[0], dtype=torch.int64) * plan.B
        return torch.from_numpy((px[:, 0] % 21).astype(np.uint8))


def test_unlabeled_clip_loop_collects_the_tags_without_waiting(tmp_path):
    from excel_amd.datasets.voc import load_cls_label_list
    from excel_amd.tools import infer_lam
    n = 8
    out = os.path.join(str(tmp_path), "tags", "cls_labels_onehot.npy")
    pipe = _TagStub()
    score, total = infer_lam.validate(_args("--unlabeled", "true", "--tags", "clip", "--save_tags", out, "--overflow_guard", "off"),
                                      dataset=_TagSet(n, labelled=False, has_cls=False, k=9), pipe=pipe)     # (k = 9 > smax: nobody checks it)
    assert score is None and int(total.sum()) == 0
    steps = [e for e in pipe.log if e[0] == "step"]
    assert steps == [("step", "fast", (0, 1, 2), True), ("step", "fast", (3, 4, 5), True), ("step", "fast", (6, 7), True)]   # labels=None
    # no wait inside the loop: the first ticket is read only after the second step was enqueued
    first_read = next(i for i, e in enumerate(pipe.log) if e[0] == "tag_read")
    assert first_read > pipe.log.index(steps[1])
    rep = infer_lam.validate.last_tags
    assert rep["images"] == n and rep["scored"] == 0 and rep["score"] is None and rep["tags_per_image"] == [0, 4, 4]
    back = load_cls_label_list(os.path.dirname(out))
    assert sorted(back) == [f"t{i:03d}" for i in range(n)]
    for i in range(n):
        assert back[f"t{i:03d}"].dtype == np.float32 and np.array_equal(back[f"t{i:03d}"], _stub_tags(i))


def test_labelled_clip_loop_scores_the_tags_and_the_rerun_replaces_rows(tmp_path):
    import json
    from excel_amd.tools import infer_lam
    n = 7
    out, js = os.path.join(str(tmp_path), "t.npy"), os.path.join(str(tmp_path), "run.json")
    pipe = _TagStub(guard="skip")
    score, total = infer_lam.validate(_args("--tags", "clip", "--save_tags", out, "--overflow_guard", "rerun", "--json_out", js),
                                      dataset=_TagSet(n), pipe=pipe)
    steps = [e for e in pipe.log if e[0] == "step"]
    assert steps[-1] == ("step", "exact", (4,), False) and len(steps) == 4
    rep = infer_lam.validate.last_tags
    assert np.array_equal(rep["rows"]["t004"], _stub_tags(4, "exact")) and not np.array_equal(_stub_tags(4, "exact"), _stub_tags(4, "fast"))
    # truth = class i; predicted = class i (+ a second one for odd i): TP n, FP 3, FN 0
    assert rep["images"] == rep["scored"] == n and rep["counts"] == {"tp": 7, "fp": 3, "fn": 0, "tn": n * F_STUB - 10}
    assert sum(rep["counts"].values()) == n * F_STUB
    assert rep["score"]["micro"]["recall"] == 1.0 and rep["score"]["micro"]["precision"] == pytest.approx(0.7)
    assert rep["image_f1"] == pytest.approx((4 * 1.0 + 3 * (2 / 3)) / 7)
    assert score is not None and int(total.sum()) > 0
    rec = json.load(open(js))["tags"]
    assert rec["counts"] == rep["counts"] and rec["tags_per_image"] == [0, 4, 3] and rec["kmax"] == 6 and len(rec["per_class"]["f1"]) == F_STUB
    saved = np.load(out, allow_pickle=True).item()
    assert np.array_equal(saved["t004"], _stub_tags(4, "exact"))


def test_clip_loop_needs_a_ticket():
    from excel_amd.tools import infer_lam

    class NoTicket(_TagStub):
        last_tag_ticket = None
    with pytest.raises(RuntimeError, match="last_tag_ticket"):
        infer_lam.validate(_args("--tags", "clip", "--overflow_guard", "off"), dataset=_TagSet(3), pipe=NoTicket())


# ------------------------------------------------------------------ two ranks on gloo, one shard empty
def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _tag_worker(rank, world, port, out_dir, q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(rank))
    import torch.distributed as dist
    from excel_amd.tools import infer_lam
    res = {}
    for n in (1, 5):                                                                        # n = 1: rank 1's shard is empty
        pipe = _TagStub()
        infer_lam.validate(_args("--unlabeled", "true", "--tags", "clip", "--save_tags", os.path.join(out_dir, f"tags{n}.npy"), "--overflow_guard", "off"),
                           dataset=_TagSet(n, labelled=False, has_cls=False), pipe=pipe)
        res[n] = ([e[2] for e in pipe.log if e[0] == "step"], sorted(infer_lam.validate.last_tags["rows"]))
    dist.barrier()
    q.put((rank, res))
    dist.barrier()
    dist.destroy_process_group()


def test_world2_every_rank_joins_the_one_gather_and_rank0_writes(tmp_path):
    import torch.multiprocessing as mp
    world = 2
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_tag_worker, args=(r, world, port, str(tmp_path), q)) for r in range(world)]
    for p in procs:
        p.start()
    res = dict(q.get(timeout=180) for _ in range(world))
    for p in procs:
        p.join(60)
        assert p.exitcode == 0
    assert res[0][1] == ([(0,)], ["t000"]) and res[1][1] == ([], ["t000"])                  # the empty shard ran no step and still joined
    assert res[0][5][0] == [(0, 2, 4)] and res[1][5][0] == [(1, 3)]
    assert res[0][5][1] == res[1][5][1] == [f"t{i:03d}" for i in range(5)]
    for n in (1, 5):
        saved = np.load(os.path.join(str(tmp_path), f"tags{n}.npy"), allow_pickle=True).item()
        assert sorted(saved) == [f"t{i:03d}" for i in range(n)]
        assert all(np.array_equal(saved[f"t{i:03d}"], _stub_tags(i)) for i in range(n))
    assert sorted(os.listdir(str(tmp_path))) == ["tags1.npy", "tags5.npy"]
