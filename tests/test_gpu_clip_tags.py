"""GPU tests of the predicted image tags: ops.clip_tags (excel_clip_tags) against the float64 restatement of its definition over the
case table of tests/_clip_tags_ref.py, the pipeline wiring on the tiny network of the pipeline tests, and tools/infer_lam
--tags clip / --unlabeled / --save_tags on tiny on-disk trees.

Score tolerance: per case, 16 times the error the float32 numpy evaluation of the same inputs has against float64 (the factor covers
another summation order and another exp, not orders of magnitude), and in any case the derived bound 6 * scale * C * 2^-24, both
relative to the image's top score.  Measured kernel errors (MI355X) are recorded in EXPERIMENTS.md."""
import os
import shutil
import sys

import numpy as np
import pytest

from oracle.vit import VitConfig, make_vit_weights

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _clip_tags_ref as R  # noqa: E402
import _scratch as S  # noqa: E402

TINY = VitConfig(width=128, layers=8, heads=2, patch=16, out_dim=64, input_resolution=64, n_surgery=5)
TINY_KW = dict(width=128, layers=8, heads=2, patch=16, output_dim=64, input_resolution=64)


@pytest.fixture(scope="module")
def gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import excel_amd.ops  # noqa: F401  (raises if libexcel_hip.so is missing: no fallback)
    return True


def dev(a):
    return torch.as_tensor(np.ascontiguousarray(a)).cuda()


def host(t):
    return t.detach().cpu().numpy()


def _check(name, x, text, F, scale, thre, kmax, x_dev=None, min_margin=R.MIN_MARGIN):
    """ops.clip_tags on (x, text) against the float64 reference: exact one-hot rows, scores within the measured tolerance, the same
    bits from a second call and from outputs that start as 0xFF bytes.  -> (kernel error, float32 numpy error)"""
    from excel_amd import ops
    ref_onehot, ref_s = R.clip_tags_ref(x, text, F, scale, thre, kmax)
    assert R.margin(ref_s, thre, kmax) >= min_margin
    _, s32 = R.clip_tags_ref(x, text, F, scale, thre, kmax, dtype=np.float32)
    err32 = R.score_error(s32, ref_s)
    xd, td = dev(x) if x_dev is None else x_dev, dev(text)
    onehot, scores = ops.clip_tags(xd, td, F, scale=scale, thre=thre, kmax=kmax)
    again = ops.clip_tags(xd, td, F, scale=scale, thre=thre, kmax=kmax)
    with S.poisoned_allocations(0xFF):
        poisoned = ops.clip_tags(xd, td, F, scale=scale, thre=thre, kmax=kmax)
    only, none = ops.clip_tags(xd, td, F, scale=scale, thre=thre, kmax=kmax, want_scores=False)
    torch.cuda.synchronize()
    assert onehot.dtype == scores.dtype == torch.float32 and tuple(onehot.shape) == tuple(scores.shape) == (x.shape[0], F)
    err = R.score_error(host(scores), ref_s)
    print(f"clip_tags {name}: kernel score error {err:.3g} of the top score (float32 numpy {err32:.3g}, allowed {16 * err32:.3g}, "
          f"bound {R.score_bound(scale, x.shape[-1]):.3g}), margin {R.margin(ref_s, thre, kmax):.3g}")
    assert np.array_equal(host(onehot), ref_onehot)
    assert err <= 16 * err32 and err <= R.score_bound(scale, x.shape[-1])
    for other in (again, poisoned):
        assert torch.equal(other[0].view(torch.int32), onehot.view(torch.int32)) and torch.equal(other[1].view(torch.int32), scores.view(torch.int32))
    assert none is None and torch.equal(only, onehot)
    return err, err32


@pytest.mark.parametrize("name", sorted(R.CASES))
def test_clip_tags_matches_the_float64_definition(gpu, name):
    x, text, F, scale, thre, kmax = R.make_case(name)
    _check(name, x, text, F, scale, thre, kmax)


def test_clip_tags_reads_row_zero_of_every_image(gpu):
    """the [B,N,C] form (N = 5): the stride is N * C and rows 1..4 are never read - NaNs there change nothing"""
    x, text, F, scale, thre, kmax = R.make_case("voc")
    x3 = np.full((x.shape[0], 5, x.shape[1]), np.nan, np.float32)
    x3[:, 0] = x
    a, _ = _check("voc [B,5,C]", x, text, F, scale, thre, kmax, x_dev=dev(x3))
    b, _ = _check("voc [B,C]", x, text, F, scale, thre, kmax)
    assert a == b


def test_clip_tags_tie_goes_to_the_lower_index(gpu):
    """two identical text rows, the best two of every image, with the cut (kmax = 1) between them: bit-identical scores, index 3 wins"""
    from excel_amd import ops
    rs = np.random.RandomState(11)
    B, C, T, F = 3, 128, 12, 9
    text = rs.standard_normal((T, C)).astype(np.float32)
    text[7] = text[3]
    x = (text[3][None] + 0.3 * rs.standard_normal((B, C))).astype(np.float32)
    ref, s = R.clip_tags_ref(x, text, F, 20.0, 0.0, 1)
    assert (s[:, 3] == s[:, 7]).all() and (s.argmax(1) == 3).all() and (ref[:, 3] == 1).all() and (ref.sum(1) == 1).all()
    _check("tie", x, text, F, 20.0, 0.0, 1)
    _, scores = ops.clip_tags(dev(x), dev(text), F, scale=20.0, thre=0.0, kmax=1)
    assert torch.equal(scores[:, 3].view(torch.int32), scores[:, 7].view(torch.int32))
    # ... and with room for both, both are tagged (thre = 1: only a score equal to the best passes)
    onehot2, _ = ops.clip_tags(dev(x), dev(text), F, scale=20.0, thre=1.0, kmax=2)
    want = np.zeros((B, F), np.float32)
    want[:, [3, 7]] = 1
    assert np.array_equal(host(onehot2), want) and np.array_equal(R.clip_tags_ref(x, text, F, 20.0, 1.0, 2)[0], want)


def test_clip_tags_nonfinite_row_gives_class_zero(gpu):
    """one image with an inf entry: class 0 and NaN scores for it, the other rows as without it"""
    from excel_amd import ops
    x, text, F, scale, thre, kmax = R.make_case("voc")
    clean = ops.clip_tags(dev(x), dev(text), F, scale=scale, thre=thre, kmax=kmax)
    for poison in (np.inf, -np.inf, np.nan):
        xb = x.copy()
        xb[1, 77] = poison
        _check(f"row 1 holds {poison}", xb, text, F, scale, thre, kmax)
        onehot, scores = ops.clip_tags(dev(xb), dev(text), F, scale=scale, thre=thre, kmax=kmax)
        assert host(onehot)[1].tolist() == [1.0] + [0.0] * (F - 1) and bool(torch.isnan(scores[1]).all())
        for b in (0, 2):
            assert torch.equal(onehot[b], clean[0][b]) and torch.equal(scores[b].view(torch.int32), clean[1][b].view(torch.int32))
    xz = x.copy()
    xz[2] = 0                                                # a zero row: 0 / 0
    onehot, scores = ops.clip_tags(dev(xz), dev(text), F, scale=scale, thre=thre, kmax=kmax)
    assert host(onehot)[2].tolist() == [1.0] + [0.0] * (F - 1) and bool(torch.isnan(scores[2]).all())


def test_clip_tags_refuses_what_the_header_lists(gpu):
    from excel_amd import ops
    x, text = torch.zeros(2, 64, device="cuda"), torch.zeros(9, 64, device="cuda")
    for kw in (dict(num_fg=10), dict(num_fg=0), dict(num_fg=4, kmax=5), dict(num_fg=4, kmax=0), dict(num_fg=4, kmax=2, thre=1.5),
               dict(num_fg=4, kmax=2, scale=0.0)):
        with pytest.raises(RuntimeError, match="clip_tags"):
            ops.clip_tags(x, text, **kw)
    with pytest.raises(RuntimeError, match="clip_tags"):
        ops.clip_tags(torch.zeros(2, 62, device="cuda"), torch.zeros(9, 62, device="cuda"), 4, kmax=2)      # C % 4
    with pytest.raises(ValueError):
        ops.clip_tags(x, torch.zeros(9, 32, device="cuda"), 4, kmax=2)
    with pytest.raises(RuntimeError):
        ops.clip_tags(torch.zeros(2, 64), torch.zeros(9, 64), 4, kmax=2)                                      # no CPU fallback


# ------------------------------------------------------------------ pipeline wiring on the tiny network
F_TINY, KMAX = 4, 2


@pytest.fixture(scope="module")
def tiny(gpu):
    from excel_amd.model import ExCEL_model
    rs = np.random.RandomState(77)
    text = rs.standard_normal((9, 64)).astype(np.float32)
    text /= np.linalg.norm(text, axis=1, keepdims=True)
    model = ExCEL_model(clip_model="tiny", num_classes=F_TINY + 1, img_size=96, mode="train", state_dict=make_vit_weights(TINY, seed=11),
                        vit_cfg=TINY_KW, text_attr=text.T.copy(), gemm_mode="f32")
    sizes = [(70, 93), (96, 96), (120, 64), (51, 77), (88, 101)]
    imgs = [rs.randint(0, 256, (h, w, 3)).astype(np.uint8) for h, w in sizes]
    return model, text, sizes, imgs


def _pick_thre(model, x_raw, text, scale):
    """a relative threshold at which the float64 reference decides every class of these images with a margin of at least 1e-3"""
    _, s = R.clip_tags_ref(host(x_raw)[:, 0], text, F_TINY, scale, 0.0, KMAX)
    for thre in (0.2, 0.3, 0.1, 0.4, 0.5, 0.05, 0.6):
        if R.margin(s, thre, KMAX) >= R.MIN_MARGIN:
            return thre
    raise AssertionError("no threshold of the list separates the scores of the tiny network")


SCALE_TINY = 30.0       # the tiny random network's cosines are large: CLIP's 100 would make every image one-hot


@pytest.mark.parametrize("flip", [False, True], ids=["plain", "flip"])
def test_ragged_step_with_a_tagger_equals_the_step_fed_its_tags(tiny, flip):
    from excel_amd import ops
    from excel_amd.pipeline import TrainingFreePipeline
    model, text, sizes, imgs = tiny
    plan = ops.RaggedPlan(sizes, "cuda")
    packed = dev(np.concatenate([im.reshape(-1) for im in imgs]))
    inputs = ops.normalize_resize_u8_ragged(packed, plan, 96)
    model(inputs)
    thre = _pick_thre(model, model.last_x_raw, text, SCALE_TINY)
    tagged = TrainingFreePipeline(model, num_classes=F_TINY + 1, smax=KMAX, tta_flip=flip, tagger=dict(thre=thre, kmax=KMAX, scale=SCALE_TINY))
    labels = tagged.run_batch_ragged(packed, plan, None, None, S=96).clone()
    onehot, scores = tagged.last_tags
    # the tags are those of the un-mirrored scale-1.0 pass: model.last_x_raw is that pass's (attr_maps leaves it alone)
    x_raw = host(model.last_x_raw)
    assert x_raw.shape == (len(sizes), 37, 64)
    ref_onehot, ref_s = R.clip_tags_ref(x_raw[:, 0], text, F_TINY, SCALE_TINY, thre, KMAX)
    assert R.margin(ref_s, thre, KMAX) >= R.MIN_MARGIN
    assert np.array_equal(host(onehot), ref_onehot)
    assert R.score_error(host(scores), ref_s) <= R.score_bound(SCALE_TINY, 64)
    assert 1 <= ref_onehot.sum(1).min() and ref_onehot.sum(1).max() <= KMAX
    t_onehot, t_scores = tagged.last_tag_ticket.tags()
    assert np.array_equal(t_onehot, host(onehot)) and np.array_equal(t_scores, host(scores)) and tagged.last_tag_ticket.ready()
    plain = TrainingFreePipeline(model, num_classes=F_TINY + 1, smax=KMAX, tta_flip=flip)
    want = plain.run_batch_ragged(packed, plan, onehot.clone(), None, S=96)
    assert plain.last_tags is None and plain.last_tag_ticket is None
    assert torch.equal(labels, want)


def test_uniform_step_with_a_tagger_equals_the_step_fed_its_tags(tiny):
    from excel_amd.pipeline import TrainingFreePipeline
    model, text, _, _ = tiny
    rs = np.random.RandomState(5)
    inputs = dev(rs.standard_normal((3, 3, 96, 96)).astype(np.float32))
    gts = dev(rs.randint(0, F_TINY + 1, (3, 96, 96)).astype(np.uint8))
    model(inputs)
    thre = _pick_thre(model, model.last_x_raw, text, SCALE_TINY)
    tagged = TrainingFreePipeline(model, num_classes=F_TINY + 1, smax=KMAX, tagger=dict(thre=thre, kmax=KMAX, scale=SCALE_TINY))
    labels = tagged.run_batch(inputs, None, gts).clone()
    onehot, _ = tagged.last_tags
    ref_onehot, ref_s = R.clip_tags_ref(host(model.last_x_raw)[:, 0], text, F_TINY, SCALE_TINY, thre, KMAX)
    assert R.margin(ref_s, thre, KMAX) >= R.MIN_MARGIN and np.array_equal(host(onehot), ref_onehot)
    wrong = torch.ones_like(onehot)                           # the values of cls_labels are ignored with a tagger
    assert torch.equal(tagged.run_batch(inputs, wrong, None), labels)
    plain = TrainingFreePipeline(model, num_classes=F_TINY + 1, smax=KMAX)
    assert torch.equal(plain.run_batch(inputs, onehot.clone(), gts), labels)
    assert torch.equal(plain.hist, tagged.hist) and int(plain.hist.sum()) == 3 * 96 * 96


def test_model_keeps_x_raw_of_forward_only(tiny):
    model, text, _, _ = tiny
    rs = np.random.RandomState(6)
    a, b = (dev(rs.standard_normal((2, 3, 96, 96)).astype(np.float32)) for _ in range(2))
    model(a)
    kept = model.last_x_raw
    bits = kept.clone()
    model.attr_maps(b)
    assert model.last_x_raw is kept and torch.equal(kept, bits)
    onehot, scores = model.image_tags(thre=0.2, kmax=KMAX, scale=SCALE_TINY)
    again, _ = model.image_tags(thre=0.2, kmax=KMAX, scale=SCALE_TINY, x_raw=bits[:, 0].contiguous())       # the compact [B,C] form
    assert tuple(onehot.shape) == (2, F_TINY) and torch.equal(onehot, again)


# ------------------------------------------------------------------ the program on tiny on-disk trees
def _png_bytes(d):
    return {f: open(os.path.join(d, f), "rb").read() for f in sorted(os.listdir(d))}


def test_infer_lam_label_free_then_two_run_route(gpu, tmp_path, monkeypatch):
    """Run A predicts the tags of an images-only tree, writes labels and the tags file; run B reads that file as its labels and writes
    byte-identical PNGs.  On the labelled tree --tags clip prints both tables and its counts add up to images x F."""
    import json
    import logging
    from _clip_files import write_tiny_clip
    from excel_amd.datasets.voc import load_cls_label_list
    from excel_amd.tools import infer_lam, synthetic
    full, full_lists = tmp_path / "VOC2012", tmp_path / "lists"
    ids, _ = synthetic.write_voc_tree(str(full), str(full_lists), 7, seed=4, split="val")
    root, lists = tmp_path / "photos", tmp_path / "photo_lists"
    os.makedirs(root)
    os.makedirs(lists)
    shutil.copytree(full / "JPEGImages", root / "JPEGImages")
    shutil.copy(full_lists / "val.txt", lists / "val.txt")
    ckpt, bpe_path, _ = write_tiny_clip(tmp_path)
    monkeypatch.chdir(tmp_path)
    parse = infer_lam.get_parser().parse_args
    common = ["--infer_set", "val", "--resize_size", "128", "--model", ckpt, "--bpe_path", bpe_path, "--batch_size", "4", "--num_workers", "2"]
    here = common + ["--data_folder", str(root), "--list_folder", str(lists), "--unlabeled", "true", "--save_label", "true"]
    tags_file = lists / "cls_labels_onehot.npy"
    score, total = infer_lam.validate(parse(here + ["--tags", "clip", "--tag_max", "3", "--save_tags", str(tags_file), "--label_dir", str(tmp_path / "a")]))
    assert score is None and int(total.sum()) == 0
    rep = infer_lam.validate.last_tags
    assert rep["images"] == 7 and rep["scored"] == 0 and sum(rep["tags_per_image"]) == 7 and len(rep["tags_per_image"]) <= 4
    saved = load_cls_label_list(str(lists))
    assert sorted(saved) == sorted(ids) and all(v.dtype == np.float32 and v.shape == (20,) and 1 <= v.sum() <= 3 for v in saved.values())
    infer_lam.validate(parse(here + ["--tags", "labels", "--label_dir", str(tmp_path / "b")]))
    a, b = _png_bytes(tmp_path / "a"), _png_bytes(tmp_path / "b")
    assert sorted(a) == sorted(n + ".png" for n in ids) and a == b
    # --tags labels on an images-only tree without the file names the file
    os.remove(tags_file)
    with pytest.raises(FileNotFoundError, match="cls_labels_onehot.npy"):
        infer_lam.validate(parse(here + ["--label_dir", str(tmp_path / "c")]))
    # the labelled tree: both tables, the counts add up
    lines = []
    handler = logging.Handler()
    handler.emit = lambda record: lines.append(record.getMessage())
    logging.getLogger().addHandler(handler)
    level = logging.getLogger().level
    logging.getLogger().setLevel(logging.INFO)
    try:
        score, total = infer_lam.validate(parse(common + ["--data_folder", str(full), "--list_folder", str(full_lists), "--tags", "clip",
                                                          "--json_out", str(tmp_path / "run.json")]))
    finally:
        logging.getLogger().removeHandler(handler)
        logging.getLogger().setLevel(level)
    rep = infer_lam.validate.last_tags
    assert score is not None and int(total.sum()) > 0
    assert rep["images"] == rep["scored"] == 7 and sum(rep["counts"].values()) == 7 * 20
    assert rep["counts"]["tp"] + rep["counts"]["fp"] == sum(k * v for k, v in enumerate(rep["tags_per_image"]))
    assert 0.0 <= rep["image_f1"] <= 1.0
    text = "\n".join(lines)
    assert "LAM_score:" in text and "tag_score:" in text and "mean image F1" in text
    assert json.load(open(tmp_path / "run.json"))["tags"]["counts"] == rep["counts"]
