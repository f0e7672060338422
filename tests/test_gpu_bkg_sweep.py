"""Background-scale sweep on the GPU: excel_bkg_sweep_ragged (bkgsweep.hip) against its numpy restatement (utils/bkg_sweep.
sweep_reference), integer for integer - counts and labels are integers, so there is no tolerance and no excluded pixel -, at sizes around
the kernel's 64 x 16 tile, every class count and number of scales its LDS is sized for, ties, pixels whose mask is no prefix, skip flags
and accumulation; its refusals, its stream contract; then the pipeline's bkg_sweep / bkg_scale and infer_lam's --bkg_sweep end to end."""
import ctypes as C
import json
import logging
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _streams as St  # noqa: E402

# 1 x 1; smaller than a tile; exactly one tile; one pixel into the next tile both ways; W no multiple of 4, several tiles
SIZES = [(1, 1), (3, 5), (16, 64), (17, 65), (40, 151)]
SCALES16 = (0.125, 0.25, 0.375, 0.5, 0.625, 0.75, 0.875, 1.0, 1.25, 1.5, 1.75, 2.0, 3.0, 4.0, 6.0, 8.0)
SCALES = {1: (1.0,), 8: (0.25, 0.5, 0.75, 1.0, 1.5, 2.0, 4.0, 8.0), 16: SCALES16}
_CASES = {}


@pytest.fixture(scope="module")
def gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import excel_amd.ops  # noqa: F401
    return True


def _dev(a):
    return torch.from_numpy(np.array(a)).cuda()


def _case(Cmax, nc, with_cls, seed=0, negative=False, sizes=SIZES, full_nchan=False):
    """A ragged batch, built once per key and read-only afterwards.  Plane values are multiples of 1/8 in [0, 2] (with `negative`:
    plane 0 in [-1, 2]) so that a * b0 == F happens often at the scales above; pad columns hold +inf, the planes >= nchan[b] NaN; the
    ground truth holds 255 and values >= nc; the class lists reach past nc - 1 (keys >= nc count only where they are background)."""
    key = (Cmax, nc, with_cls, seed, negative, tuple(sizes), full_nchan)
    if key in _CASES:
        return _CASES[key]
    rs = np.random.RandomState(1000 * Cmax + nc + seed)
    B = len(sizes)
    nchan = np.asarray(([1, 2, Cmax, 3, Cmax] * B)[:B], np.int32)
    if full_nchan:
        nchan[:] = Cmax
    planes, gts = [], []
    for b, (h, w) in enumerate(sizes):
        wp = (w + 3) // 4 * 4
        p = np.full((Cmax, h, wp), np.inf, np.float32)
        p[:, :, :w] = rs.randint(0, 17, (Cmax, h, w)).astype(np.float32) / 8
        if negative:
            p[0, :, :w] = rs.randint(-8, 17, (h, w)).astype(np.float32) / 8
        p[nchan[b]:] = np.nan
        planes.append(p.reshape(-1))
        g = rs.randint(0, nc, h * w).astype(np.uint8)
        g[rs.rand(h * w) < 0.05] = 255
        if nc < 250:
            g[rs.rand(h * w) < 0.05] = nc + rs.randint(0, 3)
        gts.append(g)
    cls = rs.randint(0, min(nc + 8, 254), (B, Cmax - 1)).astype(np.int32) if with_cls else None
    case = dict(planes=np.concatenate(planes), gts=np.concatenate(gts), nchan=nchan, cls=cls, sizes=list(sizes), Cmax=Cmax, nc=nc)
    _CASES[key] = case
    return case


def _on_device(case):
    from excel_amd import ops
    plan = ops.RaggedPlan(case["sizes"], "cuda")
    return plan, _dev(case["planes"]), _dev(case["gts"]), _dev(case["nchan"]), (None if case["cls"] is None else _dev(case["cls"]))


@pytest.mark.parametrize("with_cls", [True, False], ids=["cls_idx", "no_cls_idx"])
@pytest.mark.parametrize("nc, K", [(21, 16), (81, 16), (256, 16), (21, 1), (21, 8)])
@pytest.mark.parametrize("Cmax", [7, 19])
def test_counts_and_labels_equal_the_reference(gpu, Cmax, nc, K, with_cls):
    from excel_amd import ops
    from excel_amd.utils.bkg_sweep import sweep_reference, sweep_ragged
    case = _case(Cmax, nc, with_cls)
    scales = SCALES[K]
    sel = K // 2
    want_t, want_l = sweep_reference(case["planes"], case["sizes"], Cmax, scales, nchan=case["nchan"], cls_idx=case["cls"], gts=case["gts"],
                                     num_classes=nc, label_sel=sel)
    plan, planes, gts, nchan, cls = _on_device(case)
    labels_out = torch.full((plan.total_label_pix,), 0xFF, dtype=torch.uint8, device="cuda")
    totals, labels = sweep_ragged(planes, plan, Cmax, scales, nchan=nchan, cls_idx=cls, gts=gts, num_classes=nc, label_sel=sel, labels_out=labels_out)
    assert totals.dtype == torch.int64 and tuple(totals.shape) == (K, 3, nc) and labels.data_ptr() == labels_out.data_ptr()
    got_t, got_l = totals.cpu().numpy(), labels.cpu().numpy()
    print(f"Cmax {Cmax} nc {nc} K {K}: counted {want_t[:, 0].sum(1).tolist()} background {want_t[:, 1, 0].tolist()}")
    assert want_l.max() < 255 and np.array_equal(got_l, want_l), "labels (every byte of the 0xFF buffer written)"
    assert np.array_equal(got_t, want_t)
    assert (want_t[:, 0].sum(1) > 0).all() and (len(scales) == 1 or want_t[0, 1, 0] < want_t[-1, 1, 0])
    if with_cls and nc == 21 and K > 1:
        assert (np.diff(want_t[:, 0].sum(1)) >= 0).all() and want_t[0, 0].sum() < want_t[-1, 0].sum(), "keys >= nc drop out where they are foreground"
    # the labels of every scale; at 1.0 they are the arg-max kernel's, bit for bit
    for j in sorted({0, K - 1, scales.index(1.0)}):
        got = sweep_ragged(planes, plan, Cmax, scales, nchan=nchan, cls_idx=cls, label_sel=j)
        assert got[0] is None
        want = sweep_reference(case["planes"], case["sizes"], Cmax, scales, nchan=case["nchan"], cls_idx=case["cls"], label_sel=j)[1]
        assert np.array_equal(got[1].cpu().numpy(), want), f"labels at scale {scales[j]}"
        if scales[j] == 1.0:
            assert torch.equal(got[1], ops.argmax_label_ragged(planes, plan, Cmax, nchan, cls))


def test_nchan_null_means_every_plane(gpu):
    from excel_amd import ops
    from excel_amd.utils.bkg_sweep import sweep_reference, sweep_ragged
    case = _case(7, 21, True, seed=5, full_nchan=True)
    plan, planes, gts, _, cls = _on_device(case)
    want_t, want_l = sweep_reference(case["planes"], case["sizes"], 7, SCALES[8], cls_idx=case["cls"], gts=case["gts"], num_classes=21, label_sel=3)
    totals, labels = sweep_ragged(planes, plan, 7, SCALES[8], cls_idx=cls, gts=gts, num_classes=21, label_sel=3)
    assert np.array_equal(totals.cpu().numpy(), want_t) and np.array_equal(labels.cpu().numpy(), want_l)
    assert torch.equal(labels, ops.argmax_label_ragged(planes, plan, 7, None, cls))


@pytest.mark.parametrize("nc", [21, 256])
def test_negative_background_and_unsorted_scales(gpu, nc):
    """Plane 0 below zero turns the mask around, unsorted scales make it anything: the same bins, with signed steps."""
    from excel_amd.utils.bkg_sweep import sweep_reference, sweep_ragged
    case = _case(7, nc, True, seed=2, negative=True)
    scales = (2.0, 0.5, 1.0, 0.0, 4.0, 0.25, 1.0, 8.0, 0.75)
    want_t, want_l = sweep_reference(case["planes"], case["sizes"], 7, scales, nchan=case["nchan"], cls_idx=case["cls"], gts=case["gts"],
                                     num_classes=nc, label_sel=3)
    plan, planes, gts, nchan, cls = _on_device(case)
    totals, labels = sweep_ragged(planes, plan, 7, scales, nchan=nchan, cls_idx=cls, gts=gts, num_classes=nc, label_sel=3)
    assert np.array_equal(labels.cpu().numpy(), want_l) and np.array_equal(totals.cpu().numpy(), want_t)
    assert np.array_equal(want_t[2], want_t[6]), "the same scale twice: the same rows"
    bkg = want_t[:, 1, 0]
    assert not (np.diff(bkg) >= 0).all() and not (np.diff(bkg) <= 0).all()
    # sorted scales on the same planes: negative b0 alone (background at the SMALL scales)
    srt = tuple(sorted(set(scales)))
    want = sweep_reference(case["planes"], case["sizes"], 7, srt, nchan=case["nchan"], cls_idx=case["cls"], gts=case["gts"], num_classes=nc)[0]
    got = sweep_ragged(planes, plan, 7, srt, nchan=nchan, cls_idx=cls, gts=gts, num_classes=nc)[0]
    assert np.array_equal(got.cpu().numpy(), want)


def test_skip_flags_and_accumulation(gpu):
    from excel_amd.utils.bkg_sweep import sweep_reference, sweep_ragged
    case = _case(7, 21, True, seed=1)
    scales = SCALES[8]
    kw = dict(nchan=case["nchan"], cls_idx=case["cls"], gts=case["gts"], num_classes=21)
    plan, planes, gts, nchan, cls = _on_device(case)
    dkw = dict(nchan=nchan, cls_idx=cls, gts=gts, num_classes=21)
    skip_h = np.int32([0, 3, 0, 0, 1])
    want_skip, want_lab = sweep_reference(case["planes"], case["sizes"], 7, scales, skip=skip_h, label_sel=2, **kw)
    want_all = sweep_reference(case["planes"], case["sizes"], 7, scales, **kw)[0]
    assert not np.array_equal(want_skip, want_all)
    totals, labels = sweep_ragged(planes, plan, 7, scales, skip=_dev(skip_h), label_sel=2, **dkw)
    assert np.array_equal(totals.cpu().numpy(), want_skip)
    assert np.array_equal(labels.cpu().numpy(), want_lab), "the labels are written whatever skip says"
    zeros = sweep_ragged(planes, plan, 7, scales, skip=_dev(np.zeros(5, np.int32)), **dkw)[0]
    assert np.array_equal(zeros.cpu().numpy(), want_all)
    # a second call adds; so does a call on totals that hold something already
    again = sweep_ragged(planes, plan, 7, scales, totals=totals, **dkw)[0]
    assert again.data_ptr() == totals.data_ptr() and np.array_equal(again.cpu().numpy(), want_skip + want_all)
    start = torch.arange(8 * 3 * 21, dtype=torch.int64, device="cuda").view(8, 3, 21) * (1 << 33)
    got = sweep_ragged(planes, plan, 7, scales, totals=start.clone(), **dkw)[0]
    assert np.array_equal(got.cpu().numpy(), start.cpu().numpy() + want_all)


def test_many_tiles_per_workgroup(gpu):
    """More tiles (2280) than a counting launch takes at a time (256 workgroups x 4 tiles): every workgroup strides and flushes once."""
    from excel_amd.utils.bkg_sweep import sweep_reference, sweep_ragged
    sizes = [(33, 130)] * 240 + [(17, 65)] * 30                      # 240 * 9 + 30 * 4 = 2280 tiles
    case = _case(4, 21, False, seed=7, sizes=sizes)
    plan, planes, gts, nchan, _ = _on_device(case)
    assert plan.total_tiles == 2280
    want_t, want_l = sweep_reference(case["planes"], sizes, 4, SCALES[8], nchan=case["nchan"], gts=case["gts"], num_classes=21, label_sel=4)
    totals, labels = sweep_ragged(planes, plan, 4, SCALES[8], nchan=nchan, gts=gts, num_classes=21, label_sel=4)
    assert np.array_equal(totals.cpu().numpy(), want_t) and np.array_equal(labels.cpu().numpy(), want_l)


def test_bad_arguments_are_refused_before_any_launch(gpu):
    from excel_amd import ops
    from excel_amd.utils.bkg_sweep import sweep_ragged
    plan = ops.RaggedPlan([(2, 4), (3, 5)], "cuda")
    planes = torch.zeros(3 * plan.total_pix + 8, dtype=torch.float32, device="cuda")
    gt = torch.zeros(plan.total_label_pix, dtype=torch.uint8, device="cuda")
    totals = torch.full((16 * 3 * 256 + 1,), 77, dtype=torch.int64, device="cuda")
    labels = torch.full((plan.total_label_pix,), 0x5A, dtype=torch.uint8, device="cuda")
    lib = ops.lib()
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    pp, gp, tp, lp = (C.c_void_p(t.data_ptr()) for t in (planes, gt, totals, labels))
    info, tab = C.byref(plan.info), C.c_void_p(plan.table.data_ptr())

    def sc(*v):
        return (C.c_float * len(v))(*v)
    one, two = sc(1.0), sc(0.5, 1.0)
    seventeen = sc(*[0.1 * (i + 1) for i in range(17)])
    off = lambda t, n: C.c_void_p(t.data_ptr() + n)
    for args, word in (((None, None, None, gp, tab, info, 2, 3, two, 2, None, 21, tp, 0, lp, st), "null argument"),
                       ((pp, None, None, gp, None, info, 2, 3, two, 2, None, 21, tp, 0, lp, st), "null argument"),
                       ((pp, None, None, gp, tab, None, 2, 3, two, 2, None, 21, tp, 0, lp, st), "null argument"),
                       ((pp, None, None, gp, tab, info, 2, 3, two, 2, None, 21, None, 0, None, st), "neither totals nor labels_u8"),
                       ((pp, None, None, None, tab, info, 2, 3, two, 2, None, 21, tp, 0, lp, st), "totals needs the ground truth"),
                       ((pp, None, None, gp, tab, info, 2, 3, two, 0, None, 21, tp, 0, lp, st), "1 <= K <= 16 (K = 0)"),
                       ((pp, None, None, gp, tab, info, 2, 3, seventeen, 17, None, 21, tp, 0, lp, st), "1 <= K <= 16 (K = 17)"),
                       ((pp, None, None, gp, tab, info, 2, 3, sc(1.0, float("nan")), 2, None, 21, tp, 0, lp, st), "scale 1 is"),
                       ((pp, None, None, gp, tab, info, 2, 3, sc(float("inf")), 1, None, 21, tp, 0, lp, st), "scale 0 is inf"),
                       ((pp, None, None, gp, tab, info, 2, 3, sc(0.5, -0.25), 2, None, 21, tp, 0, lp, st), "scale 1 is -0.25"),
                       ((pp, None, None, gp, tab, info, 2, 3, two, 2, None, 21, tp, -1, lp, st), "label_sel = -1"),
                       ((pp, None, None, gp, tab, info, 2, 3, two, 2, None, 21, tp, 2, lp, st), "label_sel = 2"),
                       ((pp, None, None, gp, tab, info, 2, 3, two, 2, None, 0, tp, 0, lp, st), "num_classes"),
                       ((pp, None, None, gp, tab, info, 2, 3, two, 2, None, 257, tp, 0, lp, st), "num_classes"),
                       ((pp, None, None, gp, tab, info, 2, 3, two, 2, None, 21, off(totals, 4), 0, lp, st), "8-byte aligned"),
                       ((off(planes, 4), None, None, gp, tab, info, 2, 3, two, 2, None, 21, tp, 0, lp, st), "16-byte aligned")):
        assert lib.excel_bkg_sweep_ragged(*args) == -1, word
        assert word in lib.excel_last_error().decode(), (word, lib.excel_last_error())
    # label_sel is not looked at without a label map; a scale of zero is a scale
    assert lib.excel_bkg_sweep_ragged(pp, None, None, gp, tab, info, 2, 3, sc(0.0, 1.0), 2, None, 21, C.c_void_p(totals.data_ptr() + 8), 99, None, st) == 0
    torch.cuda.synchronize()
    assert bool((totals[0] == 77).all()) and bool((labels == 0x5A).all()), "a refused call wrote to its outputs"
    # (all planes and the ground truth are zero: every pixel is background at both scales and counts in all three rows)
    assert int((totals[1:1 + 2 * 3 * 21] - 77).sum()) == 2 * 3 * plan.total_label_pix
    # the wrapper's own checks
    with pytest.raises(ValueError, match="gts needs num_classes"):
        sweep_ragged(planes, plan, 3, (1.0,), gts=gt)
    with pytest.raises(ValueError, match="totals needs gts"):
        sweep_ragged(planes, plan, 3, (1.0,), totals=totals[:63].view(1, 3, 21))
    with pytest.raises(ValueError, match=r"totals must be int64 \[2,3,21\]"):
        sweep_ragged(planes, plan, 3, (0.5, 1.0), gts=gt, num_classes=21, totals=totals[:63].view(1, 3, 21))
    with pytest.raises(ValueError, match="skip holds 3 values for 2 images"):
        sweep_ragged(planes, plan, 3, (1.0,), gts=gt, num_classes=21, skip=torch.zeros(3, dtype=torch.int32, device="cuda"))
    with pytest.raises(RuntimeError, match="nothing to do"):
        sweep_ragged(planes, plan, 3, (1.0,))


# ------------------------------------------------------------------ the stream contract (tests/_streams.py, by import)
@pytest.fixture(scope="module")
def t_link(gpu):
    t = St.time_link()
    print(f"\n[bkg-sweep streams] one chain link: {t * 1e6:.0f} us")
    assert t > 0
    return t


@pytest.fixture(scope="module")
def stream_case(gpu):
    """fn() -> the op's two outputs, from fresh zeroed totals and an uninitialised label map, on the current stream; and its reference
    on the idle default stream."""
    from excel_amd.utils.bkg_sweep import sweep_ragged
    case = _case(7, 21, True, seed=3, sizes=[(120, 200), (75, 333), (17, 65), (200, 120)] * 4)
    plan, planes, gts, nchan, cls = _on_device(case)
    torch.cuda.synchronize()

    def fn():
        totals = torch.zeros((8, 3, 21), dtype=torch.int64, device="cuda")
        totals, labels = sweep_ragged(planes, plan, 7, SCALES[8], nchan=nchan, cls_idx=cls, gts=gts, num_classes=21, totals=totals, label_sel=3)
        return dict(totals=totals, labels=labels)
    return fn, St.reference(fn)


@pytest.mark.parametrize("arrangement", ["behind", "beside"])
def test_the_op_stays_on_its_callers_stream(gpu, stream_case, t_link, arrangement):
    fn, ref = stream_case
    links = St.links_for(ref.t_case, t_link)
    run = (St.run_behind if arrangement == "behind" else St.run_beside)(fn, links)
    print(f"\n[bkg-sweep streams] {arrangement}: t_case {ref.t_case * 1e3:.2f} ms, {run.links} links, side-stream run {run.host_s * 1e3:.2f} ms, "
          f"default stream busy afterwards: {run.busy}")
    assert int(ref.tree["totals"][:, 0].sum()) > 0
    if arrangement == "behind":
        St.assert_matches(ref.tree, run.final, None, "queued behind a busy chain on its own stream")
        return
    St.assert_matches(ref.tree, run.early, None, "(a) beside a busy default stream, read when the side stream was done")
    St.assert_matches(ref.tree, run.final, None, "(b) beside a busy default stream, read after the device had drained")
    assert run.busy, "(c) " + St.busy_message(run, ref.t_case, t_link)


# ------------------------------------------------------------------ the pipeline and the program
class _Capture(logging.Handler):
    def __init__(self):
        super().__init__(logging.INFO)
        self.lines = []

    def emit(self, record):
        self.lines.append(record.getMessage())


@pytest.fixture(scope="module")
def program(gpu, tmp_path_factory):
    """infer_lam.validate on a synthetic VOC tree (6 ragged images at batch 4: two steps) with the tiny checkpoint: once plain, once with
    --bkg_sweep and --json_out.  The model of the second run serves the pipeline tests."""
    from _clip_files import write_tiny_clip
    from excel_amd.tools import infer_lam, synthetic
    tmp = tmp_path_factory.mktemp("bkg_sweep")
    root, lists = tmp / "VOC2012", tmp / "lists"
    synthetic.write_voc_tree(str(root), str(lists), 6, seed=4, split="val")
    ckpt, bpe_path, _ = write_tiny_clip(tmp)
    common = ["--data_folder", str(root), "--list_folder", str(lists), "--infer_set", "val", "--resize_size", "128", "--model", ckpt,
              "--bpe_path", bpe_path, "--batch_size", "4", "--num_workers", "2"]
    parse = infer_lam.get_parser().parse_args
    cwd = os.getcwd()
    os.chdir(tmp)
    cap = _Capture()
    logging.getLogger().addHandler(cap)
    level = logging.getLogger().level
    logging.getLogger().setLevel(logging.INFO)
    try:
        _, plain = infer_lam.validate(parse(common))
        assert infer_lam.validate.last_bkg_sweep is None
        js = str(tmp / "run.json")
        _, swept = infer_lam.validate(parse(common + ["--bkg_sweep", "0.25,1.0,4.0", "--json_out", js]))
        report = infer_lam.validate.last_bkg_sweep
        with open(js) as f:
            record = json.load(f)
        _, at4 = infer_lam.validate(parse(common + ["--bkg_scale", "4.0"]))
    finally:
        logging.getLogger().removeHandler(cap)
        logging.getLogger().setLevel(level)
        os.chdir(cwd)
    return dict(plain=plain.cpu().numpy(), swept=swept.cpu().numpy(), at4=at4.cpu().numpy(), report=report, record=record, log="\n".join(cap.lines),
                model=infer_lam.validate.last_model)


def _margins(h):
    return np.stack([h.sum(1), h.sum(0), np.diag(h)])


def test_infer_lam_bkg_sweep(gpu, program):
    from excel_amd.tools import infer_lam
    from excel_amd.utils import bkg_sweep
    from excel_amd.utils.evaluate import scores_from_hist
    p = program
    assert np.array_equal(p["plain"], p["swept"]), "the flag changes no score"
    rep = p["report"]
    t = rep["totals"].cpu().numpy()
    print("background area per scale", t[:, 1, 0].tolist(), "mIoU", [s["miou"] for s in rep["scores"]])
    assert rep["scales"] == (0.25, 1.0, 4.0) and t.shape == (3, 3, 21)
    assert np.array_equal(t[1], _margins(p["plain"])), "the row of scale 1.0 is the run's own matrix"
    assert np.array_equal(t[2], _margins(p["at4"])), "--bkg_scale 4.0 scores the labels the sweep counted at 4.0"
    assert (np.diff(t[:, 1, 0]) >= 0).all() and t[0, 1, 0] < t[2, 1, 0]
    assert rep["scores"][1]["miou"] == scores_from_hist(p["plain"])["miou"]
    assert "bkg_sweep_score:" in p["log"] and bkg_sweep.format_sweep_table(rep["scores"], rep["scales"], infer_lam.VOC_CLASSES) in p["log"]
    assert f"bkg_sweep best scale {rep['best_scale']:g}" in p["log"]
    block = p["record"]["bkg_sweep"]
    assert block == bkg_sweep.sweep_json(rep["scores"], rep["scales"]) and block["scales"] == [0.25, 1.0, 4.0]
    assert block["miou"][1] == p["record"]["miou"] and block["best_scale"] == rep["best_scale"]


def _batch(seed=0):
    """Four small ragged images of the pipeline tests: decoded bytes, ground truth with 255, one to three present classes."""
    rs = np.random.RandomState(40 + seed)
    sizes = [(40, 151), (17, 65), (64, 96), (33, 70)]
    imgs = [rs.randint(0, 256, (h, w, 3)).astype(np.uint8) for h, w in sizes]
    gts = [rs.randint(0, 21, (h, w)).astype(np.uint8) for h, w in sizes]
    for g in gts:
        g[rs.rand(*g.shape) < 0.03] = 255
    cls = np.zeros((4, 20), np.float32)
    for b, k in enumerate([1, 3, 2, 3]):
        cls[b, rs.choice(20, size=k, replace=False)] = 1
    return sizes, _dev(np.concatenate([i.reshape(-1) for i in imgs])), _dev(np.concatenate([g.reshape(-1) for g in gts])), _dev(cls)


def test_pipeline_sweep_totals_and_scaled_labels(gpu, program):
    from excel_amd import ops
    from excel_amd.pipeline import TrainingFreePipeline
    from excel_amd.utils.bkg_sweep import sweep_ragged
    model = program["model"]
    scales = (0.25, 1.0, 4.0)
    sizes, images, gts, cls = _batch()
    plan = ops.RaggedPlan(sizes, "cuda")
    C_ = 4
    swept = TrainingFreePipeline(model, num_classes=21, smax=3, bkg_sweep=scales)
    labels, inter = swept.run_batch_ragged(images, plan, cls, gts, S=128, return_intermediates=True)
    hist = swept.hist.cpu().numpy()
    t = swept.sweep_totals.cpu().numpy()
    print("pipeline background area per scale", t[:, 1, 0].tolist())
    assert swept.sweep_totals.dtype == torch.int64 and t.shape == (3, 3, 21)
    assert np.array_equal(t[1], _margins(hist)), "sweep_totals at 1.0 = (hist.sum(1), hist.sum(0), hist.diagonal())"
    assert (np.diff(t[:, 1, 0]) >= 0).all() and t[0, 1, 0] < t[2, 1, 0], "background area is monotone over the scales"
    nchan, idx = swept.last_nchan, inter["cls_idx"]
    assert torch.equal(labels, ops.argmax_label_ragged(inter["par_out"], plan, C_, nchan, idx)), "bkg_scale 1.0: the arg-max kernel's labels"
    # a second step adds; reset() clears
    swept.run_batch_ragged(images, plan, cls, gts, S=128)
    assert np.array_equal(swept.sweep_totals.cpu().numpy(), 2 * t)
    swept.reset()
    assert swept.sweep_totals is None and swept.hist is None
    # without ground truth nothing is counted
    swept.run_batch_ragged(images, plan, cls, None, S=128)
    assert swept.sweep_totals is None
    for j in (0, 2):
        scaled = TrainingFreePipeline(model, num_classes=21, smax=3, bkg_scale=scales[j])
        lab = scaled.run_batch_ragged(images, plan, cls, gts, S=128)
        want = sweep_ragged(inter["par_out"], plan, C_, scales, nchan=nchan, cls_idx=idx, label_sel=j)[1]
        assert torch.equal(lab, want), f"bkg_scale={scales[j]}: the labels label_sel gives on the first pipeline's PAR output"
        assert np.array_equal(_margins(scaled.hist.cpu().numpy()), t[j]) and scaled.sweep_totals is None
        assert not torch.equal(lab, labels)
    # a default pipeline: the parent's behaviour, the arg-max of its own par_out, and no totals
    plain = TrainingFreePipeline(model, num_classes=21, smax=3)
    lab, own = plain.run_batch_ragged(images, plan, cls, gts, S=128, return_intermediates=True)
    assert torch.equal(lab, ops.argmax_label_ragged(own["par_out"], plan, C_, plain.last_nchan, own["cls_idx"])) and torch.equal(lab, labels)
    assert plain.sweep_totals is None and np.array_equal(plain.hist.cpu().numpy(), hist)


def test_pipeline_sweep_honours_the_guards_skip_flags(gpu, program):
    """guard="skip": the sweep gets the step's flags exactly when the matrix does, so its row at 1.0 stays the matrix's margins; with
    "observe" every image counts.  (The tiny model overflows nothing: the flags are zero, the counts equal the unguarded ones.)"""
    from excel_amd import ops
    from excel_amd.pipeline import TrainingFreePipeline
    model = program["model"]
    sizes, images, gts, cls = _batch(1)
    plan = ops.RaggedPlan(sizes, "cuda")
    got = {}
    for guard in (None, "skip", "observe"):
        p = TrainingFreePipeline(model, num_classes=21, smax=3, bkg_sweep=(0.5, 1.0), guard=guard)
        p.run_batch_ragged(images, plan, cls, gts, S=128)
        got[guard] = p.sweep_totals.cpu().numpy()
        assert np.array_equal(got[guard][1], _margins(p.hist.cpu().numpy()))
    assert np.array_equal(got[None], got["skip"]) and np.array_equal(got[None], got["observe"])
