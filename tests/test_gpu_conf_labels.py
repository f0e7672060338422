"""Two-threshold pseudo labels with an ignore band (include/excel_hip.h, "confident labels"; utils/affutils.py:101-158) on the GPU:
the two new kernels against the float64 restatement (tests/_conf_ref.py) and against the ops they fuse, ONE PAR pass over both groups
against two, the whole chain against the reference's fixture (tests/golden/conf_labels.npz), the pipeline's `conf=` option and the
program's --conf_label.  Every test prints its figure before asserting it."""
import logging
import os

import numpy as np
import pytest

import _conf_ref as R
import oracle
from test_gpu_pipeline import RAGGED_HW, _ragged_samples, dev, host, maxabs, tiny_model

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

SIZES = [(33, 50), (64, 47), (17, 96), (40, 40)]      # odd halves, a non-factor-2 axis, a width that needs pitch padding, an exact factor 2
COUNTS = {3: [3, 1, 2, 3], 18: [18, 1, 9, 17]}        # smax -> present classes per image (18: 38 planes in the fused PAR)
F = 80
HIGH, LOW = 0.7, 0.25
DIL = [1, 2, 4, 8, 12, 24]


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from excel_amd import ops as _ops
    return _ops


def _say(what, got, bound):
    print(f"\n[conf-labels] {what}: {got:.3e} (bound {bound:g})")


def _pack(plan, per_image, K):
    """per_image[b] [k_b, H_b, W_b] -> K pitched planes per image, flat; everything the contract leaves undefined (planes >= k_b, pad
    columns) is NaN, so a kernel that reads it shows"""
    out = np.full(K * plan.total_pix, np.nan, np.float32)
    for b, p in enumerate(per_image):
        H, W = int(plan.hw[b, 0]), int(plan.hw[b, 1])
        Wp = (W + 3) // 4 * 4
        v = out[K * plan.poff[b]:K * plan.poff[b] + K * H * Wp].reshape(K, H, Wp)
        v[:p.shape[0], :, :W] = p
    return dev(out)


def _cams(rs, k, hw):
    """smooth random maps in [0, 1], float32 [k, H, W]"""
    return np.clip(R.resize_planes(rs.rand(k, 5, 7), *hw), 0, 1).astype(np.float32)


def _classes(ops, counts, smax, seed=1):
    rs = np.random.RandomState(seed)
    onehot = np.zeros((len(counts), F), np.float32)
    for b, k in enumerate(counts):
        onehot[b, rs.choice(F, k, replace=False)] = 1
    idx, ncls, nchan = ops.cls_compact(dev(onehot), smax, want_nchan=True)
    assert host(ncls).tolist() == list(counts)
    return idx, nchan


@pytest.fixture(scope="module")
def planes_case(ops):
    """The inputs and the device results of test 1, computed once: cams with NaN in plane 0, in the unused planes and in the pad columns"""
    smax, counts = 3, COUNTS[3]
    rs = np.random.RandomState(7)
    plan = ops.RaggedPlan(SIZES, "cuda")
    half = ops.conf_half_plan(plan)
    cams = [_cams(rs, k, hw) for k, hw in zip(counts, SIZES)]
    packed = _pack(plan, [np.concatenate([np.full((1,) + c.shape[1:], np.nan, np.float32), c]) for c in cams], smax + 1)
    nchan = dev(np.asarray(counts, np.int32) + 1)
    planes, nchan2 = ops.conf_planes_ragged(packed, plan, half, smax, nchan, HIGH, LOW)
    raw, _ = ops.conf_planes_ragged(packed, plan, half, smax, nchan, HIGH, LOW, softmax=False)
    return dict(smax=smax, counts=counts, plan=plan, half=half, cams=cams, planes=planes, nchan2=nchan2, raw=raw)


# ------------------------------------------------------------------ 1. conf_planes
def test_conf_planes_vs_restatement(ops, planes_case):
    """The resized values are requested through the softmax-free call (softmax=False: the first group holds [high_thre, m_1 .. m_k] as
    resized) and are bit-equal to ops.bilinear_resize per image; both softmaxes are then compared with the restatement's float64
    softmax (_conf_ref.softmax0) of those same values.  Bound: 8x the largest error torch's own float32 CPU softmax of the same
    planes shows against float64 on these inputs, computed here.  Measured on MI355X: torch's error 5.69e-08, bound 4.55e-07, the
    kernel's error 6.11e-08."""
    c = planes_case
    smax, half = c["smax"], c["half"]
    assert host(c["nchan2"]).tolist() == [2 * (k + 1) for k in c["counts"]]
    worst, torch_err = 0.0, 0.0
    for b, k in enumerate(c["counts"]):
        hh, wh = (int(v) for v in half.hw[b])
        m = ops.bilinear_resize(dev(c["cams"][b]), hh, wh, align_corners=False)
        raw = half.planes(c["raw"], b, 2 * (smax + 1))
        assert torch.equal(raw[1:k + 1], m), f"image {b}: resized values differ from ops.bilinear_resize"
        assert torch.equal(raw[0], torch.full_like(raw[0], HIGH))
        got = host(half.planes(c["planes"], b, 2 * (smax + 1)))[:2 * (k + 1)]
        assert np.isfinite(got).all(), f"image {b}: a value nobody defines (plane 0, an unused plane, a pad column) was read"
        for g, thre in enumerate((HIGH, LOW)):
            x = np.concatenate([np.full((1, hh, wh), np.float32(thre), np.float32), host(m)], 0)
            ref = R.softmax0(x.astype(np.float64))
            worst = max(worst, maxabs(got[g * (k + 1):(g + 1) * (k + 1)], ref))
            torch_err = max(torch_err, maxabs(torch.softmax(torch.from_numpy(x), 0).numpy(), ref))
    _say("torch float32 CPU softmax vs float64", torch_err, 0)
    _say("conf_planes vs the float64 softmax of the same resized planes", worst, 8 * torch_err)
    assert worst <= 8 * torch_err


# ------------------------------------------------------------------ 2. one PAR over both groups
@pytest.mark.parametrize("smax", [3, 18])
def test_fused_par_is_two_pars(ops, smax):
    """par_forward_ragged over the 2 (k + 1) planes of every image == two runs over k + 1 planes each, torch.equal on every defined
    plane.  smax = 18 with [18, 1, 9, 17] classes: 38 planes through the tile kernel's plane loop (nothing caps the count:
    excel_par_guide_supported only bounds Cmax * H * Wp * 4 < 2^31 per image)."""
    counts = COUNTS[smax]
    C = smax + 1
    rs = np.random.RandomState(11 + smax)
    plan = ops.conf_half_plan(ops.RaggedPlan(SIZES, "cuda"))
    groups = []
    for k, (h, w) in zip(counts, plan.hw.tolist()):
        m = R.resize_planes(rs.rand(k, 3, 4), h, w)
        groups.append([R.softmax0(np.concatenate([np.full((1, h, w), t), m], 0)).astype(np.float32) for t in (HIGH, LOW)])
    imgs = dev(rs.standard_normal((len(counts), 3, 48, 48)).astype(np.float32))
    nchan = dev(np.asarray(counts, np.int32) + 1)
    fused = ops.par_forward_ragged(imgs, _pack(plan, [np.concatenate(g, 0) for g in groups], 2 * C), plan, 2 * C, DIL, 10, nchan=2 * nchan)
    single = [ops.par_forward_ragged(imgs, _pack(plan, [g[i] for g in groups], C), plan, C, DIL, 10, nchan=nchan) for i in range(2)]
    for b, k in enumerate(counts):
        got = plan.planes(fused, b, 2 * C)
        assert torch.isfinite(got[:2 * (k + 1)]).all()
        for i in range(2):
            assert torch.equal(got[i * (k + 1):(i + 1) * (k + 1)], plan.planes(single[i], b, C)[:k + 1]), (smax, b, i)
        moved = maxabs(host(got[:k + 1]), groups[b][0])
    _say(f"smax {smax}: PAR changed the last image's planes by", moved, 0)
    assert moved > 1e-4


# ------------------------------------------------------------------ 3. conf_merge
@pytest.mark.parametrize("smax", [3, 18])
@pytest.mark.parametrize("boxed", [False, True])
def test_conf_merge_is_the_composition(ops, smax, boxed):
    """Per image and group ops.bilinear_resize + ops.argmax_label with the keys, then the three assignments of :154-156 (and the box of
    :146-149) in torch: torch.equal."""
    counts = COUNTS[smax]
    C2 = 2 * (smax + 1)
    rs = np.random.RandomState(21 + smax)
    plan = ops.RaggedPlan(SIZES, "cuda")
    half = ops.conf_half_plan(plan)
    idx, nchan = _classes(ops, counts, smax)
    per_image = [rs.rand(2 * (k + 1), h, w).astype(np.float32) for k, (h, w) in zip(counts, half.hw.tolist())]
    packed = _pack(half, per_image, C2)
    box = np.asarray([[3, 30, 5, 41], [0, 50, 7, 47], [2, 17, 0, 90], [0, 40, 0, 40]], np.int32) if boxed else None
    lab = ops.conf_merge_ragged(packed, half, plan, smax, nchan, idx, img_box=None if box is None else dev(box), ignore_index=255)
    seen = set()
    for b, (k, (H, W)) in enumerate(zip(counts, SIZES)):
        p = dev(per_image[b])
        lh, ll = (ops.argmax_label(ops.bilinear_resize(p[None, g * (k + 1):(g + 1) * (k + 1)].contiguous(), H, W, align_corners=False),
                                   None, idx[b:b + 1].contiguous())[0] for g in range(2))
        ref = lh.clone()
        ref[lh == 0] = 255
        ref[(lh == 0) & (ll == 0)] = 0
        if box is not None:
            y0, y1, x0, x1 = box[b].tolist()
            cut = torch.full_like(ref, 255)
            cut[y0:y1, x0:x1] = ref[y0:y1, x0:x1]
            ref = cut
        assert torch.equal(plan.label(lab, b), ref), (smax, boxed, b, int((plan.label(lab, b) != ref).sum()))
        keys = set((host(idx)[b, :k] + 1).tolist())
        vals = set(np.unique(host(ref)).tolist())
        assert vals <= keys | {0, 255}
        seen |= {("class" if v in keys else v) for v in vals}
    assert seen == {"class", 0, 255}, "the inputs must reach all three outcomes of the merge"


# ------------------------------------------------------------------ 4. against the reference
@pytest.mark.parametrize("c", [0, 1])
def test_refine_cams_with_bkg_v2_vs_reference(ops, golden, c):
    """affutils.refine_cams_with_bkg_v2 on the reference's fixture: planes and PAR output at test_par_golden's 1e-4, label agreement
    >= 0.999 per image (the fixture's own float32 / float64 agreement is >= 0.9995), every label in {0, present keys, ignore_index},
    everything outside img_box ignore_index."""
    from excel_amd.utils import affutils
    from excel_amd.utils.PAR import PAR
    z = golden("conf_labels.npz")
    high, low, ignore, ds, num_iter, _ = z["meta"]
    img, cams, cls, box = (z[f"{n}_{c}"] for n in ("img", "cams", "cls", "box"))
    par = PAR(num_iter=int(num_iter), dilations=DIL)
    args = (par, dev(img), dev(cams), dev(cls), float(high), float(low), int(ignore))
    _, planes, par_out, plan, half, smax, _ = affutils._bkg_v2(*args, None, int(ds))
    for b in range(img.shape[0]):
        k = int(cls[b].sum())
        for name, got, want in (("planes", planes, z[f"planes_{c}_{b}"]), ("PAR output", par_out, z[f"par_{c}_{b}"])):
            mine = host(half.planes(got, b, 2 * (smax + 1)))[:2 * (k + 1)].reshape(2, k + 1, *want.shape[2:])
            err = maxabs(mine, want)
            _say(f"case {c} image {b}: {name} vs the reference", err, 1e-4)
            assert err < 1e-4
    for tag, bx in (("", None), ("_box", box)):
        lab = affutils.refine_cams_with_bkg_v2(*args, img_box=None if bx is None else torch.from_numpy(bx), down_scale=int(ds))
        assert tuple(lab.shape) == z[f"lab{tag}_{c}"].shape and lab.dtype == torch.float32
        lab = host(lab)
        for b in range(img.shape[0]):
            agree = float((lab[b] == z[f"lab{tag}_{c}"][b]).mean())
            _say(f"case {c}{tag} image {b}: label agreement", agree, 0.999)
            assert agree >= 0.999
            assert set(np.unique(lab[b]).tolist()) <= set((np.flatnonzero(cls[b]) + 1).tolist()) | {0, int(ignore)}
            if bx is not None:
                outside = np.ones(lab[b].shape, bool)
                outside[bx[b][0]:bx[b][1], bx[b][2]:bx[b][3]] = False
                assert outside.any() and (lab[b][outside] == ignore).all()


# ------------------------------------------------------------------ 5. the pipeline
@pytest.fixture(scope="module")
def step(ops):
    """One ragged step of the tiny model at S = 96 with conf, with conf=None and as batches of one (test_gpu_pipeline's samples)."""
    from excel_amd.pipeline import TrainingFreePipeline
    S, F_ = 96, 4
    rs = np.random.RandomState(3)
    text = rs.standard_normal((9, 64)).astype(np.float32)
    text /= np.linalg.norm(text, axis=1, keepdims=True)
    model, _ = tiny_model(text.T.copy(), gemm_mode="f32")
    imgs, gts, cls = _ragged_samples()
    flat = lambda xs: dev(np.concatenate([x.reshape(-1) for x in xs]))
    plan = ops.RaggedPlan(RAGGED_HW, "cuda")
    out = {"gts": gts, "plan": plan, "nc": F_ + 1}
    pipe = TrainingFreePipeline(model, num_classes=F_ + 1, smax=3)
    out["labels"], out["conf"] = pipe.run_batch_ragged(flat(imgs), plan, dev(cls), flat(gts), S=S, conf=(HIGH, LOW))
    assert pipe.last_conf_labels is out["conf"]
    out["hist"], out["hist_conf"] = pipe.hist.clone(), pipe.hist_conf.clone()
    pipe.reset()
    assert pipe.hist is None and pipe.hist_conf is None
    lab, conf, inter = pipe.run_batch_ragged(flat(imgs), plan, dev(cls), flat(gts), S=S, conf=(HIGH, LOW), return_intermediates=True)
    out["inter"], out["kept"] = inter, (lab, conf)
    plain = TrainingFreePipeline(model, num_classes=F_ + 1, smax=3)
    out["plain"] = plain.run_batch_ragged(flat(imgs), plan, dev(cls), flat(gts), S=S)
    out["plain_hist"], out["plain_hist_conf"] = plain.hist.clone(), plain.hist_conf
    one = TrainingFreePipeline(model, num_classes=F_ + 1, smax=3)
    out["single"] = [tuple(t.clone() for t in one.run_batch_ragged(dev(imgs[b].reshape(-1)), ops.RaggedPlan([RAGGED_HW[b]], "cuda"), dev(cls[b:b + 1]),
                                                                   dev(gts[b].reshape(-1)), S=S, conf=(HIGH, LOW))) for b in range(len(imgs))]
    out["single_hist"], out["single_hist_conf"] = one.hist.clone(), one.hist_conf.clone()
    out["cls_idx"], out["nchan"] = pipe.last_cls_idx, pipe.last_nchan
    return out


def test_pipeline_batch_equals_batches_of_one(step):
    plan = step["plan"]
    for b, (lab, conf) in enumerate(step["single"]):
        assert torch.equal(plan.label(step["labels"], b).reshape(-1), lab), b
        assert torch.equal(plan.label(step["conf"], b).reshape(-1), conf), b
    assert torch.equal(step["hist"], step["single_hist"]) and torch.equal(step["hist_conf"], step["single_hist_conf"])
    assert torch.equal(step["kept"][0], step["labels"]) and torch.equal(step["kept"][1], step["conf"]), "return_intermediates changes nothing"


def test_pipeline_without_conf_is_the_plain_step(step):
    assert isinstance(step["plain"], torch.Tensor) and step["plain_hist_conf"] is None
    assert torch.equal(step["plain"], step["labels"]) and torch.equal(step["plain_hist"], step["hist"])


def test_pipeline_hist_conf_counts_the_kept_pixels(step):
    nc, plan = step["nc"], step["plan"]
    ref = np.zeros((nc, nc), np.int64)
    kept = 0
    for b, gt in enumerate(step["gts"]):
        conf = host(plan.label(step["conf"], b))
        keep = conf < nc
        kept += int((keep & (gt < nc)).sum())
        ref += oracle.evaluate.fast_hist(gt[keep].flatten(), conf[keep].flatten(), nc)
    got = host(step["hist_conf"])
    coverage = got.sum() / host(step["hist"]).sum()
    _say("coverage of the confident labels", float(coverage), 1)
    assert np.array_equal(got, ref) and int(got.sum()) == kept
    assert 0 < got.sum() < host(step["hist"]).sum()


def test_pipeline_monotonicity(ops, step):
    """Wherever the confident label is a class the strict pass says that class; wherever it is 0 both passes said 0; 255 exactly where
    only the strict pass said 0 - a swap of the two groups breaks the second."""
    plan, inter = step["plan"], step["inter"]
    half, C2 = inter["conf_plan"], 2 * 4
    for b in range(plan.B):
        H, W = (int(v) for v in plan.hw[b])
        k = int(host(step["nchan"])[b]) - 1
        p = half.planes(inter["conf_par_out"], b, C2)[:2 * (k + 1)]
        lh, ll = (ops.argmax_label(ops.bilinear_resize(p[None, g * (k + 1):(g + 1) * (k + 1)].contiguous(), H, W, align_corners=False),
                                   None, step["cls_idx"][b:b + 1].contiguous())[0] for g in range(2))
        conf = plan.label(step["conf"], b)
        cls = (conf != 0) & (conf != 255)
        assert torch.equal(conf[cls], lh[cls]) and (lh[cls] != 0).all()
        assert ((lh == 0) & (ll == 0))[conf == 0].all() and (conf == 0)[(lh == 0) & (ll == 0)].all()
        assert ((lh == 0) & (ll != 0))[conf == 255].all()
        # the strict pass is the one with the larger background score
        planes = half.planes(inter["conf_planes"], b, C2)
        assert (planes[0] > planes[k + 1]).all()


# ------------------------------------------------------------------ 6. the program
def test_infer_lam_conf_label(ops, tmp_path, caplog):
    """infer_lam --synthetic 8 --ragged true --conf_label true on the tiny model: one PNG per image that decodes (Pillow) to the labels
    of run_batch_ragged(conf=) over the same batches, the second table and the coverage line in the log, the gathered matrix that of
    the files, and --api_path true writes identical files."""
    from PIL import Image
    from _clip_files import write_tiny_clip
    from excel_amd.datasets.loader import pack_samples
    from excel_amd.pipeline import TrainingFreePipeline
    from excel_amd.tools import infer_lam, synthetic
    ckpt, bpe_path, _ = write_tiny_clip(tmp_path)
    common = ["--synthetic", "8", "--ragged", "true", "--resize_size", "96", "--model", ckpt, "--bpe_path", bpe_path, "--batch_size", "4",
              "--num_workers", "2", "--gemm_check", "false", "--conf_label", "true"]
    parse = infer_lam.get_parser().parse_args
    d1, d2 = tmp_path / "conf", tmp_path / "conf_api"
    with caplog.at_level(logging.INFO):
        _, total = infer_lam.validate(parse(common + ["--conf_label_dir", str(d1)]))
    log = caplog.text
    assert "conf_label_score:" in log and "conf_label coverage" in log and log.index("LAM_score") < log.index("conf_label_score:")
    conf_score, conf_total, coverage = infer_lam.validate.last_conf
    assert abs(coverage - float(conf_total.sum()) / float(total.sum())) < 1e-12 and 0 < coverage < 1
    model = infer_lam.validate.last_model
    _, plain = infer_lam.validate(parse(common[:-2]))
    assert torch.equal(plain.cpu(), total.cpu()) and infer_lam.validate.last_conf is None, "the main score does not depend on the flag"
    ds = synthetic.SyntheticSegDataset(8, (96, 96), num_classes=21, seed=1234, ragged=True)
    pipe = TrainingFreePipeline(model, num_classes=21, smax=ds.max_k())
    names = []
    for lo in (0, 4):
        rb = pack_samples([ds[i] for i in range(lo, lo + 4)])
        plan = ops.RaggedPlan(rb.hw, "cuda")
        _, conf = pipe.run_batch_ragged(rb.images.cuda(), plan, rb.cls.cuda(), rb.labels.cuda(), S=96, conf=(0.7, 0.25))
        for b, name in enumerate(rb.names):
            got = np.asarray(Image.open(d1 / (name + ".png")))
            assert got.dtype == np.uint8 and np.array_equal(got, host(plan.label(conf, b))), name
            names.append(name)
    assert sorted(os.listdir(d1)) == sorted(n + ".png" for n in names)
    assert torch.equal(pipe.hist_conf.cpu(), conf_total.cpu())
    _, total_api = infer_lam.validate(parse(common + ["--conf_label_dir", str(d2), "--api_path", "true"]))
    assert torch.equal(infer_lam.validate.last_conf[1].cpu(), conf_total.cpu())
    for n in names:
        assert (d2 / (n + ".png")).read_bytes() == (d1 / (n + ".png")).read_bytes(), n


# ------------------------------------------------------------------ the other regimes: the stage only reads the step's cams
@pytest.mark.parametrize("regime", ["flip", "optimised"])
def test_other_regimes_feed_their_own_cams(ops, golden, regime):
    """TrainingFreePipeline with the flip fuse and OptimisedLamPipeline (--training_free false) through the shared back half: with
    conf= the main labels and matrix stay what conf=None gives, and the confident labels are pipeline.conf_labels_ragged over the
    step's own inputs and cams."""
    from excel_amd.pipeline import OptimisedLamPipeline, TrainingFreePipeline, conf_labels_ragged
    S, F_ = 96, 4
    if regime == "flip":
        rs = np.random.RandomState(3)
        text = rs.standard_normal((9, 64)).astype(np.float32)
        text /= np.linalg.norm(text, axis=1, keepdims=True)
        model, _ = tiny_model(text.T.copy(), gemm_mode="f32")
        make = lambda: TrainingFreePipeline(model, num_classes=F_ + 1, smax=3, tta_flip=True)
    else:
        from test_gpu_lam_optimised import _tiny_decoder_model
        model = _tiny_decoder_model(golden, "f32")[0]
        make = lambda: OptimisedLamPipeline(model, num_classes=F_ + 1, smax=3)
    imgs, gts, cls = _ragged_samples()
    flat = lambda xs: dev(np.concatenate([x.reshape(-1) for x in xs]))
    plan = ops.RaggedPlan(RAGGED_HW, "cuda")
    plain, pipe = make(), make()
    ref = plain.run_batch_ragged(flat(imgs), plan, dev(cls), flat(gts), S=S)
    lab, conf, inter = pipe.run_batch_ragged(flat(imgs), plan, dev(cls), flat(gts), S=S, conf=(HIGH, LOW), return_intermediates=True)
    assert torch.equal(lab, ref) and torch.equal(pipe.hist, plain.hist) and plain.hist_conf is None
    again = conf_labels_ragged(inter["inputs"], inter["cams"], plan, inter["conf_plan"], 3, inter["ncls"] + 1, inter["cls_idx"], HIGH, LOW,
                               pipe.dilations, pipe.num_iter)[0]
    assert torch.equal(conf, again)
    lab2, conf2 = pipe.run_batch_ragged(flat(imgs), plan, dev(cls), None, S=S, conf=(HIGH, LOW))      # step buffers: the same labels
    assert torch.equal(lab2, lab) and torch.equal(conf2, conf)
    kept = int(((host(conf) < F_ + 1) & (host(flat(gts)) < F_ + 1)).sum())
    assert int(pipe.hist_conf.sum()) == kept and 0 < kept < int(pipe.hist.sum())
