"""GPU tests of the flip / multi-scale LAM fuse: the op (excel_lam_tta_fuse) against the chain of existing ops it replaces (bit for bit)
and against a float64 restatement, its non-finite rule and argument checks; the pipeline option (tta_scales / tta_flip) composed from
the existing stages and against the oracle of the whole chain; the overflow guard behind it; and the program (infer_lam --cam_scales
--cam_flip) on the batched and the per-image path."""
import ctypes
import os
import sys

import numpy as np
import pytest

import oracle
from oracle.vit import VitConfig, make_vit_weights

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _lam_tta_ref as R  # noqa: E402

TINY = VitConfig(width=128, layers=8, heads=2, patch=16, out_dim=64, input_resolution=64, n_surgery=5)
TINY_KW = dict(width=128, layers=8, heads=2, patch=16, output_dim=64, input_resolution=64)
S = 64
SCALES = (1.0, 0.5, 1.5)
SIZES = [(64, 4), (32, 2), (96, 6)]
K_F32 = 3.0                      # tests/_attn_shapes.py K_FACTOR["f32"]


def dev(a):
    return torch.as_tensor(np.ascontiguousarray(a)).cuda()


def host(t):
    return t.detach().cpu().numpy()


def maxabs(a, b):
    return float(np.max(np.abs(np.asarray(a, np.float64) - np.asarray(b, np.float64))))


@pytest.fixture(scope="module")
def gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import excel_amd.ops  # noqa: F401  (raises if libexcel_hip.so is missing: no fallback)
    return True


def _chain(maps, grids, g_out):
    """The existing ops the fuse equals for flip = 1: lam_scale_accumulate per scale, plane_minmax_normalize_, a permute to [B,P,F]."""
    from excel_amd import ops
    acc = None
    for s, (m, g) in enumerate(zip(maps, grids)):
        acc = ops.lam_scale_accumulate(m, acc, g, g_out, g_out, init=(s == 0))
    B, F = acc.shape[:2]
    return ops.plane_minmax_normalize_(acc).reshape(B, F, g_out * g_out).permute(0, 2, 1).contiguous()


# ------------------------------------------------------------------ 1. the op
@pytest.mark.parametrize("ci", range(len(R.CASES)))
def test_fuse_vs_chain_and_float64(gpu, ci):
    from excel_amd import ops
    B, F, g_out, grids = R.CASES[ci]
    for seed in range(3):
        maps = R.case_maps(ci, seed, flip=True)
        ref, rng = R.lam_tta_ref(maps, grids, g_out, True)
        assert rng >= 1.0, rng                                      # precondition: the normalisation cannot amplify
        d = [dev(m) for m in maps]
        got = ops.lam_tta_fuse(d, grids, g_out, True)
        assert got.shape == (B, g_out * g_out, F) and got.dtype == torch.float32
        assert torch.equal(got, _chain(d, grids, g_out)), (ci, seed)
        err1 = maxabs(host(got), ref)
        half = R.case_maps(ci, seed, flip=False)
        ref0, rng0 = R.lam_tta_ref(half, grids, g_out, False)
        assert rng0 >= 1.0, rng0
        out = torch.full((B, g_out * g_out, F), float("nan"), device="cuda")
        got0 = ops.lam_tta_fuse([dev(m) for m in half], grids, g_out, False, out=out)
        assert got0 is out
        err0 = maxabs(host(got0), ref0)
        print(f"[lam_tta_fuse] case {ci} seed {seed}: flip error {err1:.2e}, no-flip error {err0:.2e} (bound 2e-5), ranges {rng:.2f} / {rng0:.2f}")
        assert err1 < 2e-5 and err0 < 2e-5


def test_single_scale_constant_and_mirror(gpu):
    from excel_amd import ops
    rs = np.random.RandomState(4)
    attr = dev((4 * rs.rand(6, 36, 5)).astype(np.float32))
    assert torch.equal(ops.lam_tta_fuse([attr], (6,), 6, True), ops.flip_max_normalize(attr, 6))
    # a constant plane gives zeros (class 1), whatever the other classes hold
    maps = [dev((4 * rs.rand(4, g * g, 3)).astype(np.float32)) for g in (4, 2)]
    for m in maps:
        m[:, :, 1] = 2.5
    out = ops.lam_tta_fuse(maps, (4, 2), 4, True)
    assert not out[:, :, 1].any() and bool((out[:, :, 0].amax(1) > 0.99).all())
    # one hot value at column 0 of a plane of the mirrored half lands at column g_out - 1
    g = 5
    one = torch.zeros((2, g * g, 2), device="cuda")
    one[1, 3 * g + 0, 1] = 1.0
    out = host(ops.lam_tta_fuse([one], (g,), g, True))
    assert out[0, 3 * g + g - 1, 1] > 0.99 and np.count_nonzero(out) == 1
    out = host(ops.lam_tta_fuse([one[1:]], (g,), g, False))                   # without the flip it stays where it is
    assert out[0, 3 * g, 1] > 0.99 and np.count_nonzero(out) == 1


@pytest.mark.parametrize("bad", [float("nan"), float("inf")])
def test_nonfinite_value_takes_its_plane_and_no_other(gpu, bad):
    from excel_amd import ops
    B, F, g_out, grids = R.CASES[0]
    maps = [dev(m) for m in R.case_maps(0, 0, flip=True)]
    clean = ops.lam_tta_fuse(maps, grids, g_out, True)
    assert bool(torch.isfinite(clean).all())
    maps[1][B + 1, 3, 2] = bad                                                # image 1, class 2, the mirrored half of scale 1
    got = ops.lam_tta_fuse(maps, grids, g_out, True)
    assert bool(torch.isnan(got[1, :, 2]).all())
    keep = torch.ones((B, F), dtype=torch.bool, device="cuda")
    keep[1, 2] = False
    assert torch.equal(got.permute(0, 2, 1)[keep], clean.permute(0, 2, 1)[keep])
    assert host(ops.nonfinite_count(got)).tolist() == [0, g_out * g_out]      # what the overflow guard sees


def test_argument_errors_launch_nothing(gpu):
    from excel_amd import ops
    from excel_amd._lib import lib
    m = torch.ones((2, 16, 3), device="cuda")
    out = torch.full((1, 16, 3), 7.0, device="cuda")
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

    def call(ns, gs, g_out, F):
        ptrs = (ctypes.c_void_p * 9)(*[m.data_ptr()] * 9)
        g = (ctypes.c_int32 * 9)(*(list(gs) + [4] * (9 - len(gs))))
        return lib().excel_lam_tta_fuse(ptrs, g, ns, 1, 1, F, g_out, ctypes.c_void_p(out.data_ptr()), st)

    assert call(1, [4], 4, 3) == 0
    torch.cuda.synchronize()
    assert bool((out == 0).all())                                             # (a plane of ones: the call itself works)
    out.fill_(7.0)
    for args in ((9, [4] * 9, 4, 3), (1, [0], 4, 3), (1, [4], 49, 3), (1, [4], 4, 0), (0, [4], 4, 3), (2, [4, 49], 4, 3)):
        assert call(*args) == -1, args                                        # EXCEL_ERR_ARG
        assert b"lam_tta_fuse" in lib().excel_last_error()
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())                                           # nothing was launched
    with pytest.raises(ValueError, match="9 scales"):
        ops.lam_tta_fuse([m] * 9, [4] * 9, 4, True)
    with pytest.raises(ValueError, match="49"):
        ops.lam_tta_fuse([m], [4], 49, True)
    with pytest.raises(ValueError, match="grid 0"):
        ops.lam_tta_fuse([m], [0], 4, True)
    with pytest.raises(ValueError, match="F >= 1"):
        ops.lam_tta_fuse([m[:, :, :0]], [4], 4, True)
    with pytest.raises(ValueError, match="must be"):
        ops.lam_tta_fuse([m, m], [4, 2], 4, True)                             # the second map is not [2, 4, 3]
    assert bool((out == 7.0).all())


# ------------------------------------------------------------------ 2. the pipeline
_NET = {}


def _net(gemm_mode=None):
    """The tiny net at S = 64 (text: 4 classes + 5 background rows), built once per GEMM mode."""
    if gemm_mode not in _NET:
        from excel_amd.model import ExCEL_model
        rs = np.random.RandomState(21)
        text = rs.standard_normal((9, 64)).astype(np.float32)
        text /= np.linalg.norm(text, axis=1, keepdims=True)
        w = make_vit_weights(TINY, seed=11)
        model = ExCEL_model(clip_model="tiny", num_classes=5, img_size=S, mode="train", state_dict=w, vit_cfg=TINY_KW,
                            text_attr=text.T.copy(), gemm_mode=gemm_mode)
        _NET[gemm_mode] = (model, w, text)
    return _NET[gemm_mode]


RAGGED_HW = [(40, 52), (64, 64), (33, 70)]


def _ragged_batch():
    rs = np.random.RandomState(6)
    imgs = [rs.randint(0, 256, (h, w, 3)).astype(np.uint8) for h, w in RAGGED_HW]
    gts = [rs.randint(0, 5, (h, w)).astype(np.uint8) for h, w in RAGGED_HW]
    cls = np.zeros((3, 4), np.float32)
    for b, c in enumerate([[0, 3], [1], [2, 0]]):
        cls[b, c] = 1
    return imgs, gts, cls


def test_pipeline_composition_ragged(gpu):
    from excel_amd import ops
    from excel_amd.pipeline import TrainingFreePipeline
    model, _, _ = _net()
    imgs, gts, cls = _ragged_batch()
    plan = ops.RaggedPlan(RAGGED_HW, "cuda")
    hwc = dev(np.concatenate([i.reshape(-1) for i in imgs]))
    gt = dev(np.concatenate([g.reshape(-1) for g in gts]))
    cls_d = dev(cls)
    pipe = TrainingFreePipeline(model, num_classes=5, smax=2, tta_scales=SCALES, tta_flip=True)
    labels, inter = pipe.run_batch_ragged(hwc, plan, cls_d, gt, S=S, return_intermediates=True)
    # attr: the fuse over maps the test makes itself, one model call per network size
    maps = [model(ops.normalize_resize_u8_ragged_mirror(hwc, plan, S_s))[2] for S_s, _ in SIZES]
    attr = ops.lam_tta_fuse(maps, [g for _, g in SIZES], S // 16, True)
    assert torch.equal(inter["attr"], attr)
    assert not torch.equal(attr, maps[0][:3])
    # w_aff: that of the plain step on the same batch
    plain = TrainingFreePipeline(model, num_classes=5, smax=2)
    x = ops.normalize_resize_u8_ragged(hwc, plan, S)
    w_aff0 = model(x)[3].w_aff.clone()                                        # before anything downstream touches it
    lab_plain, inter_plain = plain.run_batch_ragged(hwc, plan, cls_d, gt, S=S, return_intermediates=True)
    assert torch.equal(inter["w_aff"], w_aff0) and torch.equal(inter_plain["w_aff"], w_aff0)
    assert torch.equal(inter["inputs"], x)                                    # PAR reads the un-mirrored scale-1.0 input
    # labels and hist: the existing stages on that attr
    idx, ncls, nchan = ops.cls_compact(cls_d, 2, want_nchan=True)
    refined = ops.refine_cams_with_aff_batched(attr, w_aff0, idx, ncls, S // 16, 0.79)
    assert torch.equal(inter["refined"], refined)
    rest = TrainingFreePipeline(model, num_classes=5, smax=2)
    lab2 = rest._ragged_back_half(x, plan, S // 16, refined, idx, ncls, nchan, gt, False, {})
    assert torch.equal(labels, lab2) and torch.equal(pipe.hist, rest.hist)
    assert not torch.equal(pipe.hist, plain.hist)                             # (the fuse does change the result)
    # flip only, and scales only, go through the same op
    for kw, ms, gs, fl in ((dict(tta_flip=True), maps[:1], [4], True),
                           (dict(tta_scales=SCALES), [m[:3] for m in maps], [4, 2, 6], False)):
        p = TrainingFreePipeline(model, num_classes=5, smax=2, **kw)
        _, it = p.run_batch_ragged(hwc, plan, cls_d, gt, S=S, return_intermediates=True)
        assert torch.equal(it["attr"], ops.lam_tta_fuse(ms, gs, S // 16, fl)), kw
    # None / False is the step as it is
    off = TrainingFreePipeline(model, num_classes=5, smax=2, tta_scales=None, tta_flip=False)
    lab_off = off.run_batch_ragged(hwc, plan, cls_d, gt, S=S)
    assert torch.equal(lab_off, lab_plain) and torch.equal(off.hist, plain.hist)


def test_pipeline_uniform_vs_oracle(gpu):
    """run_batch in exact fp32 against the float64 oracle of the whole chain (input resize, [x; x mirrored] through the ViT and the
    patch-text CAM per scale, the fuse).  Bound: test_multi_scale_lam_vs_oracle's 5e-4 for the same chain, or 3x (K_FACTOR["f32"]) the
    fp32 oracle's own deviation from the float64 one where that is larger."""
    from excel_amd.pipeline import TrainingFreePipeline
    from excel_amd.utils.camutils import tta_attr_map
    model, w, text = _net("f32")
    wo = oracle.vit.reload_self_attn(w, TINY, S // 16, "train")
    rs = np.random.RandomState(12)
    x = rs.standard_normal((2, 3, S, S)).astype(np.float32)
    cls = np.zeros((2, 4), np.float32)
    cls[0, [1, 2]] = 1
    cls[1, [3]] = 1
    pipe = TrainingFreePipeline(model, num_classes=5, smax=2, tta_scales=SCALES, tta_flip=True)
    _, inter = pipe.run_batch(dev(x), dev(cls), None, return_intermediates=True)
    ref = R.oracle_tta_attr(x, wo, TINY, text.T.copy(), 4, SIZES, True, f64=True)
    own = maxabs(R.oracle_tta_attr(x, wo, TINY, text.T.copy(), 4, SIZES, True, f64=False), ref)
    err = maxabs(host(inter["attr"]), ref)
    bound = max(5e-4, K_F32 * own)
    print(f"[tta attr vs float64 oracle] f32: max-abs error {err:.2e}, the fp32 oracle's own deviation {own:.2e}, bound {bound:.2e}")
    assert inter["attr"].shape == (2, 16, 4) and err < bound
    # the per-image API form is the same op on the same maps
    assert torch.equal(tta_attr_map(model, dev(x), SCALES, True), inter["attr"])


def test_guard_flags_the_image_behind_the_fuse(gpu, monkeypatch):
    """An inf in ONE scale's network input of image 1 (a plain tensor write behind the resize): its maps at that scale are NaN, the fuse
    hands NaN planes on, the guard flags image 1 alone and keeps it out of the histogram.
    Where the inf goes: at these token counts (37 per image at the 6 x 6 grid) the attention kernels' 64-row tiles reach from an image
    into the next ones of the same ViT call, and a non-finite image turns the image IN FRONT of it non-finite too (the existing
    kernels' behaviour, tests/test_gpu_overflow_guard.py _six_images; the guard then flags both).  For "image 1 alone" to be a fair
    expectation the inf is written into the mirrored copy of image 1 at network size 96, which is the first image of its ViT call (the
    step cuts that pass into calls of two images) - asserted below on the calls themselves."""
    from excel_amd import ops
    from excel_amd.pipeline import TrainingFreePipeline
    model, _, _ = _net()
    imgs, gts, cls = _ragged_batch()
    plan = ops.RaggedPlan(RAGGED_HW, "cuda")
    hwc = dev(np.concatenate([i.reshape(-1) for i in imgs]))
    gt = dev(np.concatenate([g.reshape(-1) for g in gts]))
    ref = TrainingFreePipeline(model, num_classes=5, smax=2, tta_scales=SCALES, tta_flip=True)
    lab_ref = ref.run_batch_ragged(hwc, plan, dev(cls), gt, S=S)
    real = ops.normalize_resize_u8_ragged_mirror

    def poisoned(hwc_packed, plan_, S_s, out=None):
        x = real(hwc_packed, plan_, S_s, out=out)
        if S_s == 96:
            x[plan_.B + 1, 0, 5, 7] = float("inf")
        return x
    monkeypatch.setattr(ops, "normalize_resize_u8_ragged_mirror", poisoned)
    calls, real_maps = [], model.attr_maps

    def spy(x):
        calls.append((int(x.shape[-1]), int(x.shape[0])))
        return real_maps(x)
    monkeypatch.setattr(model, "attr_maps", spy)
    pipe = TrainingFreePipeline(model, num_classes=5, smax=2, guard="skip", tta_scales=SCALES, tta_flip=True)
    labels, inter = pipe.run_batch_ragged(hwc, plan, dev(cls), gt, S=S, return_intermediates=True)
    flags = np.array(pipe.last_guard.flags())
    starts = np.cumsum([0] + [n for S_s, n in calls if S_s == 96])
    assert starts[-1] == 6 and 4 in starts[:-1], calls                        # the poisoned image has nobody in front of it in its call
    assert flags[1] > 0 and flags[0] == 0 and flags[2] == 0, flags
    assert bool(torch.isnan(inter["attr"][1]).all()) and bool(torch.isfinite(inter["attr"][[0, 2]]).all())
    assert bool(torch.isfinite(inter["w_aff"]).all())                         # scale 1.0 was clean
    want = np.zeros((5, 5), np.int64)
    for b in (0, 2):
        lab_b = host(plan.label(lab_ref, b)).reshape(-1)
        assert np.array_equal(host(plan.label(labels, b)).reshape(-1), lab_b)
        want += oracle.evaluate.fast_hist(gts[b].reshape(-1), lab_b, 5)
    assert np.array_equal(host(pipe.hist), want)                              # image 1's pixels are absent


# ------------------------------------------------------------------ 3. the program
def test_infer_lam_cam_scales_and_flip(gpu, tmp_path):
    import json
    from excel_amd.tools import infer_lam
    base = ["--synthetic", "6", "--ragged", "true", "--batch_size", "3", "--resize_size", "128"]
    tta = ["--cam_scales", "1.0,0.5,1.5", "--cam_flip", "true"]
    rec = tmp_path / "run.json"
    _, total = infer_lam.validate(infer_lam.get_parser().parse_args(base + tta + ["--json_out", str(rec)]))
    total = host(total)
    assert total.sum() > 0
    r = json.load(open(rec))
    assert r["cam_scales"] == [1.0, 0.5, 1.5] and r["cam_flip"] is True
    _, total_api = infer_lam.validate(infer_lam.get_parser().parse_args(base + tta + ["--api_path", "true"]))
    assert np.abs(total - host(total_api)).sum() <= 1e-4 * total.sum()        # batched == per-image API path
    _, total_plain = infer_lam.validate(infer_lam.get_parser().parse_args(base))
    assert host(total_plain).sum() == total.sum() and not np.array_equal(host(total_plain), total)
    # the consumers behind the step work as they are: label PNGs and the inline CRF stage
    lab, crf = tmp_path / "lab", tmp_path / "crf"
    more = ["--save_label", "true", "--label_dir", str(lab), "--crf_post", "true", "--crf_inline", "true", "--crf_label_dir", str(crf)]
    _, total_files = infer_lam.validate(infer_lam.get_parser().parse_args(base + tta + more))
    assert np.array_equal(host(total_files), total)
    for d in (lab, crf):
        assert len([f for f in os.listdir(d) if f.endswith(".png")]) == 6, d
    assert infer_lam.validate.last_crf[1].sum() > 0
