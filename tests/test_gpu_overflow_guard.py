"""GPU tests of the overflow guard of the f16 GEMM modes: the per-image non-finite count (excel_nonfinite_count), the masked confusion
update (excel_confusion_accumulate_masked), the pipelines' guard on a network whose block-0 MLP really leaves the IEEE-half range for
some images of a batch and not for the others, and tools/infer_lam --overflow_guard on that network."""
import numpy as np
import pytest

import oracle
from oracle import vit as ov
from oracle.vit import VitConfig, make_vit_weights

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

TINY = VitConfig(width=128, layers=8, heads=2, patch=16, out_dim=64, input_resolution=64, n_surgery=5)      # tests/test_gpu_pipeline.py
TINY_KW = dict(width=128, layers=8, heads=2, patch=16, output_dim=64, input_resolution=64)
HALF_MAX = 65504.0          # the largest finite IEEE half
HALF_INF = 65520.0          # the smallest magnitude that rounds to infinity (round to nearest even)


def dev(a):
    return torch.as_tensor(np.ascontiguousarray(a)).cuda()


def host(t):
    return t.detach().cpu().numpy()


@pytest.fixture(scope="module")
def gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import excel_amd.ops  # noqa: F401  (raises if libexcel_hip.so is missing: no fallback)
    return True


# ------------------------------------------------------------------ 1. the count kernel against numpy
PLANTS = np.array([0x7f800000, 0xff800000, 0x7fc00000, 0x7f800001], np.uint32)       # +inf, -inf, a quiet NaN, a signalling payload
FINITE_EDGES = np.array([0x7f7fffff, 0xff7fffff, 0x00000001, 0x807fffff, 0x80000000, 0x00000000], np.uint32)   # +-FLT_MAX, denormals, -0, 0


def _count_bits(seed, B, per_image):
    """uint32 bit patterns [B, per_image]: seeded finite values with the finite edge cases sprinkled in, non-finite values planted at the
    first and last element of every image (= both sides of every image boundary, and the last element of the tensor) and, where
    there is room, inside."""
    rs = np.random.RandomState(seed)
    n = B * per_image
    u = (rs.standard_normal(n) * 10.0 ** rs.uniform(-30, 30, n)).astype(np.float32).view(np.uint32).copy()
    assert not np.any((u & 0x7f800000) == 0x7f800000)
    if per_image >= 5:
        where = rs.choice(n, min(n // 2, 4 * len(FINITE_EDGES)), replace=False)
        u[where] = FINITE_EDGES[np.arange(len(where)) % len(FINITE_EDGES)]
    spots = sorted({b * per_image for b in range(B)} | {(b + 1) * per_image - 1 for b in range(B)})
    if per_image >= 181:
        spots = sorted(set(spots) | {int(i) for i in rs.choice(n, 9 + seed % 5, replace=False)} | {per_image + 3, per_image + 4, 2 * per_image - 5})
    u[spots] = PLANTS[np.arange(len(spots)) % len(PLANTS)]
    return u.reshape(B, per_image)


def _np_count(u):
    return ((u & 0x7f800000) == 0x7f800000).sum(1).astype(np.int32)


@pytest.mark.parametrize("per_image", [1, 5, 181, 4099])
def test_nonfinite_count_vs_numpy(gpu, per_image):
    from excel_amd import ops
    B = 3
    u1, u2 = _count_bits(per_image, B, per_image), _count_bits(per_image + 1, B, per_image)
    e1, e2 = _np_count(u1), _np_count(u2)
    assert e1.min() >= 1 and (per_image == 1 or e1.max() < per_image)              # every image is hit, and not everything counts
    for shift in (0, 1):                 # the tensor as allocated / a view that starts one float in (4-byte aligned only)
        xs = []
        for u in (u1, u2):
            raw = torch.zeros(B * per_image + shift, dtype=torch.int32, device="cuda")
            raw[shift:] = dev(u.reshape(-1).view(np.int32))
            x = raw.view(torch.float32)[shift:].view(B, per_image)
            assert x.data_ptr() % 16 == 4 * shift and x.is_contiguous()
            assert np.array_equal(host(x.view(torch.int32)).view(np.uint32), u)    # the bits arrived (payload NaNs included)
            xs.append(x)
        c = ops.nonfinite_count(xs[0])
        assert c.dtype == torch.int32 and tuple(c.shape) == (B,)
        assert np.array_equal(host(c), e1), (shift, host(c), e1)
        c2 = ops.nonfinite_count(xs[1], out=c, init=False)                          # a second tensor's counts are added
        assert c2 is c and np.array_equal(host(c), e1 + e2), (shift, host(c), e1 + e2)
        junk = torch.full((B,), 12345, dtype=torch.int32, device="cuda")
        assert np.array_equal(host(ops.nonfinite_count(xs[1], out=junk, init=True)), e2)     # init writes, whatever was there
        clean = torch.from_numpy(np.where((u1 & 0x7f800000) == 0x7f800000, FINITE_EDGES[0], u1).view(np.int32)).cuda().view(torch.float32)
        assert np.array_equal(host(ops.nonfinite_count(clean)), np.zeros(B, np.int32))


def test_nonfinite_count_argument_checks(gpu):
    from excel_amd import ops
    x = torch.zeros((2, 8), device="cuda")
    with pytest.raises(ValueError):
        ops.nonfinite_count(x, init=False)                                                    # nothing to add to
    with pytest.raises(ValueError):
        ops.nonfinite_count(x, out=torch.zeros(3, dtype=torch.int32, device="cuda"))
    with pytest.raises(TypeError):
        ops.nonfinite_count(x.double())


# ------------------------------------------------------------------ 2. the masked confusion update
RAGGED_SIZES = [(5, 7), (16, 64), (17, 65), (1, 1)]
NC = 21


def _conf_maps(seed, sizes):
    rs = np.random.RandomState(seed)
    gts, preds = [], []
    for h, w in sizes:
        gt = rs.randint(0, NC, (h, w)).astype(np.uint8)
        r = rs.rand(h, w)
        gt[r < 0.1] = 255                                               # ignore
        gt[(r >= 0.1) & (r < 0.2)] = rs.randint(NC, 255)                # a label beyond the classes: dropped like 255
        pr = rs.randint(0, NC, (h, w)).astype(np.uint8)
        gts.append(gt)
        preds.append(pr)
    gts[-1][...] = 3                                                    # (the 1 x 1 image counts: a valid pair)
    return gts, preds


def _np_conf(gts, preds, keep):
    out = np.zeros((NC, NC), np.int64)
    for b in keep:
        g, p = gts[b].reshape(-1).astype(np.int64), preds[b].reshape(-1).astype(np.int64)
        m = (g < NC) & (p < NC)
        out += np.bincount(NC * g[m] + p[m], minlength=NC * NC).reshape(NC, NC)
    return out


@pytest.mark.parametrize("layout", ["ragged", "uniform"])
def test_masked_confusion_vs_numpy(gpu, layout):
    from excel_amd import ops
    sizes = RAGGED_SIZES if layout == "ragged" else [(9, 11)] * 3
    B = len(sizes)
    gts, preds = _conf_maps(7 + B, sizes)
    if layout == "ragged":
        plan = ops.RaggedPlan(sizes, "cuda")
        gt_d = dev(np.concatenate([g.reshape(-1) for g in gts]))
        pr_d = dev(np.concatenate([p.reshape(-1) for p in preds]))
    else:
        plan = None
        gt_d, pr_d = dev(np.stack(gts)), dev(np.stack(preds))
    start = np.random.RandomState(3).randint(0, 1000, (NC, NC)).astype(np.int64)             # a non-zero histogram to add to
    patterns = [[]] + [[b] for b in range(B)] + [list(range(B))]
    for skipped in patterns:
        skip = np.zeros(B, np.int32)
        skip[skipped] = [1, 7, 2 ** 30, -1][:len(skipped)] if len(skipped) > 1 else 5        # any non-zero value skips
        hist = dev(start.copy())
        out = ops.confusion_accumulate_masked(gt_d, pr_d, NC, dev(skip), hist, plan=plan)
        assert out is hist
        keep = [b for b in range(B) if b not in skipped]
        assert np.array_equal(host(hist), start + _np_conf(gts, preds, keep)), (layout, skipped)
        if not skipped:                                                                     # bit for bit the unmasked entry
            plain = ops.confusion_accumulate(gt_d, pr_d, NC, dev(start.copy()))
            assert torch.equal(hist, plain)
    fresh = ops.confusion_accumulate_masked(gt_d, pr_d, NC, dev(np.zeros(B, np.int32)), plan=plan)
    assert np.array_equal(host(fresh), _np_conf(gts, preds, range(B)))
    with pytest.raises(ValueError):
        ops.confusion_accumulate_masked(gt_d, pr_d, NC, dev(np.zeros(B + 1, np.int32)), plan=plan)


# ------------------------------------------------------------------ 3. the pipelines on a real overflow
MEAN = np.array([123.675, 116.28, 103.53], np.float32)
STD = np.array([58.395, 57.12, 57.375], np.float32)
B6, S6, NFG = 6, 64, 4
FC = "transformer.resblocks.0.mlp.c_fc."


HOT_GROUP = [0, 1, 2]


def _six_images(seed=56):
    """Six 64 x 64 uint8 images: a block texture each, blended with noise of a different level per image, mirror-symmetric (the optimised
    regime also runs the mirrored image: it then sees the same maxima).  The order puts the three images with the largest block-0
    maxima FIRST (asserted in _overflowing_weights): the f16 attention kernels read a full 64-row tile from an image's first token on,
    which at 17 tokens covers the next three images, and a NaN row there reaches the image through 0 x NaN products.  Measured on the
    device: with images 1 and 2 over the limit, image 0 (15 % under it, finite after block 0) left block 1 non-finite, images 3-5 stayed
    finite; with images 3-5 over the limit all six were non-finite.  The guard flags what IS non-finite either way (an image next to a
    hot one is simply re-run too); for "exactly the expected images" to be a fair precondition no cold image precedes a hot one."""
    rs = np.random.RandomState(seed)
    out = []
    for b in range(B6):
        base = rs.randint(0, 256, (4, 2, 3)).astype(np.float32)
        half = np.kron(base, np.ones((16, 16, 1), np.float32))
        amp = [0, 4, 16, 48, 96, 160][b]
        half = half * (1.0 - amp / 200.0) + rs.standard_normal((64, 32, 3)) * amp
        half = np.clip(np.rint(half), 0, 255).astype(np.uint8)
        out.append(np.concatenate([half, half[:, ::-1]], 1))
    out = [out[i] for i in (1, 2, 5, 0, 3, 4)]
    rs = np.random.RandomState(seed + 1)
    gts = []
    for _ in range(B6):
        gt = rs.randint(0, NFG + 1, (S6, S6)).astype(np.uint8)
        gt[rs.rand(S6, S6) < 0.03] = 255
        gts.append(gt)
    cls = np.zeros((B6, NFG), np.float32)
    for b, c in enumerate([[0], [1, 2], [0, 1, 2, 3], [3], [2, 0], [1]]):
        cls[b, c] = 1
    return out, gts, cls


def _normalised(u8):
    return ((u8.astype(np.float32) - MEAN) / STD).transpose(2, 0, 1).astype(np.float32)


def _gelu_max(img, w):
    """max |QuickGELU output| of block 0's MLP for one normalised image [3,S,S], from the oracle's own functions."""
    x = ov.patch_embed(img, w, TINY)
    x = np.concatenate([w["class_embedding"][None, :], x], 0) + w["positional_embedding"]
    x = ov.layer_norm(x, w["ln_pre.weight"], w["ln_pre.bias"]).astype(np.float32)
    p = "transformer.resblocks.0."
    o, _ = ov.mha_block_attention(ov.layer_norm(x, w[p + "ln_1.weight"], w[p + "ln_1.bias"]), p, w, TINY)
    y = ov.layer_norm(x + o, w[p + "ln_2.weight"], w[p + "ln_2.bias"])
    return float(np.abs(ov.quick_gelu(y @ w[FC + "weight"].T + w[FC + "bias"])).max())


def _to_half_values(w):
    return {k: (np.asarray(v, np.float32).astype(np.float16).astype(np.float32) if np.asarray(v).dtype == np.float32 else v) for k, v in w.items()}


def _overflowing_weights(imgs_u8, fp16_weights, with_flip):
    """seed-11 TINY weights with block 0's mlp.c_fc scaled by s, s = 65 504 / the geometric mean of the widest gap between the sorted
    per-image maxima (with_flip: an image's maximum is taken over the image and its mirror - the optimised regime runs both).
    -> (weights, per-image maxima WITH the final weights, expected flags).  The three preconditions on the maxima are asserted here."""
    views = [[_normalised(u)] + ([_normalised(u)[:, :, ::-1].copy()] if with_flip else []) for u in imgs_u8]
    w = make_vit_weights(TINY, seed=11)
    if fp16_weights:
        w = _to_half_values(w)
    m1 = np.array([max(_gelu_max(v, w) for v in vs) for vs in views])
    srt = np.sort(m1)
    k = int(np.argmax(srt[1:] / srt[:-1]))
    s = np.float32(HALF_MAX / np.sqrt(srt[k] * srt[k + 1]))
    w[FC + "weight"] = (w[FC + "weight"] * s).astype(np.float32)
    w[FC + "bias"] = (w[FC + "bias"] * s).astype(np.float32)
    if fp16_weights:
        w = _to_half_values(w)
        assert np.isfinite(w[FC + "weight"]).all()
    m = np.array([max(_gelu_max(v, w) for v in vs) for vs in views])
    expect = m >= HALF_INF
    print("overflow case: s = %.1f, maxima at s = 1 %s, with the scaled weights %s -> flagged %s" % (s, np.round(m1, 3), np.round(m), np.flatnonzero(expect)))
    assert 1 <= int(expect.sum()) <= B6 - 1, m                                     # somebody overflows, somebody does not
    assert np.all(np.abs(m / HALF_MAX - 1.0) >= 0.01), m                             # nobody within 1 % of the limit
    assert np.all(np.isfinite(m))
    assert list(np.flatnonzero(expect)) == HOT_GROUP, m                              # the hot images come first (see _six_images)
    return w, m, expect


def _np_hist(gts, labels, which, nc=NFG + 1):
    out = np.zeros((nc, nc), np.int64)
    for b in which:
        out += oracle.evaluate.fast_hist(gts[b].reshape(-1), labels[b].reshape(-1), nc)
    return out


def _nonfinite_images(t):
    a = host(t)
    return ~np.isfinite(a.reshape(a.shape[0], -1)).all(1)


_CASES = {}


def _case(kind, mode, golden):
    """One overflow case, checked once and shared (test 4 composes its expectation from it): kind "tf" = TrainingFreePipeline,
    "opt" = OptimisedLamPipeline on the tiny decoder head of tests/test_gpu_lam_optimised.py; mode = the f16 GEMM mode."""
    key = (kind, mode)
    if key in _CASES:
        return _CASES[key]
    from excel_amd import ops
    from excel_amd.model import ExCEL_model
    from excel_amd.pipeline import OptimisedLamPipeline, TrainingFreePipeline
    imgs, gts, cls = _six_images()
    w, maxima, expect = _overflowing_weights(imgs, fp16_weights=(mode == "f16x2"), with_flip=(kind == "opt"))
    rs = np.random.RandomState(1)
    text = rs.standard_normal((9, 64)).astype(np.float32)
    text /= np.linalg.norm(text, axis=1, keepdims=True)
    kw = {}
    if kind == "opt":
        g = golden("decoder_tiny.npz")
        sd = {"decoder_fts_fuse." + k[len("fuse."):]: g[k] for k in g.files if k.startswith("fuse.")}
        sd.update({"decoder." + k[len("dec."):]: g[k] for k in g.files if k.startswith("dec.")})
        kw = dict(embedding_dim=32, in_channels=128, decoder_state_dict=sd)
    model = ExCEL_model(clip_model="tiny", num_classes=NFG + 1, img_size=S6, mode="train", state_dict=w, vit_cfg=TINY_KW,
                        text_attr=text.T.copy(), gemm_mode=mode, **kw)
    h = model.encoder.visual.handle()
    assert h.gemm_mode() == mode
    Pipe = OptimisedLamPipeline if kind == "opt" else TrainingFreePipeline
    mk = lambda guard: Pipe(model, num_classes=NFG + 1, smax=NFG, guard=guard)

    def run(pipe, which, want_inter=False):
        plan = ops.RaggedPlan([(S6, S6)] * len(which), "cuda")
        hwc = dev(np.concatenate([imgs[b].reshape(-1) for b in which]))
        gt = dev(np.concatenate([gts[b].reshape(-1) for b in which]))
        out = pipe.run_batch_ragged(hwc, plan, dev(cls[which]), gt, S=S6, return_intermediates=want_inter)
        lab = host(out[0] if want_inter else out).reshape(len(which), S6, S6)
        return (lab, out[1]) if want_inter else lab

    everyone = list(range(B6))
    flagged = [int(b) for b in np.flatnonzero(expect)]
    clean = [b for b in everyone if b not in flagged]
    # precondition 3: exact fp32 is finite everywhere; the f16 mode is non-finite in attr for exactly the expected images
    h.set_gemm_mode("f32")
    _, inter = run(mk(None), everyone, want_inter=True)
    for name in ("attr", "w_aff", "refined"):
        assert not _nonfinite_images(inter[name]).any(), name
    f32_sub = run(mk(None), flagged)                                                  # the reference of the second pass: the same sub-batch, guard off
    h.set_gemm_mode(mode)
    off = mk(None)
    lab_off, inter = run(off, everyone, want_inter=True)
    assert np.array_equal(_nonfinite_images(inter["attr"]), expect), (_nonfinite_images(inter["attr"]), expect, maxima)
    inputs = inter["inputs"]
    assert off.last_guard is None and off.last_flags is None
    # the guarded step
    skip = mk("skip")
    lab_skip = run(skip, everyone)
    ticket = skip.last_guard
    flags = np.array(ticket.flags())
    assert ticket.ready()
    assert np.array_equal(flags != 0, expect), (flags, expect)
    assert np.array_equal(host(skip.last_flags), flags) and skip.last_flags.dtype == torch.int32
    assert np.array_equal(lab_skip[clean], lab_off[clean])                            # bit for bit where nothing overflowed
    assert np.array_equal(host(skip.hist), _np_hist(gts, lab_skip, clean))            # only the unflagged images are scored
    assert not np.array_equal(host(off.hist), host(skip.hist))                        # (the unguarded run did score the others)
    # the second pass as infer_lam runs it: flagged images, ascending, one batch, exact fp32, observe
    obs = mk("observe")
    with obs.exact_mode() as same:
        assert same is obs and h.gemm_mode() == "f32"
        lab_second = run(obs, flagged)
        flags2 = np.array(obs.last_guard.flags())
    assert h.gemm_mode() == mode                                                      # the mode it found is back
    assert not flags2.any(), flags2                                                   # fp32 is finite on these weights
    assert np.array_equal(lab_second, f32_sub)
    composed = lab_skip.copy()
    composed[flagged] = lab_second
    assert np.array_equal(host(skip.hist) + host(obs.hist), _np_hist(gts, composed, everyone))
    _CASES[key] = dict(model=model, imgs=imgs, gts=gts, cls=cls, expect=expect, flagged=flagged, composed=composed, lab_off=lab_off,
                       inputs=inputs, mk=mk, mode=mode)
    return _CASES[key]


@pytest.mark.parametrize("kind,mode", [("tf", "f16x3"), ("tf", "f16x2"), ("opt", "f16x3")])
def test_pipeline_guard_on_a_real_overflow(gpu, golden, kind, mode):
    """Block 0's MLP of the tiny network leaves the half range for some images of the batch and not for the others.  The guarded step
    flags exactly those, scores exactly the others, and the exact-fp32 second pass gives the flagged ones fp32's labels.
    (All the assertions of the shared case live in _case.)"""
    c = _case(kind, mode, golden)
    assert 1 <= len(c["flagged"]) <= B6 - 1


def test_uniform_step_and_unsupported_paths(gpu, golden):
    """run_batch carries the same guard as run_batch_ragged; the bench / training paths refuse a guard with a reason."""
    from excel_amd.pipeline import TrainingFreePipeline, ValidationPipeline
    c = _case("tf", "f16x3", golden)
    gts, cls = dev(np.stack(c["gts"])), dev(c["cls"])
    pipe = c["mk"]("skip")
    labels = host(pipe.run_batch(c["inputs"], cls, gts))
    flags = np.array(pipe.last_guard.flags())
    assert np.array_equal(flags != 0, c["expect"])
    clean = [b for b in range(B6) if b not in c["flagged"]]
    assert np.array_equal(labels[clean], c["lab_off"][clean])
    assert np.array_equal(host(pipe.hist), _np_hist(c["gts"], labels, clean))
    watch = c["mk"]("observe")
    labels_w = host(watch.run_batch(c["inputs"], cls, gts))
    assert np.array_equal(np.array(watch.last_guard.flags()), flags)                  # the same counts ...
    assert np.array_equal(host(watch.hist), _np_hist(c["gts"], labels_w, range(B6)))  # ... and nothing skipped
    for call in (lambda: pipe.run_batch_split(c["inputs"], cls, gts), lambda: pipe.run_batch_overlapped(c["inputs"], cls, gts)):
        with pytest.raises(ValueError, match="overflow guard"):
            call()
    with pytest.raises(ValueError, match="guard"):
        TrainingFreePipeline(c["model"], num_classes=NFG + 1, smax=NFG, guard="maybe")
    opt = _case("opt", "f16x3", golden)
    with pytest.raises(ValueError, match="overflow guard"):
        ValidationPipeline(opt["model"], num_classes=NFG + 1, smax=NFG, guard="skip")


# ------------------------------------------------------------------ 4. the program
class _SixSet:
    """The six images of case 3 as a ragged data set (name, image u8 [h,w,3], label u8 [h,w], cls f32 [F])."""

    def __init__(self, case):
        self.c = case

    def __len__(self):
        return B6

    def max_k(self):
        return NFG

    def __getitem__(self, i):
        return f"g{int(i):03d}", self.c["imgs"][i], self.c["gts"][i], self.c["cls"][i]


def test_infer_lam_overflow_guard_policies(gpu, golden, tmp_path):
    from PIL import Image
    from excel_amd.tools import infer_lam
    c = _case("tf", "f16x3", golden)
    names = [f"g{b:03d}" for b in range(B6)]
    bad = [names[b] for b in c["flagged"]]

    def run(policy, guard, tag):
        d = tmp_path / tag
        args = infer_lam.get_parser().parse_args(["--num_classes", str(NFG + 1), "--resize_size", str(S6), "--batch_size", str(B6),
                                                  "--num_workers", "2", "--overflow_guard", policy, "--save_label", "true",
                                                  "--label_dir", str(d)])
        _, total = infer_lam.validate(args, dataset=_SixSet(c), pipe=c["mk"](guard))
        return host(total), d

    total, d = run("rerun", "skip", "rerun")
    assert np.array_equal(total, _np_hist(c["gts"], c["composed"], range(B6)))
    for b, n in enumerate(names):
        assert np.array_equal(np.array(Image.open(d / (n + ".png"))), c["composed"][b]), n
    rep = infer_lam.validate.last_guard
    assert rep["policy"] == "rerun" and rep["mode"] == "f16x3" and rep["checked"] == B6
    assert rep["flagged"] == bad and rep["rerun"] == len(bad) and rep["nonfinite_in_f32"] == []
    assert c["model"].encoder.visual.handle().gemm_mode() == "f16x3"
    with pytest.raises(RuntimeError) as e:
        run("raise", "skip", "raise")
    assert all(n in str(e.value) for n in bad) and "f16x3" in str(e.value)
    assert not any(n in str(e.value) for n in names if n not in bad)
    total_off, _ = run("off", None, "off")
    assert np.array_equal(total_off, _np_hist(c["gts"], c["lab_off"], range(B6)))     # today's histogram, NaN images and all
    assert infer_lam.validate.last_guard["policy"] == "off" and infer_lam.validate.last_guard["checked"] == 0
    total_auto, _ = run("auto", "skip", "auto")                                        # auto on the batched GPU loop in an f16 mode = rerun
    assert infer_lam.validate.last_guard["policy"] == "rerun" and np.array_equal(total_auto, total)
