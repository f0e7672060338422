"""The CAM-to-label chain at COCO class counts: up to 18 present classes per image (datasets/coco.py: max_k() == 18), Smax = 18, Cmax = 19.

Everything behind the ViT works per present class, and past 8 classes the kernels are not plain loops: the random-walk mat-vec and the
streamed PAR step go through their channels in chunks of 8 (a second and a third chunk exist only here), the recomputing PAR step streams
3 + nch planes through a two-buffer LDS ring, the LAM DenseCRF keeps one value-row stride per group next to images of 2 channels, and
every workspace has Smax- / Cmax-dependent regions.  Each stage runs at the present-class pattern K = [18, 17, 16, 9, 8, 1] out of
F = 80 classes against the numpy oracle with the tolerance the suite already uses for that quantity, or bit for bit against the second
GPU path that must agree with it.  The last tests pin what an image with MORE present classes than Smax does (include/excel_hip.h,
excel_cls_compact) and run the tiny pipeline end to end with 18 classes.  Every test prints its figure before asserting it."""
import contextlib

import numpy as np
import pytest

import oracle
import _scratch as S
import test_gpu_cam_overlay as OV
import test_gpu_dcrf_lam as CRF
from _cam_overlay_ref import overlays
from _scratch_cases import pitched_mask
from test_gpu_ops import _smooth_maps, dev, host, maxabs, relmax

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

F = 80
SMAX, CMAX = 18, 19
K = [18, 17, 16, 9, 8, 1]
SIZES = [(40, 56), (17, 29), (20, 160), (33, 47), (5, 7), (16, 64)]
DIL = [1, 2, 4, 8, 12, 24]


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from excel_amd import ops as _ops
    return _ops


def _class_lists(seed=1, counts=K):
    """Sorted present classes per image; image 0 holds class 0 and class F - 1 (the first and the last column of the one-hot row)."""
    rs = np.random.RandomState(seed)
    lists = [np.sort(rs.choice(F, k, replace=False)) for k in counts]
    lists[0] = np.sort(np.concatenate([[0, F - 1], 1 + rs.choice(F - 2, counts[0] - 2, replace=False)]))
    return lists


def _onehot(lists):
    onehot = np.zeros((len(lists), F), np.float32)
    for b, c in enumerate(lists):
        onehot[b, c] = 1
    return onehot


@pytest.fixture(scope="module")
def classes(ops):
    """(class lists, one-hot [6,F], cls_idx [6,18], ncls, nchan) of the pattern K, compacted once and checked against numpy"""
    lists = _class_lists()
    assert [len(c) for c in lists] == K and lists[0][0] == 0 and lists[0][-1] == F - 1
    onehot = _onehot(lists)
    idx, ncls, nchan = ops.cls_compact(dev(onehot), SMAX, want_nchan=True)
    assert host(ncls).tolist() == K and host(nchan).tolist() == [k + 1 for k in K]
    for b, c in enumerate(lists):
        assert np.array_equal(host(idx)[b, :K[b]], c) and np.all(host(idx)[b, K[b]:] == -1)
    return lists, onehot, idx, ncls, nchan


def _say(what, got, bound):
    print(f"\n[many-classes] {what}: {got:.3e} (bound {bound:g})")


# ------------------------------------------------------------------ 1. random-walk refinement
@pytest.mark.parametrize("g", [6, 9])
def test_refine_18_classes_vs_oracle(ops, classes, g):
    """g = 6: P = 36 < 64, one lane pass; g = 9: P = 81, two lane passes with a ragged tail.  The mat-vec runs its second and third
    chunk of 8 classes (s0 = 8, 16), twice (u = T v, refined = T u)."""
    lists, onehot, idx, ncls, _ = classes
    rs = np.random.RandomState(100 + g)
    B, P = len(K), g * g
    attr = _smooth_maps(rs, B, g, F)
    w_aff = (rs.rand(B, P, P).astype(np.float32) ** 6 + 1e-4)
    out_d = ops.refine_cams_with_aff_batched(dev(attr), dev(w_aff), idx, ncls, g, 0.79)
    out = host(out_d)
    errs = {}
    for b in range(B):
        trans = oracle.aff.compute_trans_mat(w_aff[b])
        for s, cls in enumerate(lists[b]):
            gmap = attr[b, :, cls].reshape(g, g)
            mask = oracle.aff.box_mask(gmap, 0.79).reshape(1, -1)
            ref = ((trans * mask) @ gmap.reshape(-1, 1)).reshape(-1)
            errs[b, s, int(cls)] = relmax(out[b, s], ref)
    _say(f"refine g={g} relmax", max(errs.values()), 2e-5)
    for key, e in errs.items():
        assert e < 2e-5, key
    for b in range(B):
        assert not out[b, K[b]:].any(), b                          # rows >= K[b]: exactly zero
    # batch independence: image b alone with Smax = K[b] has the bits it gets in the batch with Smax = 18
    for b in range(B):
        idx1, n1 = ops.cls_compact(dev(onehot[b:b + 1]), K[b])
        one = ops.refine_cams_with_aff_batched(dev(attr[b:b + 1]), dev(w_aff[b:b + 1]), idx1, n1, g, 0.79)
        assert tuple(one.shape) == (1, K[b], P)
        assert torch.equal(one[0], out_d[b, :K[b]]), b


# ------------------------------------------------------------------ 2. up-sampling and background
def _refined(seed=2, g=6):
    return np.random.RandomState(seed).rand(len(K), SMAX, g * g).astype(np.float32) * 0.3


def test_cam_upsample_bkg_18_classes_vs_oracle(ops, classes):
    _, _, _, ncls, _ = classes
    g, H, W = 6, 40, 56
    r = _refined()
    cams = host(ops.cam_upsample_bkg(dev(r), ncls, g, H, W))
    assert cams.shape == (len(K), CMAX, H, W)
    errs = []
    for b, k in enumerate(K):
        maps = np.stack([oracle.aff.scale_cam_image(r[b, s].reshape(g, g), (W, H)) for s in range(k)])
        errs.append((maxabs(cams[b, 1:1 + k], maps), maxabs(cams[b, 0], 1 - maps.max(0))))     # background = 1 - max over the image's OWN classes
    _say("cam_upsample_bkg max |err|", max(max(e) for e in errs), 2e-6)
    for b, k in enumerate(K):
        assert errs[b][0] < 2e-6 and errs[b][1] < 2e-6, (b, errs[b])
        assert not cams[b, 1 + k:].any(), b


def test_cam_upsample_bkg_ragged_18_classes_equals_uniform(ops, classes):
    _, _, _, ncls, _ = classes
    g = 6
    r = dev(_refined())
    plan = ops.RaggedPlan(SIZES, "cuda")
    n = np.array(K)
    m_all, m_used = dev(pitched_mask(plan, CMAX)), dev(pitched_mask(plan, CMAX, n + 1))
    zeroed = ops.cam_upsample_bkg_ragged(r, ncls, g, plan)
    kept = S.fill_bytes(torch.empty((CMAX * plan.total_pix,), dtype=torch.float32, device="cuda"), 0xFF)
    assert ops.cam_upsample_bkg_ragged(r, ncls, g, plan, out=kept, zero_unused=False) is kept
    for b, (H, W) in enumerate(SIZES):
        k = K[b]
        c1 = ops.cam_upsample_bkg(r[b:b + 1], ncls[b:b + 1], g, H, W)
        assert torch.equal(plan.planes(zeroed, b, CMAX)[:k + 1], c1[0, :k + 1]), (b, H, W)
        assert torch.equal(plan.planes(kept, b, CMAX)[:k + 1], c1[0, :k + 1]), (b, H, W)
        assert not plan.planes(zeroed, b, CMAX)[k + 1:].any(), b   # zero_unused=True: channels above K[b] are exactly zero
    assert (m_all & ~m_used).any() and (~m_all).any()
    S.assert_holds(kept[~m_used], 0xFF)                             # zero_unused=False: they - and the pad columns - keep the fill


# ------------------------------------------------------------------ 3. PAR with 19 channels
def test_par_19_channels_interior_tile_both_kernels_vs_oracle(ops):
    """W = 160: the tile at x0 = 64 has x0 - 24 >= 0 and x0 + 88 <= 160 and takes the 16-byte interior staging, the other two clamp;
    H = 20: a second, partly empty tile row.  3 + 19 planes go through the two-buffer ring of the recomputing kernel; the streamed
    kernel runs its chunks 8 + 8 + 3 / 8 + 8 + 1 / 8 + 8 / 8 + 1."""
    B, C, H, W, it = 4, CMAX, 20, 160, 3
    nch = [19, 17, 16, 9]
    rs = np.random.RandomState(C * H)
    img = rs.standard_normal((B, 3, H, W)).astype(np.float32)
    masks = rs.rand(B, C, H, W).astype(np.float32)
    nchan = dev(np.array(nch, np.int32))
    got = ops.par_forward(dev(img), dev(masks), DIL, it, nchan=nchan)
    streamed = ops.par_forward(dev(img), dev(masks), DIL, it, nchan=nchan, stream_affinities=True)
    par = oracle.par.PAR(DIL, it)
    refs = [par(img[b:b + 1], masks[b:b + 1, :nch[b]])[0] for b in range(B)]
    _say("PAR recompute max |err|", max(maxabs(host(got[b, :nch[b]]), refs[b]) for b in range(B)), 5e-5)
    _say("PAR streamed max |err|", max(maxabs(host(streamed[b, :nch[b]]), refs[b]) for b in range(B)), 5e-5)
    for b in range(B):
        assert torch.equal(got[b, :nch[b]], streamed[b, :nch[b]]), b
        assert maxabs(host(got[b, :nch[b]]), refs[b]) < 5e-5, b
        assert maxabs(host(streamed[b, :nch[b]]), refs[b]) < 5e-5, b


def test_par_19_channels_streamed_kernel_vs_oracle(ops):
    """W % 4 != 0: the default call takes the streamed kernel, chunks 8 + 8 + 3 and an exact 8 + 8."""
    B, C, H, W, it = 2, CMAX, 33, 47, 3
    nch = [19, 16]
    rs = np.random.RandomState(C * H)
    img = rs.standard_normal((B, 3, H, W)).astype(np.float32)
    masks = rs.rand(B, C, H, W).astype(np.float32)
    got = host(ops.par_forward(dev(img), dev(masks), DIL, it, nchan=dev(np.array(nch, np.int32))))
    par = oracle.par.PAR(DIL, it)
    refs = [par(img[b:b + 1], masks[b:b + 1, :nch[b]])[0] for b in range(B)]
    _say("PAR streamed (W=47) max |err|", max(maxabs(got[b, :nch[b]], refs[b]) for b in range(B)), 5e-5)
    for b in range(B):
        assert maxabs(got[b, :nch[b]], refs[b]) < 5e-5, b
        assert not got[b, nch[b]:].any(), b


def test_par_ragged_19_channels_equals_per_image(ops):
    """Cmax = 19 next to images of 2 and 9 channels, narrow and tiny images included; pad columns and planes >= nchan[b] of the input
    hold NaN: none may reach a valid output element."""
    nch = [k + 1 for k in K]
    rs = np.random.RandomState(33)
    plan = ops.RaggedPlan(SIZES, "cuda")
    planes = [rs.rand(c, H, W).astype(np.float32) for (H, W), c in zip(SIZES, nch)]
    imgs = dev(rs.standard_normal((len(K), 3, 32, 32)).astype(np.float32))
    nchan = dev(np.array(nch, np.int32))
    out = ops.par_forward_ragged(imgs, dev(CRF._pitched(plan, planes, CMAX)), plan, CMAX, DIL, 3, nchan=nchan)
    for b, (H, W) in enumerate(SIZES):
        c = nch[b]
        tight = np.full((1, CMAX, H, W), np.nan, np.float32)
        tight[0, :c] = planes[b]
        ref = ops.par_forward(imgs[b:b + 1], dev(tight), DIL, 3, nchan=nchan[b:b + 1])
        mine = plan.planes(out, b, CMAX)[:c]
        assert not torch.isnan(mine).any(), (b, H, W)
        assert torch.equal(mine, ref[0, :c]), (b, H, W)


# ------------------------------------------------------------------ 4. arg-max and key lookup
def _tied_cams(rs, H, W):
    """19 channels in [0, 1) with exact ties at the top: channel 0 against 18 in the first rows / columns, 8 against 9 behind them"""
    c = rs.rand(CMAX, H, W).astype(np.float32)
    a, bnd = max(H // 3, 1), max(W // 3, 1)
    c[0, :a, :bnd] = c[18, :a, :bnd] = 2.0
    c[8, :a, bnd:2 * bnd] = c[9, :a, bnd:2 * bnd] = 3.0
    return c


def test_argmax_19_channels_key_lookup_and_ties(ops, classes):
    lists, _, idx, _, nchan = classes
    rs = np.random.RandomState(44)
    plan = ops.RaggedPlan(SIZES, "cuda")
    cams = [_tied_cams(rs, H, W) for H, W in SIZES]
    lab = ops.argmax_label_ragged(dev(CRF._pitched(plan, cams, CMAX)), plan, CMAX, nchan, idx)
    seen = set()
    for b, (H, W) in enumerate(SIZES):
        key = np.pad(lists[b] + 1, (1, 0))
        am = cams[b][:K[b] + 1].argmax(0)                            # numpy: the first maximum
        ref = key[am]
        seen |= set(np.unique(am).tolist())
        l8, l64 = ops.argmax_label(dev(cams[b][None]), nchan[b:b + 1], idx[b:b + 1], want_i64=True)
        assert np.array_equal(host(l8)[0], ref.astype(np.uint8)), b
        assert np.array_equal(host(l64)[0], ref.astype(np.int64)), b
        assert torch.equal(plan.label(lab, b), l8[0]), b
    a, bnd = SIZES[0][0] // 3, SIZES[0][1] // 3
    am = cams[0].argmax(0)
    assert (am[:a, :bnd] == 0).all() and (am[:a, bnd:2 * bnd] == 8).all()          # the reference itself: the first index wins both ties
    assert len(seen) == CMAX                                        # every channel is the maximum somewhere
    assert int(host(plan.label(lab, 0)).max()) == F                 # class 79 -> key 80
    # one uniform batch of 6: the image stride b * Cmax * HW
    H, W = SIZES[1]
    batch = np.stack([_tied_cams(rs, H, W) for _ in K])
    l8 = host(ops.argmax_label(dev(batch), nchan, idx))
    for b in range(len(K)):
        assert np.array_equal(l8[b], np.pad(lists[b] + 1, (1, 0))[batch[b, :K[b] + 1].argmax(0)].astype(np.uint8)), b


# ------------------------------------------------------------------ 5. more present classes than Smax
SLACK = 4096


@contextlib.contextmanager
def _slack_allocations(record):
    """torch.empty / torch.zeros of a device tensor (what ops allocates its outputs with) hand out the front of a larger allocation
    whose last SLACK bytes hold tests/_scratch.py's sentinel; (buffer, bytes in front) goes to `record`.  torch.empty starts as 0xFF
    bytes.  Restored on exit."""
    real_empty, real_zeros = torch.empty, torch.zeros

    def wrap(real, zero):
        def alloc(*size, **kw):
            device = kw.get("device")
            if device is None or torch.device(device).type != "cuda" or set(kw) - {"dtype", "device"}:
                return real(*size, **kw)
            shape = tuple(size[0]) if len(size) == 1 and isinstance(size[0], (tuple, list, torch.Size)) else tuple(int(s) for s in size)
            dtype = kw.get("dtype") or torch.float32
            nbytes = int(np.prod(shape, dtype=np.int64)) * real_empty(0, dtype=dtype).element_size()
            buf = torch.full((nbytes + SLACK,), S.SENTINEL, dtype=torch.uint8, device=device)
            buf[:nbytes] = 0 if zero else 0xFF
            record.append((buf, nbytes))
            return buf[:nbytes].view(dtype).view(shape)
        return alloc

    torch.empty, torch.zeros = wrap(real_empty, False), wrap(real_zeros, True)
    try:
        yield
    finally:
        torch.empty, torch.zeros = real_empty, real_zeros


OVER_SIZES = [(33, 47), (20, 160)]


def _chain(ops, onehot, attr, w_aff, imgs, plan, tied):
    """items 1 - 4 on one batch, uniform at (40, 56) and ragged at OVER_SIZES, with Smax = 18 -> dict of outputs"""
    g = 6
    idx, ncls, nchan = ops.cls_compact(onehot, SMAX, want_nchan=True)
    refined = ops.refine_cams_with_aff_batched(attr, w_aff, idx, ncls, g, 0.79)
    cams = ops.cam_upsample_bkg(refined, ncls, g, 40, 56)
    par = ops.par_forward(imgs, cams, DIL, 3, nchan=nchan)
    par_s = ops.par_forward(imgs, cams, DIL, 3, nchan=nchan, stream_affinities=True)
    lab = ops.argmax_label(par, nchan, idx)
    lab_t = ops.argmax_label(tied, nchan, idx)
    rcams = ops.cam_upsample_bkg_ragged(refined, ncls, g, plan)
    rpar = ops.par_forward_ragged(imgs, rcams, plan, CMAX, DIL, 3, nchan=nchan)
    rlab = ops.argmax_label_ragged(rpar, plan, CMAX, nchan, idx)
    return dict(idx=idx, ncls=ncls, nchan=nchan, refined=refined, cams=cams, par=par, par_s=par_s, lab=lab, lab_t=lab_t, rcams=rcams,
                rpar=rpar, rlab=rlab)


def test_more_present_classes_than_smax(ops, monkeypatch):
    """The overflow contract of include/excel_hip.h (excel_cls_compact): with 20 (19) present classes and Smax = 18, ncls reports the
    true count, cls_idx keeps the first 18 class indices in ascending order, and every stage gives the bits of the same image with
    only those 18 classes marked present, writing nothing behind its outputs or workspaces."""
    rs = np.random.RandomState(55)
    lists = _class_lists(seed=5, counts=[20, 19])
    full = _onehot(lists)
    cut = _onehot([c[:SMAX] for c in lists])
    g, B = 6, 2
    attr = dev(_smooth_maps(rs, B, g, F))
    w_aff = dev(rs.rand(B, g * g, g * g).astype(np.float32) ** 6 + 1e-4)
    imgs = dev(rs.standard_normal((B, 3, 32, 32)).astype(np.float32))
    tied = dev(np.stack([_tied_cams(rs, 17, 29) for _ in range(B)]))
    plan = ops.RaggedPlan(OVER_SIZES, "cuda")
    ws = S.guarded_ws(ops, monkeypatch)
    record = []
    with _slack_allocations(record):
        over = _chain(ops, dev(full), attr, w_aff, imgs, plan, tied)
        want = _chain(ops, dev(cut), attr, w_aff, imgs, plan, tied)
    torch.cuda.synchronize()
    assert host(over["ncls"]).tolist() == [20, 19] and host(want["ncls"]).tolist() == [SMAX, SMAX]
    assert host(over["nchan"]).tolist() == [CMAX, CMAX]
    for b in range(B):
        assert np.array_equal(host(over["idx"])[b], lists[b][:SMAX]), b
    for name in ("idx", "nchan", "refined", "cams", "par", "par_s", "lab", "lab_t", "rlab"):
        assert torch.equal(over[name], want[name]), name
    assert torch.equal(over["par"], over["par_s"])
    for name in ("rcams", "rpar"):
        for b in range(B):
            assert torch.equal(plan.planes(over[name], b, CMAX), plan.planes(want[name], b, CMAX)), (name, b)
    assert len(record) >= 2 * 11 and ws.bufs
    for buf, n in record:
        assert bool((buf[n:] == S.SENTINEL).all()), f"a kernel wrote behind an output of {n} bytes"
    ws.check_tails()


# ------------------------------------------------------------------ 6. DenseCRF for LAMs
CRF_NCHAN = [19, 2, 9, 17, 1, 8]


@pytest.mark.parametrize("iters", [0, 10])
def test_dcrf_lam_stride_19_next_to_2_channels(ops, iters):
    """One group whose value-row stride is 19 (image 0) holds images of 2, 1 and 8 channels: every image has the bits of
    ops.dcrf_inference alone on its tight planes, labels looked up through cls_idx keys up to 79."""
    gpu = torch.device("cuda")
    sizes = CRF.SIZES
    lists = _class_lists(seed=6, counts=[max(c - 1, 1) for c in CRF_NCHAN])
    cls_idx = np.full((len(sizes), SMAX), -1, np.int32)
    for b, c in enumerate(CRF_NCHAN):
        cls_idx[b, :c - 1] = lists[b][:c - 1]
    assert cls_idx[0, 0] == 0 and cls_idx[0, SMAX - 1] == F - 1
    imgs, probs = CRF._batch(sizes, CRF_NCHAN, seed=61)
    plan = ops.RaggedPlan(sizes, gpu)
    images = torch.from_numpy(np.concatenate([i.reshape(-1) for i in imgs])).to(gpu)
    cams = torch.from_numpy(CRF._pitched(plan, probs, CMAX)).to(gpu)
    nc = torch.tensor(CRF_NCHAN, dtype=torch.int32, device=gpu)
    with S.poisoned_allocations(0xFF):                              # q_out (torch.empty) starts as 0xFF bytes
        labels, q = ops.dcrf_lam_ragged(images, plan, cams, CMAX, nc, CRF_NCHAN, torch.from_numpy(cls_idx).to(gpu), iters, *CRF.LAM_SET,
                                        want_labels=True, want_q=True)
    for b in range(len(sizes)):
        q_ref, l_ref = CRF._alone(gpu, imgs[b], probs[b], iters, keys=cls_idx[b, :CRF_NCHAN[b] - 1])
        assert np.array_equal(plan.planes(q, b, CMAX)[:CRF_NCHAN[b]].cpu().numpy(), q_ref), (b, sizes[b], CRF_NCHAN[b])
        assert np.array_equal(plan.label(labels, b).cpu().numpy(), l_ref), b
    mask = torch.from_numpy(CRF._valid_mask(plan, CRF_NCHAN, CMAX)).to(gpu)
    assert bool(torch.isfinite(q[mask]).all())
    S.assert_holds(q[~mask], 0xFF)                                  # nothing outside the valid region was written


def test_dcrf_19_classes_vs_oracle(ops):
    """test_gpu_ops.py::test_dcrf_vs_oracle at C = 19: the same comparison, the same per-element tolerances."""
    H, W, C, params = 24, 30, CMAX, (10, 3, 1, 4, 67, 3)
    rs = np.random.RandomState(H + C)
    img = (rs.rand(H, W, 3) * 255).astype(np.uint8)
    img[:, : W // 2] = (img[:, : W // 2] * 0.15 + 140).astype(np.uint8)
    p = rs.rand(C, H, W).astype(np.float32) ** 2 + 1e-3
    p /= p.sum(0, keepdims=True)
    ref = oracle.dcrf.dense_crf_2d(img, oracle.dcrf.unary_from_softmax(p), *params)
    got = host(ops.dcrf_inference(dev(img, torch.uint8), dev(p), *params))
    _say("dcrf C=19 max |err|", maxabs(got, ref), 1e-3)
    _say("dcrf C=19 mean |err|", float(np.abs(got - ref).mean()), 2e-5)
    assert maxabs(got, ref) < 1e-3 and float(np.abs(got - ref).mean()) < 2e-5
    np.testing.assert_allclose(got.sum(0), 1.0, atol=1e-5)
    top2 = np.sort(ref, 0)[-2:]
    clear = (top2[1] - top2[0]) > 1e-3
    assert np.array_equal(got.argmax(0)[clear], ref.argmax(0)[clear])
    again = host(ops.dcrf_inference(dev(img, torch.uint8), dev(p), *params))
    assert np.array_equal(got, again)


# ------------------------------------------------------------------ 7. overlays
@pytest.mark.parametrize("mode", ["max", "per_class"])
def test_cam_overlay_18_classes_byte_exact(ops, mode):
    lut, rt = OV._tables()
    rs = np.random.RandomState(7)
    plan, imgs, cams, per_img = OV._case(rs, SIZES, K, CMAX)
    out, off = ops.cam_overlay_ragged(torch.from_numpy(imgs).cuda(), torch.from_numpy(cams).cuda(), plan, CMAX, K, mode)
    got = out.cpu().numpy()
    if mode == "per_class":
        sizes = np.array([3 * k * H * W for k, (H, W) in zip(K, SIZES)], np.int64)
        assert np.array_equal(np.asarray(off, np.int64), np.concatenate([[0], np.cumsum(sizes)])[:len(K)])
        assert out.numel() == int(sizes.sum())
    for b, (H, W) in enumerate(SIZES):
        want = overlays(per_img[b][0], per_img[b][1], mode, lut, rt)
        assert len(want) == (1 if mode == "max" else K[b])
        for c, w in enumerate(want):
            g = got[int(off[b]) + 3 * c * H * W:][:3 * H * W].reshape(H, W, 3)
            assert np.array_equal(g, w), (mode, b, c, int((g != w).sum()))


# ------------------------------------------------------------------ 8. end to end
E2E_SEED = 5
E2E_COUNTS = [18, 1, 9, 17]
E2E_HW = [(96, 96), (40, 56), (20, 160), (33, 47)]


def _e2e_inputs(seed=E2E_SEED, counts=E2E_COUNTS, nfg=20, S=96):
    rs = np.random.RandomState(seed)
    B = len(counts)
    text = rs.standard_normal((nfg + 5, 64)).astype(np.float32)     # 20 foreground rows + the 5 background rows of the tiny test
    text /= np.linalg.norm(text, axis=1, keepdims=True)
    imgs = rs.standard_normal((B, 3, S, S)).astype(np.float32)
    gts = rs.randint(0, nfg + 1, (B, S, S)).astype(np.uint8)
    gts[rs.rand(B, S, S) < 0.02] = 255
    cls = np.zeros((B, nfg), np.float32)
    for b, k in enumerate(counts):
        cls[b, rs.choice(nfg, k, replace=False)] = 1
    return rs, text, imgs, gts, cls


def test_pipeline_tiny_18_classes_vs_oracle(ops):
    """test_gpu_pipeline.py::test_batched_pipeline_tiny_vs_oracle with 20 foreground text rows, smax = 18 and present counts
    [18, 1, 9, 17], with that test's bounds (attr < 2e-4, cams < 1e-3, label agreement >= 0.999 per image, confusion matrix
    integer-exact), then run_batch_ragged against its batch-of-one runs, bit for bit.

    The seed.  The wish was a seed at which the ORACLE's own top-two margin of the PAR output exceeds 1e-2 at all but 0.05 % (4) of
    each image's 9216 pixels.  No such seed exists for these inputs, at any count above 1: 18 competing min-max normalised maps
    up-sampled from a 6 x 6 grid cross each other along long boundaries.  CPU scan of seeds 0..23, pixels per image with margin
    <= 1e-2: 18 classes 528..2305, 17 classes 572..2531, 9 classes 169..1642, 1 class 0..315; and with present counts [1, 2, 3, 1]
    over seeds 0..5: 2 classes 6..513, 3 classes 12..860.  Reducing 18 to "the largest count that does" would mean 1, which is no
    many-class test, so the counts stay and the seed is the one of the scan with the fewest pixels whose margin is <= 1e-4 in its
    worst image (seed 5: 9 / 0 / 6 / 10 pixels <= 1e-4, 0 / 0 / 1 / 1 pixels <= 1e-5, 1217 / 12 / 647 / 1094 pixels <= 1e-2;
    the 0.999 gate allows 9).  The gate itself is untouched."""
    from excel_amd.pipeline import TrainingFreePipeline
    from test_gpu_pipeline import TINY, _oracle_batch, tiny_model
    rs, text, imgs, gts, cls = _e2e_inputs()
    B, S, nfg = len(E2E_COUNTS), 96, 20
    model, w = tiny_model(text.T.copy(), gemm_mode="f32", num_classes=nfg + 1)
    wo = oracle.vit.reload_self_attn(w, TINY, 6, "train")
    pipe = TrainingFreePipeline(model, num_classes=nfg + 1, smax=SMAX)
    labels, inter = pipe.run_batch(dev(imgs), dev(cls), dev(gts), return_intermediates=True)
    ref = _oracle_batch(imgs, gts, cls, wo, TINY, text.T.copy(), nfg, S)
    lab = host(labels)
    ref_hist = np.zeros((nfg + 1, nfg + 1), np.int64)
    figs = []
    for b in range(B):
        k = E2E_COUNTS[b]
        figs.append((maxabs(host(inter["attr"])[b], ref[b]["attr_maps_raw"][0]), maxabs(host(inter["cams"])[b, :k + 1], ref[b]["cams"]),
                     float(np.mean(lab[b] == ref[b]["label"]))))
        ref_hist += oracle.evaluate.fast_hist(gts[b].flatten(), lab[b].flatten(), nfg + 1)
    print("\n[many-classes] end to end (attr err, cams err, label agreement) per image:", [(f"{a:.2e}", f"{c:.2e}", f"{l:.5f}") for a, c, l in figs])
    for b, (a, c, l) in enumerate(figs):
        assert a < 2e-4, b
        assert c < 1e-3, b
        assert l >= 0.999, b
    assert np.array_equal(host(pipe.hist), ref_hist)                # integer-exact on identical labels
    # the ragged form at four label sizes: every image as in its batch-of-one run
    u8 = [rs.randint(0, 256, (h, wd, 3)).astype(np.uint8) for h, wd in E2E_HW]
    plan = ops.RaggedPlan(E2E_HW, "cuda")
    cls_d = dev(cls)
    rlab, rint = pipe.run_batch_ragged(dev(np.concatenate([i.reshape(-1) for i in u8])), plan, cls_d, S=S, return_intermediates=True)
    for b, hw in enumerate(E2E_HW):
        k = E2E_COUNTS[b]
        plan1 = ops.RaggedPlan([hw], "cuda")
        l1, i1 = pipe.run_batch_ragged(dev(u8[b].reshape(-1)), plan1, cls_d[b:b + 1], S=S, return_intermediates=True)
        assert torch.equal(plan.label(rlab, b), plan1.label(l1, 0)), b
        for name in ("cams", "par_out"):
            assert torch.equal(plan.planes(rint[name], b, CMAX)[:k + 1], plan1.planes(i1[name], 0, CMAX)[:k + 1]), (name, b)
        keys = np.concatenate([[0], np.where(cls[b])[0] + 1])
        assert np.isin(host(plan.label(rlab, b)), keys).all(), b
