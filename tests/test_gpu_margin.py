"""Arg-max margin on the GPU: excel_margin_sweep_ragged (margin.hip) against its numpy restatement (utils/margin.margin_reference),
integer for integer and margin for margin bit for bit (where the reference is NaN the device must be NaN) - no tolerance, no excluded
pixel -, at sizes around the kernel's 64 x 16 tile, every class count and number of thresholds its LDS is sized for, margins that sit ON
a threshold, skip flags and accumulation; against the background sweep's kernel at threshold 0; its refusals, its stream, scratch-free
and alignment contracts; then the pipeline's margin_sweep / margin_min and infer_lam's --margin_sweep / --margin_min end to end."""
import ctypes as C
import csv
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
THR16 = tuple(i / 8 for i in range(16))
THR = {0: (), 1: (0.25,), 8: (0.0, 0.125, 0.25, 0.5, 0.75, 1.0, 1.5, 2.0), 16: THR16}
UNWRITTEN = -1e30                     # margin_out's pre-fill: no margin of these planes
_CASES = {}


@pytest.fixture(scope="module")
def gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import excel_amd.ops  # noqa: F401
    return True


def _dev(a):
    return torch.from_numpy(np.array(a)).cuda()


def _case(Cmax, nc, with_cls, seed=0, sizes=SIZES, arbitrary=False, key0=True, full_nchan=False):
    """A ragged batch, built once per key and read-only afterwards.  Plane values are multiples of 1/8 in [0, 2], so that a margin equal
    to a threshold happens often (`arbitrary`: any float32 in [0, 2), plus a few inf and NaN pixels); pad columns hold +inf, the planes
    >= nchan[b] NaN; the ground truth holds 255 and values >= nc; the class lists reach past nc - 1 and, with `key0`, hold the slot
    value -1, which gives key 0."""
    key = (Cmax, nc, with_cls, seed, tuple(sizes), arbitrary, key0, full_nchan)
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
        if arbitrary:
            p[:, :, :w] = (rs.rand(Cmax, h, w) * 2).astype(np.float32)
            for v in (np.inf, -np.inf, np.nan):
                p[rs.randint(0, Cmax, 3), rs.randint(0, h, 3), rs.randint(0, w, 3)] = v
            if h * w > 100:
                p[:, 0, :2] = np.inf                                   # inf - inf
        else:
            p[:, :, :w] = rs.randint(0, 17, (Cmax, h, w)).astype(np.float32) / 8
        p[nchan[b]:] = np.nan
        planes.append(p.reshape(-1))
        g = rs.randint(0, nc, h * w).astype(np.uint8)
        g[rs.rand(h * w) < 0.05] = 255
        if nc < 250:
            g[rs.rand(h * w) < 0.05] = nc + rs.randint(0, 3)
        gts.append(g)
    cls = None
    if with_cls:
        cls = rs.randint(0, min(nc + 8, 254), (B, Cmax - 1)).astype(np.int32)
        if key0:
            cls[:, 0] = np.where(rs.rand(B) < 0.5, -1, cls[:, 0])
            cls[-1, 0] = -1
    case = dict(planes=np.concatenate(planes), gts=np.concatenate(gts), nchan=nchan, cls=cls, sizes=list(sizes), Cmax=Cmax, nc=nc)
    _CASES[key] = case
    return case


def _on_device(case):
    from excel_amd import ops
    plan = ops.RaggedPlan(case["sizes"], "cuda")
    return plan, _dev(case["planes"]), _dev(case["gts"]), _dev(case["nchan"]), (None if case["cls"] is None else _dev(case["cls"]))


def _same_margins(got, want, what="margins"):
    """Bit for bit; where the reference is NaN the device is NaN (sign and payload differ between hosts)."""
    got, want = np.asarray(got, np.float32), np.asarray(want, np.float32)
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan), what + ": NaN where the reference is NaN, and nowhere else"
    assert np.array_equal(got[~nan].view(np.uint32), want[~nan].view(np.uint32)), what


@pytest.mark.parametrize("with_cls", [True, False], ids=["cls_idx", "no_cls_idx"])
@pytest.mark.parametrize("nc, K", [(21, 16), (81, 16), (256, 16), (21, 1), (21, 8), (21, 0)])
@pytest.mark.parametrize("Cmax", [2, 7, 19])
def test_every_output_equals_the_reference(gpu, Cmax, nc, K, with_cls):
    from excel_amd.utils.margin import margin_ragged, margin_reference
    case = _case(Cmax, nc, with_cls)
    thr, cut = THR[K], 0.375
    kw = dict(nchan=case["nchan"], cls_idx=case["cls"], gts=case["gts"], num_classes=nc)
    want_t, want_k, want_l, want_m = margin_reference(case["planes"], case["sizes"], Cmax, thr, label_thre=cut, **kw)
    plan, planes, gts, nchan, cls = _on_device(case)
    dkw = dict(nchan=nchan, cls_idx=cls, gts=gts, num_classes=nc)
    n = plan.total_label_pix
    labels_out = torch.full((n,), 0xFF, dtype=torch.uint8, device="cuda")
    margin_out = torch.full((n,), UNWRITTEN, dtype=torch.float32, device="cuda")
    totals, kept, labels, m = margin_ragged(planes, plan, Cmax, thr, kept=K > 0, label_thre=cut, labels_out=labels_out, margin_out=margin_out, **dkw)
    assert labels.data_ptr() == labels_out.data_ptr() and m.data_ptr() == margin_out.data_ptr()
    got_m = m.cpu().numpy()
    assert not (want_m == np.float32(UNWRITTEN)).any() and not (got_m == np.float32(UNWRITTEN)).any(), "every margin written"
    _same_margins(got_m, want_m)
    assert np.array_equal(labels.cpu().numpy(), want_l)
    assert (want_m == np.float32(cut)).any() and (want_l == 255).any() and (want_l < 255).any()
    if K == 0:
        assert totals is None and kept is None and want_t is None and want_k is None
    else:
        assert totals.dtype == torch.int64 and tuple(totals.shape) == (K, 3, nc) and kept.dtype == torch.int64 and tuple(kept.shape) == (K + 1,)
        print(f"Cmax {Cmax} nc {nc} K {K}: kept {want_k.tolist()} counted {want_t[:, 0].sum(1).tolist()}")
        assert np.array_equal(kept.cpu().numpy(), want_k) and np.array_equal(totals.cpu().numpy(), want_t)
        assert want_k[-1] == n and (np.diff(want_k[:-1]) <= 0).all() and want_t[0].sum() > 0
        for t in thr[:3]:
            assert (want_m == np.float32(t)).any(), f"a margin sits on the threshold {t}"
        if K > 1:
            assert want_k[0] > want_k[K - 1]
        # each output alone: the same values
        only_k = margin_ragged(planes, plan, Cmax, thr, nchan=nchan, cls_idx=cls, kept=True)
        assert only_k[0] is None and only_k[2] is None and only_k[3] is None and np.array_equal(only_k[1].cpu().numpy(), want_k)
        only_t = margin_ragged(planes, plan, Cmax, thr, **dkw)
        assert only_t[1] is None and only_t[2] is None and np.array_equal(only_t[0].cpu().numpy(), want_t)
    # a cut that drops nothing here (no NaN in these planes): every byte of the 0xFF buffer is written, negative margins included
    want_all = margin_reference(case["planes"], case["sizes"], Cmax, (), label_thre=-np.inf, **kw)[2]
    assert want_all.max() < 255
    labels_out.fill_(0xFF)
    got_all = margin_ragged(planes, plan, Cmax, (), label_thre=-np.inf, labels_out=labels_out, **dkw)
    assert got_all[0] is None and got_all[1] is None and got_all[3] is None and np.array_equal(got_all[2].cpu().numpy(), want_all)
    if with_cls and Cmax > 2:
        assert (want_m < 0).any(), "a slot that maps to key 0 loses with a negative margin"


@pytest.mark.parametrize("with_cls", [True, False], ids=["cls_idx", "no_cls_idx"])
def test_arbitrary_planes_scale_and_thresholds(gpu, with_cls):
    """Any float32 plane values, a = 1.2 and thresholds that are no dyadic fractions: the rounded multiply and the rounded subtract (an
    fma in either place would show), inf - inf and NaN planes."""
    from excel_amd.utils.margin import margin_ragged, margin_reference
    case = _case(7, 21, with_cls, seed=9, arbitrary=True)
    thr = (0.0, 0.013, 0.05, 0.1, 0.2, 0.3, 0.7, 1.1)
    kw = dict(nchan=case["nchan"], cls_idx=case["cls"], gts=case["gts"], num_classes=21)
    want_t, want_k, want_l, want_m = margin_reference(case["planes"], case["sizes"], 7, thr, label_thre=0.1, bkg_scale=1.2, **kw)
    plan, planes, gts, nchan, cls = _on_device(case)
    totals, kept, labels, m = margin_ragged(planes, plan, 7, thr, nchan=nchan, cls_idx=cls, gts=gts, num_classes=21, kept=True, label_thre=0.1,
                                            margin_out=True, bkg_scale=1.2)
    assert np.isnan(want_m).sum() >= 3 and np.isinf(want_m).any()
    _same_margins(m.cpu().numpy(), want_m)
    assert np.array_equal(labels.cpu().numpy(), want_l) and np.array_equal(kept.cpu().numpy(), want_k) and np.array_equal(totals.cpu().numpy(), want_t)
    other = margin_reference(case["planes"], case["sizes"], 7, (), bkg_scale=1.0, **kw)[3]
    assert not np.array_equal(other[~np.isnan(other)], want_m[~np.isnan(other)]), "the scale is in the margins"


@pytest.mark.parametrize("a", [1.0, 1.2])
def test_threshold_zero_is_the_background_sweeps_kernel(gpu, a):
    """Planes with b0 >= 0, no NaN and no slot that maps to key 0: the labels and totals at threshold 0 are excel_bkg_sweep_ragged's."""
    from excel_amd.utils.bkg_sweep import sweep_ragged
    from excel_amd.utils.margin import margin_ragged
    for with_cls in (True, False):
        case = _case(7, 21, with_cls, seed=4, key0=False)
        plan, planes, gts, nchan, cls = _on_device(case)
        want_t, want_l = sweep_ragged(planes, plan, 7, (a,), nchan=nchan, cls_idx=cls, gts=gts, num_classes=21, label_sel=0)
        totals, kept, labels, _ = margin_ragged(planes, plan, 7, (0.0,), nchan=nchan, cls_idx=cls, gts=gts, num_classes=21, kept=True, label_thre=0.0,
                                                bkg_scale=a)
        assert torch.equal(labels, want_l) and torch.equal(totals, want_t)
        assert int(kept[0]) == int(kept[1]) == plan.total_label_pix


def test_skip_flags_and_accumulation(gpu):
    from excel_amd.utils.margin import margin_ragged, margin_reference
    case = _case(7, 21, True, seed=1)
    thr = THR[8]
    kw = dict(nchan=case["nchan"], cls_idx=case["cls"], gts=case["gts"], num_classes=21)
    plan, planes, gts, nchan, cls = _on_device(case)
    dkw = dict(nchan=nchan, cls_idx=cls, gts=gts, num_classes=21)
    skip_h = np.int32([0, 3, 0, 0, 1])
    want_ts, want_ks, want_lab, want_m = margin_reference(case["planes"], case["sizes"], 7, thr, skip=skip_h, label_thre=0.25, **kw)
    want_ta, want_ka, _, _ = margin_reference(case["planes"], case["sizes"], 7, thr, **kw)
    assert not np.array_equal(want_ts, want_ta) and want_ks[-1] == want_ka[-1] - 3 * 5 - 40 * 151
    totals, kept, labels, m = margin_ragged(planes, plan, 7, thr, skip=_dev(skip_h), kept=True, label_thre=0.25, margin_out=True, **dkw)
    assert np.array_equal(totals.cpu().numpy(), want_ts) and np.array_equal(kept.cpu().numpy(), want_ks)
    assert np.array_equal(labels.cpu().numpy(), want_lab), "the labels are written whatever skip says"
    _same_margins(m.cpu().numpy(), want_m, "the margins are written whatever skip says")
    zeros = margin_ragged(planes, plan, 7, thr, skip=_dev(np.zeros(5, np.int32)), kept=True, **dkw)
    assert np.array_equal(zeros[0].cpu().numpy(), want_ta) and np.array_equal(zeros[1].cpu().numpy(), want_ka)
    # a second call adds; so does a call on counters that hold something already
    again = margin_ragged(planes, plan, 7, thr, totals=totals, kept=kept, **dkw)
    assert again[0].data_ptr() == totals.data_ptr() and again[1].data_ptr() == kept.data_ptr()
    assert np.array_equal(again[0].cpu().numpy(), want_ts + want_ta) and np.array_equal(again[1].cpu().numpy(), want_ks + want_ka)
    start_t = torch.arange(8 * 3 * 21, dtype=torch.int64, device="cuda").view(8, 3, 21) * (1 << 33)
    start_k = torch.arange(9, dtype=torch.int64, device="cuda") * (1 << 35)
    got = margin_ragged(planes, plan, 7, thr, totals=start_t.clone(), kept=start_k.clone(), **dkw)
    assert np.array_equal(got[0].cpu().numpy(), start_t.cpu().numpy() + want_ta) and np.array_equal(got[1].cpu().numpy(), start_k.cpu().numpy() + want_ka)


def test_many_tiles_per_workgroup(gpu):
    """More tiles (2280) than a counting launch takes at a time (256 workgroups x 4 tiles): every workgroup strides and flushes once."""
    from excel_amd.utils.margin import margin_ragged, margin_reference
    sizes = [(33, 130)] * 240 + [(17, 65)] * 30                      # 240 * 9 + 30 * 4 = 2280 tiles
    case = _case(4, 21, False, seed=7, sizes=sizes)
    plan, planes, gts, nchan, _ = _on_device(case)
    assert plan.total_tiles == 2280
    want_t, want_k, want_l, _ = margin_reference(case["planes"], sizes, 4, THR[8], nchan=case["nchan"], gts=case["gts"], num_classes=21, label_thre=0.5)
    totals, kept, labels, _ = margin_ragged(planes, plan, 4, THR[8], nchan=nchan, gts=gts, num_classes=21, kept=True, label_thre=0.5)
    assert np.array_equal(totals.cpu().numpy(), want_t) and np.array_equal(kept.cpu().numpy(), want_k) and np.array_equal(labels.cpu().numpy(), want_l)


def test_bad_arguments_are_refused_before_any_launch(gpu):
    from excel_amd import ops
    from excel_amd.utils.margin import margin_ragged
    plan = ops.RaggedPlan([(2, 4), (3, 5)], "cuda")
    empty = ops.RaggedPlan([(2, 4)], "cuda")
    planes = torch.zeros(3 * plan.total_pix + 8, dtype=torch.float32, device="cuda")
    gt = torch.zeros(plan.total_label_pix, dtype=torch.uint8, device="cuda")
    totals = torch.full((16 * 3 * 256 + 1,), 77, dtype=torch.int64, device="cuda")
    kept = torch.full((18,), 55, dtype=torch.int64, device="cuda")
    labels = torch.full((plan.total_label_pix,), 0x5A, dtype=torch.uint8, device="cuda")
    margins = torch.full((plan.total_label_pix + 1,), 9.0, dtype=torch.float32, device="cuda")
    ints = torch.zeros(8, dtype=torch.int32, device="cuda")
    lib = ops.lib()
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    pp, gp, tp, kp, lp, mp, ip = (C.c_void_p(t.data_ptr()) for t in (planes, gt, totals, kept, labels, margins, ints))
    info, tab = C.byref(plan.info), C.c_void_p(plan.table.data_ptr())
    no_tiles = type(plan.info)()
    C.memmove(C.byref(no_tiles), C.byref(empty.info), C.sizeof(no_tiles))
    no_tiles.total_tiles = 0

    def th(*v):
        return (C.c_float * max(len(v), 1))(*v)
    two = th(0.5, 1.0)
    seventeen = th(*[0.1 * i for i in range(17)])
    off = lambda t, n: C.c_void_p(t.data_ptr() + n)
    nan, inf = float("nan"), float("inf")
    # (planes, nchan, cls_idx, gt, table, info, Smax, Cmax, bkg_scale, thresholds, K, skip, nc, totals, kept, label_thre, labels, margin_out, stream)
    for args, word in (((None, None, None, gp, tab, info, 2, 3, 1.0, two, 2, None, 21, tp, kp, 0.0, lp, mp, st), "null argument"),
                       ((pp, None, None, gp, None, info, 2, 3, 1.0, two, 2, None, 21, tp, kp, 0.0, lp, mp, st), "null argument"),
                       ((pp, None, None, gp, tab, None, 2, 3, 1.0, two, 2, None, 21, tp, kp, 0.0, lp, mp, st), "null argument"),
                       ((pp, None, None, gp, tab, info, 2, 3, 1.0, two, 2, None, 21, None, None, 0.0, None, None, st), "nothing to do"),
                       ((pp, None, None, None, tab, info, 2, 3, 1.0, two, 2, None, 21, tp, kp, 0.0, lp, mp, st), "totals needs the ground truth"),
                       ((pp, None, None, gp, tab, info, 2, 3, 1.0, two, -1, None, 21, tp, kp, 0.0, lp, mp, st), "0 <= K <= 16 (K = -1)"),
                       ((pp, None, None, gp, tab, info, 2, 3, 1.0, seventeen, 17, None, 21, tp, kp, 0.0, lp, mp, st), "0 <= K <= 16 (K = 17)"),
                       ((pp, None, None, gp, tab, info, 2, 3, 1.0, two, 0, None, 21, tp, None, 0.0, lp, mp, st), "at least one threshold"),
                       ((pp, None, None, gp, tab, info, 2, 3, 1.0, two, 0, None, 21, None, kp, 0.0, lp, mp, st), "at least one threshold"),
                       ((pp, None, None, gp, tab, info, 2, 3, 1.0, None, 2, None, 21, tp, kp, 0.0, lp, mp, st), "null thresholds"),
                       ((pp, None, None, gp, tab, info, 2, 3, 1.0, th(0.5, nan), 2, None, 21, tp, kp, 0.0, lp, mp, st), "threshold 1 is"),
                       ((pp, None, None, gp, tab, info, 2, 3, 1.0, th(inf), 1, None, 21, tp, kp, 0.0, lp, mp, st), "threshold 0 is inf"),
                       ((pp, None, None, gp, tab, info, 2, 3, 1.0, th(-0.25, 0.5), 2, None, 21, tp, kp, 0.0, lp, mp, st), "threshold 0 is -0.25"),
                       ((pp, None, None, gp, tab, info, 2, 3, 1.0, th(0.5, 0.25), 2, None, 21, tp, kp, 0.0, lp, mp, st), "strictly increasing"),
                       ((pp, None, None, gp, tab, info, 2, 3, 1.0, th(0.5, 0.5), 2, None, 21, tp, kp, 0.0, lp, mp, st), "strictly increasing"),
                       ((pp, None, None, gp, tab, info, 2, 3, 1.0, two, 2, None, 21, tp, kp, nan, lp, mp, st), "label_thre is NaN"),
                       ((pp, None, None, gp, tab, info, 2, 3, nan, two, 2, None, 21, tp, kp, 0.0, lp, mp, st), "bkg_scale is"),
                       ((pp, None, None, gp, tab, info, 2, 3, inf, two, 2, None, 21, tp, kp, 0.0, lp, mp, st), "bkg_scale is inf"),
                       ((pp, None, None, gp, tab, info, 2, 3, -1.0, two, 2, None, 21, tp, kp, 0.0, lp, mp, st), "bkg_scale is -1"),
                       ((pp, None, None, gp, tab, info, 2, 3, 1.0, two, 2, None, 0, tp, kp, 0.0, lp, mp, st), "num_classes"),
                       ((pp, None, None, gp, tab, info, 2, 3, 1.0, two, 2, None, 257, tp, kp, 0.0, lp, mp, st), "num_classes"),
                       ((off(planes, 4), None, None, gp, tab, info, 2, 3, 1.0, two, 2, None, 21, tp, kp, 0.0, lp, mp, st), "planes must be 16-byte aligned"),
                       ((pp, None, None, gp, tab, info, 2, 3, 1.0, two, 2, None, 21, off(totals, 4), kp, 0.0, lp, mp, st), "8-byte aligned"),
                       ((pp, None, None, gp, tab, info, 2, 3, 1.0, two, 2, None, 21, tp, off(kept, 4), 0.0, lp, mp, st), "8-byte aligned"),
                       ((pp, None, None, gp, tab, info, 2, 3, 1.0, two, 2, None, 21, tp, kp, 0.0, lp, off(margins, 2), st), "4-byte aligned"),
                       ((pp, off(ints, 2), None, gp, tab, info, 2, 3, 1.0, two, 2, None, 21, tp, kp, 0.0, lp, mp, st), "4-byte aligned"),
                       ((pp, None, off(ints, 1), gp, tab, info, 2, 3, 1.0, two, 2, None, 21, tp, kp, 0.0, lp, mp, st), "4-byte aligned"),
                       ((pp, None, None, gp, tab, info, 2, 3, 1.0, two, 2, off(ints, 2), 21, tp, kp, 0.0, lp, mp, st), "4-byte aligned"),
                       ((pp, None, None, gp, off(plan.table, 2), info, 2, 3, 1.0, two, 2, None, 21, tp, kp, 0.0, lp, mp, st), "4-byte aligned"),
                       ((pp, None, ip, gp, tab, info, 1, 3, 1.0, two, 2, None, 21, tp, kp, 0.0, lp, mp, st), "Smax >= Cmax - 1"),
                       ((pp, None, None, gp, tab, C.byref(no_tiles), 2, 3, 1.0, two, 2, None, 21, tp, kp, 0.0, lp, mp, st), "holds no tile")):
        assert lib.excel_margin_sweep_ragged(*args) == -1, word
        assert word in lib.excel_last_error().decode(), (word, lib.excel_last_error())
    torch.cuda.synchronize()
    assert bool((totals == 77).all()) and bool((kept == 55).all()) and bool((labels == 0x5A).all()) and bool((margins == 9.0).all()), \
        "a refused call wrote to its outputs"
    # label_thre is not looked at without a label map; a threshold of zero is a threshold; K = 0 writes labels and margins
    assert lib.excel_margin_sweep_ragged(pp, None, None, gp, tab, info, 2, 3, 1.0, th(0.0, 1.0), 2, None, 21, off(totals, 8), off(kept, 8), nan, None, None, st) == 0
    assert lib.excel_margin_sweep_ragged(pp, None, None, None, tab, info, 2, 3, 0.0, None, 0, None, 21, None, None, -inf, lp, off(margins, 4), st) == 0
    torch.cuda.synchronize()
    n = plan.total_label_pix
    # (all planes are zero: every pixel is background with margin 0 - kept at threshold 0 only, counted in all three rows there)
    assert int(totals[0]) == 77 and int((totals[1:1 + 3 * 21] - 77).sum()) == 3 * n and int((totals[1 + 3 * 21:] - 77).sum()) == 0
    assert (kept.cpu() - 55).tolist() == [0, n, 0, n] + [0] * 14
    assert bool((labels == 0).all()) and float(margins[0]) == 9.0 and bool((margins[1:] == 0).all())
    # the wrapper's own checks
    with pytest.raises(ValueError, match="gts needs num_classes"):
        margin_ragged(planes, plan, 3, (0.5,), gts=gt)
    with pytest.raises(ValueError, match="totals needs gts"):
        margin_ragged(planes, plan, 3, (0.5,), totals=totals[:63].view(1, 3, 21))
    with pytest.raises(ValueError, match=r"totals must be int64 \[2,3,21\]"):
        margin_ragged(planes, plan, 3, (0.5, 1.0), gts=gt, num_classes=21, totals=totals[:63].view(1, 3, 21))
    with pytest.raises(ValueError, match=r"kept must be int64 \[3\]"):
        margin_ragged(planes, plan, 3, (0.5, 1.0), kept=kept[:2])
    with pytest.raises(ValueError, match="kept needs at least one threshold"):
        margin_ragged(planes, plan, 3, (), kept=True)
    with pytest.raises(ValueError, match="labels_out needs label_thre"):
        margin_ragged(planes, plan, 3, (0.5,), labels_out=labels)
    with pytest.raises(ValueError, match="skip holds 3 values for 2 images"):
        margin_ragged(planes, plan, 3, (0.5,), kept=True, skip=torch.zeros(3, dtype=torch.int32, device="cuda"))
    with pytest.raises(RuntimeError, match="nothing to do"):
        margin_ragged(planes, plan, 3, (0.5,))


# ------------------------------------------------------------------ alignment, scratch
def test_outputs_and_ground_truth_at_odd_addresses(gpu):
    """labels_out and gt one byte into their storage, margin_out four bytes into its: the same bits.  Planes four bytes off: refused."""
    from excel_amd.utils.margin import margin_ragged
    case = _case(7, 21, True, seed=6)
    plan, planes, gts, nchan, cls = _on_device(case)
    n = plan.total_label_pix
    kw = dict(nchan=nchan, cls_idx=cls, num_classes=21, kept=True, label_thre=0.25)
    want = margin_ragged(planes, plan, 7, THR[8], gts=gts, margin_out=True, **kw)
    gt_store = torch.zeros(n + 1, dtype=torch.uint8, device="cuda")
    gt_store[1:].copy_(gts)
    lab_store = torch.full((n + 1,), 0xFF, dtype=torch.uint8, device="cuda")
    m_store = torch.full((n + 1,), UNWRITTEN, dtype=torch.float32, device="cuda")
    assert gt_store[1:].data_ptr() % 2 == 1 and lab_store[1:].data_ptr() % 2 == 1 and m_store[1:].data_ptr() % 16 == 4
    got = margin_ragged(planes, plan, 7, THR[8], gts=gt_store[1:], labels_out=lab_store[1:], margin_out=m_store[1:], **kw)
    for g, w in zip(got, want):
        assert torch.equal(g.view(torch.int32) if g.dtype == torch.float32 else g, w.view(torch.int32) if w.dtype == torch.float32 else w)
    assert int(lab_store[0]) == 0xFF and float(m_store[0]) == np.float32(UNWRITTEN)
    shifted = torch.zeros(planes.numel() + 1, dtype=torch.float32, device="cuda")
    shifted[1:].copy_(planes)
    with pytest.raises(RuntimeError, match="planes must be 16-byte aligned"):
        margin_ragged(shifted[1:], plan, 7, THR[8], gts=gts, **kw)


def test_the_kernel_is_built_without_scratch(gpu):
    """The build's guard covers the kernel: both lists name it, and hipcc's figures of the object in use report no scratch and no spilled
    vector register."""
    from excel_amd import build
    assert "margin_kernel" in build.NO_SCRATCH and build.NO_SCRATCH_EXPECTED["margin"] == "margin_kernel" and "margin.hip" in build.SOURCES
    with open(os.path.join(build.CSRC, ".build_resources.json")) as f:        # written by the build that made the library in use
        res = json.load(f)["margin.o"]
    mine = [v for k, v in res.items() if "margin_kernel" in k]
    assert mine and all(v["scratch"] == 0 and v.get("vgpr_spill", 0) == 0 for v in mine), res


# ------------------------------------------------------------------ the stream contract (tests/_streams.py, by import)
@pytest.fixture(scope="module")
def t_link(gpu):
    t = St.time_link()
    print(f"\n[margin streams] one chain link: {t * 1e6:.0f} us")
    assert t > 0
    return t


@pytest.fixture(scope="module")
def stream_case(gpu):
    """fn() -> the op's four outputs, from fresh zeroed counters and uninitialised maps (the runs give them memory of 0xFF bytes: an
    output that is not fully written, or read before it is written, shows), on the current stream; and its reference on the idle default
    stream.  Every image has all its planes: a one-plane image has margin +inf, and the comparison wants finite floats."""
    from excel_amd.utils.margin import margin_ragged
    case = _case(7, 21, True, seed=3, sizes=[(120, 200), (75, 333), (17, 65), (200, 120)] * 4, full_nchan=True)
    plan, planes, gts, nchan, cls = _on_device(case)
    torch.cuda.synchronize()

    def fn():
        totals = torch.zeros((8, 3, 21), dtype=torch.int64, device="cuda")
        kept = torch.zeros((9,), dtype=torch.int64, device="cuda")
        totals, kept, labels, m = margin_ragged(planes, plan, 7, THR[8], nchan=nchan, cls_idx=cls, gts=gts, num_classes=21, totals=totals, kept=kept,
                                                label_thre=0.25, margin_out=True)
        return dict(totals=totals, kept=kept, labels=labels, margins=m)
    return fn, St.reference(fn)


@pytest.mark.parametrize("arrangement", ["behind", "beside"])
def test_the_op_stays_on_its_callers_stream(gpu, stream_case, t_link, arrangement):
    fn, ref = stream_case
    links = St.links_for(ref.t_case, t_link)
    run = (St.run_behind if arrangement == "behind" else St.run_beside)(fn, links)
    print(f"\n[margin streams] {arrangement}: t_case {ref.t_case * 1e3:.2f} ms, {run.links} links, side-stream run {run.host_s * 1e3:.2f} ms, "
          f"default stream busy afterwards: {run.busy}")
    assert int(ref.tree["totals"][:, 0].sum()) > 0 and int(ref.tree["kept"][-1]) > 0
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


SWEEP = "0,0.02,0.05,0.1,0.3"
SWEEP_T = (0.0, 0.02, 0.05, 0.1, 0.3)
CUT = 0.05


@pytest.fixture(scope="module")
def program(gpu, tmp_path_factory):
    """infer_lam.validate on a synthetic VOC tree (6 ragged images at batch 4: two steps) with the tiny checkpoint: plain; with
    --margin_sweep, --margin_min and every output they have; and without ground truth.  The model of the last run serves the pipeline
    tests."""
    from _clip_files import write_tiny_clip
    from excel_amd.tools import infer_lam, synthetic
    tmp = tmp_path_factory.mktemp("mrg")                          # (no "margin" in any path: the plain log must not say the word)
    root, lists = tmp / "VOC2012", tmp / "lists"
    synthetic.write_voc_tree(str(root), str(lists), 6, seed=4, split="val")
    ckpt, bpe_path, _ = write_tiny_clip(tmp)
    common = ["--data_folder", str(root), "--list_folder", str(lists), "--infer_set", "val", "--resize_size", "128", "--model", ckpt,
              "--bpe_path", bpe_path, "--batch_size", "4", "--num_workers", "2", "--save_label", "true"]
    parse = infer_lam.get_parser().parse_args
    cwd = os.getcwd()
    os.chdir(tmp)
    cap = _Capture()
    logging.getLogger().addHandler(cap)
    level = logging.getLogger().level
    logging.getLogger().setLevel(logging.INFO)
    try:
        _, plain = infer_lam.validate(parse(common + ["--label_dir", str(tmp / "plain"), "--json_out", str(tmp / "plain.json")]))
        assert infer_lam.validate.last_margin is None and not any("margin" in x for x in cap.lines)
        js, table = str(tmp / "run.json"), str(tmp / "rows.csv")
        _, flagged = infer_lam.validate(parse(common + ["--label_dir", str(tmp / "labels"), "--margin_sweep", SWEEP, "--margin_min", str(CUT),
                                                        "--margin_label_dir", str(tmp / "margin"), "--json_out", js, "--per_image_scores", table,
                                                        "--boundary_scores", "true"]))
        last = infer_lam.validate.last_margin
        with open(js) as f:
            record = json.load(f)
        with open(tmp / "plain.json") as f:
            plain_record = json.load(f)
        mark = len(cap.lines)
        score_u, total_u = infer_lam.validate(parse(common + ["--label_dir", str(tmp / "u_labels"), "--unlabeled", "true", "--margin_sweep", SWEEP,
                                                              "--margin_min", str(CUT), "--margin_label_dir", str(tmp / "u_margin"),
                                                              "--json_out", str(tmp / "u.json")]))
        assert score_u is None and int(total_u.sum()) == 0
        with open(tmp / "u.json") as f:
            record_u = json.load(f)
    finally:
        logging.getLogger().removeHandler(cap)
        logging.getLogger().setLevel(level)
        os.chdir(cwd)
    with open(lists / "val.txt") as f:
        names = [x.split()[0] for x in f.read().split("\n") if x.strip()]
    return dict(common=common, tmp=tmp, root=root, names=names, plain=plain.cpu().numpy(), flagged=flagged.cpu().numpy(), record=record,
                plain_record=plain_record, record_u=record_u, table=table, log="\n".join(cap.lines[:mark]), log_u="\n".join(cap.lines[mark:]),
                last=last, last_u=infer_lam.validate.last_margin, model=infer_lam.validate.last_model)


def _png(path):
    from PIL import Image
    return np.asarray(Image.open(path))


def _hist(g, p, nc=21):
    g, p = g.reshape(-1).astype(np.int64), p.reshape(-1).astype(np.int64)
    m = (g < nc) & (p < nc)
    return np.bincount(nc * g[m] + p[m], minlength=nc * nc).reshape(nc, nc)


def _margins_of(h):
    return np.stack([h.sum(1), h.sum(0), np.diag(h)])


def test_infer_lam_margin_flags(gpu, program):
    from excel_amd.tools import infer_lam
    from excel_amd.utils import bkg_sweep, margin
    from excel_amd.utils.evaluate import scores_from_hist
    p = program
    assert np.array_equal(p["plain"], p["flagged"]), "the flags change no score of the main labels"
    same = {k: v for k, v in p["record"].items() if k in p["plain_record"] and "second" not in k and "per_s" not in k}
    assert same == {k: p["plain_record"][k] for k in same} and set(p["record"]) - set(p["plain_record"]) == {"margin_sweep", "margin", "boundary"}
    hist, pixels, kept_pix = np.zeros((21, 21), np.int64), 0, 0
    for n in p["names"]:
        assert open(p["tmp"] / "labels" / f"{n}.png", "rb").read() == open(p["tmp"] / "plain" / f"{n}.png", "rb").read(), "same bytes without the flags"
        main, cut = _png(p["tmp"] / "labels" / f"{n}.png"), _png(p["tmp"] / "margin" / f"{n}.png")
        assert cut.shape == main.shape and np.array_equal(cut[cut != 255], main[cut != 255]) and main.max() < 255, "the main labels, or 255"
        hist += _hist(_png(p["root"] / "SegmentationClassAug" / f"{n}.png"), cut)
        pixels += cut.size
        kept_pix += int((cut != 255).sum())
        assert np.array_equal(_png(p["tmp"] / "u_margin" / f"{n}.png"), cut), "the same maps without ground truth"
    last = p["last"]
    j = SWEEP_T.index(CUT)
    kept, totals = last["kept"].cpu().numpy(), last["totals"].cpu().numpy()
    print("kept", kept.tolist(), "coverage", last["coverage"], "mIoU", [s["miou"] for s in last["scores"]])
    assert last["thresholds"] == SWEEP_T and kept.shape == (6,) and totals.shape == (5, 3, 21)
    assert kept[-1] == pixels == kept[0] and kept[j] == kept_pix and (np.diff(kept[:-1]) <= 0).all() and 0 < kept[-2] < kept[0]
    assert np.array_equal(totals[0], _margins_of(p["plain"])), "threshold 0 keeps everything: the run's own matrix"
    assert np.array_equal(totals[j], _margins_of(hist)), "the sweep's row at --margin_min is the matrix of the files"
    assert np.array_equal(last["hist"].cpu().numpy(), hist), "margin_label_score is `evaluate` on the margin files"
    want_score = scores_from_hist(torch.from_numpy(hist))
    assert last["score"]["miou"] == want_score["miou"] and last["label_coverage"] == hist.sum() / p["plain"].sum()
    assert "margin_sweep_score" in p["log"] and margin.format_margin_table(SWEEP_T, kept, last["scores"], infer_lam.VOC_CLASSES) in p["log"]
    assert f"margin_label_score (--margin_min {CUT:g}):" in p["log"] and infer_lam.format_scores_table(want_score, infer_lam.VOC_CLASSES) in p["log"]
    assert f"margin coverage (kept pixels over labelled pixels): {last['label_coverage'] * 100:.3f} %" in p["log"]
    assert p["record"]["margin_sweep"] == margin.margin_json(SWEEP_T, kept, bkg_sweep.scores_from_totals(totals))
    assert list(p["record"]["margin_sweep"]) == ["thresholds", "coverage", "miou", "pacc"] and p["record"]["margin_sweep"]["miou"][0] == p["record"]["miou"]
    assert p["record"]["margin"] == margin.margin_min_json(CUT, want_score, last["label_coverage"])
    with open(p["table"]) as f:
        table = list(csv.reader(f))
    for col in ("margin_pacc", "margin_miou", "margin_scored", "margin_biou"):
        assert col in table[0], (col, table[0])
    assert "boundary_score of the margin labels" in p["log"]
    npz = np.load(p["table"] + ".npz")
    assert np.array_equal(npz["counts_margin"].sum(0), _margins_of(hist)) and "bcounts_margin" in npz
    # without ground truth: the coverage alone, the same counts
    u = p["last_u"]
    assert np.array_equal(u["kept"].cpu().numpy(), kept) and u["totals"] is None and u["scores"] is None and u["score"] is None
    assert margin.format_margin_table(SWEEP_T, kept) in p["log_u"] and "margin_label_score" not in p["log_u"]
    assert p["record_u"]["margin_sweep"] == margin.margin_json(SWEEP_T, kept) and p["record_u"]["margin"] == {"margin_min": CUT}


def test_infer_lam_refuses_before_anything_is_built(gpu, program, monkeypatch):
    from excel_amd.tools import infer_lam
    p = program
    monkeypatch.chdir(p["tmp"])
    parse = infer_lam.get_parser().parse_args
    for extra, word in ((["--margin_sweep", "0,0.1", "--api_path", "true"], "--margin_sweep runs on the batched loop"),
                        (["--margin_label_dir", "d"], "--margin_label_dir needs --margin_min"),
                        (["--margin_sweep", "0.2,0.1"], "strictly increasing"),
                        (["--margin_min", "-1"], "--margin_min"),
                        (["--margin_min", "0.1", "--unlabeled", "true"], "give --margin_label_dir")):
        with pytest.raises(ValueError, match=word):
            infer_lam.validate(parse(p["common"] + extra))
    with pytest.raises(ValueError, match="--margin_min runs behind the ragged step"):
        infer_lam.validate(parse(["--synthetic", "4", "--resize_size", "128", "--margin_min", "0.1"]))


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


@pytest.mark.parametrize("bkg_scale", [1.0, 1.2])
def test_pipeline_margin_outputs_equal_the_reference(gpu, program, bkg_scale):
    from excel_amd import ops
    from excel_amd.pipeline import TrainingFreePipeline
    from excel_amd.utils.margin import margin_reference
    model = program["model"]
    sizes, images, gts, cls = _batch()
    plan = ops.RaggedPlan(sizes, "cuda")
    kw = dict(num_classes=21, smax=3, image_scores=True, **({"bkg_scale": bkg_scale} if bkg_scale != 1.0 else {}))
    plain = TrainingFreePipeline(model, **kw)
    want_labels = plain.run_batch_ragged(images, plan, cls, gts, S=128).clone()
    assert plain.margin_totals is None and plain.margin_kept is None and plain.last_margin_labels is None and plain.hist_margin is None
    assert "margin" not in plain.last_score_ticket.counts()
    pipe = TrainingFreePipeline(model, margin_sweep=SWEEP_T, margin_min=CUT, **kw)
    labels, inter = pipe.run_batch_ragged(images, plan, cls, gts, S=128, return_intermediates=True)
    assert torch.equal(labels, want_labels) and torch.equal(pipe.hist, plain.hist), "the main labels and hist: bit-identical without the arguments"
    assert np.array_equal(pipe.last_score_ticket.counts()["main"], plain.last_score_ticket.counts()["main"])
    ref = margin_reference(inter["par_out"].cpu().numpy(), sizes, 4, SWEEP_T, nchan=pipe.last_nchan.cpu().numpy(), cls_idx=inter["cls_idx"].cpu().numpy(),
                           gts=gts.cpu().numpy(), num_classes=21, label_thre=CUT, bkg_scale=bkg_scale)
    got_l = pipe.last_margin_labels.cpu().numpy()
    print(f"bkg_scale {bkg_scale}: kept {ref[1].tolist()}")
    assert np.array_equal(got_l, ref[2]) and np.array_equal(pipe.margin_totals.cpu().numpy(), ref[0]) and np.array_equal(pipe.margin_kept.cpu().numpy(), ref[1])
    lab = labels.cpu().numpy()
    assert np.array_equal(got_l[got_l != 255], lab[got_l != 255]) and 0 < (got_l == 255).sum() < got_l.size
    if bkg_scale != 1.0:
        other = margin_reference(inter["par_out"].cpu().numpy(), sizes, 4, SWEEP_T, nchan=pipe.last_nchan.cpu().numpy(), cls_idx=inter["cls_idx"].cpu().numpy())[1]
        assert not np.array_equal(other, ref[1]), "bkg_scale is honoured"
    hist = _hist(gts.cpu().numpy(), got_l)
    assert np.array_equal(pipe.hist_margin.cpu().numpy(), hist)
    assert np.array_equal(pipe.last_score_ticket.counts()["margin"].sum(0), _margins_of(hist))
    # a second step adds; a step without ground truth adds to the coverage only; reset() clears
    pipe.run_batch_ragged(images, plan, cls, gts, S=128)
    assert np.array_equal(pipe.margin_totals.cpu().numpy(), 2 * ref[0]) and np.array_equal(pipe.margin_kept.cpu().numpy(), 2 * ref[1])
    pipe.run_batch_ragged(images, plan, cls, None, S=128)
    assert np.array_equal(pipe.margin_totals.cpu().numpy(), 2 * ref[0]) and np.array_equal(pipe.margin_kept.cpu().numpy(), 3 * ref[1])
    assert np.array_equal(pipe.last_margin_labels.cpu().numpy(), ref[2])
    pipe.reset()
    assert pipe.margin_totals is None and pipe.margin_kept is None and pipe.hist_margin is None


def test_pipeline_one_argument_alone_and_the_refusals(gpu, program):
    from excel_amd import ops
    from excel_amd.pipeline import OptimisedLamPipeline, TrainingFreePipeline, ValidationPipeline
    import inspect
    model = program["model"]
    sizes, images, gts, cls = _batch(1)
    plan = ops.RaggedPlan(sizes, "cuda")
    both = TrainingFreePipeline(model, num_classes=21, smax=3, margin_sweep=SWEEP_T, margin_min=CUT, guard="skip")
    both.run_batch_ragged(images, plan, cls, gts, S=128)
    sweep = TrainingFreePipeline(model, num_classes=21, smax=3, margin_sweep=SWEEP_T)
    sweep.run_batch_ragged(images, plan, cls, gts, S=128)
    assert sweep.last_margin_labels is None and sweep.hist_margin is None
    assert torch.equal(sweep.margin_totals, both.margin_totals) and torch.equal(sweep.margin_kept, both.margin_kept), "the guard's flags are zero here"
    cut = TrainingFreePipeline(model, num_classes=21, smax=3, margin_min=CUT)
    cut.run_batch_ragged(images, plan, cls, gts, S=128)
    assert cut.margin_totals is None and cut.margin_kept is None
    assert torch.equal(cut.last_margin_labels, both.last_margin_labels) and torch.equal(cut.hist_margin, both.hist_margin)
    for name in ("run_batch", "run_batch_split", "run_batch_overlapped"):
        with pytest.raises(ValueError, match=f"{name} has no margin sweep"):
            getattr(sweep, name)(None, None)
        with pytest.raises(ValueError, match=f"{name} has no margin labels"):
            getattr(cut, name)(None, None)
    with pytest.raises(ValueError, match="strictly increasing"):
        TrainingFreePipeline(model, num_classes=21, smax=3, margin_sweep=(0.1, 0.1))
    with pytest.raises(ValueError, match="margin_min"):
        TrainingFreePipeline(model, num_classes=21, smax=3, margin_min=-1.0)
    for klass in (OptimisedLamPipeline, ValidationPipeline):
        assert {"margin_sweep", "margin_min"} <= set(inspect.signature(klass.__init__).parameters)
