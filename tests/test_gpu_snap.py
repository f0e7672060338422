"""The superpixel snap on the GPU: excel_slic_superpixels and excel_snap_labels_to_superpixels (superpixels.hip) against the loop judge
of tests/_snap_ref.py and the numpy restatement, integer for integer - everything is integer arithmetic with fixed tie rules, so there
is no tolerance and no pixel is left out -, at the smallest shapes at which a kernel can go wrong, in ragged and uniform batches, at odd
byte addresses, into poisoned outputs; a wrong cent_off row; the refusals; the stream contract; the pipeline step, infer_lam and
eval_labels end to end."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _snap_ref as R  # noqa: E402
import _streams as St  # noqa: E402

VOTES = ((R.NC, 0), (R.NC, 500), (R.NC, 1000), (1, 0), (255, 0))      # (num_classes, min_share_pm)


@pytest.fixture(scope="module")
def gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import excel_amd.ops  # noqa: F401
    return True


def _dev(a):
    return torch.from_numpy(np.array(a)).cuda()


def _poisoned(n, dtype):
    """n elements whose every byte is 0xFF"""
    return torch.full((n * torch.empty((), dtype=dtype).element_size(),), 0xFF, dtype=torch.uint8, device="cuda").view(dtype)


def _ragged(arrays):
    """[H,W] maps or [H,W,3] images -> (plan, the flat device tensor)"""
    from excel_amd import ops
    plan = ops.RaggedPlan([a.shape[:2] for a in arrays], "cuda")
    return plan, _dev(np.concatenate([a.reshape(-1) for a in arrays]))


def _split(flat, maps):
    out, o = [], 0
    flat = flat.cpu().numpy()
    for m in maps:
        n = m.shape[0] * m.shape[1]
        out.append(flat[o:o + n].reshape(m.shape[:2]))
        o += n
    return out


def _restated(img, lab, S, T, m, nc, pm):
    from excel_amd.utils import superpixels as sx
    sp, cen = sx.slic_numpy(img, S, m, T)
    out, cnt = sx.snap_numpy(lab, sp, cen.shape[0], nc, pm / 1000)
    return sp, cen, out, cnt


@pytest.mark.parametrize("iters,compactness", R.PARAMS)
@pytest.mark.parametrize("shape,step", R.SHAPES)
def test_both_entries_equal_the_judge_and_the_restatement(gpu, shape, step, iters, compactness):
    """The three patterns (noise on blocks, a constant colour, a 0/255 checkerboard) of one shape as a ragged batch and as a uniform one,
    into outputs whose every byte was 0xFF; then the vote at every (num_classes, min_share) of the table; a second run gives identical
    bits."""
    from excel_amd.utils import superpixels as sx
    pats = sorted(R.PATTERNS)
    cases = [R.want_slic(p, shape, step, iters, compactness) for p in pats]
    imgs = [c[0] for c in cases]
    plan, hwc = _ragged(imgs)
    n, k = plan.total_label_pix, cases[0][2].shape[0]
    sp, cen, cent = sx.slic_superpixels(hwc, step, compactness, iters, plan=plan, out=(_poisoned(n, torch.int32), _poisoned(5 * 3 * k, torch.int32)))
    assert cent[1] == 3 * k and cent[0].tolist() == [0, k, 2 * k, 3 * k]
    sp_u, cen_u, _ = sx.slic_superpixels(_dev(np.stack(imgs)), step, compactness, iters)
    assert sp_u.shape == (3,) + shape and torch.equal(sp_u.reshape(-1), sp) and torch.equal(cen_u, cen), "uniform and ragged launches differ"
    for b, ((img, want_sp, want_cen, _), got_sp) in enumerate(zip(cases, _split(sp, imgs))):
        assert np.array_equal(got_sp, want_sp), f"sp of {pats[b]} {shape}"
        assert np.array_equal(cen[b * k:(b + 1) * k].cpu().numpy(), want_cen), f"centres of {pats[b]} {shape}"
        r_sp, r_cen = sx.slic_numpy(img, step, compactness, iters)
        assert np.array_equal(got_sp, r_sp) and np.array_equal(want_cen, r_cen)
    for nc, pm in VOTES:
        votes = [R.want_snap(p, shape, step, iters, compactness, nc, pm) for p in pats]
        labs = [v[0] for v in votes]
        lab = _ragged(labs)[1]
        out, counts = sx.snap_labels(lab, sp, step, nc, pm / 1000, plan=plan, cent=cent, out=(_poisoned(n, torch.uint8), _poisoned(9, torch.int32)))
        out_u, counts_u = sx.snap_labels(_dev(np.stack(labs)), sp_u, step, nc, pm / 1000)
        assert torch.equal(out_u.reshape(-1), out) and torch.equal(counts_u, counts)
        again = sx.snap_labels(lab, sp, step, nc, pm / 1000, plan=plan, cent=cent)
        assert torch.equal(again[0], out) and torch.equal(again[1], counts), "two runs differ"
        for b, ((_, want_out, want_cnt), got) in enumerate(zip(votes, _split(out, labs))):
            assert np.array_equal(got, want_out), f"out of {pats[b]} {shape} nc {nc} share {pm}"
            assert counts[b].tolist() == want_cnt.tolist(), (pats[b], shape, nc, pm, counts[b].tolist(), want_cnt.tolist())


def test_a_ragged_batch_of_three_sizes_with_a_single_pixel_in_the_middle(gpu):
    """Nothing reaches across images: the neighbours of the 1 x 1 image carry other colours and other labels, and its only pixel sits
    between their last and first bytes.  Each image equals the judge's answer on that image alone."""
    from excel_amd.utils import superpixels as sx
    imgs = [R.blocks(11, 14), np.asarray([[[250, 3, 120]]], np.uint8), R.checker(6, 5), R.blocks(70, 130, seed=3)]
    labs = [np.full((11, 14), 4, np.uint8), np.asarray([[9]], np.uint8), np.full((6, 5), 2, np.uint8), None]
    labs[0][:, ::3] = 1
    S, m, T = 5, 3, 4
    want = [R.slic(im, S, m, T) for im in imgs]
    labs[3] = R.labels_for(want[3][0], want[3][1].shape[0])
    plan, hwc = _ragged(imgs)
    sp, cen, cent = sx.slic_superpixels(hwc, S, m, T, plan=plan)
    off = cent[0].tolist()
    assert off == sx.centre_offsets([im.shape[:2] for im in imgs], S).tolist() and off[2] - off[1] == 1
    out, counts = sx.snap_labels(_ragged(labs)[1], sp, S, R.NC, 0.5, plan=plan, cent=cent)
    for b, (w, got_sp, got_out) in enumerate(zip(want, _split(sp, imgs), _split(out, imgs))):
        assert np.array_equal(got_sp, w[0]) and np.array_equal(cen[off[b]:off[b + 1]].cpu().numpy(), w[1]), b
        want_out, want_cnt = R.snap(labs[b], w[0], R.NC, 500)
        assert np.array_equal(got_out, want_out) and counts[b].tolist() == want_cnt.tolist(), b
    assert cen[off[1]].tolist() == [0, 0, 250, 3, 120] and counts[1].tolist() == [1, 1, 0]


def test_the_pinned_empty_centre(gpu):
    from excel_amd.utils import superpixels as sx
    e = R.EMPTY_CASE
    img = R.tiny_image(e["seed"], colours=e["colours"])
    want_sp, want_cen, emptied = R.slic(img, e["S"], e["m"], e["T"])
    assert emptied
    sp, cen, _ = sx.slic_superpixels(_dev(img[None]), e["S"], e["m"], e["T"])
    assert np.array_equal(sp[0].cpu().numpy(), want_sp) and np.array_equal(cen.cpu().numpy(), want_cen)


@pytest.mark.parametrize("offset", [1, 3])
def test_maps_that_start_at_odd_bytes(gpu, offset):
    from excel_amd.utils import superpixels as sx
    shapes = [(17, 63), (1, 65), (16, 64)]
    imgs = [R.blocks(h, w, seed=offset) for h, w in shapes]
    S, m, T = 8, 10, 2
    want = [R.slic(im, S, m, T) for im in imgs]
    labs = [R.labels_for(w[0], w[1].shape[0]) for w in want]
    plan, flat_img = _ragged(imgs)
    flat_lab = _ragged(labs)[1]
    n = plan.total_label_pix
    bufs = [torch.zeros(3 * n + 64, dtype=torch.uint8, device="cuda"), torch.zeros(n + 64, dtype=torch.uint8, device="cuda"),
            torch.zeros(n + 64, dtype=torch.uint8, device="cuda")]
    hwc, lab, out = bufs[0][offset:offset + 3 * n], bufs[1][offset:offset + n], bufs[2][offset:offset + n]
    hwc.copy_(flat_img)
    lab.copy_(flat_lab)
    assert hwc.data_ptr() % 2 == 1 and lab.data_ptr() % 2 == 1 and out.data_ptr() % 2 == 1
    sp, cen, cent = sx.slic_superpixels(hwc, S, m, T, plan=plan)
    got_out, counts = sx.snap_labels(lab, sp, S, R.NC, 0.0, plan=plan, cent=cent, out=(out, torch.empty(9, dtype=torch.int32, device="cuda")))
    assert got_out.data_ptr() == out.data_ptr()
    off = cent[0].tolist()
    for b, (w, got_sp, got) in enumerate(zip(want, _split(sp, imgs), _split(got_out, imgs))):
        assert np.array_equal(got_sp, w[0]) and np.array_equal(cen[off[b]:off[b + 1]].cpu().numpy(), w[1]), (offset, b)
        want_out, want_cnt = R.snap(labs[b], w[0], R.NC, 0)
        assert np.array_equal(got, want_out) and counts[b].tolist() == want_cnt.tolist(), (offset, b)
    assert bool((bufs[2][:offset] == 0).all()) and bool((bufs[2][offset + n:] == 0).all()), "a write outside the maps"


def test_a_wrong_cent_off_row_refuses_that_image(gpu):
    """One centre too many in the middle image's row: its sp is -1, its centres and its labels are untouched, it counts nothing; its
    neighbours - the last one at shifted offsets - are computed as ever.  Likewise an end beyond the total and a negative start."""
    from excel_amd.utils import superpixels as sx
    imgs = [R.blocks(11, 14), R.blocks(1, 1), R.blocks(6, 5)]
    S, m, T = 5, 10, 3
    want = [R.slic(im, S, m, T) for im in imgs]
    labs = [R.labels_for(w[0], w[1].shape[0]) for w in want]
    labs[1][:] = 6
    plan, hwc = _ragged(imgs)
    lab = _ragged(labs)[1]
    n = plan.total_label_pix
    assert sx.centre_offsets([im.shape[:2] for im in imgs], S).tolist() == [0, 9, 10, 12]
    for offs, total, refused in (([0, 9, 11, 13], 13, [1]), ([0, 9, 10, 12], 11, [2]), ([-9, 0, 1, 3], 3, [0]), ([0, 9, 10, 12], 12, [])):
        cent = (_dev(np.asarray(offs, np.int32)), total)
        sp, cen = _poisoned(n, torch.int32), _poisoned(5 * total, torch.int32)
        sx.slic_superpixels(hwc, S, m, T, plan=plan, cent=cent, out=(sp, cen))
        out, counts = sx.snap_labels(lab, sp, S, R.NC, 0.0, plan=plan, cent=cent, out=(_poisoned(n, torch.uint8), _poisoned(9, torch.int32)))
        rest = sx.snap_batch_numpy(imgs, labs, S, R.NC, m, T, 0.0, cent_off=offs, cent_total=total)
        cen = cen.view(total, 5).cpu().numpy()
        written = np.zeros(total, bool)
        for b, (w, got_sp, got_out) in enumerate(zip(want, _split(sp, imgs), _split(out, imgs))):
            assert np.array_equal(got_sp, rest[b][0]) and np.array_equal(got_out, rest[b][2]) and counts[b].tolist() == rest[b][3].tolist(), (offs, b)
            if b in refused:
                assert (got_sp == -1).all() and np.array_equal(got_out, labs[b]) and counts[b].tolist() == [0, 0, 0], (offs, b)
            else:
                want_out, want_cnt = R.snap(labs[b], w[0], R.NC, 0)
                assert np.array_equal(got_sp, w[0]) and np.array_equal(cen[offs[b]:offs[b + 1]], w[1]), (offs, b)
                assert np.array_equal(got_out, want_out) and counts[b].tolist() == want_cnt.tolist(), (offs, b)
                written[offs[b]:offs[b + 1]] = True
        assert (cen[~written] == -1).all(), "a centre of a refused image (or of nobody) was written"


def test_bad_arguments_are_refused_before_any_launch(gpu):
    from excel_amd import ops
    from excel_amd.utils import superpixels as sx
    plan = ops.RaggedPlan([(2, 4), (3, 5)], "cuda")
    n = plan.total_label_pix
    hwc = torch.zeros(3 * n + 8, dtype=torch.uint8, device="cuda")
    lab = torch.zeros(n + 8, dtype=torch.uint8, device="cuda")
    out = torch.full((2 * n + 8,), 0x5A, dtype=torch.uint8, device="cuda")
    sp = torch.full((n + 8,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    cen = torch.full((5 * 4 + 8,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    counts = torch.full((16,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    coff = torch.tensor([0, 1, 3, 0], dtype=torch.int32, device="cuda")
    lib = ops.lib()
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    ip, lp, op, sp_, kp, cp, fp = (C.c_void_p(t.data_ptr()) for t in (hwc, lab, out, sp, cen, counts, coff))
    info, tab = C.byref(plan.info), C.c_void_p(plan.table.data_ptr())
    off = lambda t, k: C.c_void_p(t.data_ptr() + k)
    big = plan.info.__class__.from_buffer_copy(plan.info)
    big.total_label_pix = 2 ** 31
    #        hwc  B  H  W  table info cent_off total step m  T  sp  centres stream
    good = (ip, 2, 0, 0, tab, info, fp, 3, 4, 10, 5, sp_, kp, st)
    def slic(**kw):
        names = ["hwc", "B", "H", "W", "table", "info", "cent_off", "cent_total", "step", "compactness", "iters", "sp", "centres", "stream"]
        a = dict(zip(names, good))
        a.update(kw)
        return [a[k] for k in names]
    for args, word in ((slic(hwc=None), "null argument"), (slic(sp=None), "null argument"), (slic(centres=None), "null argument"),
                       (slic(cent_off=None), "null cent_off"), (slic(step=1), "2 <= step <= 64 (got 1)"), (slic(step=65), "2 <= step <= 64 (got 65)"),
                       (slic(compactness=0), "1 <= compactness <= 64 (got 0)"), (slic(compactness=65), "1 <= compactness <= 64 (got 65)"),
                       (slic(iters=-1), "0 <= iters <= 16 (got -1)"), (slic(iters=17), "0 <= iters <= 16 (got 17)"),
                       (slic(sp=off(sp, 2)), "4-byte aligned"), (slic(centres=off(cen, 1)), "4-byte aligned"), (slic(cent_off=off(coff, 2)), "4-byte aligned"),
                       (slic(B=0, H=2, W=4, table=None, info=None), "1 <= B <= 65535 (B = 0)"),
                       (slic(B=65536, H=1, W=1, table=None, info=None), "1 <= B <= 65535 (B = 65536)"),
                       (slic(B=3), "the plan holds 2 images, B = 3"), (slic(B=1, H=0, W=4, table=None, info=None), "H >= 1 and W >= 1"),
                       (slic(info=C.byref(big)), "outside [1, 2^31)"), (slic(B=64, H=8192, W=8192, table=None, info=None), "outside [1, 2^31)"),
                       (slic(cent_total=0), "centres in all, outside [1, 2^31)"), (slic(cent_total=2 ** 31), "centres in all, outside [1, 2^31)"),
                       (slic(cent_total=n + 1), "centres for")):
        assert lib.excel_slic_superpixels(*args) == -1, word
        assert word in lib.excel_last_error().decode(), (word, lib.excel_last_error())
    #        labels sp B H W table info cent_off total step nc pm out counts stream
    good2 = (lp, sp_, 2, 0, 0, tab, info, fp, 3, 4, 21, 0, op, cp, st)
    def snap(**kw):
        names = ["labels", "sp", "B", "H", "W", "table", "info", "cent_off", "cent_total", "step", "num_classes", "min_share_pm", "out", "counts", "stream"]
        a = dict(zip(names, good2))
        a.update(kw)
        return [a[k] for k in names]
    for args, word in ((snap(labels=None), "null argument"), (snap(sp=None), "null argument"), (snap(out=None), "null argument"),
                       (snap(counts=None), "null argument"), (snap(cent_off=None), "null cent_off"), (snap(step=0), "2 <= step <= 64 (got 0)"),
                       (snap(num_classes=0), "num_classes"), (snap(num_classes=256), "num_classes"),
                       (snap(min_share_pm=-1), "0 <= min_share_pm <= 1000 (got -1)"), (snap(min_share_pm=1001), "0 <= min_share_pm <= 1000 (got 1001)"),
                       (snap(sp=off(sp, 1)), "4-byte aligned"), (snap(counts=off(counts, 2)), "4-byte aligned"),
                       (snap(B=0, H=2, W=4, table=None, info=None), "1 <= B <= 65535 (B = 0)"), (snap(B=3), "the plan holds 2 images, B = 3"),
                       (snap(info=C.byref(big)), "outside [1, 2^31)"), (snap(cent_total=0), "centres in all, outside [1, 2^31)"),
                       (snap(out=lp), "out overlaps labels"), (snap(out=off(lab, n - 1)), "out overlaps labels"),
                       (snap(out=C.c_void_p(sp.data_ptr() + 4 * n - 1)), "out overlaps sp")):
        assert lib.excel_snap_labels_to_superpixels(*args) == -1, word
        assert word in lib.excel_last_error().decode(), (word, lib.excel_last_error())
    torch.cuda.synchronize()
    for t, v in ((out, 0x5A), (sp, 0x5A5A5A5A), (cen, 0x5A5A5A5A), (counts, 0x5A5A5A5A)):
        assert bool((t == v).all()), "a refused call wrote to its outputs"
    # the wrappers' own checks
    for kw, word in ((dict(step=1), "grid step"), (dict(step=4, compactness=0), "snap_compactness"), (dict(step=4, iters=17), "snap_iters")):
        with pytest.raises(ValueError, match=word):
            sx.slic_superpixels(hwc[:3 * n], plan=plan, **kw)
    with pytest.raises(ValueError, match="the plan holds 23 pixels of 3"):
        sx.slic_superpixels(hwc, 4, plan=plan)
    with pytest.raises(ValueError, match=r"uniform images must be \[B,H,W,3\]"):
        sx.slic_superpixels(hwc, 4)
    with pytest.raises(ValueError, match="must be uint8"):
        sx.slic_superpixels(hwc[:3 * n].int(), 4, plan=plan)
    good_sp = sx.slic_superpixels(hwc[:3 * n], 4, plan=plan)[0]
    for kw, word in ((dict(min_share=1.5), "snap_min_share"), (dict(min_share="half"), "snap_min_share"), (dict(num_classes=256), r"outside \[1, 255\]")):
        with pytest.raises(ValueError, match=word):
            sx.snap_labels(lab[:n], good_sp, 4, **{"num_classes": 21, **kw}, plan=plan)
    with pytest.raises(ValueError, match="sp must hold"):
        sx.snap_labels(lab[:n], good_sp[:-1], 4, 21, plan=plan)
    with pytest.raises(ValueError, match="labels must be uint8"):
        sx.snap_labels(lab[:n].int(), good_sp, 4, 21, plan=plan)
    with pytest.raises(RuntimeError, match="out overlaps labels"):
        sx.snap_labels(lab[:n], good_sp, 4, 21, plan=plan, out=(lab[:n], counts[:6]))


# ------------------------------------------------------------------ the stream contract (tests/_streams.py, by import)
@pytest.fixture(scope="module")
def t_link(gpu):
    t = St.time_link()
    print(f"\n[snap streams] one chain link: {t * 1e6:.0f} us")
    assert t > 0
    return t


@pytest.fixture(scope="module")
def stream_case(gpu):
    """fn() -> both entries' outputs from uninitialised memory on the current stream, and the reference on the idle default stream."""
    from excel_amd.utils import superpixels as sx
    shapes = [(120, 200), (75, 333), (17, 65), (200, 120)] * 4
    imgs = [R.blocks(h, w, seed=i) for i, (h, w) in enumerate(shapes)]
    rs = np.random.RandomState(3)
    labs = [rs.randint(0, 4, (h, w)).astype(np.uint8) for h, w in shapes]
    plan, hwc = _ragged(imgs)
    lab = _ragged(labs)[1]
    cent = sx.centre_table(shapes, 16, "cuda")
    torch.cuda.synchronize()

    def fn():
        sp, cen, _ = sx.slic_superpixels(hwc, 16, 10, 5, plan=plan, cent=cent)
        out, counts = sx.snap_labels(lab, sp, 16, R.NC, 0.0, plan=plan, cent=cent)
        return dict(sp=sp, centres=cen, out=out, counts=counts)
    return fn, St.reference(fn)


@pytest.mark.parametrize("arrangement", ["behind", "beside"])
def test_the_ops_stay_on_their_callers_stream(gpu, stream_case, t_link, arrangement):
    fn, ref = stream_case
    links = St.links_for(ref.t_case, t_link)
    run = (St.run_behind if arrangement == "behind" else St.run_beside)(fn, links)
    print(f"\n[snap streams] {arrangement}: t_case {ref.t_case * 1e3:.2f} ms, {run.links} links, side-stream run {run.host_s * 1e3:.2f} ms, "
          f"default stream busy afterwards: {run.busy}")
    assert int(ref.tree["counts"][:, 2].sum()) > 0
    if arrangement == "behind":
        St.assert_matches(ref.tree, run.final, None, "queued behind a busy chain on its own stream")
        return
    St.assert_matches(ref.tree, run.early, None, "(a) beside a busy default stream, read when the side stream was done")
    St.assert_matches(ref.tree, run.final, None, "(b) beside a busy default stream, read after the device had drained")
    assert run.busy, "(c) " + St.busy_message(run, ref.t_case, t_link)


# ------------------------------------------------------------------ the pipeline and the programs
def _png(path):
    from PIL import Image
    return np.asarray(Image.open(path))


def _hist(g, p, nc=21):
    g, p = g.reshape(-1).astype(np.int64), p.reshape(-1).astype(np.int64)
    m = (g < nc) & (p < nc)
    return np.bincount(nc * g[m] + p[m], minlength=nc * nc).reshape(nc, nc)


def _run_infer_lam(tmp, tag, extra):
    """infer_lam.validate on the synthetic ragged set (6 images at batch 4: two steps) with the tiny checkpoint -> what it left"""
    import json
    import logging
    from _clip_files import write_tiny_clip
    from excel_amd.tools import infer_lam
    ckpt, bpe_path, _ = write_tiny_clip(tmp)
    js, table = str(tmp / f"run_{tag}.json"), str(tmp / f"rows_{tag}.csv")
    argv = ["--synthetic", "6", "--ragged", "true", "--resize_size", "96", "--model", ckpt, "--bpe_path", bpe_path, "--batch_size", "4",
            "--num_workers", "2", "--gemm_check", "false", "--save_label", "true", "--label_dir", str(tmp / f"labels_{tag}"), "--json_out", js,
            "--per_image_scores", table] + extra
    lines = []

    class Capture(logging.Handler):
        def emit(self, record):
            lines.append(record.getMessage())
    cap = Capture(logging.INFO)
    cwd = os.getcwd()
    os.chdir(tmp)
    logging.getLogger().addHandler(cap)
    level = logging.getLogger().level
    logging.getLogger().setLevel(logging.INFO)
    try:
        _, total = infer_lam.validate(infer_lam.get_parser().parse_args(argv))
        with open(js) as f:
            record = json.load(f)
    finally:
        logging.getLogger().removeHandler(cap)
        logging.getLogger().setLevel(level)
        os.chdir(cwd)
    return dict(tmp=tmp, tag=tag, total=total.cpu().numpy(), record=record, table=table, log="\n".join(lines), last=infer_lam.validate.last_snap,
                image_scores=infer_lam.validate.last_image_scores, model=infer_lam.validate.last_model)


@pytest.fixture(scope="module")
def program(gpu, tmp_path_factory):
    tmp = tmp_path_factory.mktemp("snap")
    return _run_infer_lam(tmp, "snap", ["--snap_superpixels", "16", "--snap_label_dir", str(tmp / "snapped"), "--boundary_scores", "true"])


def test_infer_lam_snap_superpixels(gpu, program):
    import csv
    from excel_amd.tools import infer_lam, synthetic
    from excel_amd.utils import superpixels as sx
    from excel_amd.utils.evaluate import scores_from_hist
    p = program
    ds = synthetic.SyntheticSegDataset(6, num_classes=21, seed=1234, ragged=True)
    hist, rows, names, pixels = np.zeros((21, 21), np.int64), [], [], 0
    for i in range(6):
        name, img, gt = ds[i][0], np.ascontiguousarray(np.asarray(ds[i][1], np.uint8)), ds[i][2]
        main = _png(p["tmp"] / "labels_snap" / f"{name}.png")
        _, _, want, cnt = _restated(img, main, 16, 5, 10, 21, 0)
        assert np.array_equal(_png(p["tmp"] / "snapped" / f"{name}.png"), want), name
        hist += _hist(np.asarray(gt), want)
        rows.append(cnt.tolist())
        names.append(name)
        pixels += main.size
    last = p["last"]
    print("superpixels, snapped, changed per image:", rows)
    assert sum(r[2] for r in rows) > 0, "the case changes nothing"
    assert last["names"] == names and last["counts"].tolist() == rows and (last["step"], last["compactness"], last["iters"], last["min_share"]) == (16, 10, 5, 0.0)
    assert np.array_equal(last["hist"].cpu().numpy(), hist), "snap_label_score is `evaluate` on the snapped files"
    want_score = scores_from_hist(torch.from_numpy(hist))
    assert last["score"]["miou"] == want_score["miou"] and last["coverage"] == hist.sum() / p["total"].sum()
    stats = sx.snap_stats(np.asarray(rows), pixels)
    assert last["stats"] == stats
    assert "snap_label_score (--snap_superpixels 16, compactness 10, 5 iterations, min share 0):" in p["log"]
    assert infer_lam.format_scores_table(want_score, infer_lam.VOC_CLASSES) in p["log"]
    assert sx.format_snap_summary(stats, last["coverage"]) in p["log"] and "boundary_score of the snapped labels" in p["log"]
    snap = dict(step=16, compactness=10, iters=5, min_share=0.0)
    assert p["record"]["snap"] == sx.snap_json(snap, stats, want_score, last["coverage"]) and p["record"]["snap"]["changed"] == stats["changed"]
    with open(p["table"]) as f:
        table = list(csv.reader(f))
    assert table[0][-3:] == ["superpixels", "snapped", "pixels_changed"] and "snap_miou" in table[0] and "snap_biou" in table[0]
    assert [r[0] for r in table[1:]] == names and [[int(v) for v in r[-3:]] for r in table[1:]] == rows
    npz = np.load(p["table"] + ".npz")
    assert npz["snaps"].tolist() == rows and np.array_equal(npz["counts_snap"].sum(0), np.stack([hist.sum(1), hist.sum(0), np.diag(hist)]))
    assert "bcounts_snap" in npz.files


def test_without_the_flag_a_run_is_byte_identical_to_a_run_of_the_same_command(gpu, program):
    """Two runs without --snap_superpixels: the same label files, score table, JSON record (but for its three timing fields) and per-image rows; no
    `snap` key, no column.  And the main labels of the run with the flag are those files too: the snap leaves them alone."""
    tmp = program["tmp"]
    a, b = _run_infer_lam(tmp, "off1", []), _run_infer_lam(tmp, "off2", [])
    timing = lambda rec: {k: v for k, v in rec.items() if k not in ("seconds_rank0", "images_per_s_rank0", "images_per_s_job")}
    assert "snap" not in a["record"] and a["last"] is None and "snap_label_score" not in a["log"] and "snapped" not in a["log"]
    assert np.array_equal(a["total"], b["total"]) and np.array_equal(a["total"], program["total"])
    assert a["record"].keys() == b["record"].keys() and timing(a["record"]) == timing(b["record"])
    assert open(a["table"], "rb").read() == open(b["table"], "rb").read() and b"snap" not in open(a["table"], "rb").read()
    names = sorted(os.listdir(tmp / "labels_off1"))
    assert len(names) == 6 and names == sorted(os.listdir(tmp / "labels_off2")) == sorted(os.listdir(tmp / "labels_snap"))
    for n in names:
        raw = open(tmp / "labels_off1" / n, "rb").read()
        assert raw == open(tmp / "labels_off2" / n, "rb").read() == open(tmp / "labels_snap" / n, "rb").read(), n


def test_pipeline_snap_step(gpu, program):
    """snap= on the ragged step: the snapped maps are the restatement's answer on the step's own main labels, hist_snap the host confusion
    of those maps; with clean= and fill= the order is snap -> clean -> fill, against the three restatements chained; and the main outputs
    equal those of a pipeline built without snap."""
    from excel_amd import ops
    from excel_amd.pipeline import TrainingFreePipeline
    from excel_amd.utils import components as cc
    from excel_amd.utils import label_fill as lf
    model = program["model"]
    rs = np.random.RandomState(41)
    sizes = [(40, 151), (17, 65), (64, 96), (33, 70)]
    imgs_h = [R.blocks(h, w, seed=b) for b, (h, w) in enumerate(sizes)]
    images = _dev(np.concatenate([im.reshape(-1) for im in imgs_h]))
    gts_h = [rs.randint(0, 21, (h, w)).astype(np.uint8) for h, w in sizes]
    gts = _dev(np.concatenate([g.reshape(-1) for g in gts_h]))
    cls = np.zeros((4, 20), np.float32)
    for b, k in enumerate([1, 3, 2, 3]):
        cls[b, rs.choice(20, size=k, replace=False)] = 1
    cls = _dev(cls)
    plan = ops.RaggedPlan(sizes, "cuda")
    maps = [np.empty(s, np.uint8) for s in sizes]
    clean = dict(min_region=6, connectivity=4)
    plain = TrainingFreePipeline(model, num_classes=21, smax=3, image_scores=True, clean=clean, fill=dict(radius=None))
    plain_labels = plain.run_batch_ragged(images, plan, cls, gts, S=96)
    assert plain.last_snap_labels is None and plain.last_snap_counts is None and plain.last_snap_sp is None and plain.hist_snap is None
    assert "snap" not in plain.last_score_ticket.counts()
    for snap in (dict(step=8), dict(step=16, compactness=3, iters=2, min_share=0.6)):
        full = {**dict(compactness=10, iters=5, min_share=0.0), **snap}
        p = TrainingFreePipeline(model, num_classes=21, smax=3, image_scores=True, snap=snap)
        labels = p.run_batch_ragged(images, plan, cls, gts, S=96)
        assert torch.equal(labels, plain_labels) and torch.equal(p.hist, plain.hist) and p.last_clean_labels is None
        q = TrainingFreePipeline(model, num_classes=21, smax=3, image_scores=True, snap=snap, clean=clean, fill=dict(radius=None))
        assert torch.equal(q.run_batch_ragged(images, plan, cls, gts, S=96), plain_labels) and torch.equal(q.last_snap_labels, p.last_snap_labels)
        hist, changed = np.zeros((21, 21), np.int64), 0
        for b, (main, got, got_sp, g) in enumerate(zip(_split(labels, maps), _split(p.last_snap_labels, maps), _split(p.last_snap_sp, maps), gts_h)):
            sp, _, want, cnt = _restated(imgs_h[b], main, full["step"], full["iters"], full["compactness"], 21, int(round(1000 * full["min_share"])))
            assert np.array_equal(got_sp, sp) and np.array_equal(got, want) and p.last_snap_counts[b].tolist() == cnt.tolist(), (snap, b)
            hist += _hist(g, want)
            changed += int(cnt[2])
            cleaned, ccnt = cc.clean_numpy(want, 6, 21, 4)
            filled, _, fcnt = lf.fill_numpy(cleaned, 21, mask=want)
            assert np.array_equal(_split(q.last_clean_labels, maps)[b], cleaned) and q.last_clean_counts[b].tolist() == ccnt.tolist(), (snap, b)
            assert np.array_equal(_split(q.last_fill_labels, maps)[b], filled) and q.last_fill_counts[b].tolist() == fcnt.tolist(), (snap, b)
        assert changed > 0, "the case changes nothing"
        assert np.array_equal(p.hist_snap.cpu().numpy(), hist) and p.hist_snap.dtype == torch.int64
        assert np.array_equal(p.last_score_ticket.counts()["snap"].sum(0), np.stack([hist.sum(1), hist.sum(0), np.diag(hist)]))
        p.reset()
        assert p.hist_snap is None
    with pytest.raises(ValueError, match="snap must be"):
        TrainingFreePipeline(model, num_classes=21, smax=3, snap=dict(compactness=3))
    p = TrainingFreePipeline(model, num_classes=21, smax=3, snap=dict(step=8))
    for fn in (p.run_batch, p.run_batch_split, p.run_batch_overlapped):
        with pytest.raises(ValueError, match="has no superpixel snap"):
            fn(torch.zeros(2, 3, 96, 96, device="cuda"), cls[:2])


def test_eval_labels_on_the_device_equals_its_numpy_path(gpu, program, monkeypatch):
    """eval_labels --snap_superpixels on infer_lam's own label PNGs, with the images written as JPEGs: the device path and the numpy path
    give the same matrices, rows and files, and both are the restatement on the decoded JPEGs."""
    from excel_amd.tools import eval_labels, synthetic
    from PIL import Image
    p = program
    ds = synthetic.SyntheticSegDataset(6, num_classes=21, seed=1234, ragged=True)
    root, lists = p["tmp"] / "VOC", p["tmp"] / "lists"
    (root / "SegmentationClassAug").mkdir(parents=True, exist_ok=True)
    (root / "JPEGImages").mkdir(exist_ok=True)
    lists.mkdir(exist_ok=True)
    names = [ds[i][0] for i in range(6)]
    for i, n in enumerate(names):
        Image.fromarray(np.asarray(ds[i][2], np.uint8)).save(root / "SegmentationClassAug" / f"{n}.png")
        Image.fromarray(np.ascontiguousarray(np.asarray(ds[i][1], np.uint8))).save(root / "JPEGImages" / f"{n}.jpg", quality=90)
    (lists / "val.txt").write_text("\n".join(names) + "\n")
    parse = eval_labels.get_parser().parse_args
    base = ["--pred_dir", str(p["tmp"] / "labels_snap"), "--data_folder", str(root), "--list_folder", str(lists), "--infer_set", "val",
            "--num_workers", "2", "--batch_size", "4", "--snap_superpixels", "16", "--snap_compactness", "20", "--clean_min_region", "12", "--fill_ignore", "3"]
    with monkeypatch.context() as mp:
        dev = eval_labels.validate(parse(base + ["--snap_label_dir", str(p["tmp"] / "ev_dev"), "--fill_label_dir", str(p["tmp"] / "ev_dev_fill")]))
        mp.setattr(torch.cuda, "is_available", lambda: False)
        host = eval_labels.validate(parse(base + ["--snap_label_dir", str(p["tmp"] / "ev_host"), "--fill_label_dir", str(p["tmp"] / "ev_host_fill")]))
    for which in ("snap", "clean", "fill"):
        assert np.array_equal(dev[which]["hist"].numpy(), host[which]["hist"].numpy()) and dev[which]["counts"].tolist() == host[which]["counts"].tolist(), which
    assert dev["snap"]["stats"] == host["snap"]["stats"] and int(dev["snap"]["counts"][:, 2].sum()) > 0
    for i, n in enumerate(names):
        got = _png(p["tmp"] / "ev_dev" / f"{n}.png")
        assert np.array_equal(got, _png(p["tmp"] / "ev_host" / f"{n}.png")), n
        assert np.array_equal(_png(p["tmp"] / "ev_dev_fill" / f"{n}.png"), _png(p["tmp"] / "ev_host_fill" / f"{n}.png")), n
        img = np.asarray(Image.open(root / "JPEGImages" / f"{n}.jpg").convert("RGB"))
        want = _restated(img, _png(p["tmp"] / "labels_snap" / f"{n}.png"), 16, 5, 20, 21, 0)[2]
        assert np.array_equal(got, want), n
