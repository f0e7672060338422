"""The DenseCRF stage for LAMs on ragged batches (excel_dcrf_lam_ragged): every image of a group runs the mean field over its OWN number
of classes, on pitched step cams whose pad columns and unused planes are never read.  Marginals and labels against the per-image entry
on the image's tight planes (bit for bit), independence of neighbours and grouping, ties, the key lookup, the numpy oracle, refusals -
and infer_lam --crf_inline true against the record path and the per-image path."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

SIZES = [(37, 50), (23, 3), (30, 41), (16, 64), (9, 1), (25, 66)]
CMAX = 7
MIXED = [2, 7, 3, 2, 5, 2]
LAM_SET = (3, 1, 4, 67, 3)                # tools/infer_lam.py:191-198 as (pos_w, pos_xy_std, bi_w, bi_xy_std, bi_rgb_std)


@pytest.fixture(scope="module")
def gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from excel_amd import _lib
    _lib.lib()
    return torch.device("cuda")


def _image(rs, H, W):
    img = (rs.rand(H, W, 3) * 255).astype(np.uint8)
    img[:, : W // 2] = (img[:, : W // 2] * 0.15 + 140).astype(np.uint8)
    return img


def _prob(rs, C, H, W):
    p = rs.rand(C, H, W).astype(np.float32) ** 2 + 1e-3
    return p / p.sum(0, keepdims=True)


def _batch(sizes, nchan, seed):
    rs = np.random.RandomState(seed)
    return [_image(rs, H, W) for H, W in sizes], [_prob(rs, c, H, W) for (H, W), c in zip(sizes, nchan)]


def _pitched(plan, planes, Cmax, fill=np.nan):
    """Cmax pitched planes per image, `fill` in every pad column and every plane >= the image's own count."""
    out = np.full(Cmax * plan.total_pix, fill, np.float32)
    for b, p in enumerate(planes):
        c, H, W = p.shape
        Wp = (W + 3) // 4 * 4
        o = Cmax * int(plan.poff[b])
        out[o:o + Cmax * H * Wp].reshape(Cmax, H, Wp)[:c, :, :W] = p
    return out


def _valid_mask(plan, nchan, Cmax):
    m = np.zeros(Cmax * plan.total_pix, bool)
    for b, c in enumerate(nchan):
        H, W = int(plan.hw[b, 0]), int(plan.hw[b, 1])
        Wp = (W + 3) // 4 * 4
        o = Cmax * int(plan.poff[b])
        m[o:o + Cmax * H * Wp].reshape(Cmax, H, Wp)[:c, :, :W] = True
    return m


def _run(gpu, sizes, imgs, probs, nchan, iters, cls_idx=None, Cmax=CMAX, q_fill=None, **kw):
    from excel_amd import ops
    plan = ops.RaggedPlan(sizes, gpu)
    images = torch.from_numpy(np.concatenate([i.reshape(-1) for i in imgs])).to(gpu)
    cams = torch.from_numpy(_pitched(plan, probs, Cmax)).to(gpu)
    nc = torch.tensor(nchan, dtype=torch.int32, device=gpu)
    ci = None if cls_idx is None else torch.tensor(cls_idx, dtype=torch.int32, device=gpu)
    labels, q = ops.dcrf_lam_ragged(images, plan, cams, Cmax, nc, nchan, ci, iters, *LAM_SET, **kw)
    return plan, labels, q


def _alone(gpu, img, prob, iters, keys=None):
    """The per-image chain of crf_proc: ops.dcrf_inference on the tight planes, arg-max, key lookup."""
    from excel_amd import ops
    q = ops.dcrf_inference(torch.from_numpy(img).to(gpu), torch.from_numpy(prob).to(gpu), iters, *LAM_SET)
    lab = ops.argmax_label(q[None])[0].cpu().numpy()
    if keys is not None:
        lab = np.pad(np.asarray(keys) + 1, (1, 0))[lab]
    return q.cpu().numpy(), lab.astype(np.uint8)


_REF = {}


def _reference(gpu, nchan_key, seed, iters):
    """Per-image references of a batch, computed once per (class counts, seed, iters) and shared."""
    key = (tuple(nchan_key), seed, iters)
    if key not in _REF:
        sizes = SIZES[:len(nchan_key)]
        imgs, probs = _batch(sizes, nchan_key, seed)
        _REF[key] = (imgs, probs, [_alone(gpu, i, p, iters) for i, p in zip(imgs, probs)])
    return _REF[key]


@pytest.mark.parametrize("iters", [0, 10])
@pytest.mark.parametrize("nchan", [MIXED, [3] * 6, [4]], ids=["mixed", "uniform3", "one"])
def test_every_image_has_the_bits_it_gets_alone(gpu, nchan, iters):
    from excel_amd import ops
    sizes = SIZES[:len(nchan)]
    imgs, probs, refs = _reference(gpu, nchan, 31, iters)
    plan = ops.RaggedPlan(sizes, gpu)
    images = torch.from_numpy(np.concatenate([i.reshape(-1) for i in imgs])).to(gpu)
    cams = torch.from_numpy(_pitched(plan, probs, CMAX)).to(gpu)
    nc = torch.tensor(nchan, dtype=torch.int32, device=gpu)
    labels, q = ops.dcrf_lam_ragged(images, plan, cams, CMAX, nc, nchan, None, iters, *LAM_SET, want_labels=True, want_q=True)
    lab_only, none = ops.dcrf_lam_ragged(images, plan, cams, CMAX, nc, nchan, None, iters, *LAM_SET, want_labels=True, want_q=False)
    assert none is None and torch.equal(lab_only, labels)
    for b, (q_ref, l_ref) in enumerate(refs):
        got = plan.planes(q, b, CMAX)[:nchan[b]].cpu().numpy()
        assert np.array_equal(got, q_ref), f"image {b} {sizes[b]} nchan {nchan[b]}: Q differs from excel_dcrf_inference"
        assert np.array_equal(plan.label(labels, b).cpu().numpy(), l_ref), f"image {b}: labels differ"
    # nothing outside the valid region of a pre-filled q_out is modified: the entry itself, on a buffer of a known pattern
    from excel_amd import _lib
    import ctypes as C
    q2 = torch.full((CMAX * plan.total_pix,), -7.5, dtype=torch.float32, device=gpu)
    host = np.asarray(nchan, np.int32)
    ws = torch.empty(ops.dcrf_lam_ragged_workspace_bytes(sizes, nchan), dtype=torch.uint8, device=gpu)
    rc = _lib.lib().excel_dcrf_lam_ragged(images.data_ptr(), cams.data_ptr(), nc.data_ptr(), host.ctypes.data_as(C.POINTER(C.c_int32)), None,
                                          plan.table.data_ptr(), C.byref(plan.info), CMAX - 1, CMAX, iters, *[float(v) for v in LAM_SET], None,
                                          q2.data_ptr(), ws.data_ptr(), torch.cuda.current_stream().cuda_stream)
    assert rc == 0
    q2, mask = q2.cpu().numpy(), _valid_mask(plan, nchan, CMAX)
    assert np.array_equal(q2[mask], q.cpu().numpy()[mask]) and np.all(q2[~mask] == -7.5)


def test_neighbours_and_grouping_change_nothing(gpu):
    from excel_amd import ops
    a = 2
    imgs, probs = _batch(SIZES, MIXED, seed=11)
    plan, labels, q = _run(gpu, SIZES, imgs, probs, MIXED, 10, want_labels=True, want_q=True)
    ref_q, ref_l = plan.planes(q, a, CMAX)[:MIXED[a]].clone(), plan.label(labels, a).clone()
    # the others get other class counts and other contents
    other = [7, 1, MIXED[a], 6, 1, 4]
    imgs2, probs2 = _batch(SIZES, other, seed=12)
    imgs2[a], probs2[a] = imgs[a], probs[a]
    plan2, labels2, q2 = _run(gpu, SIZES, imgs2, probs2, other, 10, want_labels=True, want_q=True)
    assert torch.equal(plan2.planes(q2, a, CMAX)[:MIXED[a]], ref_q) and torch.equal(plan2.label(labels2, a), ref_l)
    assert not torch.equal(plan2.label(labels2, 0), plan.label(labels, 0))
    # 1, 2 and 6 groups
    ws = ops.dcrf_lam_ragged_workspace_bytes
    budgets = {1: ws(SIZES, MIXED), 2: max(ws(SIZES[:3], MIXED[:3]), ws(SIZES[3:], MIXED[3:])), 6: 1}
    assert ops.dcrf_lam_groups(SIZES, MIXED, budgets[2]) == [(0, 3), (3, 6)]
    mask = torch.from_numpy(_valid_mask(plan, MIXED, CMAX)).to(gpu)
    import warnings
    for n, budget in budgets.items():
        assert len(ops.dcrf_lam_groups(SIZES, MIXED, budget)) == n
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            _, l3, q3 = _run(gpu, SIZES, imgs, probs, MIXED, 10, want_labels=True, want_q=True, budget_bytes=budget)
        assert ops.dcrf_lam_ragged.last_groups == n
        assert torch.equal(l3, labels) and torch.equal(q3[mask], q[mask]), n


def test_ties_resolve_to_the_first_maximum(gpu):
    nchan = [3, 2, 4, 2, 3, 2]
    imgs, probs = _batch(SIZES, nchan, seed=5)
    for p in probs:
        p[:, : max(p.shape[1] // 2, 1)] = 0.25               # every class equal on the top half: exact ties
    for iters in (0, 10):
        plan, labels, q = _run(gpu, SIZES, imgs, probs, nchan, iters, want_labels=True, want_q=True)
        ties = 0
        for b in range(len(SIZES)):
            q_ref, l_ref = _alone(gpu, imgs[b], probs[b], iters)
            assert np.array_equal(plan.planes(q, b, CMAX)[:nchan[b]].cpu().numpy(), q_ref)
            lab = plan.label(labels, b).cpu().numpy()
            assert np.array_equal(lab, l_ref)
            top = q_ref.max(0)
            tied = (q_ref == top).sum(0) > 1
            ties += int(tied.sum())
            assert np.array_equal(lab[tied], q_ref.argmax(0)[tied])      # numpy's argmax = the first maximum
        if iters == 0:
            assert ties > 0


def test_key_lookup(gpu):
    nchan = [3, 2, 3, 1, 3, 2]
    smax = CMAX - 1
    cls_idx = [[4, 17] + [0] * (smax - 2), [19] + [0] * (smax - 1), [4, 17] + [0] * (smax - 2), [0] * smax, [0, 1] + [0] * (smax - 2),
               [7] + [0] * (smax - 1)]
    imgs, probs = _batch(SIZES, nchan, seed=21)
    for p in probs:                                         # bands that favour one class each: every class survives the mean field
        c, H, W = p.shape
        band = (np.arange(H * W) * c // (H * W)).reshape(H, W)
        p += 4.0 * (np.arange(c)[:, None, None] == band[None])
        p /= p.sum(0, keepdims=True)
    plan, mapped, _ = _run(gpu, SIZES, imgs, probs, nchan, 10, cls_idx=cls_idx)
    _, raw, _ = _run(gpu, SIZES, imgs, probs, nchan, 10, cls_idx=None)
    for b in range(len(SIZES)):
        _, l_ref = _alone(gpu, imgs[b], probs[b], 10, keys=cls_idx[b][:nchan[b] - 1])
        _, r_ref = _alone(gpu, imgs[b], probs[b], 10)
        assert np.array_equal(plan.label(mapped, b).cpu().numpy(), l_ref)
        assert np.array_equal(plan.label(raw, b).cpu().numpy(), r_ref)
    assert set(np.unique(plan.label(mapped, 0).cpu().numpy())) == {0, 5, 18}
    assert set(np.unique(plan.label(raw, 0).cpu().numpy())) == {0, 1, 2}
    assert set(np.unique(plan.label(mapped, 3).cpu().numpy())) == {0}


def test_image_0_against_the_oracle(gpu):
    import oracle
    imgs, probs = _batch(SIZES, MIXED, seed=77)
    plan, _, q = _run(gpu, SIZES, imgs, probs, MIXED, 10, want_labels=False, want_q=True)
    got = plan.planes(q, 0, CMAX)[:MIXED[0]].cpu().numpy()
    ref = oracle.dcrf.dense_crf_2d(imgs[0], oracle.dcrf.unary_from_softmax(probs[0]), 10, *LAM_SET)
    err = float(np.abs(got - ref).max())
    print(f"\nmax |Q - oracle| = {err:.3e}")
    assert err < 1e-3


def test_refusals(gpu):
    from excel_amd import ops
    nchan = [3] * 6
    imgs, probs = _batch(SIZES, nchan, seed=1)
    plan = ops.RaggedPlan(SIZES, gpu)
    images = torch.from_numpy(np.concatenate([i.reshape(-1) for i in imgs])).to(gpu)
    cams = torch.from_numpy(_pitched(plan, probs, CMAX, fill=0.5)).to(gpu)
    nc = torch.tensor(nchan, dtype=torch.int32, device=gpu)
    for bad in (0, CMAX + 1):
        host = list(nchan)
        host[4] = bad
        with pytest.raises(RuntimeError, match="classes"):
            ops.dcrf_lam_ragged(images, plan, cams, CMAX, nc, host, None, 10, *LAM_SET)
    with pytest.raises(ValueError):
        ops.dcrf_lam_ragged(images, plan, cams, CMAX, nc, nchan, None, 10, *LAM_SET, want_labels=False, want_q=False)
    for k in (1, 3, 4):                                                       # pos_xy_std, bi_xy_std, bi_rgb_std
        for v in (0.0, -1.0):
            params = list(LAM_SET)
            params[k] = v
            with pytest.raises(RuntimeError, match="positive"):
                ops.dcrf_lam_ragged(images, plan, cams, CMAX, nc, nchan, None, 10, *params)
    with pytest.raises(ValueError):
        ops.dcrf_lam_ragged(images[:-3], plan, cams, CMAX, nc, nchan, None, 10, *LAM_SET)
    with pytest.raises(ValueError):
        ops.dcrf_lam_ragged(images, plan, cams[:-1], CMAX, nc, nchan, None, 10, *LAM_SET)
    # a device array that disagrees with the host counts is clamped to the group's stride: no write outside the valid planes
    big = torch.full((6,), 1000, dtype=torch.int32, device=gpu)
    _, q = ops.dcrf_lam_ragged(images, plan, cams, CMAX, big, nchan, None, 1, *LAM_SET, want_labels=False, want_q=True)
    _, q_ok = ops.dcrf_lam_ragged(images, plan, cams, CMAX, nc, nchan, None, 1, *LAM_SET, want_labels=False, want_q=True)
    mask = torch.from_numpy(_valid_mask(plan, nchan, CMAX)).to(gpu)
    assert torch.equal(q[mask], q_ok[mask])


# ------------------------------------------------------------------ the program
PROGRAM_HW = [(90, 120), (97, 111), (104, 102), (111, 93)]


def _write_tree(tmp_path, n=12):
    """An on-disk VOC tree: n images of 4 sizes with 1..3 present classes each."""
    from PIL import Image
    from excel_amd.utils import imutils
    root, lists = tmp_path / "VOC2012", tmp_path / "lists"
    (root / "JPEGImages").mkdir(parents=True)
    (root / "SegmentationClassAug").mkdir()
    lists.mkdir()
    rs = np.random.RandomState(9)
    ids, onehot, gts, ks = [], {}, {}, []
    for k in range(n):
        h, w = PROGRAM_HW[k % len(PROGRAM_HW)]
        name = f"2009_{k:06d}"
        ids.append(name)
        coarse = rs.randint(0, 256, (h // 8 + 2, w // 8 + 2, 3)).astype(np.uint8)
        Image.fromarray(np.repeat(np.repeat(coarse, 8, 0), 8, 1)[:h, :w]).save(root / "JPEGImages" / (name + ".jpg"), quality=90)
        lab = rs.randint(0, 21, (h, w)).astype(np.uint8)
        lab[:2] = 255
        gts[name] = lab
        im = Image.fromarray(lab, mode="P")
        im.putpalette(imutils.colormap().flatten().tolist())
        im.save(root / "SegmentationClassAug" / (name + ".png"))
        oh = np.zeros(20, np.float32)
        present = sorted({(k + 7 * j) % 20 for j in range(1 + k % 3)})
        oh[present] = 1
        ks.append(len(present))
        onehot[name] = oh
    (lists / "val.txt").write_text("\n".join(ids) + "\n")
    np.save(lists / "cls_labels_onehot.npy", onehot)
    return root, lists, ids, gts, ks


def _files(d, ids):
    assert sorted(os.listdir(d)) == sorted(n + ".png" for n in ids), d
    return {n: open(os.path.join(d, n + ".png"), "rb").read() for n in ids}


def test_program_inline_stage_equals_the_record_path(gpu, tmp_path):
    """infer_lam --crf_post true over an on-disk tree at --batch_size 5: --crf_inline true (ragged batches, one chain of launches per
    group) gives the record path's CRF confusion matrix and colour-coded files, as does the per-image path, whatever --crf_ws_gb; no
    record is written; --crf_label_dir holds the labels that were scored; the main loop's histogram does not depend on the flag."""
    from PIL import Image
    from _clip_files import write_tiny_clip
    import oracle
    from excel_amd import ops
    from excel_amd.tools import infer_lam
    root, lists, ids, gts, ks = _write_tree(tmp_path)
    assert set(ks) == {1, 2, 3} and len(set(PROGRAM_HW)) >= 4
    ckpt, bpe_path, _ = write_tiny_clip(tmp_path)
    common = ["--data_folder", str(root), "--list_folder", str(lists), "--infer_set", "val", "--resize_size", "128", "--model", ckpt,
              "--bpe_path", bpe_path, "--batch_size", "5", "--num_workers", "2", "--gemm_check", "false", "--crf_post", "true"]

    def run(tag, *extra):
        infer_lam.validate.last_crf = None
        logits = tmp_path / ("logits_" + tag)
        _, total = infer_lam.validate(infer_lam.get_parser().parse_args(common + ["--logits_dir", str(logits), "--segs_crf_rgb_dir",
                                                                                  str(tmp_path / ("rgb_" + tag))] + list(extra)))
        return dict(total=total.cpu().numpy(), crf=infer_lam.validate.last_crf[1].cpu().numpy(), rgb=_files(tmp_path / ("rgb_" + tag), ids),
                    logits=logits, stats=infer_lam.build_validation.last_crf_stats)

    hw = [PROGRAM_HW[k % 4] for k in range(5)]
    budget = ops.dcrf_lam_ragged_workspace_bytes(hw[:2], [k + 1 for k in ks[:2]]) + 4096
    assert len(ops.dcrf_lam_groups(hw, [k + 1 for k in ks[:5]], budget)) > 1
    record = run("record", "--crf_inline", "false")
    inline = run("inline", "--crf_inline", "true", "--crf_label_dir", str(tmp_path / "crf_labels"))
    api = run("api", "--crf_inline", "true", "--api_path", "true")
    groups = run("groups", "--crf_inline", "true", "--crf_ws_gb", repr(budget / 2 ** 30))
    npix = sum(int((g < 21).sum()) for g in gts.values())
    assert int(record["crf"].sum()) == npix and record["stats"] is None and record["logits"].is_dir()
    assert inline["stats"]["calls"] == 3 and inline["stats"]["groups"] == 3 and groups["stats"]["groups"] > 3
    assert 0 < groups["stats"]["peak_workspace_bytes"] <= budget < inline["stats"]["peak_workspace_bytes"]
    for key, r in (("inline", inline), ("api", api), ("groups", groups)):
        assert np.array_equal(r["crf"], record["crf"]), key
        assert np.array_equal(r["total"], record["total"]), key
        assert r["rgb"] == record["rgb"], key
        assert not r["logits"].exists(), key
    # the PNGs of --crf_label_dir are the labels that were scored
    hist = np.zeros((21, 21), np.int64)
    assert sorted(os.listdir(tmp_path / "crf_labels")) == sorted(n + ".png" for n in ids)
    for n in ids:
        im = Image.open(tmp_path / "crf_labels" / (n + ".png"))
        assert im.mode == "P"
        lab = np.asarray(im)
        assert lab.shape == gts[n].shape
        hist += oracle.evaluate.fast_hist(gts[n].flatten(), lab.flatten(), 21)
    assert np.array_equal(hist, record["crf"])
