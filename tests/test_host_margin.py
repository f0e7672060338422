"""The host side of the arg-max margin (utils/margin.py) without a GPU: the numpy reference on a hand-written case and on its special
values, against the background sweep's reference at threshold 0, the threshold parsing, the flags' refusals, the table and the JSON."""
import argparse
import math

import numpy as np
import pytest

from excel_amd.utils import bkg_sweep, margin

INF, NAN = np.inf, np.nan


def _pack(imgs):
    """[(Cmax,H,W) float arrays] -> the packed pitched planes (pad columns +inf) and the sizes."""
    out, sizes = [], []
    for im in imgs:
        c, h, w = im.shape
        p = np.full((c, h, (w + 3) // 4 * 4), INF, np.float32)
        p[:, :, :w] = im
        out.append(p.reshape(-1))
        sizes.append((h, w))
    return np.concatenate(out), sizes


HAND = np.float32([[[1.0, 0.25, 0.5], [0.5, 0.0, 0.75]],      # the background
                   [[0.5, 1.0, 0.25], [0.5, 0.25, 0.5]],
                   [[0.25, 0.5, 1.5], [0.25, 0.25, 1.0]]])


def test_hand_written_case():
    """2 x 3 pixels, three planes.  Row 0: background by 0.5; class 1 over class 2 (0.5) and the background; class 2 over the background
    by 1.0.  Row 1: a tie of the background with class 1 (background, margin 0); a tie of classes 1 and 2 (class 1, margin 0); class 2
    over the background by 0.25."""
    planes, sizes = _pack([HAND])
    gt = np.uint8([0, 1, 1, 0, 255, 2])
    thr = (0.0, 0.25, 0.5, 1.0)
    totals, kept, labels, m = margin.margin_reference(planes, sizes, 3, thr, gts=gt, num_classes=3, label_thre=0.25)
    assert m.dtype == np.float32 and m.tolist() == [0.5, 0.5, 1.0, 0.0, 0.0, 0.25]
    assert labels.dtype == np.uint8 and labels.tolist() == [0, 1, 2, 255, 255, 2]
    assert kept.tolist() == [6, 4, 3, 1, 6]
    assert totals.tolist() == [[[2, 2, 1], [2, 1, 2], [2, 1, 1]],
                               [[1, 2, 1], [1, 1, 2], [1, 1, 1]],
                               [[1, 2, 0], [1, 1, 1], [1, 1, 0]],
                               [[0, 1, 0], [0, 0, 1], [0, 0, 0]]]
    # the label cut is independent of the list, and every output is optional
    t2, k2, l2, m2 = margin.margin_reference(planes, sizes, 3, (), label_thre=0.75)
    assert t2 is None and k2 is None and l2.tolist() == [255, 255, 2, 255, 255, 255] and np.array_equal(m2, m)
    t3, k3, l3, _ = margin.margin_reference(planes, sizes, 3, thr)
    assert t3 is None and l3 is None and k3.tolist() == [6, 4, 3, 1, 6], "the coverage needs no ground truth"
    # a class list: slot value -1 maps to key 0, which is background whatever the planes say - with a negative margin where it lost
    cls = np.int32([[-1, 7]])
    _, _, l4, m4 = margin.margin_reference(planes, sizes, 3, (), cls_idx=cls, label_thre=-INF)
    assert l4.tolist() == [0, 0, 8, 0, 0, 8] and m4.tolist() == [0.5, -0.75, 1.0, 0.0, -0.25, 0.25]


def test_kept_is_nested_and_skip_and_accumulation():
    rs = np.random.RandomState(3)
    imgs = [(rs.randint(0, 17, (4, h, w)) / 8).astype(np.float32) for h, w in [(5, 7), (3, 9), (6, 2)]]
    planes, sizes = _pack(imgs)
    n = sum(h * w for h, w in sizes)
    gt = rs.randint(0, 6, n).astype(np.uint8)
    thr = (0.0, 0.125, 0.5, 0.75, 1.0)
    totals, kept, _, m = margin.margin_reference(planes, sizes, 4, thr, gts=gt, num_classes=5)
    assert (np.diff(kept[:-1]) <= 0).all() and kept[0] > kept[-2] > 0 and kept[-1] == n
    assert (np.diff(totals, axis=0) <= 0).all(), "the kept sets are nested: every count falls with the threshold"
    for j, t in enumerate(thr):
        assert kept[j] == int((m >= np.float32(t)).sum())
    skip = np.int32([0, 1, 0])
    ts, ks, _, ms = margin.margin_reference(planes, sizes, 4, thr, gts=gt, num_classes=5, skip=skip)
    assert ks[-1] == n - 27 and np.array_equal(ms, m) and (ts <= totals).all() and ts.sum() < totals.sum()
    ta, ka, _, _ = margin.margin_reference(planes, sizes, 4, thr, gts=gt, num_classes=5, totals=ts, kept=ks)
    assert np.array_equal(ta, ts + totals) and np.array_equal(ka, ks + kept) and ks[-1] == n - 27, "added to a copy"


def test_one_and_two_planes():
    one = np.float32([[[0.25, NAN, -3.0]]])
    two = np.float32([[[0.5, 0.25, 1.0]], [[0.25, 1.0, 1.0]]])
    planes, sizes = _pack([np.concatenate([one, np.full((1, 1, 3), NAN, np.float32)]), two])
    nchan = np.int32([1, 2])
    thr = (0.0, 1e30)
    _, kept, labels, m = margin.margin_reference(planes, sizes, 2, thr, nchan=nchan, label_thre=3e38)
    assert m[:3].tolist() == [INF, INF, INF] and labels[:3].tolist() == [0, 0, 0], "one plane: +inf, kept everywhere, plane 0 plays no part"
    assert m[3:].tolist() == [0.25, 0.75, 0.0] and labels[3:].tolist() == [255, 255, 255], "two planes: the runner-up of a foreground pixel is v0"
    assert kept.tolist() == [6, 3, 6]
    # the scale is on plane 0 before anything else
    _, _, l2, m2 = margin.margin_reference(planes, sizes, 2, (), nchan=nchan, label_thre=0.0, bkg_scale=4.0)
    assert m2[3:].tolist() == [1.75, 0.0, 3.0] and l2[3:].tolist() == [0, 0, 0]


def test_nan_and_inf_minus_inf_are_dropped_everywhere():
    img = np.float32([[[NAN, 0.5, 0.5, INF, INF, 0.25]],
                      [[0.25, NAN, 0.25, INF, 0.5, INF]],
                      [[0.25, 0.25, NAN, 0.5, 0.5, INF]]])
    planes, sizes = _pack([img])
    gt = np.zeros(6, np.uint8)
    totals, kept, labels, m = margin.margin_reference(planes, sizes, 3, (0.0, 0.5), gts=gt, num_classes=3, label_thre=-INF)
    assert np.isnan(m[:4]).all() and np.isnan(m[5]) and m[4] == INF, "NaN planes; inf - inf both ways; a lone inf wins by inf"
    assert labels.tolist() == [255, 255, 255, 255, 0, 255]
    assert kept.tolist() == [1, 1, 6] and totals.sum() == 6 and totals[:, :, 0].tolist() == [[1, 1, 1], [1, 1, 1]]


@pytest.mark.parametrize("a", [1.0, 1.2])
@pytest.mark.parametrize("with_cls", [False, True])
def test_threshold_zero_is_the_background_sweep(a, with_cls):
    """Code the parent already has: on planes with b0 >= 0, no NaN and no class slot that maps to key 0, every margin is >= 0, so the
    labels and totals at threshold 0 are bkg_sweep.sweep_reference's at scale a."""
    rs = np.random.RandomState(11)
    sizes = [(1, 1), (3, 5), (9, 13), (4, 6)]
    Cmax, nc = 5, 7
    nchan = np.int32([1, 2, 5, 3])
    imgs = []
    for (h, w), k in zip(sizes, nchan):
        im = rs.rand(Cmax, h, w).astype(np.float32) * 2
        im[:, rs.rand(h, w) < 0.3] = (rs.randint(0, 9, (Cmax, 1)) / 4).astype(np.float32)     # ties between planes
        im[k:] = NAN
        imgs.append(im)
    planes, _ = _pack(imgs)
    n = sum(h * w for h, w in sizes)
    gt = rs.randint(0, nc + 2, n).astype(np.uint8)
    gt[rs.rand(n) < 0.1] = 255
    cls = rs.randint(0, nc + 2, (4, Cmax - 1)).astype(np.int32) if with_cls else None
    kw = dict(nchan=nchan, cls_idx=cls, gts=gt, num_classes=nc)
    want_t, want_l = bkg_sweep.sweep_reference(planes, sizes, Cmax, (a,), label_sel=0, **kw)
    totals, kept, labels, m = margin.margin_reference(planes, sizes, Cmax, (0.0,), label_thre=0.0, bkg_scale=a, **kw)
    assert (m >= 0).all() and np.array_equal(labels, want_l) and np.array_equal(totals[0], want_t[0]) and kept[0] == kept[1] == n
    assert len(set(labels.tolist())) > 2


def test_thresholds_are_checked_and_parsed():
    assert margin.check_thresholds([0, 0.05, 1]) == (0.0, 0.05, 1.0)
    assert margin.parse_thresholds("0, 0.05,0.1 ") == (0.0, 0.05, 0.1)
    assert margin.parse_thresholds(None) is None and margin.parse_thresholds("  ") is None
    assert margin.parse_thresholds([0.5]) == (0.5,)
    assert margin.check_thresholds((), allow_empty=True) == ()
    assert len(margin.check_thresholds([i / 16 for i in range(16)])) == 16
    for bad, word in (((), "need 1..16"), ([i for i in range(17)], "need 1..16"), ([0.1, NAN], "finite"), ([INF], "finite"), ([-0.5], ">= 0"),
                      ([0.2, 0.1], "strictly increasing"), ([0.1, 0.1], "strictly increasing"), ([1.0, 1.0 + 1e-12], "as float32"),
                      ([1e39], "float32 range"), (["x"], "must be numbers"), (3, "must be numbers")):
        with pytest.raises(ValueError, match=word):
            margin.check_thresholds(bad)
    with pytest.raises(ValueError, match="--margin_sweep: 'a' is not a number"):
        margin.parse_thresholds("0,a")
    assert margin.check_min(0) == 0.0 and margin.check_min("0.25") == 0.25
    for bad in (-1, NAN, INF, 1e39):
        with pytest.raises(ValueError, match="margin_min: value"):
            margin.check_min(bad)


def _args(*argv):
    p = argparse.ArgumentParser()
    margin.add_flags(p)
    p.add_argument("--api_path", default=False, type=lambda s: s == "true")
    p.add_argument("--unlabeled", default=False, type=lambda s: s == "true")
    return p.parse_args(list(argv))


def test_resolve_and_its_refusals():
    assert margin.resolve(_args()) == (None, None)
    assert margin.resolve(_args(), ragged=False) == (None, None), "off: nothing to refuse"
    assert margin.resolve(_args("--margin_sweep", "0,0.1"), ragged=True) == ((0.0, 0.1), None)
    assert margin.resolve(_args("--margin_min", "0.2")) == (None, dict(min=0.2, label_dir=None))
    assert margin.resolve(_args("--margin_sweep", "0.5", "--margin_min", "0", "--margin_label_dir", "d")) == ((0.5,), dict(min=0.0, label_dir="d"))
    # allowed without ground truth: the coverage needs none, and the maps are an output of their own
    assert margin.resolve(_args("--margin_sweep", "0,0.1", "--unlabeled", "true"))[0] == (0.0, 0.1)
    assert margin.resolve(_args("--margin_min", "0.1", "--margin_label_dir", "d", "--unlabeled", "true"))[1]["label_dir"] == "d"
    for argv, ragged, word in ((("--margin_sweep", "0,0.1", "--api_path", "true"), None, "--margin_sweep runs on the batched loop"),
                               (("--margin_min", "0.1", "--api_path", "true"), None, "--margin_min runs on the batched loop"),
                               (("--margin_sweep", "0,0.1"), False, "--margin_sweep runs behind the ragged step"),
                               (("--margin_min", "0.1"), False, "--margin_min runs behind the ragged step"),
                               (("--margin_label_dir", "d"), None, "--margin_label_dir needs --margin_min"),
                               (("--margin_sweep", "0.1,0.1"), None, "strictly increasing"),
                               (("--margin_sweep", "0,x"), None, "'x' is not a number"),
                               (("--margin_sweep", "-1"), None, ">= 0"),
                               (("--margin_min", "-0.5"), None, "--margin_min: margin_min: value -0.5"),
                               (("--margin_min", "nan"), None, "--margin_min"),
                               (("--margin_min", "0.1", "--unlabeled", "true"), None, "give --margin_label_dir")):
        with pytest.raises(ValueError, match=word):
            margin.resolve(_args(*argv), ragged=ragged)


def test_table_and_json():
    planes, sizes = _pack([HAND])
    gt = np.uint8([0, 1, 1, 0, 255, 2])
    thr = (0.0, 0.25, 0.5, 1.0)
    totals, kept, _, _ = margin.margin_reference(planes, sizes, 3, thr, gts=gt, num_classes=3)
    cover = margin.coverage_from_kept(kept)
    assert cover == [1.0, 4 / 6, 0.5, 1 / 6]
    assert all(math.isnan(c) for c in margin.coverage_from_kept([0, 0, 0]))
    scores = bkg_sweep.scores_from_totals(totals)
    assert scores[0]["pAcc"] == 4 / 5 and scores[1]["pAcc"] == 3 / 4
    table = margin.format_margin_table(thr, kept, scores, ["background", "a", "b"])
    lines = table.splitlines()
    assert len(lines) == 4 + len(thr) and len({len(x) for x in lines}) == 1
    assert [c.strip() for c in lines[1].strip("|").split("|")] == ["margin >=", "coverage %", "pAcc", "mIoU", "IoU background", "mIoU foreground"]
    assert [c.strip() for c in lines[4].strip("|").split("|")][:3] == ["0.25", "66.667", "75.000"]
    bare = margin.format_margin_table(thr, kept)
    assert [c.strip() for c in bare.splitlines()[1].strip("|").split("|")] == ["margin >=", "coverage %"]
    assert [c.strip() for c in bare.splitlines()[6].strip("|").split("|")] == ["1", "16.667"] and "pAcc" not in bare
    block = margin.margin_json(thr, kept, scores)
    assert list(block) == ["thresholds", "coverage", "miou", "pacc"] and block["thresholds"] == list(thr) and block["coverage"] == cover
    assert block["pacc"][:2] == [0.8, 0.75] and block["miou"][0] == scores[0]["miou"]
    assert block["miou"][3] == 0.0 and block["pacc"][3] == 0.0
    assert margin.margin_json(thr, kept) == {"thresholds": list(thr), "coverage": cover}
    assert margin.margin_json((0.5,), [0, 0]) == {"thresholds": [0.5], "coverage": [None]}
    assert margin.margin_min_json(0.25) == {"margin_min": 0.25}
    assert margin.margin_min_json(0.25, scores[1], 0.8) == {"margin_min": 0.25, "miou": scores[1]["miou"], "pAcc": 0.75, "coverage": 0.8}
    with pytest.raises(ValueError, match="one coverage and one score per threshold"):
        margin.format_margin_table(thr[:2], kept)
