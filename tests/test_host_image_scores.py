"""--per_image_scores on the host: the score arithmetic against a direct numpy computation, the files, the worst-K ranking, the
refusals, eval_labels end to end on the CPU and the two-rank merge."""
import csv
import os
import socket

import numpy as np
import pytest

torch = pytest.importorskip("torch")

NC = 6


def _pairs(n_img, nc=NC, seed=0):
    """Random label pairs: image 1 is all-ignore, class nc - 1 is in neither map of any image"""
    rs = np.random.RandomState(seed)
    out = []
    for i in range(n_img):
        h, w = int(rs.randint(3, 12)), int(rs.randint(3, 12))
        gt = rs.randint(0, nc - 1, (h, w))
        pr = np.where(rs.rand(h, w) < 0.6, gt, rs.randint(0, nc - 1, (h, w)))
        gt = np.where(rs.rand(h, w) < 0.1, 255, gt)
        if i == 1:
            gt[:] = 255
        out.append((gt.astype(np.uint8), pr.astype(np.uint8)))
    return out


def _counts(pairs, nc=NC):
    from excel_amd.utils.image_scores import counts_numpy
    return np.stack([counts_numpy(g, p, nc) for g, p in pairs])


def test_image_score_rows_against_direct_numpy():
    from excel_amd.utils.evaluate import image_score_rows
    pairs = _pairs(7)
    rows = image_score_rows(_counts(pairs))
    for i, (gt, pr) in enumerate(pairs):
        m = gt < NC
        iou, present = [], []
        for c in range(NC):
            union = int((((gt == c) | (pr == c)) & m).sum())
            inter = int(((gt == c) & (pr == c) & m).sum())
            iou.append(inter / union if union else float("nan"))
            present.append(bool(((gt == c) & m).any()))
        assert np.allclose(rows["iou"][i], iou, rtol=0, atol=1e-15, equal_nan=True)
        assert rows["scored"][i] == int(m.sum())
        if m.any():
            assert rows["miou"][i] == pytest.approx(np.mean([v for v, p in zip(iou, present) if p]), abs=1e-15)
            assert rows["pacc"][i] == pytest.approx(((gt == pr) & m).sum() / m.sum(), abs=1e-15)
        else:
            assert np.isnan(rows["miou"][i]) and np.isnan(rows["pacc"][i])
    assert np.isnan(rows["miou"][1]) and rows["scored"][1] == 0, "the all-ignore image"
    assert np.isnan(rows["iou"][:, NC - 1]).all(), "a class absent from both maps has no IoU"
    with pytest.raises(ValueError, match=r"\[N,3,nc\]"):
        image_score_rows(np.zeros((3, NC)))


def test_image_miou_agrees_with_scores_from_hist_on_one_image():
    from excel_amd.tools.eval_labels import _hist_numpy
    from excel_amd.utils.evaluate import image_score_rows, scores_from_hist
    pairs = _pairs(4, seed=3)
    rows = image_score_rows(_counts(pairs))
    for i in (0, 2, 3):
        s = scores_from_hist(_hist_numpy(pairs[i][0].reshape(-1), pairs[i][1].reshape(-1), NC))
        assert rows["miou"][i] == pytest.approx(s["miou"], abs=1e-15) and rows["pacc"][i] == pytest.approx(s["pAcc"], abs=1e-15)


def test_hist_margins_against_bincount_matrices():
    from excel_amd.tools.eval_labels import _hist_numpy
    from excel_amd.utils.evaluate import hist_margins
    pairs = _pairs(9, seed=5)
    hist = sum(_hist_numpy(g.reshape(-1), p.reshape(-1), NC) for g, p in pairs)
    rows, cols, diag = hist_margins(_counts(pairs))
    assert rows.dtype == np.int64
    assert np.array_equal(rows, hist.sum(1)) and np.array_equal(cols, hist.sum(0)) and np.array_equal(diag, np.diagonal(hist))


def _log(pairs, order, sets=("main",)):
    from excel_amd.utils.image_scores import ImageScoreLog, counts_numpy
    log = ImageScoreLog(NC, sets)
    for i in order:
        for s in sets:
            log.put(i, f"img{i:02d}", pairs[i][0].shape, s, counts_numpy(pairs[i][0], pairs[i][1] if s == "main" else pairs[i][0], NC))
    return log


def test_csv_and_npz_round_trip_in_dataset_order(tmp_path):
    from excel_amd.utils import image_scores
    from excel_amd.utils.evaluate import image_score_rows
    pairs = _pairs(6, seed=8)
    log = _log(pairs, [4, 0, 5, 2, 1, 3], sets=("main", "crf"))
    merged = log.merged()
    assert merged["names"] == [f"img{i:02d}" for i in range(6)] and merged["index"].tolist() == list(range(6))
    path = str(tmp_path / "sub" / "scores.csv")
    cats = ["background", "a", "b", "c", "d", "e"]
    image_scores.write_files(path, merged, cats)
    z = np.load(path + ".npz")
    assert sorted(z.files) == ["counts_crf", "counts_main", "hw", "names"]
    assert z["counts_main"].dtype == np.int64 and z["counts_main"].shape == (6, 3, NC)
    assert np.array_equal(z["counts_main"], _counts(pairs)) and list(z["names"]) == merged["names"]
    assert np.array_equal(z["hw"], [p[0].shape for p in pairs])
    with open(path, newline="") as f:
        rows = list(csv.reader(f))
    assert rows[0] == ["name", "height", "width", "scored", "pacc", "miou", "present"] + ["iou_" + c for c in cats] + ["crf_pacc", "crf_miou", "crf_scored"]
    ref = image_score_rows(z["counts_main"])
    for i, r in enumerate(rows[1:]):
        assert r[0] == f"img{i:02d}" and (int(r[1]), int(r[2])) == pairs[i][0].shape and int(r[3]) == ref["scored"][i]
        assert np.allclose(float(r[5]), ref["miou"][i], atol=1e-6, equal_nan=True)
        assert r[6] == "|".join(cats[c] for c in range(NC) if z["counts_main"][i, 0, c])
        assert np.allclose([float(v) for v in r[7:7 + NC]], ref["iou"][i], atol=1e-6, equal_nan=True)
        assert int(r[-1]) == ref["scored"][i]                 # the crf set here is gt against gt: the same pixels, all correct
        assert r[-3] == ("nan" if i == 1 else "1.000000")
    assert rows[2][4:7] == ["nan", "nan", ""], "the all-ignore image: no scores, no present class"


def test_a_later_row_replaces_an_earlier_one_and_a_missing_set_is_an_error():
    from excel_amd.utils.image_scores import ImageScoreLog
    log = ImageScoreLog(NC, ("main", "conf"))
    log.put(3, "x", (2, 2), "main", np.zeros((3, NC)))
    log.put(3, "x", (2, 2), "main", np.ones((3, NC)))
    with pytest.raises(RuntimeError, match="'x' has no counts for \\['conf'\\]"):
        log.merged()
    log.put(3, "x", (2, 2), "conf", np.zeros((3, NC)))
    assert log.merged()["counts"]["main"].sum() == 3 * NC
    with pytest.raises(ValueError, match="not recorded"):
        log.put(3, "x", (2, 2), "crf", np.zeros((3, NC)))
    with pytest.raises(ValueError, match="expected"):
        log.put(3, "x", (2, 2), "main", np.zeros((3, NC + 1)))


class _Ticket:
    def __init__(self, counts, is_ready):
        self._c, self._r, self.waited = counts, is_ready, False

    def ready(self):
        return self._r

    def counts(self):
        self.waited = True
        return self._c


def test_deferred_tickets_are_read_when_ready_and_never_waited_for_in_the_loop():
    from excel_amd.utils.image_scores import ImageScoreLog
    log = ImageScoreLog(NC, ("main", "crf"))
    a = _Ticket({"main": np.ones((2, 3, NC), np.int32)}, False)
    b = _Ticket({"crf": np.full((2, 3, NC), 2, np.int32)}, True)
    log.defer(a, [0, 1], ["p", "q"], [(1, 1), (2, 2)])
    log.defer(b, [0, 1], ["p", "q"], [(1, 1), (2, 2)])
    assert not a.waited and not b.waited and not log.records, "the oldest ticket is not ready: nothing is read, nobody waits"
    a._r = True
    log.poll(False)
    assert a.waited and b.waited
    m = log.merged()
    assert m["counts"]["main"].sum() == 2 * 3 * NC and m["counts"]["crf"].sum() == 2 * 2 * 3 * NC


def test_worst_k_leaves_nan_rows_out_and_counts_them():
    from excel_amd.utils import image_scores
    names = list("abcdef")
    miou = np.array([0.5, np.nan, 0.1, 0.5, np.nan, 0.9])
    worst, nan = image_scores.worst_k(names, miou, 3)
    assert worst == [("c", 0.1), ("a", 0.5), ("d", 0.5)] and nan == 2
    assert image_scores.worst_k(names, miou, 20)[0][-1] == ("f", 0.9) and len(image_scores.worst_k(names, miou, 20)[0]) == 4
    assert image_scores.worst_k(names, miou, 0) == ([], 2)
    lines = image_scores.report_lines(dict(names=names), dict(miou=miou), 2)
    assert "image-averaged mIoU 50.000 over 4 images" in lines[0] and "2 without a scored pixel" in lines[0] and len(lines) == 3
    assert "nan" in image_scores.report_lines(dict(names=["a"]), dict(miou=np.array([np.nan])), 5)[0]


def test_refusals_unlabeled_and_test_splits(tmp_path):
    from excel_amd.tools import eval_labels, infer_lam, infer_seg_coco, infer_seg_voc
    out = str(tmp_path / "s.csv")
    for prog in (infer_lam, infer_seg_voc, infer_seg_coco, eval_labels):
        extra = ["--pred_dir", "x", "--data_folder", "x", "--list_folder", "x"] if prog is eval_labels else []
        a = prog.get_parser().parse_args(extra + ["--per_image_scores", out])
        assert a.per_image_scores == out and a.per_image_worst == 20
        assert prog.get_parser().parse_args(extra).per_image_scores is None
    with pytest.raises(ValueError, match="--per_image_scores needs ground truth: --unlabeled true"):
        infer_lam.validate(infer_lam.get_parser().parse_args(["--unlabeled", "true", "--data_folder", str(tmp_path), "--per_image_scores", out,
                                                              "--save_label", "true"]))
    with pytest.raises(ValueError, match="--per_image_scores needs ground truth: --infer_set test is a test split"):
        infer_seg_voc.validate(infer_seg_voc.get_parser().parse_args(["--infer_set", "test", "--test_data_folder", str(tmp_path),
                                                                      "--per_image_scores", out]))
    with pytest.raises(ValueError, match="must not be negative"):
        infer_seg_voc.validate(infer_seg_voc.get_parser().parse_args(["--per_image_scores", out, "--per_image_worst", "-1"]))
    assert not os.path.exists(out)


def test_pipelines_take_the_flag_and_the_side_stream_paths_refuse_it():
    import inspect
    from excel_amd import pipeline
    for cls in (pipeline.TrainingFreePipeline, pipeline.OptimisedLamPipeline, pipeline.ValidationPipeline):
        assert inspect.signature(cls.__init__).parameters["image_scores"].default is False
    p = pipeline.TrainingFreePipeline(model=None, image_scores=True)
    assert p.image_scores and p.last_score_ticket is None
    for name in ("run_batch_split", "run_batch_overlapped"):
        with pytest.raises(ValueError, match="no per-image scores"):
            getattr(p, name)(None, None)
    assert pipeline.TrainingFreePipeline(model=None).image_scores is False


def test_ops_image_scores_takes_no_workspace():
    import inspect
    import re
    from excel_amd import ops
    assert list(inspect.signature(ops.image_scores).parameters) == ["gt_u8", "pred_u8", "num_classes", "skip", "plan", "out"]
    assert not re.search(r"_ws\(|workspace", inspect.getsource(ops.image_scores))


def test_eval_labels_on_the_cpu_writes_the_table(tmp_path, monkeypatch):
    """eval_labels without a GPU (the numpy path): the npz holds the counts of every listed image in list order, whatever the batch
    size, and their margins are the program's own matrix."""
    from PIL import Image
    from excel_amd.tools import eval_labels, synthetic
    from excel_amd.utils.evaluate import hist_margins
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    root, lists, pred = tmp_path / "VOC2012", tmp_path / "lists", tmp_path / "pred"
    ids, _ = synthetic.write_voc_tree(str(root), str(lists), 5, seed=2, split="val")
    os.makedirs(pred)
    rs = np.random.RandomState(0)
    want = []
    for n in ids:
        gt = np.asarray(Image.open(root / "SegmentationClassAug" / (n + ".png")))
        pr = np.where(rs.rand(*gt.shape) < 0.7, np.where(gt == 255, 0, gt), rs.randint(0, 21, gt.shape)).astype(np.uint8)
        Image.fromarray(pr).save(pred / (n + ".png"))
        want.append((gt, pr))
    out = str(tmp_path / "scores.csv")
    res = eval_labels.validate(eval_labels.get_parser().parse_args(
        ["--pred_dir", str(pred), "--data_folder", str(root), "--list_folder", str(lists), "--infer_set", "val", "--num_workers", "2",
         "--batch_size", "2", "--per_image_scores", out, "--per_image_worst", "2"]))
    z = np.load(out + ".npz")
    assert list(z["names"]) == ids and np.array_equal(z["hw"], [g.shape for g, _ in want])
    assert np.array_equal(z["counts_main"], _counts(want, 21))
    rows, cols, diag = hist_margins(z["counts_main"])
    h = res["hist"].numpy()
    assert np.array_equal(rows, h.sum(1)) and np.array_equal(cols, h.sum(0)) and np.array_equal(diag, np.diagonal(h))
    with open(out, newline="") as f:
        assert [r[0] for r in csv.reader(f)][1:] == ids
    plain = eval_labels.validate(eval_labels.get_parser().parse_args(
        ["--pred_dir", str(pred), "--data_folder", str(root), "--list_folder", str(lists), "--infer_set", "val", "--num_workers", "2"]))
    assert np.array_equal(plain["hist"].numpy(), h) and "image_scores" not in plain


# ------------------------------------------------------------------ world_size 2 on gloo
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _worker(rank, world, port, n, path, q):
    import argparse
    import torch.distributed as dist
    from excel_amd.tools.infer_lam import shard_indices
    from excel_amd.utils import image_scores
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    pairs = _pairs(n, seed=21)
    log = _log(pairs, [int(i) for i in shard_indices(n, rank, world)][::-1])
    merged = image_scores.finish(log, argparse.Namespace(per_image_scores=path, per_image_worst=3), [f"c{i}" for i in range(NC)], rank)
    q.put((rank, merged["names"], merged["counts"]["main"]))
    dist.barrier()
    dist.destroy_process_group()


def test_world2_merge_of_interleaved_shards_with_an_uneven_tail(tmp_path):
    import torch.multiprocessing as mp
    n, world = 7, 2                                           # rank 0: 0 2 4 6, rank 1: 1 3 5
    path = str(tmp_path / "scores.csv")
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, world, port, n, path, q)) for r in range(world)]
    for p in procs:
        p.start()
    res = [q.get(timeout=120) for _ in range(world)]
    for p in procs:
        p.join(60)
        assert p.exitcode == 0
    want = _counts(_pairs(n, seed=21))
    for _, names, counts in res:
        assert names == [f"img{i:02d}" for i in range(n)] and np.array_equal(counts, want)
    z = np.load(path + ".npz")
    assert list(z["names"]) == [f"img{i:02d}" for i in range(n)] and np.array_equal(z["counts_main"], want)
    with open(path, newline="") as f:
        assert [r[0] for r in csv.reader(f)][1:] == [f"img{i:02d}" for i in range(n)]
