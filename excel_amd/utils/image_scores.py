"""--per_image_scores: the table of every image's own scores, shared by infer_lam, infer_seg_voc, infer_seg_coco and eval_labels.

The programs score batches on the device into one confusion matrix; ops.image_scores keeps what each image contributed (ground-truth
area, predicted area and intersection per class) and a ScoreTicket (pipeline.py) brings it to the host behind an event.  This module is
the host side: it collects (data-set index, name, H, W, counts) per set of labels the program scores - "main", "crf", "conf" -, merges
the ranks' shards with one all_gather_object, and on rank 0 writes

    PATH          a CSV in data-set order: name,height,width,scored,pacc,miou,present,iou_<class>...  for the main set, then
                  <set>_pacc,<set>_miou,<set>_scored for every further set;  `present` = the ground-truth classes, |-joined
    PATH + .npz   names, hw [N,2], counts_<set> int64 [N,3,nc] for every set: anything can be recomputed from it

and logs the image-averaged mIoU and the K images with the lowest mIoU (an image without a scored pixel has no mIoU: it is left out
of the ranking and counted).  No GPU code here; numpy only, torch.distributed only when the run has more than one rank.
"""
import csv
import logging
import os
from collections import deque

import numpy as np

from .evaluate import image_score_rows

SETS = ("main", "crf", "conf")


def add_flags(parser):
    parser.add_argument("--per_image_scores", default=None, type=str,
                        help="write every image's own scores to this CSV (and PATH.npz with the raw per-class counts)")
    parser.add_argument("--per_image_worst", default=20, type=int, help="log the K images with the lowest mIoU (--per_image_scores)")


def refuse(args, unlabeled=False, test_split=False):
    """--per_image_scores where nothing is scored: a label-free run, a test split.  The refusal names the flag that excludes it."""
    if not getattr(args, "per_image_scores", None):
        return
    if unlabeled:
        raise ValueError("--per_image_scores needs ground truth: --unlabeled true scores nothing")
    if test_split:
        raise ValueError(f"--per_image_scores needs ground truth: --infer_set {getattr(args, 'infer_set', '?')} is a test split, which has none")
    if int(getattr(args, "per_image_worst", 0)) < 0:
        raise ValueError(f"--per_image_worst {args.per_image_worst} must not be negative")


def counts_numpy(gt, pred, num_classes):
    """What ops.image_scores computes for one image, in numpy: int64 [3,nc] over the pixels with gt < nc and pred < nc."""
    gt, pred = np.asarray(gt).reshape(-1).astype(np.int64), np.asarray(pred).reshape(-1).astype(np.int64)
    m = (gt < num_classes) & (pred < num_classes)
    g, p = gt[m], pred[m]
    return np.stack([np.bincount(g, minlength=num_classes), np.bincount(p, minlength=num_classes),
                     np.bincount(g[g == p], minlength=num_classes)]).astype(np.int64)


class ImageScoreLog:
    """The records of one rank: index -> (name, (H, W), {set: counts int64 [3,nc]}).  put() replaces what an earlier pass recorded for the
    same image and set (the overflow guard's exact-fp32 second pass); defer() takes a ticket and reads it when it is ready."""

    def __init__(self, num_classes, sets=("main",)):
        bad = [s for s in sets if s not in SETS]
        if bad or "main" not in sets:
            raise ValueError(f"image score sets {tuple(sets)}: 'main' plus any of {SETS[1:]}")
        self.nc, self.sets = int(num_classes), tuple(s for s in SETS if s in sets)
        self.records = {}
        self._pending = deque()

    def put(self, index, name, hw, which, counts):
        if which not in self.sets:
            raise ValueError(f"image scores: set {which!r} is not recorded by this run ({self.sets})")
        c = np.array(counts, np.int64)
        if c.shape != (3, self.nc):
            raise ValueError(f"image scores: counts of {name!r} are {c.shape}, expected (3, {self.nc})")
        rec = self.records.setdefault(int(index), (str(name), (int(hw[0]), int(hw[1])), {}))
        rec[2][which] = c

    def put_batch(self, indices, names, hws, which, counts):
        for b, (i, n, hw) in enumerate(zip(indices, names, hws)):
            self.put(i, n, hw, which, counts[b])

    def defer(self, ticket, indices, names, hws):
        """ticket.counts() -> {set: [B,3,nc]} is read once ticket.ready().  Never waits: poll(wait=True) after the loop does."""
        self._pending.append((ticket, [int(i) for i in indices], [str(n) for n in names], [tuple(int(x) for x in hw) for hw in hws]))
        self.poll(False)

    def poll(self, wait=False):
        while self._pending and (wait or self._pending[0][0].ready()):
            ticket, indices, names, hws = self._pending.popleft()
            for which, counts in ticket.counts().items():
                self.put_batch(indices, names, hws, which, np.asarray(counts))

    def merged(self, group=None):
        """Every rank's records in data-set order -> dict(index, names, hw, counts={set: int64 [N,3,nc]}), on every rank (one
        all_gather_object when the run has more than one rank).  An image without the counts of a recorded set is an error."""
        self.poll(True)
        parts = [self.records]
        try:
            import torch.distributed as dist
            world = dist.get_world_size(group) if dist.is_available() and dist.is_initialized() else 1
        except ImportError:
            world = 1
        if world > 1:
            parts = [None] * world
            dist.all_gather_object(parts, self.records, group=group)
        allrec = {}
        for p in parts:
            allrec.update(p)
        order = sorted(allrec)
        for i in order:
            missing = [s for s in self.sets if s not in allrec[i][2]]
            if missing:
                raise RuntimeError(f"image scores: {allrec[i][0]!r} has no counts for {missing}")
        return dict(index=np.asarray(order, np.int64), names=[allrec[i][0] for i in order],
                    hw=np.asarray([allrec[i][1] for i in order], np.int32).reshape(-1, 2),
                    counts={s: np.stack([allrec[i][2][s] for i in order]) if order else np.zeros((0, 3, self.nc), np.int64)
                            for s in self.sets})


def _fmt(v):
    return "nan" if np.isnan(v) else f"{float(v):.6f}"


def write_files(path, merged, class_names):
    """The CSV and the npz of one merged table (module docstring) -> the main set's image_score_rows."""
    nc = merged["counts"]["main"].shape[2]
    cats = [str(c) for c in class_names][:nc] + [f"class{i}" for i in range(len(class_names), nc)]
    rows = {s: image_score_rows(c) for s, c in merged["counts"].items()}
    main, extra = rows["main"], [s for s in merged["counts"] if s != "main"]
    d = os.path.dirname(os.path.abspath(path))
    os.makedirs(d, exist_ok=True)
    with open(path, "w", newline="") as f:
        w = csv.writer(f)
        w.writerow(["name", "height", "width", "scored", "pacc", "miou", "present"] + ["iou_" + c for c in cats]
                   + [f"{s}_{k}" for s in extra for k in ("pacc", "miou", "scored")])
        for i, name in enumerate(merged["names"]):
            present = "|".join(cats[c] for c in np.nonzero(merged["counts"]["main"][i, 0])[0])
            w.writerow([name, int(merged["hw"][i, 0]), int(merged["hw"][i, 1]), int(main["scored"][i]), _fmt(main["pacc"][i]),
                        _fmt(main["miou"][i]), present] + [_fmt(v) for v in main["iou"][i]]
                       + [x for s in extra for x in (_fmt(rows[s]["pacc"][i]), _fmt(rows[s]["miou"][i]), int(rows[s]["scored"][i]))])
    np.savez(path + ".npz", names=np.asarray(merged["names"], dtype=str), hw=merged["hw"],
             **{"counts_" + s: c.astype(np.int64) for s, c in merged["counts"].items()})
    return main


def worst_k(names, miou, k):
    """-> ([(name, miou)] of the k lowest, lowest first - ties in data-set order -, the number of NaN rows left out)"""
    miou = np.asarray(miou, np.float64)
    ok = np.nonzero(~np.isnan(miou))[0]
    order = ok[np.argsort(miou[ok], kind="stable")][:max(int(k), 0)]
    return [(names[i], float(miou[i])) for i in order], int(len(miou) - len(ok))


def report_lines(merged, rows, k, what="label_score"):
    worst, nan = worst_k(merged["names"], rows["miou"], k)
    n = len(merged["names"])
    with np.errstate(invalid="ignore"):
        mean = float(np.nanmean(rows["miou"])) if n > nan else float("nan")
    lines = [f"per-image {what}: image-averaged mIoU {mean * 100:.3f} over {n - nan} images"
             + (f" ({nan} without a scored pixel left out)" if nan else "")]
    lines += [f"  worst {j + 1:3d}: {name}  mIoU {v * 100:.3f}" for j, (name, v) in enumerate(worst)]
    return lines


def finish(log, args, class_names, rank=0, what="label_score", group=None):
    """After the loop, on every rank: merge, and on rank 0 write --per_image_scores' files and log the summary -> the merged table."""
    merged = log.merged(group)
    if rank == 0:
        rows = write_files(args.per_image_scores, merged, class_names)
        for line in report_lines(merged, rows, getattr(args, "per_image_worst", 20), what):
            logging.info(line)
        logging.info(f"per-image scores: {len(merged['names'])} rows -> {args.per_image_scores} (+ .npz)")
    return merged
