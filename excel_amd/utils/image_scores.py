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

--boundary_scores true (with or without --per_image_scores): every set also gets its Boundary IoU counts (ops.boundary_scores; Cheng et
al., CVPR 2021) - the same [3,nc] rows restricted to the band within `radius` pixels of each map's own contours, radius =
boundary_radius(H, W): 2 % of the image diagonal unless --boundary_px fixes it.  They travel in the same tickets under "<set>_bd", the
log gets a boundary_score table per set (Boundary IoU per class from the SUMMED counts, the mean, the ground-truth band pixels), and
the files, when written, gain `radius`, `biou` and `<set>_biou` columns and `radius`, `bcounts_<set>` arrays.  Without the flag nothing
here changes: same columns, same bytes.

--clean_min_region (infer_lam; utils/components.py): the cleaned labels are one more set, "clean", and every image also has a row
(regions, regions removed, pixels removed) of the filter: the files gain `clean_pacc, clean_miou, clean_scored` and, last, `regions,
regions_removed, pixels_removed`, the npz `counts_clean` and `regions`.  Without the flag, again, nothing changes.

--fill_ignore (infer_lam; utils/label_fill.py): the filled labels are one more set, "fill", by the same route, and every image has a row
(holes, holes filled, largest squared distance) of the fill: the files gain `fill_pacc, fill_miou, fill_scored` and, last of all, `holes,
filled, max_fill_dist` (the distance in pixels), the npz `counts_fill` and `fills` (the raw rows).  Without the flag nothing changes.

--snap_superpixels (infer_lam; utils/superpixels.py): the snapped labels are one more set, "snap", by the same route, and every image has
a row (superpixels with a vote, superpixels snapped, pixels changed) of the vote: the files gain `snap_pacc, snap_miou, snap_scored` and,
last of all, `superpixels, snapped, pixels_changed`, the npz `counts_snap` and `snaps`.  Without the flag nothing changes.
--margin_min (infer_lam; utils/margin.py): the labels cut at an arg-max margin are one more set, "margin": the files gain `margin_pacc,
margin_miou, margin_scored` (and `margin_biou` with --boundary_scores), the npz `counts_margin`.  Without the flag nothing changes.
"""
import csv
import logging
import os
from collections import deque
from types import SimpleNamespace

import numpy as np

from .evaluate import boundary_scores_from_counts, image_score_rows
from .label_stages import ROW_SETS

SETS = ("main", "crf", "conf", "clean", "fill", "snap", "margin")
MAX_RADIUS = 72              # what ops.boundary_max_radius() answers (boundary.hip's halo); the CPU path refuses the same radii


def add_flags(parser):
    parser.add_argument("--per_image_scores", default=None, type=str,
                        help="write every image's own scores to this CSV (and PATH.npz with the raw per-class counts)")
    parser.add_argument("--per_image_worst", default=20, type=int, help="log the K images with the lowest mIoU (--per_image_scores)")


def _bool(v):
    if isinstance(v, bool):
        return v
    if str(v).lower() in ("true", "1", "yes"):
        return True
    if str(v).lower() in ("false", "0", "no"):
        return False
    raise ValueError(f"expected true or false, got {v!r}")


def add_boundary_flags(parser):
    parser.add_argument("--boundary_scores", default=False, type=_bool,
                        help="also score Boundary IoU (the IoU inside the band around each map's contours) for every scored set of labels")
    parser.add_argument("--boundary_ratio", default=0.02, type=float, help="band radius as a fraction of the image diagonal (--boundary_scores)")
    parser.add_argument("--boundary_px", default=0, type=int, help="a fixed band radius in pixels instead of --boundary_ratio (0: off)")


def boundary_radius(h, w, ratio=0.02, px=0):
    """The band radius of an H x W image, on the host: px when given, else max(1, round(ratio * diagonal)) with Python's round (ties
    to even: 75 x 100 -> 2.5 -> 2), as the original implementation computes it."""
    if int(px) > 0:
        return int(px)
    return max(1, int(round(float(ratio) * float(np.sqrt(int(h) * int(h) + int(w) * int(w))))))


def checked_radius(name, h, w, boundary):
    """boundary_radius of one named image, refused beyond MAX_RADIUS (what ops.boundary_scores refuses on the device path)."""
    d = boundary_radius(h, w, **boundary)
    if d > MAX_RADIUS:
        raise ValueError(f"--boundary_scores: {name!r} ({int(h)} x {int(w)}) has radius {d}, beyond the largest this build accepts ({MAX_RADIUS})")
    return d


def boundary_of(args):
    """--boundary_scores -> dict(ratio=, px=) for the pipelines and tickets, or None when the flag is off.  Refused: a ratio outside
    (0, 1], a negative px."""
    if not getattr(args, "boundary_scores", False):
        return None
    ratio, px = float(getattr(args, "boundary_ratio", 0.02)), int(getattr(args, "boundary_px", 0))
    if not 0.0 < ratio <= 1.0:
        raise ValueError(f"--boundary_ratio {ratio} must be in (0, 1]")
    if px < 0:
        raise ValueError(f"--boundary_px {px} must not be negative")
    if px > MAX_RADIUS:
        raise ValueError(f"--boundary_px {px} is beyond the largest radius this build accepts ({MAX_RADIUS})")
    return dict(ratio=ratio, px=px)


def check_boundary(boundary):
    """boundary = None | dict(ratio=, px=) as the pipelines and ScoreTicket.launch take it -> the complete dict, or None."""
    if boundary is None:
        return None
    bad = set(boundary) - {"ratio", "px"}
    if bad:
        raise ValueError(f"boundary: unknown keys {sorted(bad)} (ratio, px)")
    return boundary_of(SimpleNamespace(boundary_scores=True, boundary_ratio=boundary.get("ratio", 0.02), boundary_px=boundary.get("px", 0)))


def wanted(args):
    """The run collects per-image counts: for --per_image_scores' files, for --boundary_scores' tables, or both."""
    return bool(getattr(args, "per_image_scores", None)) or bool(getattr(args, "boundary_scores", False))


def refuse(args, unlabeled=False, test_split=False):
    """--per_image_scores / --boundary_scores where nothing is scored: a label-free run, a test split.  The refusal names the flag that
    excludes it."""
    if boundary_of(args) is not None:
        if unlabeled:
            raise ValueError("--boundary_scores needs ground truth: --unlabeled true scores nothing")
        if test_split:
            raise ValueError(f"--boundary_scores needs ground truth: --infer_set {getattr(args, 'infer_set', '?')} is a test split, which has none")
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


def boundary_counts_numpy(gt, pred, num_classes, d):
    """What ops.boundary_scores computes for one [H,W] image, in numpy: int64 [3,nc].  A pixel is in the band of a map iff the minimum
    and the maximum of its (2d+1) x (2d+1) window differ, the map padded with -1 (a position outside the image is `different`)."""
    gt, pred = np.asarray(gt), np.asarray(pred)
    if gt.ndim != 2 or gt.shape != pred.shape:
        raise ValueError(f"boundary_counts_numpy: need two [H,W] maps of one size (got {gt.shape}, {pred.shape})")
    d = int(d)
    if d < 1:
        raise ValueError(f"boundary_counts_numpy: radius {d} < 1")
    H, W = gt.shape

    def band(m):
        lo = np.pad(m.astype(np.int16), min(d, max(H, W)), constant_values=-1)      # a halo beyond the image's size changes nothing
        r = (lo.shape[0] - H) // 2
        hi = lo
        for axis in (0, 1):
            n = lo.shape[axis] - 2 * r
            sl = lambda a, k: a[k:k + n] if axis == 0 else a[:, k:k + n]
            lo2, hi2 = sl(lo, 0), sl(hi, 0)
            for k in range(1, 2 * r + 1):
                lo2, hi2 = np.minimum(lo2, sl(lo, k)), np.maximum(hi2, sl(hi, k))
            lo, hi = lo2, hi2
        return lo != hi

    g, p = gt.astype(np.int64), pred.astype(np.int64)
    valid = (g < num_classes) & (p < num_classes)
    eg, ep = band(gt) & valid, band(pred) & valid
    return np.stack([np.bincount(g[eg], minlength=num_classes), np.bincount(p[ep], minlength=num_classes),
                     np.bincount(g[eg & ep & (g == p)], minlength=num_classes)]).astype(np.int64)


class ImageScoreLog:
    """The records of one rank: index -> (name, (H, W), {set: counts int64 [3,nc]}).  put() replaces what an earlier pass recorded for the
    same image and set (the overflow guard's exact-fp32 second pass); defer() takes a ticket and reads it when it is ready."""

    def __init__(self, num_classes, sets=("main",), boundary=None, rows=()):
        """boundary = None | dict(ratio=, px=): with it every set has a twin "<set>_bd" (ops.boundary_scores' counts) that is recorded
        and required like the set itself, and merged() adds the radius of every image.  rows = the keys of the row sets the run has
        (utils/label_stages.ROW_SETS: "regions" with --clean_min_region, "fills" with --fill_ignore, "snaps" with
        --snap_superpixels): every image also has a row of three counts of that stage, put_rows() records it."""
        self.rows = tuple(r.key for r in ROW_SETS if r.key in rows)
        bad = [s for s in sets if s not in SETS]
        if bad or "main" not in sets:
            raise ValueError(f"image score sets {tuple(sets)}: 'main' plus any of {SETS[1:]}")
        self.nc, self.sets = int(num_classes), tuple(s for s in SETS if s in sets)
        self.boundary = check_boundary(boundary)
        self.twins = tuple(s + "_bd" for s in self.sets) if self.boundary is not None else ()
        self.records = {}
        self._pending = deque()

    def put(self, index, name, hw, which, counts):
        if which not in self.sets and which not in self.twins:
            raise ValueError(f"image scores: set {which!r} is not recorded by this run ({self.sets})")
        c = np.array(counts, np.int64)
        if c.shape != (3, self.nc):
            raise ValueError(f"image scores: counts of {name!r} are {c.shape}, expected (3, {self.nc})")
        rec = self.records.setdefault(int(index), (str(name), (int(hw[0]), int(hw[1])), {}))
        rec[2][which] = c

    def put_rows(self, kind, indices, names, hws, counts):
        """counts [B,3]: the rows of one step for the row set `kind`; a later row of an image replaces the earlier one."""
        if kind not in self.rows:
            raise ValueError(f"image scores: row set {kind!r} is not recorded by this run ({self.rows})")
        for b, (i, n, hw) in enumerate(zip(indices, names, hws)):
            rec = self.records.setdefault(int(i), (str(n), (int(hw[0]), int(hw[1])), {}))
            rec[2][kind] = np.array(counts[b], np.int64).reshape(3)

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
            missing = [s for s in self.sets + self.twins + self.rows if s not in allrec[i][2]]
            if missing:
                raise RuntimeError(f"image scores: {allrec[i][0]!r} has no counts for {missing}")
        stack = lambda s: np.stack([allrec[i][2][s] for i in order]) if order else np.zeros((0, 3, self.nc), np.int64)
        out = dict(index=np.asarray(order, np.int64), names=[allrec[i][0] for i in order],
                   hw=np.asarray([allrec[i][1] for i in order], np.int32).reshape(-1, 2), counts={s: stack(s) for s in self.sets})
        if self.boundary is not None:                         # only then: a table without the flag has the keys it always had
            out["radius"] = np.asarray([boundary_radius(*allrec[i][1], **self.boundary) for i in order], np.int32)
            out["bcounts"] = {s: stack(s + "_bd") for s in self.sets}
        for k in self.rows:                                   # likewise
            out[k] = np.stack([allrec[i][2][k] for i in order]) if order else np.zeros((0, 3), np.int64)
        return out


def _fmt(v):
    return "nan" if np.isnan(v) else f"{float(v):.6f}"


def write_files(path, merged, class_names):
    """The CSV and the npz of one merged table (module docstring) -> the main set's image_score_rows.  A table with boundary counts
    (merged["bcounts"]) appends its columns and arrays; one without is written exactly as before."""
    nc = merged["counts"]["main"].shape[2]
    cats = [str(c) for c in class_names][:nc] + [f"class{i}" for i in range(len(class_names), nc)]
    rows = {s: image_score_rows(c) for s, c in merged["counts"].items()}
    main, extra = rows["main"], [s for s in merged["counts"] if s != "main"]
    brows = {s: image_score_rows(c) for s, c in merged.get("bcounts", {}).items()}
    bhead = ["radius", "biou"] + [f"{s}_biou" for s in extra] if brows else []
    stage_rows = [r for r in ROW_SETS if merged.get(r.key) is not None]
    d = os.path.dirname(os.path.abspath(path))
    os.makedirs(d, exist_ok=True)
    with open(path, "w", newline="") as f:
        w = csv.writer(f)
        w.writerow(["name", "height", "width", "scored", "pacc", "miou", "present"] + ["iou_" + c for c in cats]
                   + [f"{s}_{k}" for s in extra for k in ("pacc", "miou", "scored")] + bhead + [h for r in stage_rows for h in r.heads])
        for i, name in enumerate(merged["names"]):
            present = "|".join(cats[c] for c in np.nonzero(merged["counts"]["main"][i, 0])[0])
            w.writerow([name, int(merged["hw"][i, 0]), int(merged["hw"][i, 1]), int(main["scored"][i]), _fmt(main["pacc"][i]),
                        _fmt(main["miou"][i]), present] + [_fmt(v) for v in main["iou"][i]]
                       + [x for s in extra for x in (_fmt(rows[s]["pacc"][i]), _fmt(rows[s]["miou"][i]), int(rows[s]["scored"][i]))]
                       + ([int(merged["radius"][i]), _fmt(brows["main"]["miou"][i])] + [_fmt(brows[s]["miou"][i]) for s in extra]
                          if brows else [])
                       + [c for r in stage_rows for c in r.cells(merged[r.key][i], _fmt)])
    more = {}
    if brows:
        more = dict(radius=merged["radius"].astype(np.int32), **{"bcounts_" + s: c.astype(np.int64) for s, c in merged["bcounts"].items()})
    for r in stage_rows:
        more[r.key] = np.asarray(merged[r.key], np.int64)
    np.savez(path + ".npz", names=np.asarray(merged["names"], dtype=str), hw=merged["hw"],
             **{"counts_" + s: c.astype(np.int64) for s, c in merged["counts"].items()}, **more)
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


BOUNDARY_SET_NAMES = {"main": "labels", "conf": "confident labels", "crf": "CRF labels", "clean": "cleaned labels", "fill": "filled labels", "snap": "snapped labels", "margin": "margin labels"}


def boundary_summary(merged):
    """-> {set: evaluate.boundary_scores_from_counts of the set's summed counts}; {} for a table without boundary counts"""
    return {s: boundary_scores_from_counts(c) for s, c in merged.get("bcounts", {}).items()}


def boundary_table(score, class_names):
    """One set's boundary_score table: the class rows of the region table with Boundary IoU and the ground-truth band pixels."""
    nc = len(score["biou"])
    cats = [str(c) for c in class_names][:nc] + [f"class{i}" for i in range(len(class_names), nc)]
    width = max(len(c) for c in cats + ["mean"])
    lines = [f"{'class'.ljust(width)}  {'bIoU':>8}  {'band_pixels':>12}"]
    lines += [f"{c.ljust(width)}  {_fmt100(score['biou'][i]):>8}  {int(score['band_pixels'][i]):>12d}" for i, c in enumerate(cats)]
    lines.append(f"{'mean'.ljust(width)}  {_fmt100(score['mbiou']):>8}  {int(np.sum(score['band_pixels'])):>12d}")
    return "\n".join(lines)


def _fmt100(v):
    return "nan" if np.isnan(v) else f"{float(v) * 100:.3f}"


def boundary_json(merged, boundary):
    """The `boundary` block of a program's JSON record."""
    rad = merged["radius"]
    return {"ratio": boundary["ratio"], "px": boundary["px"], "radius_min": int(rad.min()) if len(rad) else None,
            "radius_max": int(rad.max()) if len(rad) else None,
            "sets": {s: {"mbiou": None if np.isnan(v["mbiou"]) else float(v["mbiou"]),
                         "biou": [None if np.isnan(x) else float(x) for x in v["biou"]],
                         "band_pixels": [int(x) for x in v["band_pixels"]]} for s, v in boundary_summary(merged).items()}}


def finish(log, args, class_names, rank=0, what="label_score", group=None):
    """After the loop, on every rank: merge, and on rank 0 write --per_image_scores' files (when that flag is given), log the summary
    and, with --boundary_scores, the boundary_score table of every set -> the merged table."""
    merged = log.merged(group)
    if rank == 0:
        if getattr(args, "per_image_scores", None):
            rows = write_files(args.per_image_scores, merged, class_names)
            for line in report_lines(merged, rows, getattr(args, "per_image_worst", 20), what):
                logging.info(line)
            logging.info(f"per-image scores: {len(merged['names'])} rows -> {args.per_image_scores} (+ .npz)")
        for s, score in boundary_summary(merged).items():
            logging.info(f"boundary_score of the {BOUNDARY_SET_NAMES[s]} ({what}; radius {int(merged['radius'].min()) if len(merged['radius']) else 0}"
                         f"..{int(merged['radius'].max()) if len(merged['radius']) else 0} px):")
            logging.info("\n" + boundary_table(score, class_names))
    return merged
