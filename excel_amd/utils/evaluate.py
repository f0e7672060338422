"""scores / _fast_hist - mirror of utils/evaluate.py:9-50 with the histogram on the device."""
import numpy as np
import torch

from .. import ops


def hist_from_labels(label_trues, label_preds, num_classes=21, device="cuda", hist=None):
    """Accumulate the [nc,nc] int64 confusion matrix on the GPU (evaluate.py:9-20)."""
    for lt, lp in zip(label_trues, label_preds):
        lt = torch.as_tensor(np.asarray(lt) if not torch.is_tensor(lt) else lt)
        lp = torch.as_tensor(np.asarray(lp) if not torch.is_tensor(lp) else lp)
        # labels are small non-negative ints, 255 = ignore; uint8 is lossless for them
        gt = lt.to(device=device).to(torch.uint8)
        pr = lp.to(device=device).to(torch.uint8)
        hist = ops.confusion_accumulate(gt, pr, num_classes, hist)
    return hist


def scores_from_hist(hist):
    """The metric arithmetic of evaluate.py:21-50 on a 21x21 (81x81) matrix - host-side float64 like the reference."""
    hist = np.asarray(hist.detach().cpu().numpy() if torch.is_tensor(hist) else hist, np.float64)
    n = hist.shape[0]
    with np.errstate(divide="ignore", invalid="ignore"):
        acc = np.diag(hist).sum() / hist.sum()
        acc_cls = np.nanmean(np.diag(hist) / hist.sum(axis=1))
        iu = np.diag(hist) / (hist.sum(axis=1) + hist.sum(axis=0) - np.diag(hist))
        valid = hist.sum(axis=1) > 0
        mean_iu = np.nanmean(iu[valid])
        TP = np.diag(hist)
        FN = hist.sum(axis=1) - TP
        FP = hist.sum(axis=0) - TP
        cr = FP / TP
        precision = TP / (TP + FP)
        recall = TP / (TP + FN)
    return {"pAcc": acc, "mAcc": acc_cls, "miou": mean_iu, "iou": dict(zip(range(n), iu)),
            "confusion": dict(zip(range(n), cr)), "precision": dict(zip(range(n), precision)),
            "recall": dict(zip(range(n), recall))}


def scores(label_trues, label_preds, num_classes=21):
    return scores_from_hist(hist_from_labels(label_trues, label_preds, num_classes))


def image_score_rows(counts):
    """The scores of every image on its own, from ops.image_scores' counts: int [N,3,nc] = per image and class (ground-truth area,
    predicted area, intersection) -> {"iou" [N,nc], "miou" [N], "pacc" [N], "scored" [N]} - host-side float64 like scores_from_hist.
      iou    = inter / (gt + pred - inter), NaN where the union is 0 (the class is in neither map);
      miou   = the mean of iou over the classes with gt area > 0 (the `valid` rule of scores_from_hist); NaN for an image without a
               scored pixel;
      pacc   = sum inter / sum gt area (NaN likewise);   scored = sum gt area, the number of pixels that counted (int64)."""
    c = np.asarray(counts)
    if c.ndim != 3 or c.shape[1] != 3:
        raise ValueError(f"image_score_rows: counts must be [N,3,nc], got {c.shape}")
    c = c.astype(np.float64)
    gt, pred, inter = c[:, 0], c[:, 1], c[:, 2]
    valid = gt > 0
    with np.errstate(divide="ignore", invalid="ignore"):
        iou = inter / (gt + pred - inter)
        miou = np.where(valid, iou, 0.0).sum(1) / valid.sum(1)
        pacc = inter.sum(1) / gt.sum(1)
    return {"iou": iou, "miou": miou, "pacc": pacc, "scored": np.asarray(counts)[:, 0].astype(np.int64).sum(1)}


def hist_margins(counts):
    """counts int [N,3,nc] -> (row sums, column sums, diagonal) int64 [nc] each, summed over the images: what the confusion matrix of
    the same pixels must show (hist.sum(1), hist.sum(0), hist.diagonal())."""
    c = np.asarray(counts).astype(np.int64)
    if c.ndim != 3 or c.shape[1] != 3:
        raise ValueError(f"hist_margins: counts must be [N,3,nc], got {c.shape}")
    s = c.sum(0)
    return s[0], s[1], s[2]


def boundary_scores_from_counts(counts):
    """Data-set Boundary IoU from ops.boundary_scores' counts: int [N,3,nc] = per image and class (ground-truth band, predicted band,
    their intersection).  Radii differ per image, so the COUNTS are summed over the images and image_score_rows' formula is applied to
    the sum -> {"biou" [nc] (NaN for a class with no band pixel in either map), "mbiou" (the mean over the classes with a ground-truth
    band; NaN without one), "band_pixels" [nc] int64 (the summed ground-truth band)}."""
    c = np.asarray(counts)
    if c.ndim != 3 or c.shape[1] != 3:
        raise ValueError(f"boundary_scores_from_counts: counts must be [N,3,nc], got {c.shape}")
    s = c.astype(np.int64).sum(0)
    rows = image_score_rows(s[None])
    return {"biou": rows["iou"][0], "mbiou": float(rows["miou"][0]), "band_pixels": s[0]}


def multilabel_score(y_true, y_pred):
    """utils/evaluate.py:4-6 (sklearn.metrics.f1_score on one binary row) in numpy: 2 TP / (2 TP + FP + FN), 0 where that denominator
    is 0 (sklearn's zero_division default returns 0 there too)."""
    t, p = np.asarray(y_true).reshape(-1) != 0, np.asarray(y_pred).reshape(-1) != 0
    tp, fp, fn = int((t & p).sum()), int((~t & p).sum()), int((t & ~p).sum())
    den = 2 * tp + fp + fn
    return 2.0 * tp / den if den else 0.0


def tag_scores(counts):
    """Predicted image tags against the image-level labels: counts int64 [F,3] = per class (TP, FP, FN) over the images ->
    {"precision", "recall", "f1": {class: value}, "micro": {"precision", "recall", "f1"}, "tp", "fp", "fn"} - a ratio whose denominator
    is 0 is 0 (a class nobody has and nobody predicted scores 0, like multilabel_score)."""
    c = np.asarray(counts, np.float64).reshape(-1, 3)

    def prf(tp, fp, fn):
        with np.errstate(divide="ignore", invalid="ignore"):
            p = np.where(tp + fp > 0, tp / (tp + fp), 0.0)
            r = np.where(tp + fn > 0, tp / (tp + fn), 0.0)
            f = np.where(2 * tp + fp + fn > 0, 2 * tp / (2 * tp + fp + fn), 0.0)
        return p, r, f
    p, r, f = prf(c[:, 0], c[:, 1], c[:, 2])
    mp, mr, mf = prf(c[:, 0].sum(), c[:, 1].sum(), c[:, 2].sum())
    n = c.shape[0]
    return {"precision": dict(zip(range(n), p)), "recall": dict(zip(range(n), r)), "f1": dict(zip(range(n), f)),
            "micro": {"precision": float(mp), "recall": float(mr), "f1": float(mf)},
            "tp": int(c[:, 0].sum()), "fp": int(c[:, 1].sum()), "fn": int(c[:, 2].sum())}
