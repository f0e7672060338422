"""--bkg_sweep / --bkg_scale: score the pseudo labels over a range of background scales, and label at one of them.

The labels are the arg-max over [b0 ; cam_1 .. cam_k] of PAR's output, b0 = PAR(1 - max_c cam_c) (utils/affutils.py:161-174, where
the background is written torch.pow(1 - max, 1.)).  PAR is linear per channel, so the labels a background scaled by `a` would have
given are `a * b0 >= F` on the planes the step already has: excel_bkg_sweep_ragged (csrc/bkgsweep.hip) scores K scales in one pass
and / or writes the label map of one.  This module is its host side:

    check_scales / parse_scales   the scales of a sweep: 1..16 values, finite, > 0, strictly increasing
    sweep_ragged                  the ctypes binding (device tensors in, device tensors out, the caller's stream)
    sweep_reference               the same contract in numpy - float32 multiply and compare, so it is exact: the judge of the GPU tests
    scores_from_totals            int64 [K,3,nc] margins -> the dict of utils/evaluate.scores_from_hist, per scale
    format_sweep_table, best_scale, sweep_json   what tools/infer_lam reports;  add_flags, resolve: its flags and their refusals

The exponent of the reference's pow is NOT swept: pow(b, p) is not linear under PAR, every value would need a PAR plane of its own.
"""
import ctypes as C
import math

import numpy as np

MAX_SCALES = 16


# ------------------------------------------------------------------ the scales
def check_scales(seq):
    """-> the scales as a tuple of floats.  Refused (ValueError naming the value): none or more than 16, a value that is not a finite
    number > 0, values that are not strictly increasing."""
    try:
        vals = [float(v) for v in seq]
    except (TypeError, ValueError) as e:
        raise ValueError(f"bkg_sweep: scales must be numbers ({e})")
    if not 1 <= len(vals) <= MAX_SCALES:
        raise ValueError(f"bkg_sweep: need 1..{MAX_SCALES} scales, got {len(vals)}")
    for i, v in enumerate(vals):
        if not math.isfinite(v) or not v > 0.0:
            raise ValueError(f"bkg_sweep: scale {v!r} must be a finite number > 0")
        if not math.isfinite(float(np.float32(v))) or not float(np.float32(v)) > 0.0:
            raise ValueError(f"bkg_sweep: scale {v!r} is outside the float32 range")
        if i and not float(np.float32(v)) > float(np.float32(vals[i - 1])):
            raise ValueError(f"bkg_sweep: scale {v!r} follows {vals[i - 1]!r}: the scales must be strictly increasing")
    return tuple(vals)


def parse_scales(text):
    """"0.5,0.7,1.0" -> (0.5, 0.7, 1.0) through check_scales; None or "" -> None (no sweep)."""
    if text is None or (isinstance(text, str) and not text.strip()):
        return None
    if not isinstance(text, str):
        return check_scales(text)
    parts = [p.strip() for p in text.split(",")]
    vals = []
    for p in parts:
        try:
            vals.append(float(p))
        except ValueError:
            raise ValueError(f"--bkg_sweep: {p!r} is not a number (a comma-separated list such as \"0.5,0.7,1.0,1.5\")")
    return check_scales(vals)


def check_scale(value):
    """--bkg_scale: one finite scale > 0 -> float."""
    return check_scales([value])[0]


# ------------------------------------------------------------------ the device op
def sweep_ragged(par_out, plan, Cmax, scales, nchan=None, cls_idx=None, gts=None, num_classes=None, skip=None, totals=None, label_sel=None,
                 labels_out=None):
    """excel_bkg_sweep_ragged (include/excel_hip.h, "background-scale sweep") -> (totals, labels).
    par_out: packed float32 planes, Cmax pitched planes per image (ops.par_forward_ragged's output); plan: its ops.RaggedPlan;
    scales: host sequence of K floats; nchan int32 [B], cls_idx int32 [B,Smax], skip int32 [B]: device or None.
    gts (flat tight uint8, device) asks for the counts: `totals` int64 [K,3,num_classes] is ADDED to (None: a fresh zeroed tensor).
    label_sel (an index into scales) asks for that scale's label map: flat uint8 [plan.total_label_pix], into labels_out if given.
    Whatever is not asked for comes back as None.  One launch on the current stream, no workspace, no synchronisation."""
    import torch
    from .. import ops
    scales = [float(s) for s in scales]
    K = len(scales)
    arr = (C.c_float * max(K, 1))(*scales)
    smax = int(cls_idx.shape[1]) if cls_idx is not None else int(Cmax) - 1
    if gts is not None:
        if num_classes is None:
            raise ValueError("sweep_ragged: gts needs num_classes")
        gts = gts.contiguous().view(-1)
        if gts.numel() != plan.total_label_pix:
            raise ValueError(f"sweep_ragged: gts holds {gts.numel()} pixels, the plan {plan.total_label_pix}")
        if totals is None:
            totals = torch.zeros((K, 3, int(num_classes)), dtype=torch.int64, device=par_out.device)
        elif tuple(totals.shape) != (K, 3, int(num_classes)) or totals.dtype != torch.int64:
            raise ValueError(f"sweep_ragged: totals must be int64 [{K},3,{int(num_classes)}], got {totals.dtype} {tuple(totals.shape)}")
    elif totals is not None:
        raise ValueError("sweep_ragged: totals needs gts")
    labels = None
    if label_sel is not None:
        labels = ops._out(labels_out, (plan.total_label_pix,), torch.uint8, par_out.device)
    elif labels_out is not None:
        raise ValueError("sweep_ragged: labels_out needs label_sel")
    if par_out.numel() < int(Cmax) * plan.total_pix:
        raise ValueError(f"sweep_ragged: par_out holds {par_out.numel()} floats, the plan needs {int(Cmax) * plan.total_pix}")
    for name, t in (("nchan", nchan), ("skip", skip)):
        if t is not None and t.numel() != plan.B:
            raise ValueError(f"sweep_ragged: {name} holds {t.numel()} values for {plan.B} images")
    if cls_idx is not None and int(cls_idx.shape[0]) != plan.B:
        raise ValueError(f"sweep_ragged: cls_idx has {int(cls_idx.shape[0])} rows for {plan.B} images")
    ops.check(ops.lib().excel_bkg_sweep_ragged(
        ops._p(par_out), ops._p(nchan, torch.int32), ops._p(cls_idx, torch.int32), ops._p(gts, torch.uint8), ops._p(plan.table, torch.int32),
        C.byref(plan.info), smax, int(Cmax), arr, K, ops._p(skip, torch.int32), int(num_classes) if num_classes is not None else 1,
        ops._p(totals, torch.int64), int(label_sel) if label_sel is not None else 0, ops._p(labels, torch.uint8), ops._stream()),
        "excel_bkg_sweep_ragged")
    return totals, labels


# ------------------------------------------------------------------ the same contract in numpy
def _sizes(plan):
    hw = np.asarray(getattr(plan, "hw", plan), np.int64).reshape(-1, 2)
    wp = (hw[:, 1] + 3) // 4 * 4
    poff = np.concatenate([[0], np.cumsum(hw[:, 0] * wp)])
    loff = np.concatenate([[0], np.cumsum(hw[:, 0] * hw[:, 1])])
    return hw, wp, poff, loff


def sweep_reference(par_out, plan, Cmax, scales, nchan=None, cls_idx=None, gts=None, num_classes=None, skip=None, totals=None, label_sel=None):
    """sweep_ragged in numpy -> (totals int64 [K,3,nc] or None, labels uint8 flat or None).  plan: an ops.RaggedPlan or a sequence of
    (H, W); par_out: the packed pitched planes as a flat float32 array; the other arguments as arrays or None.  key_j is one float32
    multiply and one compare, as on the device; pad columns and the planes >= nchan[b] are never read.  `totals` is added to (a copy)."""
    hw, wp, poff, loff = _sizes(plan)
    planes = np.asarray(par_out, np.float32).reshape(-1)
    s32 = np.asarray([np.float32(s) for s in scales], np.float32)
    K, Cmax = len(s32), int(Cmax)
    if gts is not None:
        nc = int(num_classes)
        gts = np.asarray(gts, np.uint8).reshape(-1)
        totals = np.zeros((K, 3, nc), np.int64) if totals is None else np.array(totals, np.int64)
    labels = np.zeros(int(loff[-1]), np.uint8) if label_sel is not None else None
    for b in range(hw.shape[0]):
        H, W = int(hw[b, 0]), int(hw[b, 1])
        nch = min(int(np.asarray(nchan).reshape(-1)[b]), Cmax) if nchan is not None else Cmax
        img = planes[Cmax * int(poff[b]):Cmax * int(poff[b]) + Cmax * H * int(wp[b])].reshape(Cmax, H, int(wp[b]))[:nch, :, :W]
        b0 = img[0]
        if nch > 1:
            ci = np.argmax(img[1:], axis=0) + 1                   # the first plane that attains the maximum
            F = np.take_along_axis(img, ci[None], 0)[0]
            key_fg = (np.asarray(cls_idx).reshape(hw.shape[0], -1)[b][ci - 1].astype(np.int64) + 1) if cls_idx is not None else ci.astype(np.int64)
        for j in range(K):
            if nch > 1:
                with np.errstate(invalid="ignore", over="ignore"):
                    bkg = (s32[j] * b0).astype(np.float32) >= F  # float32 * float32 -> float32, then the compare
                key = np.where(bkg, 0, key_fg)
            else:
                key = np.zeros((H, W), np.int64)
            if label_sel is not None and j == int(label_sel):
                labels[int(loff[b]):int(loff[b + 1])] = key.reshape(-1).astype(np.uint8)
            if gts is None or (skip is not None and int(np.asarray(skip).reshape(-1)[b]) != 0):
                continue
            g = gts[int(loff[b]):int(loff[b + 1])].astype(np.int64)
            k = key.reshape(-1)
            ok = (g < nc) & (k < nc)
            totals[j, 0] += np.bincount(g[ok], minlength=nc)
            totals[j, 1] += np.bincount(k[ok], minlength=nc)
            totals[j, 2] += np.bincount(g[ok & (g == k)], minlength=nc)
    return (totals if gts is not None else None), labels


# ------------------------------------------------------------------ scores
def scores_from_totals(totals):
    """int [K,3,nc] (ground-truth area, predicted area, intersection per class: the margins of the confusion matrix at every scale) ->
    one dict per scale with the keys and the float64 arithmetic of utils/evaluate.scores_from_hist: equal to it key for key on the
    matrix of the same labels (row sums, column sums and the diagonal are all it reads)."""
    t = np.asarray(totals.detach().cpu().numpy() if hasattr(totals, "detach") else totals)
    if t.ndim != 3 or t.shape[1] != 3:
        raise ValueError(f"scores_from_totals: totals must be [K,3,nc], got {t.shape}")
    out = []
    for rows in t.astype(np.float64):
        area, pred, tp = rows
        n = area.shape[0]
        with np.errstate(divide="ignore", invalid="ignore"):
            acc = tp.sum() / area.sum()
            acc_cls = np.nanmean(tp / area)
            iu = tp / (area + pred - tp)
            valid = area > 0
            mean_iu = np.nanmean(iu[valid])
            fn, fp = area - tp, pred - tp
            cr = fp / tp
            precision = tp / (tp + fp)
            recall = tp / (tp + fn)
        out.append({"pAcc": acc, "mAcc": acc_cls, "miou": mean_iu, "iou": dict(zip(range(n), iu)), "confusion": dict(zip(range(n), cr)),
                    "precision": dict(zip(range(n), precision)), "recall": dict(zip(range(n), recall))})
    return out


def _fg_miou(score):
    """The mean IoU of the foreground classes that have ground truth (recall is NaN exactly where a class has none)."""
    iou = np.asarray(list(score["iou"].values()), np.float64)[1:]
    have = ~np.isnan(np.asarray(list(score["recall"].values()), np.float64)[1:])
    return float(np.mean(iou[have])) if have.any() else float("nan")


def best_scale(scores, scales):
    """-> (index, scale) of the best mIoU; on a tie the scale nearest 1.0 wins (then the smaller one).  A NaN mIoU never wins."""
    best = None
    for j, (sc, s) in enumerate(zip(scores, scales)):
        m = float(sc["miou"])
        key = (-(m if m == m else -math.inf), abs(float(s) - 1.0), float(s))
        if best is None or key < best[0]:
            best = (key, j)
    if best is None:
        raise ValueError("best_scale: no scales")
    return best[1], float(scales[best[1]])


def format_sweep_table(scores, scales, class_list):
    """One row per scale: pAcc, mIoU, the background's IoU and the mean foreground IoU (in percent); the best mIoU is marked with *."""
    jb, _ = best_scale(scores, scales)
    bkg = class_list[0] if len(class_list) else "0"
    rows = [["bkg_scale", "pAcc", "mIoU", f"IoU {bkg}", "mIoU foreground", ""]]
    for j, (sc, s) in enumerate(zip(scores, scales)):
        rows.append([f"{float(s):g}", f"{sc['pAcc'] * 100:.3f}", f"{sc['miou'] * 100:.3f}", f"{sc['iou'][0] * 100:.3f}", f"{_fg_miou(sc) * 100:.3f}",
                     "*" if j == jb else ""])
    widths = [max(len(r[c]) for r in rows) for c in range(len(rows[0]))]
    line = "+" + "+".join("-" * (w + 2) for w in widths) + "+"
    out = [line]
    for i, r in enumerate(rows):
        out.append("|" + "|".join(" " + r[c].ljust(widths[c]) + " " for c in range(len(r))) + "|")
        if i == 0:
            out.append(line)
    out.append(line)
    return "\n".join(out)


def sweep_json(scores, scales):
    """The `bkg_sweep` block of --json_out: the scales, the mIoU at each of them and the best scale."""
    _, s = best_scale(scores, scales)
    return {"scales": [float(x) for x in scales], "miou": [None if sc["miou"] != sc["miou"] else float(sc["miou"]) for sc in scores],
            "best_scale": s}


# ------------------------------------------------------------------ the program's flags (tools/infer_lam.py)
def add_flags(parser):
    parser.add_argument("--bkg_sweep", default=None, type=str,
                        help="score the pseudo labels at these background scales as well, e.g. \"0.5,0.7,0.85,1.0,1.2,1.5,2.0\" (1..16 increasing "
                             "values > 0): one more launch per step on the PAR output the step already has, a bkg_sweep_score table and the best scale")
    parser.add_argument("--bkg_scale", default=1.0, type=float,
                        help="label with the background scaled by this factor (1.0: the reference's labels); everything downstream - scores, "
                             "PNGs - takes those labels")


def resolve(args):
    """--bkg_sweep / --bkg_scale -> (scales tuple or None, scale float), checked; the refusals name the flag that excludes them."""
    sweep = parse_scales(getattr(args, "bkg_sweep", None))
    try:
        scale = check_scale(getattr(args, "bkg_scale", 1.0))
    except ValueError as e:
        raise ValueError(f"--bkg_scale: {e}")
    if sweep is not None and getattr(args, "unlabeled", False):
        raise ValueError("--bkg_sweep scores the labels against ground truth: --unlabeled true has none, there is nothing to score")
    if (sweep is not None or scale != 1.0) and getattr(args, "api_path", False):
        which = "--bkg_sweep" if sweep is not None else "--bkg_scale"
        raise ValueError(f"{which} runs on the batched loop: --api_path true is the reference's per-image call sequence, which has the fixed background")
    return sweep, scale
