"""--margin_sweep / --margin_min: score the pseudo labels over a range of arg-max margins, and cut them at one.

The labels are the arg-max over [a * b0 ; cam_1 .. cam_k] of PAR's output (utils/bkg_sweep.py; a = bkg_scale).  The margin of a pixel
is the winning plane minus the runner-up: a confidence the step's PAR output already holds, at no second PAR pass and with no threshold
inherited from anywhere.  excel_margin_sweep_ragged (csrc/margin.hip) reads the planes once and counts, for K margin thresholds at once,
the pixels with margin >= t_j (coverage: no ground truth needed) and their confusion-matrix margins against the ground truth (risk),
and / or writes the label map with 255 below one threshold, and / or the margins themselves.  This module is its host side:

    check_thresholds / parse_thresholds   the thresholds of a sweep: 1..16 values, finite, >= 0, strictly increasing (as float32)
    margin_ragged                         the ctypes binding (device tensors in, device tensors out, the caller's stream)
    margin_reference                      the same contract in numpy - float32 multiply, subtract and compare: the judge of the GPU tests
    coverage_from_kept                    int64 [K+1] -> kept[j] / kept[K]
    format_margin_table, margin_json, margin_min_json    what tools/infer_lam reports;  add_flags, resolve: its flags and their refusals

The scores per threshold come from utils/bkg_sweep.scores_from_totals: the totals have its layout.
No threshold is a default: nothing here has been measured on real data, the values in the examples are illustrations.
"""
import ctypes as C
import math

import numpy as np

MAX_THRESHOLDS = 16
IGNORE = 255


# ------------------------------------------------------------------ the thresholds
def check_thresholds(seq, allow_empty=False):
    """-> the thresholds as a tuple of floats.  Refused (ValueError naming the value): none (unless allow_empty) or more than 16, a value
    that is not a finite number >= 0 (as float32 too), values that are not strictly increasing as float32."""
    try:
        vals = [float(v) for v in seq]
    except (TypeError, ValueError) as e:
        raise ValueError(f"margin_sweep: thresholds must be numbers ({e})")
    if not (0 if allow_empty else 1) <= len(vals) <= MAX_THRESHOLDS:
        raise ValueError(f"margin_sweep: need {0 if allow_empty else 1}..{MAX_THRESHOLDS} thresholds, got {len(vals)}")
    for i, v in enumerate(vals):
        if not math.isfinite(v) or not v >= 0.0:
            raise ValueError(f"margin_sweep: threshold {v!r} must be a finite number >= 0")
        with np.errstate(over="ignore"):
            v32 = float(np.float32(v))
        if not math.isfinite(v32):
            raise ValueError(f"margin_sweep: threshold {v!r} is outside the float32 range")
        if i and not v32 > float(np.float32(vals[i - 1])):
            raise ValueError(f"margin_sweep: threshold {v!r} follows {vals[i - 1]!r}: the thresholds must be strictly increasing (as float32)")
    return tuple(vals)


def parse_thresholds(text):
    """"0,0.05,0.1" -> (0.0, 0.05, 0.1) through check_thresholds; None or "" -> None (no sweep)."""
    if text is None or (isinstance(text, str) and not text.strip()):
        return None
    if not isinstance(text, str):
        return check_thresholds(text)
    vals = []
    for p in (q.strip() for q in text.split(",")):
        try:
            vals.append(float(p))
        except ValueError:
            raise ValueError(f"--margin_sweep: {p!r} is not a number (a comma-separated list such as \"0,0.05,0.1,0.2\")")
    return check_thresholds(vals)


def check_min(value):
    """--margin_min / margin_min=: one finite threshold >= 0 -> float."""
    try:
        return check_thresholds([value])[0]
    except ValueError as e:
        raise ValueError(str(e).replace("margin_sweep: threshold", "margin_min: value").replace("margin_sweep: thresholds", "margin_min: the value"))


# ------------------------------------------------------------------ the device op
def margin_ragged(par_out, plan, Cmax, thresholds, nchan=None, cls_idx=None, gts=None, num_classes=None, skip=None, totals=None, kept=None,
                  label_thre=None, labels_out=None, margin_out=None, bkg_scale=1.0):
    """excel_margin_sweep_ragged (include/excel_hip.h, "arg-max margin") -> (totals, kept, labels, margin).
    par_out: packed float32 planes, Cmax pitched planes per image (ops.par_forward_ragged's output); plan: its ops.RaggedPlan;
    thresholds: host sequence of K floats (K = 0: labels and margins only); nchan int32 [B], cls_idx int32 [B,Smax], skip int32 [B]:
    device or None.
    gts (flat tight uint8, device) with K >= 1 asks for the counts: `totals` int64 [K,3,num_classes] is ADDED to (None: a fresh zeroed
    tensor).  kept=True asks for a fresh int64 [K+1], a tensor is ADDED to.  label_thre (a float) asks for the label map cut there: flat
    uint8 [plan.total_label_pix], into labels_out if given.  margin_out=True asks for the margins, flat float32 [plan.total_label_pix],
    a tensor receives them.  Whatever is not asked for comes back as None.  One launch on the current stream, no workspace, no
    synchronisation."""
    import torch
    from .. import ops
    thresholds = [float(t) for t in thresholds]
    K = len(thresholds)
    arr = (C.c_float * max(K, 1))(*thresholds)
    smax = int(cls_idx.shape[1]) if cls_idx is not None else int(Cmax) - 1
    dev = par_out.device
    if gts is not None:
        if num_classes is None:
            raise ValueError("margin_ragged: gts needs num_classes")
        gts = gts.contiguous().view(-1)
        if gts.numel() != plan.total_label_pix:
            raise ValueError(f"margin_ragged: gts holds {gts.numel()} pixels, the plan {plan.total_label_pix}")
        if K >= 1:
            if totals is None:
                totals = torch.zeros((K, 3, int(num_classes)), dtype=torch.int64, device=dev)
            elif tuple(totals.shape) != (K, 3, int(num_classes)) or totals.dtype != torch.int64:
                raise ValueError(f"margin_ragged: totals must be int64 [{K},3,{int(num_classes)}], got {totals.dtype} {tuple(totals.shape)}")
        elif totals is not None:
            raise ValueError("margin_ragged: totals needs at least one threshold")
    elif totals is not None:
        raise ValueError("margin_ragged: totals needs gts")
    if kept is False:
        kept = None
    if kept is not None:
        if K < 1:
            raise ValueError("margin_ragged: kept needs at least one threshold")
        if kept is True:
            kept = torch.zeros((K + 1,), dtype=torch.int64, device=dev)
        elif tuple(kept.shape) != (K + 1,) or kept.dtype != torch.int64:
            raise ValueError(f"margin_ragged: kept must be int64 [{K + 1}], got {kept.dtype} {tuple(kept.shape)}")
    labels = None
    if label_thre is not None:
        labels = ops._out(labels_out, (plan.total_label_pix,), torch.uint8, dev)
    elif labels_out is not None:
        raise ValueError("margin_ragged: labels_out needs label_thre")
    if margin_out is False:
        margin_out = None
    if margin_out is not None:
        margin_out = ops._out(None if margin_out is True else margin_out, (plan.total_label_pix,), torch.float32, dev)
    if par_out.numel() < int(Cmax) * plan.total_pix:
        raise ValueError(f"margin_ragged: par_out holds {par_out.numel()} floats, the plan needs {int(Cmax) * plan.total_pix}")
    for name, t in (("nchan", nchan), ("skip", skip)):
        if t is not None and t.numel() != plan.B:
            raise ValueError(f"margin_ragged: {name} holds {t.numel()} values for {plan.B} images")
    if cls_idx is not None and int(cls_idx.shape[0]) != plan.B:
        raise ValueError(f"margin_ragged: cls_idx has {int(cls_idx.shape[0])} rows for {plan.B} images")
    ops.check(ops.lib().excel_margin_sweep_ragged(
        ops._p(par_out), ops._p(nchan, torch.int32), ops._p(cls_idx, torch.int32), ops._p(gts if totals is not None else None, torch.uint8),
        ops._p(plan.table, torch.int32), C.byref(plan.info), smax, int(Cmax), float(bkg_scale), arr, K, ops._p(skip, torch.int32),
        int(num_classes) if num_classes is not None else 1, ops._p(totals, torch.int64), ops._p(kept, torch.int64),
        float(label_thre) if label_thre is not None else 0.0, ops._p(labels, torch.uint8), ops._p(margin_out, torch.float32), ops._stream()),
        "excel_margin_sweep_ragged")
    return totals, kept, labels, margin_out


# ------------------------------------------------------------------ the same contract in numpy
def _sizes(plan):
    hw = np.asarray(getattr(plan, "hw", plan), np.int64).reshape(-1, 2)
    wp = (hw[:, 1] + 3) // 4 * 4
    poff = np.concatenate([[0], np.cumsum(hw[:, 0] * wp)])
    loff = np.concatenate([[0], np.cumsum(hw[:, 0] * hw[:, 1])])
    return hw, wp, poff, loff


def margin_reference(par_out, plan, Cmax, thresholds, nchan=None, cls_idx=None, gts=None, num_classes=None, skip=None, totals=None, kept=None,
                     label_thre=None, bkg_scale=1.0):
    """margin_ragged in numpy -> (totals int64 [K,3,nc] or None, kept int64 [K+1] or None, labels uint8 flat or None, margin float32
    flat).  plan: an ops.RaggedPlan or a sequence of (H, W); par_out: the packed pitched planes as a flat float32 array; the other
    arguments as arrays or None.  The margin is one float32 multiply and one float32 subtract, the cuts are float32 compares, as on the
    device; pad columns and the planes >= nchan[b] are never read.  Totals come with gts and K >= 1, kept with K >= 1 (both are added
    to copies of `totals` / `kept` when given), labels with label_thre; the margins always."""
    hw, wp, poff, loff = _sizes(plan)
    planes = np.asarray(par_out, np.float32).reshape(-1)
    t32 = np.asarray([np.float32(t) for t in thresholds], np.float32)
    K, Cmax = len(t32), int(Cmax)
    a = np.float32(bkg_scale)
    want_totals = gts is not None and K >= 1
    if want_totals:
        nc = int(num_classes)
        gts = np.asarray(gts, np.uint8).reshape(-1)
        totals = np.zeros((K, 3, nc), np.int64) if totals is None else np.array(totals, np.int64)
    if K >= 1:
        kept = np.zeros(K + 1, np.int64) if kept is None or kept is True else np.array(kept, np.int64)
    labels = np.zeros(int(loff[-1]), np.uint8) if label_thre is not None else None
    margins = np.zeros(int(loff[-1]), np.float32)
    for b in range(hw.shape[0]):
        H, W = int(hw[b, 0]), int(hw[b, 1])
        nch = min(int(np.asarray(nchan).reshape(-1)[b]), Cmax) if nchan is not None else Cmax
        img = planes[Cmax * int(poff[b]):Cmax * int(poff[b]) + Cmax * H * int(wp[b])].reshape(Cmax, H, int(wp[b]))[:nch, :, :W]
        if nch == 1:
            key = np.zeros((H, W), np.int64)
            margin = np.full((H, W), np.inf, np.float32)
        else:
            with np.errstate(invalid="ignore", over="ignore"):
                v0 = (a * img[0]).astype(np.float32)                         # float32 * float32 -> float32
                bad = np.isnan(v0) | np.isnan(img[1:]).any(0)
                v0 = np.where(bad, np.float32(0), v0)
                fg = np.where(bad[None], np.float32(0), img[1:])
                ci = np.argmax(fg, axis=0)                                   # the first plane that attains the maximum (0-based here)
                F = np.take_along_axis(fg, ci[None], 0)[0]
                key_fg = (np.asarray(cls_idx).reshape(hw.shape[0], -1)[b][ci].astype(np.int64) + 1) if cls_idx is not None else ci.astype(np.int64) + 1
                bkg = (v0 >= F) | (key_fg == 0)
                key = np.where(bkg, 0, key_fg)
                if nch > 2:
                    others = np.where(np.arange(nch - 1)[:, None, None] == ci[None], np.float32(-np.inf), fg)
                    R = np.maximum(v0, others.max(0))
                else:
                    R = v0
                margin = np.where(bkg, v0 - F, F - R).astype(np.float32)     # float32 - float32 -> float32
                margin = np.where(bad, np.float32(np.nan), margin).astype(np.float32)
        sl = slice(int(loff[b]), int(loff[b + 1]))
        margins[sl] = margin.reshape(-1)
        with np.errstate(invalid="ignore"):
            if labels is not None:
                labels[sl] = np.where(margin >= np.float32(label_thre), key, IGNORE).reshape(-1).astype(np.uint8)
            if K < 1 or (skip is not None and int(np.asarray(skip).reshape(-1)[b]) != 0):
                continue
            kept[K] += H * W
            k = key.reshape(-1)
            for j in range(K):
                keep = (margin >= t32[j]).reshape(-1)
                kept[j] += int(keep.sum())
                if not want_totals:
                    continue
                g = gts[sl].astype(np.int64)
                ok = keep & (g < nc) & (k < nc)
                totals[j, 0] += np.bincount(g[ok], minlength=nc)
                totals[j, 1] += np.bincount(k[ok], minlength=nc)
                totals[j, 2] += np.bincount(g[ok & (g == k)], minlength=nc)
    return (totals if want_totals else None), (kept if K >= 1 else None), labels, margins


# ------------------------------------------------------------------ what the programs report
def _np(x):
    return np.asarray(x.detach().cpu().numpy() if hasattr(x, "detach") else x)


def coverage_from_kept(kept):
    """int [K+1] (kept[j] = pixels with margin >= t_j, kept[K] = all pixels) -> K floats kept[j] / kept[K]; NaN when there is no pixel."""
    k = _np(kept).astype(np.float64).reshape(-1)
    if k.shape[0] < 2:
        raise ValueError(f"coverage_from_kept: kept must be [K+1] with K >= 1, got {k.shape}")
    return [float(v / k[-1]) if k[-1] > 0 else float("nan") for v in k[:-1]]


def _table(rows):
    widths = [max(len(r[c]) for r in rows) for c in range(len(rows[0]))]
    line = "+" + "+".join("-" * (w + 2) for w in widths) + "+"
    out = [line]
    for i, r in enumerate(rows):
        out.append("|" + "|".join(" " + r[c].ljust(widths[c]) + " " for c in range(len(r))) + "|")
        if i == 0:
            out.append(line)
    out.append(line)
    return "\n".join(out)


def format_margin_table(thresholds, kept, scores=None, class_list=()):
    """One row per threshold: the coverage (kept pixels over all pixels, in percent), then pAcc, mIoU, the background's IoU and the mean
    foreground IoU of the kept pixels (bkg_sweep.scores_from_totals of the totals).  scores=None (no ground truth): the coverage alone."""
    from .bkg_sweep import _fg_miou
    cover = coverage_from_kept(kept)
    if len(cover) != len(thresholds) or (scores is not None and len(scores) != len(thresholds)):
        raise ValueError("format_margin_table: one coverage and one score per threshold")
    bkg = class_list[0] if len(class_list) else "0"
    rows = [["margin >=", "coverage %"] + (["pAcc", "mIoU", f"IoU {bkg}", "mIoU foreground"] if scores is not None else [])]
    for j, t in enumerate(thresholds):
        row = [f"{float(t):g}", f"{cover[j] * 100:.3f}"]
        if scores is not None:
            sc = scores[j]
            row += [f"{sc['pAcc'] * 100:.3f}", f"{sc['miou'] * 100:.3f}", f"{sc['iou'][0] * 100:.3f}", f"{_fg_miou(sc) * 100:.3f}"]
        rows.append(row)
    return _table(rows)


def _nn(x):
    return None if x is None or x != x else float(x)


def margin_json(thresholds, kept, scores=None):
    """The `margin_sweep` block of --json_out: thresholds and coverage, and with ground truth the mIoU and pAcc at each threshold."""
    block = {"thresholds": [float(t) for t in thresholds], "coverage": [_nn(c) for c in coverage_from_kept(kept)]}
    if scores is not None:
        block["miou"] = [_nn(sc["miou"]) for sc in scores]
        block["pacc"] = [_nn(sc["pAcc"]) for sc in scores]
    return block


def margin_min_json(margin_min, score=None, cover=None):
    """The `margin` block of --json_out: the cut and, with ground truth, the score of the kept pixels and their share of the labelled ones."""
    block = {"margin_min": float(margin_min)}
    if score is not None:
        block.update(miou=_nn(score["miou"]), pAcc=_nn(score["pAcc"]), coverage=_nn(cover))
    return block


# ------------------------------------------------------------------ the program's flags (tools/infer_lam.py)
def add_flags(parser):
    parser.add_argument("--margin_sweep", default=None, type=str,
                        help="score the pseudo labels cut at these arg-max margins (winner minus runner-up of the PAR planes), e.g. "
                             "\"0,0.05,0.1,0.2,0.3\" (1..16 increasing values >= 0; illustrations, no value has been measured on real data): one "
                             "more launch per step, a margin_sweep_score table of coverage and scores per threshold; the coverage needs no "
                             "ground truth")
    parser.add_argument("--margin_min", default=None, type=float,
                        help="a further label set: the labels with 255 where the arg-max margin is below this value (no default: nothing has "
                             "been measured on real data)")
    parser.add_argument("--margin_label_dir", default=None, type=str, help="write the --margin_min label maps here as palette PNGs")


def resolve(args, ragged=None):
    """--margin_sweep / --margin_min / --margin_label_dir -> (thresholds tuple or None, dict(min=, label_dir=) or None), checked before
    anything is built; the refusals name the flag that excludes them.  `ragged` = whether the run has ragged batches (None: not known
    yet, not checked)."""
    sweep = parse_thresholds(getattr(args, "margin_sweep", None))
    raw = getattr(args, "margin_min", None)
    out_dir = getattr(args, "margin_label_dir", None)
    cut = None
    if raw is None:
        if out_dir is not None:
            raise ValueError("--margin_label_dir needs --margin_min: there are no margin labels to write")
    else:
        try:
            cut = dict(min=check_min(raw), label_dir=out_dir)
        except ValueError as e:
            raise ValueError(f"--margin_min: {e}")
    if sweep is None and cut is None:
        return None, None
    which = "--margin_sweep" if sweep is not None else "--margin_min"
    if getattr(args, "api_path", False):
        raise ValueError(f"{which} runs on the batched loop: --api_path true is the reference's per-image call sequence, which keeps no margin")
    if cut is not None and getattr(args, "unlabeled", False) and out_dir is None:
        raise ValueError("--margin_min with --unlabeled true scores nothing: give --margin_label_dir, the margin labels are its only output")
    if ragged is not None and not ragged:
        raise ValueError(f"{which} runs behind the ragged step: ragged batches (--data_folder or --ragged true) on the batched loop")
    return sweep, cut
