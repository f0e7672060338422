"""--fill_ignore: give every cleaned-away or ignore pixel (255) of a label map the value of the nearest labelled pixel of its image.

--clean_min_region (utils/components.py) turns the small regions of a pseudo-label map into 255; this is the other half: a pin-hole
inside an object becomes object again instead of a pixel the training loss ignores.  One device entry (csrc/fill.hip;
include/excel_hip.h, "nearest-label fill"), an exact Euclidean nearest-label transform in integers:

    fill_nearest_label   every hole - a 255 pixel, and with a mask only where the mask is not 255 - takes the value of the seed (a pixel
                         with a value < num_classes) of its own image with the smallest squared distance, the first one in raster order
                         on a tie, if that distance is within the radius; dist2 = the squared distance (0 at seeds, -1 where nothing
                         was filled); counts[b] = (holes, holes filled, the largest squared distance of a filled hole)
    fill_numpy           the same contract as two separable passes in numpy (no scipy): what tools/eval_labels uses without a GPU
    radius_rule          the flag's value -> max_dist2: None / "inf" is unlimited, an integer >= 1 is pixels
    fill_stats, format_fill_summary, fill_json, add_flags, resolve   what the programs report, their flags and refusals

Values in [num_classes, 255) are neither seeds nor holes: they pass through and block nothing.  Not done here: a fill that respects
region borders (a hole between two objects takes the nearer one, whatever lies between).  What the fill does to the score of real data is
unmeasured: no real checkpoint or data set is available to this project.
"""
import ctypes as C

import numpy as np

FILL_ROW_THREADS = 256              # the workgroup width of fill_row_kernel: a row is walked in strides of this many pixels
FILL_MAX_SIDE = 8192                # an image may not be higher or wider: d2 fits 28 bits, a row of candidates fits in LDS
UNLIMITED = 2 ** 31 - 1
IGNORE = 255


# ------------------------------------------------------------------ the radius
def radius_rule(value):
    """--fill_ignore VALUE -> max_dist2 (int in [1, 2^31 - 1]).  None or "inf": unlimited; an integer >= 1: pixels, max_dist2 = value^2
    (capped at 2^31 - 1, beyond every distance inside FILL_MAX_SIDE).  Anything else - 0, a negative, 2.5, True, "far" - is a ValueError."""
    if value is None or (isinstance(value, str) and value == "inf"):
        return UNLIMITED
    if isinstance(value, bool) or not isinstance(value, (int, np.integer)):
        raise ValueError(f"fill_ignore: {value!r} must be 'inf' or an integer number of pixels >= 1")
    if int(value) < 1:
        raise ValueError(f"fill_ignore: {value!r} must be 'inf' or an integer number of pixels >= 1")
    return min(int(value) ** 2, UNLIMITED)


# ------------------------------------------------------------------ the device op
def fill_nearest_label(labels_u8, num_classes, plan=None, mask=None, radius=None, out=None):
    """excel_fill_nearest_label -> (filled uint8, dist2 int32, both shaped like labels_u8; counts int32 [B,3]) on the device.  plan=None:
    uniform [B,H,W] maps; with an ops.RaggedPlan: its tight label maps back to back (a flat uint8 tensor, which may start at any byte).
    mask: a uint8 tensor like labels_u8 - a 255 of the labels is a hole only where the mask is not 255 - or None: every 255 is a hole.
    radius: radius_rule.  out = (filled, dist2, counts) buffers to fill instead of fresh ones; the filled map may be neither input.  Two
    launches behind one clearing on the current stream, no workspace, no synchronisation."""
    import torch
    from .. import ops
    from .components import _geometry
    lab = labels_u8.contiguous()
    if lab.dtype != torch.uint8:
        raise ValueError(f"fill_nearest_label: labels must be uint8 (got {lab.dtype})")
    max_dist2 = radius_rule(radius)
    nc = int(num_classes)
    if not 1 <= nc <= 255:
        raise ValueError(f"fill_nearest_label: num_classes = {nc} is outside [1, 255] (255 is the hole)")
    B, H, W = _geometry(lab, plan, "fill_nearest_label")
    sides = [(H, W)] if plan is None else [(int(h), int(w)) for h, w in plan.hw]
    for b, (h, w) in enumerate(sides):
        if h > FILL_MAX_SIDE or w > FILL_MAX_SIDE:
            raise ValueError(f"fill_nearest_label: image {b} is {h} x {w}, beyond {FILL_MAX_SIDE} pixels a side")
    msk = None
    if mask is not None:
        msk = mask.contiguous()
        if msk.dtype != torch.uint8 or msk.numel() != lab.numel() or msk.device != lab.device:
            raise ValueError(f"fill_nearest_label: mask must hold {lab.numel()} uint8 on {lab.device} (got {msk.numel()} {msk.dtype} on {msk.device})")
    if out is None:
        filled = torch.empty(lab.shape, dtype=torch.uint8, device=lab.device)
        dist2 = torch.empty(lab.shape, dtype=torch.int32, device=lab.device)
        counts = torch.empty((B, 3), dtype=torch.int32, device=lab.device)
    else:
        filled, dist2, counts = out
        if filled.dtype != torch.uint8 or filled.numel() != lab.numel() or not filled.is_contiguous():
            raise ValueError(f"fill_nearest_label: out map must hold {lab.numel()} contiguous uint8 (got {filled.numel()} {filled.dtype})")
        if dist2.dtype != torch.int32 or dist2.numel() != lab.numel() or not dist2.is_contiguous():
            raise ValueError(f"fill_nearest_label: out dist2 must hold {lab.numel()} contiguous int32 (got {dist2.numel()} {dist2.dtype})")
        if counts.dtype != torch.int32 or counts.numel() != 3 * B or not counts.is_contiguous():
            raise ValueError(f"fill_nearest_label: out counts must hold {3 * B} contiguous int32 (got {counts.numel()} {counts.dtype})")
        counts = counts.view(B, 3)
    ops.check(ops.lib().excel_fill_nearest_label(
        ops._p(lab, torch.uint8), ops._p(msk, torch.uint8), B, H, W, ops._p(plan.table, torch.int32) if plan is not None else None,
        C.byref(plan.info) if plan is not None else None, nc, max_dist2, ops._p(filled, torch.uint8), ops._p(dist2, torch.int32),
        ops._p(counts, torch.int32), ops._stream()), "excel_fill_nearest_label")
    return filled, dist2, counts


# ------------------------------------------------------------------ the same contract in numpy
def fill_numpy(label, num_classes, mask=None, radius=None):
    """One [H,W] uint8 map -> (filled uint8 [H,W], dist2 int32 [H,W], counts int64 [3]): fill_nearest_label's contract as two separable
    passes.  Column pass: per pixel the row of the nearest seed of its column (the upper one on a tie), from two running extrema.  Row
    pass: per row that has a hole, the keys (d2, y', x') of every hole against every column, and their minimum."""
    max_dist2 = radius_rule(radius)
    nc = int(num_classes)
    if not 1 <= nc <= 255:
        raise ValueError(f"fill_numpy: num_classes = {nc} is outside [1, 255] (255 is the hole)")
    lab = np.ascontiguousarray(label).astype(np.uint8)
    if lab.ndim != 2 or lab.size == 0 or max(lab.shape) > FILL_MAX_SIDE:
        raise ValueError(f"fill_numpy: need one non-empty [H,W] map of at most {FILL_MAX_SIDE} pixels a side (got {lab.shape})")
    H, W = lab.shape
    seed = lab < nc
    hole = lab == IGNORE
    if mask is not None:
        m = np.asarray(mask)
        if m.shape != lab.shape:
            raise ValueError(f"fill_numpy: the mask is {m.shape}, the map {lab.shape}")
        hole &= m != IGNORE
    rows = np.arange(H, dtype=np.int64)[:, None]
    far = 4 * FILL_MAX_SIDE
    up = np.maximum.accumulate(np.where(seed, rows, -far), axis=0)                    # the last seed at or above, or -far
    down = np.minimum.accumulate(np.where(seed, rows, far)[::-1], axis=0)[::-1]       # the first seed at or below, or far
    cand = np.where(rows - up <= down - rows, up, down)                               # the upper one keeps a tie
    none = ~seed.any(axis=0)
    filled = lab.copy()
    dist2 = np.where(seed, 0, -1).astype(np.int32)
    cols = np.arange(W, dtype=np.int64)
    worst = np.int64(1) << 62
    for y in np.flatnonzero(hole.any(axis=1)):
        xs = np.flatnonzero(hole[y])
        c = cand[y]
        d2 = (xs[:, None] - cols[None, :]) ** 2 + ((y - c) ** 2)[None, :]
        key = np.where(none[None, :], worst, (d2 << 26) | (c << 13)[None, :] | cols[None, :])
        best = key.min(axis=1)
        ok = (best != worst) & ((best >> 26) <= max_dist2)
        qy, qx = (best[ok] >> 13) & (FILL_MAX_SIDE - 1), best[ok] & (FILL_MAX_SIDE - 1)
        filled[y, xs[ok]] = lab[qy, qx]
        dist2[y, xs[ok]] = (best[ok] >> 26).astype(np.int32)
    got = hole & (dist2 >= 0)
    return filled, dist2, np.asarray([int(hole.sum()), int(got.sum()), int(dist2[got].max()) if got.any() else 0], np.int64)


# ------------------------------------------------------------------ what the programs report
def fill_stats(counts):
    """[N,3] count rows (refused rows of -1 left out) -> dict of the totals: images, holes, filled, the largest squared distance."""
    c = np.asarray(counts, np.int64).reshape(-1, 3)
    c = c[(c >= 0).all(1)]
    return dict(images=int(c.shape[0]), holes=int(c[:, 0].sum()), filled=int(c[:, 1].sum()), max_dist2=int(c[:, 2].max()) if c.shape[0] else 0)


def format_fill_summary(stats, cover=None):
    """The summary line of the log: holes, holes filled, the largest distance and (when there was ground truth) the coverage."""
    line = (f"fill holes: {stats['holes']}, filled: {stats['filled']}, largest distance: {float(np.sqrt(stats['max_dist2'])):.2f} px "
            f"over {stats['images']} images")
    if cover is not None:
        line += f"; fill coverage (kept pixels over labelled pixels): {cover * 100:.3f} %"
    return line


def fill_json(radius, stats, score=None, cover=None):
    """The `fill` block of --json_out."""
    nn = lambda x: None if x is None or x != x else float(x)
    block = dict(radius="inf" if radius is None else int(radius), images=stats["images"], holes=stats["holes"], filled=stats["filled"],
                 max_dist2=stats["max_dist2"], max_dist=float(np.sqrt(stats["max_dist2"])))
    if score is not None:
        block.update(miou=nn(score["miou"]), pAcc=nn(score["pAcc"]), coverage=nn(cover))
    return block


# ------------------------------------------------------------------ the programs' flags (tools/infer_lam.py, tools/eval_labels.py)
def _flag_value(text):
    if text == "inf":
        return None
    try:
        return int(text)
    except ValueError:
        raise ValueError(f"--fill_ignore: {text!r} must be 'inf' or an integer number of pixels >= 1")


def add_flags(parser):
    parser.add_argument("--fill_ignore", default=None, type=str,
                        help="give every cleaned-away (infer_lam) or ignore (eval_labels) pixel the value of the nearest labelled pixel of its "
                             "image: 'inf', or the largest distance in pixels, an integer >= 1 (absent: off - no launch, no output)")
    parser.add_argument("--fill_label_dir", default=None, type=str, help="write the filled label maps here as palette PNGs")


def resolve(args, program="infer_lam"):
    """The two flags -> dict(radius=None | int, label_dir=) or None (off), checked before anything is built; the refusals name the flag
    that excludes them."""
    raw = getattr(args, "fill_ignore", None)
    out_dir = getattr(args, "fill_label_dir", None)
    if raw is None:
        if out_dir is not None:
            raise ValueError("--fill_label_dir needs --fill_ignore: there are no filled maps to write")
        return None
    radius = _flag_value(raw) if isinstance(raw, str) else raw
    try:
        radius_rule(radius)
    except ValueError as e:
        raise ValueError(f"--{e}")
    if program == "infer_lam":
        if getattr(args, "clean_min_region", None) is None:
            raise ValueError("--fill_ignore needs --clean_min_region: the main arg-max map has no 255 pixel, there is nothing to fill")
        if getattr(args, "api_path", False):
            raise ValueError("--fill_ignore runs on the batched loop: --api_path true is the reference's per-image call sequence, "
                             "which has no fill")
        if getattr(args, "unlabeled", False) and out_dir is None:
            raise ValueError("--fill_ignore with --unlabeled true scores nothing: give --fill_label_dir, the filled maps are its only output")
    return dict(radius=None if radius is None else int(radius), label_dir=out_dir)
