"""--snap_superpixels: over-segment every image into superpixels and give each superpixel the majority class of the labels inside it.

Behind the arg-max, every stage of the label chain (scores, cleaning, fill) works on the label geometry alone; this one looks at the
image again: contours move onto colour edges and speckle inside a superpixel is voted away.  Two device entries (csrc/superpixels.hip;
include/excel_hip.h, "superpixel snap"), integers only, so the result is canonical:

    slic_superpixels     integer SLIC on a fixed grid (the gSLIC form): step S in [2, 64], compactness m in [1, 64], T in [0, 16]
                         iterations.  gx = ceil(W / S), gy = ceil(H / S), centre k = cy gx + cx starts at (min(W-1, cx S + S/2),
                         min(H-1, cy S + S/2)) with the colour there; a pixel of cell (x / S, y / S) takes, among the centres of the up to
                         nine cells within +-1, the smallest D = S^2 |colour difference|^2 + m^2 |position difference|^2, the smallest k on a
                         tie; a centre becomes the rounded mean (2 sum + cnt) // (2 cnt) of x, y, r, g, b over its pixels, one without a
                         pixel keeps its values; init, T x (assign, update), a final assign.  -> sp (int32 per pixel, the image-local
                         centre), centres (int32 [*,5] = x, y, r, g, b)
    snap_labels          a pixel votes iff label < num_classes; per superpixel tot votes, top = the largest class count, win = the
                         smallest class with it; snapped iff tot > 0 and 1000 top >= min_share_pm tot; out = win at the voting pixels of a
                         snapped superpixel, the label everywhere else; counts[b] = (superpixels with a vote, snapped, pixels changed)
    centre_offsets       the cent_off rule: [B+1] running sums of gy_b gx_b from the host sizes
    share_rule           --snap_min_share, a fraction in [0, 1] -> min_share_pm = int(round(1000 f))
    slic_numpy, snap_numpy, snap_batch_numpy   the same contracts, vectorised in numpy: what tools/eval_labels uses without a GPU
    snap_stats, format_snap_summary, snap_json, add_flags, resolve   what the programs report, their flags and refusals

Superpixels are not made connected (a superpixel may consist of several pieces); --clean_min_region can follow the snap.  No Lab colour
conversion: distances are taken in the decoded RGB bytes.  What the snap does to the score of real data is unmeasured: no real
checkpoint or data set is available to this project.
"""
import ctypes as C

import numpy as np

MIN_STEP, MAX_STEP = 2, 64
MAX_COMPACTNESS = 64
MAX_ITERS = 16
DEFAULTS = dict(compactness=10, iters=5, min_share=0.0)


# ------------------------------------------------------------------ the rules
def _int_in(value, lo, hi, what):
    if isinstance(value, bool) or not isinstance(value, (int, np.integer)) or not lo <= int(value) <= hi:
        raise ValueError(f"{what}: {value!r} must be an integer in [{lo}, {hi}]")
    return int(value)


def check_params(step, compactness=DEFAULTS["compactness"], iters=DEFAULTS["iters"]):
    """-> (step, compactness, iters) as ints, or a ValueError that names the parameter and its range."""
    return (_int_in(step, MIN_STEP, MAX_STEP, "snap_superpixels (the grid step)"), _int_in(compactness, 1, MAX_COMPACTNESS, "snap_compactness"),
            _int_in(iters, 0, MAX_ITERS, "snap_iters"))


def share_rule(value):
    """--snap_min_share VALUE, a fraction in [0, 1] -> min_share_pm = int(round(1000 * value)) in [0, 1000].  Anything else - a negative,
    1.5, 50 (per cent), True, "half", NaN - is a ValueError."""
    if isinstance(value, bool) or not isinstance(value, (int, float, np.integer, np.floating)):
        raise ValueError(f"snap_min_share: {value!r} must be a fraction in [0, 1]")
    f = float(value)
    if not 0.0 <= f <= 1.0:                                   # NaN fails both comparisons
        raise ValueError(f"snap_min_share: {value!r} must be a fraction in [0, 1]")
    return int(round(1000 * f))


def grid_of(h, w, step):
    """-> (gy, gx) = (ceil(h / step), ceil(w / step))"""
    return (int(h) + step - 1) // step, (int(w) + step - 1) // step


def centre_offsets(hws, step):
    """The cent_off rule: sizes [(H_b, W_b)] -> int32 [B+1], cent_off[0] = 0, cent_off[b+1] = cent_off[b] + gy_b * gx_b; the last entry is
    the total the entries take with it.  A batch with 2^31 centres or more is refused."""
    step = _int_in(step, MIN_STEP, MAX_STEP, "snap_superpixels (the grid step)")
    off = [0]
    for h, w in hws:
        if int(h) < 1 or int(w) < 1:
            raise ValueError(f"centre_offsets: an image of {h} x {w}")
        gy, gx = grid_of(h, w, step)
        off.append(off[-1] + gy * gx)
    if len(off) < 2 or off[-1] >= 2 ** 31:
        raise ValueError(f"centre_offsets: {len(off) - 1} images with {off[-1]} centres in all, outside [1, 2^31)")
    return np.asarray(off, np.int32)


# ------------------------------------------------------------------ the device ops
def _sizes(t, plan, who, per_pixel=1):
    """-> (B, H, W, the sizes [(H_b, W_b)]) of uniform [B,H,W(,3)] maps or of a plan's tight ones"""
    if plan is None:
        if t.dim() != (3 if per_pixel == 1 else 4) or (per_pixel == 3 and t.shape[-1] != 3):
            raise ValueError(f"{who}: uniform {'maps must be [B,H,W]' if per_pixel == 1 else 'images must be [B,H,W,3]'} (got {tuple(t.shape)}); "
                             "a ragged batch needs its plan")
        B, H, W = (int(x) for x in t.shape[:3])
        if B < 1 or H < 1 or W < 1:
            raise ValueError(f"{who}: at least one image with a pixel is needed (got {tuple(t.shape)})")
        return B, H, W, [(H, W)] * B
    if t.numel() != per_pixel * plan.total_label_pix:
        raise ValueError(f"{who}: {t.numel()} values, the plan holds {plan.total_label_pix} pixels of {per_pixel}")
    return plan.B, 0, 0, [(int(h), int(w)) for h, w in plan.hw]


def centre_table(sizes, step, device):
    """-> (cent_off on the device, int32 [B+1]; the host total): what both entries take as `cent`.  One copy of a few hundred bytes;
    callers that run the same sizes again keep the pair (the pipelines cache it on the plan)."""
    import torch
    off = centre_offsets(sizes, step)
    return torch.from_numpy(off).to(device, non_blocking=True), int(off[-1])


def slic_superpixels(hwc_u8, step, compactness=DEFAULTS["compactness"], iters=DEFAULTS["iters"], plan=None, cent=None, out=None):
    """excel_slic_superpixels -> (sp int32, centres int32 [total,5], (cent_off, total)) on the device.  plan=None: uniform [B,H,W,3] uint8
    images, sp is [B,H,W]; with an ops.RaggedPlan: the decoded images back to back (a flat uint8 tensor of 3 * total_label_pix, which may
    start at any byte), sp is flat like the plan's label maps.  cent = (cent_off, total) of an earlier call with the same sizes and step
    (centre_table), or None to compute it.  out = (sp, centres) buffers to fill instead of fresh ones.  2 * iters + 2 launches on the
    current stream, no workspace, no synchronisation."""
    import torch
    from .. import ops
    step, compactness, iters = check_params(step, compactness, iters)
    img = hwc_u8.contiguous()
    if img.dtype != torch.uint8:
        raise ValueError(f"slic_superpixels: the images must be uint8 (got {img.dtype})")
    B, H, W, sizes = _sizes(img, plan, "slic_superpixels", 3)
    cent_off, total = centre_table(sizes, step, img.device) if cent is None else cent
    n = img.numel() // 3
    if out is None:
        sp = torch.empty((B, H, W) if plan is None else (n,), dtype=torch.int32, device=img.device)
        centres = torch.empty((total, 5), dtype=torch.int32, device=img.device)
    else:
        sp, centres = out
        if sp.dtype != torch.int32 or sp.numel() != n or not sp.is_contiguous():
            raise ValueError(f"slic_superpixels: out sp must hold {n} contiguous int32 (got {sp.numel()} {sp.dtype})")
        if centres.dtype != torch.int32 or centres.numel() != 5 * total or not centres.is_contiguous():
            raise ValueError(f"slic_superpixels: out centres must hold {5 * total} contiguous int32 (got {centres.numel()} {centres.dtype})")
        centres = centres.view(total, 5)
    ops.check(ops.lib().excel_slic_superpixels(
        ops._p(img, torch.uint8), B, H, W, ops._p(plan.table, torch.int32) if plan is not None else None,
        C.byref(plan.info) if plan is not None else None, ops._p(cent_off, torch.int32), total, step, compactness, iters,
        ops._p(sp, torch.int32), ops._p(centres, torch.int32), ops._stream()), "excel_slic_superpixels")
    return sp, centres, (cent_off, total)


def snap_labels(labels_u8, sp, step, num_classes, min_share=DEFAULTS["min_share"], plan=None, cent=None, out=None):
    """excel_snap_labels_to_superpixels -> (snapped uint8 shaped like labels_u8, counts int32 [B,3]) on the device.  sp, step and cent are
    those of slic_superpixels on the same batch; min_share: share_rule.  out = (snapped, counts) buffers to fill instead of fresh ones;
    the snapped map may not be the input.  A copy, a clearing and one launch on the current stream, no workspace, no synchronisation."""
    import torch
    from .. import ops
    step = _int_in(step, MIN_STEP, MAX_STEP, "snap_superpixels (the grid step)")
    pm = share_rule(min_share)
    nc = int(num_classes)
    if not 1 <= nc <= 255:
        raise ValueError(f"snap_labels: num_classes = {nc} is outside [1, 255] (255 never votes)")
    lab = labels_u8.contiguous()
    if lab.dtype != torch.uint8:
        raise ValueError(f"snap_labels: labels must be uint8 (got {lab.dtype})")
    B, H, W, sizes = _sizes(lab, plan, "snap_labels")
    spc = sp.contiguous()
    if spc.dtype != torch.int32 or spc.numel() != lab.numel() or spc.device != lab.device:
        raise ValueError(f"snap_labels: sp must hold {lab.numel()} int32 on {lab.device} (got {spc.numel()} {spc.dtype} on {spc.device})")
    cent_off, total = centre_table(sizes, step, lab.device) if cent is None else cent
    if out is None:
        snapped = torch.empty(lab.shape, dtype=torch.uint8, device=lab.device)
        counts = torch.empty((B, 3), dtype=torch.int32, device=lab.device)
    else:
        snapped, counts = out
        if snapped.dtype != torch.uint8 or snapped.numel() != lab.numel() or not snapped.is_contiguous():
            raise ValueError(f"snap_labels: out map must hold {lab.numel()} contiguous uint8 (got {snapped.numel()} {snapped.dtype})")
        if counts.dtype != torch.int32 or counts.numel() != 3 * B or not counts.is_contiguous():
            raise ValueError(f"snap_labels: out counts must hold {3 * B} contiguous int32 (got {counts.numel()} {counts.dtype})")
        counts = counts.view(B, 3)
    ops.check(ops.lib().excel_snap_labels_to_superpixels(
        ops._p(lab, torch.uint8), ops._p(spc, torch.int32), B, H, W, ops._p(plan.table, torch.int32) if plan is not None else None,
        C.byref(plan.info) if plan is not None else None, ops._p(cent_off, torch.int32), total, step, nc, pm,
        ops._p(snapped, torch.uint8), ops._p(counts, torch.int32), ops._stream()), "excel_snap_labels_to_superpixels")
    return snapped, counts


# ------------------------------------------------------------------ the same contracts in numpy
def _assign_numpy(img, cen, S, m, gy, gx):
    H, W = img.shape[:2]
    ys, xs = np.mgrid[0:H, 0:W].astype(np.int64)
    py, px = ys // S, xs // S
    best = np.full((H, W), np.iinfo(np.int64).max, np.int64)
    sp = np.full((H, W), -1, np.int64)
    for dy in (-1, 0, 1):                                     # ascending k: a strictly smaller D replaces, so a tie keeps the smaller k
        for dx in (-1, 0, 1):
            cy, cx = py + dy, px + dx
            ok = (cy >= 0) & (cy < gy) & (cx >= 0) & (cx < gx)
            k = np.where(ok, cy * gx + cx, 0)
            c = cen[k]                                        # [H,W,5]
            D = S * S * ((img - c[..., 2:]) ** 2).sum(-1) + m * m * ((xs - c[..., 0]) ** 2 + (ys - c[..., 1]) ** 2)
            take = ok & (D < best)
            best[take] = D[take]
            sp[take] = k[take]
    return sp


def slic_numpy(image, step, compactness=DEFAULTS["compactness"], iters=DEFAULTS["iters"]):
    """One [H,W,3] uint8 image -> (sp int32 [H,W], centres int32 [gy * gx, 5]): slic_superpixels' contract, every pixel at once."""
    S, m, T = check_params(step, compactness, iters)
    img = np.ascontiguousarray(image)
    if img.ndim != 3 or img.shape[2] != 3 or img.size == 0 or img.dtype != np.uint8:
        raise ValueError(f"slic_numpy: need one non-empty [H,W,3] uint8 image (got {img.shape} {img.dtype})")
    H, W = img.shape[:2]
    img = img.astype(np.int64)
    gy, gx = grid_of(H, W, S)
    K = gy * gx
    cy, cx = np.divmod(np.arange(K, dtype=np.int64), gx)
    x0, y0 = np.minimum(W - 1, cx * S + S // 2), np.minimum(H - 1, cy * S + S // 2)
    cen = np.concatenate([x0[:, None], y0[:, None], img[y0, x0]], axis=1)
    ys, xs = np.mgrid[0:H, 0:W].astype(np.int64)
    feats = np.concatenate([xs.reshape(-1, 1), ys.reshape(-1, 1), img.reshape(-1, 3)], axis=1)       # [HW,5]
    for _ in range(T):
        sp = _assign_numpy(img, cen, S, m, gy, gx).reshape(-1)
        cnt = np.bincount(sp, minlength=K).astype(np.int64)
        sums = np.zeros((K, 5), np.int64)
        np.add.at(sums, sp, feats)
        has = cnt > 0
        cen = cen.copy()
        cen[has] = (2 * sums[has] + cnt[has, None]) // (2 * cnt[has, None])
    return _assign_numpy(img, cen, S, m, gy, gx).astype(np.int32), cen.astype(np.int32)


def snap_numpy(label, sp, num_centres, num_classes, min_share=DEFAULTS["min_share"]):
    """One [H,W] uint8 map and its sp -> (snapped uint8 [H,W], counts int64 [3]): snap_labels' contract.  Pixels with sp < 0 keep their
    label and belong to no superpixel."""
    pm = share_rule(min_share)
    nc = int(num_classes)
    if not 1 <= nc <= 255:
        raise ValueError(f"snap_numpy: num_classes = {nc} is outside [1, 255] (255 never votes)")
    lab = np.ascontiguousarray(label).astype(np.uint8)
    s = np.asarray(sp, np.int64)
    if lab.ndim != 2 or s.shape != lab.shape:
        raise ValueError(f"snap_numpy: the map is {lab.shape}, sp {s.shape}")
    K = int(num_centres)
    votes = (lab < nc) & (s >= 0) & (s < K)
    hist = np.bincount(s[votes] * 256 + lab[votes].astype(np.int64), minlength=K * 256).reshape(K, 256)
    tot, top, win = hist.sum(1), hist.max(1), hist.argmax(1)  # argmax: the first, i.e. the smallest class among equals
    snapped = (tot > 0) & (1000 * top >= pm * tot)
    out = lab.copy()
    hit = votes.copy()
    hit[votes] = snapped[s[votes]]
    out[hit] = win[s[hit]].astype(np.uint8)
    return out, np.asarray([int((tot > 0).sum()), int(snapped.sum()), int((out != lab).sum())], np.int64)


def snap_batch_numpy(images, labels, step, num_classes, compactness=DEFAULTS["compactness"], iters=DEFAULTS["iters"],
                     min_share=DEFAULTS["min_share"], cent_off=None, cent_total=None):
    """Lists of [H,W,3] images and [H,W] maps -> list of (sp, centres, snapped, counts) per image: both entries on a batch.  cent_off:
    None for the rule's own offsets (centre_offsets), or a caller's [B+1] array with its total (default: the last entry): an image whose
    row is wrong - a negative start, an end beyond the total, a difference other than gy * gx - is refused like the kernels refuse it: sp = -1, centres None, the
    labels unchanged, counts 0."""
    hws = [im.shape[:2] for im in images]
    off = centre_offsets(hws, step) if cent_off is None else np.asarray(cent_off, np.int64)
    total = int(off[-1]) if cent_total is None else int(cent_total)
    res = []
    for b, (im, lab) in enumerate(zip(images, labels)):
        gy, gx = grid_of(im.shape[0], im.shape[1], step)
        if off[b] < 0 or off[b + 1] > total or off[b + 1] - off[b] != gy * gx:
            res.append((np.full(im.shape[:2], -1, np.int32), None, np.array(lab, np.uint8), np.zeros(3, np.int64)))
            continue
        sp, cen = slic_numpy(im, step, compactness, iters)
        out, cnt = snap_numpy(lab, sp, gy * gx, num_classes, min_share)
        res.append((sp, cen, out, cnt))
    return res


# ------------------------------------------------------------------ what the programs report
def snap_stats(counts, pixels=None):
    """[N,3] count rows -> dict of the totals: images, superpixels with a vote, superpixels snapped, pixels changed (and, with the
    pixel total, the share of pixels changed)."""
    c = np.asarray(counts, np.int64).reshape(-1, 3)
    stats = dict(images=int(c.shape[0]), superpixels=int(c[:, 0].sum()), snapped=int(c[:, 1].sum()), changed=int(c[:, 2].sum()))
    if pixels is not None:
        stats["pixels"] = int(pixels)
    return stats


def format_snap_summary(stats, cover=None):
    """The summary line of the log: superpixels with a vote, snapped, pixels changed with their share and (with ground truth) coverage."""
    line = f"snap superpixels with a vote: {stats['superpixels']}, snapped: {stats['snapped']}, pixels changed: {stats['changed']}"
    if stats.get("pixels"):
        line += f" ({100.0 * stats['changed'] / stats['pixels']:.3f} % of {stats['pixels']})"
    line += f" over {stats['images']} images"
    if cover is not None:
        line += f"; snap coverage (kept pixels over labelled pixels): {cover * 100:.3f} %"
    return line


def snap_json(snap, stats, score=None, cover=None):
    """The `snap` block of --json_out.  snap: the resolved flags (step, compactness, iters, min_share)."""
    nn = lambda x: None if x is None or x != x else float(x)
    block = dict(step=int(snap["step"]), compactness=int(snap["compactness"]), iters=int(snap["iters"]), min_share=float(snap["min_share"]),
                 images=stats["images"], superpixels=stats["superpixels"], snapped=stats["snapped"], changed=stats["changed"])
    if stats.get("pixels"):
        block.update(pixels=stats["pixels"], changed_share=stats["changed"] / stats["pixels"])
    if score is not None:
        block.update(miou=nn(score["miou"]), pAcc=nn(score["pAcc"]), coverage=nn(cover))
    return block


# ------------------------------------------------------------------ the programs' flags (tools/infer_lam.py, tools/eval_labels.py)
def add_flags(parser):
    parser.add_argument("--snap_superpixels", default=0, type=int,
                        help=f"snap the label maps to superpixels of this grid step, {MIN_STEP}..{MAX_STEP} pixels: every superpixel (integer SLIC "
                             "on the image) takes the majority class of the labels inside it (0: off - no launch, no output)")
    parser.add_argument("--snap_compactness", default=DEFAULTS["compactness"], type=int,
                        help=f"weight of the spatial term of the superpixels, 1..{MAX_COMPACTNESS} (larger: squarer superpixels)")
    parser.add_argument("--snap_iters", default=DEFAULTS["iters"], type=int, help=f"update iterations of the superpixels, 0..{MAX_ITERS}")
    parser.add_argument("--snap_min_share", default=DEFAULTS["min_share"], type=float,
                        help="snap a superpixel only if its majority class holds at least this fraction of its votes, 0..1")
    parser.add_argument("--snap_label_dir", default=None, type=str, help="write the snapped label maps here as palette PNGs")


def resolve(args, program="infer_lam"):
    """The five flags -> dict(step=, compactness=, iters=, min_share=, label_dir=) or None (off), checked before anything is built; the
    refusals name the flag that excludes them."""
    step = getattr(args, "snap_superpixels", 0)
    rest = {k: getattr(args, "snap_" + k, v) for k, v in DEFAULTS.items()}
    out_dir = getattr(args, "snap_label_dir", None)
    if step is None or (not isinstance(step, bool) and isinstance(step, (int, np.integer)) and int(step) == 0):
        if out_dir is not None:
            raise ValueError("--snap_label_dir needs --snap_superpixels: there are no snapped maps to write")
        for k, v in DEFAULTS.items():
            if rest[k] != v:
                raise ValueError(f"--snap_{k} needs --snap_superpixels: nothing is snapped")
        return None
    try:
        step, compactness, iters = check_params(step, rest["compactness"], rest["iters"])
        share_rule(rest["min_share"])
    except ValueError as e:
        raise ValueError(f"--{e}")
    if program == "infer_lam":
        if getattr(args, "api_path", False):
            raise ValueError("--snap_superpixels runs on the batched loop: --api_path true is the reference's per-image call sequence, "
                             "which has no snap")
        if getattr(args, "unlabeled", False) and out_dir is None:
            raise ValueError("--snap_superpixels with --unlabeled true scores nothing: give --snap_label_dir, the snapped maps are its only output")
    return dict(step=step, compactness=compactness, iters=iters, min_share=float(rest["min_share"]), label_dir=out_dir)
