"""--clean_min_region: relabel every connected region of a pseudo-label map below a minimum size as ignore (255).

The arg-max over PAR's output leaves islands of a few pixels and pin-holes of background inside objects.  Two device entries
(csrc/components.hip; include/excel_hip.h, "connected components") remove them without a round trip through the host:

    label_components       comp[i] = the image-local index of the first pixel, in raster order, of i's component; area[i] = its size.
                           Two pixels are connected when they are 4- or 8-neighbours and hold the same raw value
    filter_small_regions   out = 255 where labels < num_classes and area < min_area (a region of exactly min_area pixels stays);
                           counts[b] = (components with a class value, those removed, pixels set to 255)
    components_numpy, clean_numpy   the same contracts in numpy (no scipy): what tools/eval_labels uses without a GPU, and the judge of
                           the GPU tests
    min_area_rule          the flag's value -> pixels: an integer >= 1 is pixels, a fraction in (0, 1) is a share of the image's area
    clean_json, format_clean_summary, add_flags, resolve   what the programs report, their flags and refusals

Filling what was removed with the nearest class instead of leaving 255 is utils/label_fill.py (--fill_ignore), the step behind this one.
Not done here, on purpose: an ignore band along the contours; a sweep over several minimum sizes in one run (the API allows it: one
label_components, one filter_small_regions per size); the `conf` and `crf` label sets of infer_lam (their PNGs can go through eval_labels
--clean_min_region and --fill_ignore).  Whether the score on the kept pixels improves on real data is unmeasured: no real checkpoint or
data set is available to this project.
"""
import ctypes as C

import numpy as np

COMPONENTS_TILE = (16, 64)          # (TH, TW) of cc_tile_kernel: one workgroup labels one tile in LDS, the seams are merged afterwards
IGNORE = 255


# ------------------------------------------------------------------ the threshold
def min_area_rule(value, H, W):
    """--clean_min_region VALUE for an H x W image -> pixels (int >= 1).  A value >= 1 has to be an integer and means pixels; 0 < value
    < 1 is a fraction of the image's area, max(1, int(round(value * H * W))) (Python's round: a tie goes to the even integer).  Anything
    else - 0, a negative, 1.5, NaN, a string - is a ValueError: the device receives integers only."""
    if isinstance(value, bool) or not isinstance(value, (int, float, np.integer, np.floating)):
        raise ValueError(f"clean_min_region: {value!r} is not a number")
    v = float(value)
    if v >= 1.0:
        if v >= 2 ** 31 or v != int(v):
            raise ValueError(f"clean_min_region: {value!r}: a value >= 1 is a number of pixels and has to be an integer below 2^31")
        return int(v)
    if 0.0 < v < 1.0:
        return max(1, int(round(v * (int(H) * int(W)))))
    raise ValueError(f"clean_min_region: {value!r} must be an integer number of pixels >= 1 or a fraction of the image area in (0, 1)")


def check_connectivity(c):
    if c not in (4, 8) or isinstance(c, bool):
        raise ValueError(f"clean_connectivity: {c!r} must be 4 or 8")
    return int(c)


# ------------------------------------------------------------------ the device ops
def _geometry(labels_u8, plan, who):
    if plan is None:
        if labels_u8.dim() != 3:
            raise ValueError(f"{who}: uniform maps must be [B,H,W] (got {tuple(labels_u8.shape)}); a ragged batch needs its plan")
        B, H, W = (int(x) for x in labels_u8.shape)
    else:
        B, H, W = plan.B, 0, 0
        if labels_u8.numel() != plan.total_label_pix:
            raise ValueError(f"{who}: {labels_u8.numel()} pixels, the plan holds {plan.total_label_pix}")
    if B < 1 or labels_u8.numel() < 1:
        raise ValueError(f"{who}: at least one image with a pixel is needed (got {tuple(labels_u8.shape)})")
    return B, H, W


def label_components(labels_u8, plan=None, connectivity=8, out=None):
    """excel_label_components -> (comp, area), int32 tensors shaped like labels_u8 (device).  plan=None: uniform [B,H,W] maps; with an
    ops.RaggedPlan: its tight label maps back to back (a flat uint8 tensor, which may start at any byte).  out = (comp, area) buffers
    to fill instead of fresh ones.  Four launches behind one clearing on the current stream, no workspace, no synchronisation."""
    import torch
    from .. import ops
    lab = labels_u8.contiguous()
    if lab.dtype != torch.uint8:
        raise ValueError(f"label_components: labels must be uint8 (got {lab.dtype})")
    connectivity = check_connectivity(connectivity)
    B, H, W = _geometry(lab, plan, "label_components")
    if out is None:
        comp = torch.empty(lab.shape, dtype=torch.int32, device=lab.device)
        area = torch.empty(lab.shape, dtype=torch.int32, device=lab.device)
    else:
        comp, area = out
        for name, t in (("comp", comp), ("area", area)):
            if t.dtype != torch.int32 or t.numel() != lab.numel() or not t.is_contiguous():
                raise ValueError(f"label_components: out {name} must hold {lab.numel()} contiguous int32 (got {t.numel()} {t.dtype})")
    ops.check(ops.lib().excel_label_components(
        ops._p(lab, torch.uint8), B, H, W, ops._p(plan.table, torch.int32) if plan is not None else None,
        C.byref(plan.info) if plan is not None else None, connectivity, ops._p(comp, torch.int32), ops._p(area, torch.int32), ops._stream()),
        "excel_label_components")
    return comp, area


def filter_small_regions(labels_u8, comp, area, min_area, num_classes, plan=None, out=None):
    """excel_filter_small_regions -> (cleaned uint8 shaped like labels_u8, counts int32 [B,3]).  min_area: an int (every image), a host
    sequence of B ints (uploaded without a wait) or a device int32 tensor [B].  Host values below 1 are refused here, naming the image;
    an image whose DEVICE value is below 1 gets a counts row of -1 and its map copied unchanged.  out = (cleaned, counts) buffers; the
    cleaned map may not be the input.  One launch behind one clearing on the current stream, no workspace, no synchronisation."""
    import torch
    from .. import ops
    lab = labels_u8.contiguous()
    if lab.dtype != torch.uint8:
        raise ValueError(f"filter_small_regions: labels must be uint8 (got {lab.dtype})")
    B, H, W = _geometry(lab, plan, "filter_small_regions")
    nc = int(num_classes)
    if not 1 <= nc <= 256:
        raise ValueError(f"filter_small_regions: num_classes = {nc} is outside [1, 256]")
    for name, t in (("comp", comp), ("area", area)):
        if t.dtype != torch.int32 or t.numel() != lab.numel() or not t.is_contiguous():
            raise ValueError(f"filter_small_regions: {name} must hold {lab.numel()} contiguous int32 (got {t.numel()} {t.dtype})")
    thr, thr_all = None, 0
    if isinstance(min_area, torch.Tensor):
        if min_area.dtype != torch.int32 or min_area.numel() != B or min_area.device != lab.device:
            raise ValueError(f"filter_small_regions: a min_area tensor must hold {B} int32 on {lab.device} "
                             f"(got {min_area.numel()} {min_area.dtype} on {min_area.device})")
        thr = min_area.contiguous()
    elif np.ndim(min_area) == 0:
        thr_all = int(min_area)
        if thr_all < 1 or thr_all != min_area:
            raise ValueError(f"filter_small_regions: min_area = {min_area!r} must be an integer >= 1 (min_area_rule)")
    else:
        host = np.asarray([int(m) for m in min_area], np.int32)
        if host.shape != (B,):
            raise ValueError(f"filter_small_regions: {host.size} thresholds for {B} images")
        for b in np.nonzero(host < 1)[0]:
            raise ValueError(f"filter_small_regions: image {int(b)} has min_area {int(host[b])}, below 1 (min_area_rule)")
        thr = torch.from_numpy(host).to(lab.device, non_blocking=True)
    if out is None:
        cleaned = torch.empty(lab.shape, dtype=torch.uint8, device=lab.device)
        counts = torch.empty((B, 3), dtype=torch.int32, device=lab.device)
    else:
        cleaned, counts = out
        if cleaned.dtype != torch.uint8 or cleaned.numel() != lab.numel() or not cleaned.is_contiguous():
            raise ValueError(f"filter_small_regions: out map must hold {lab.numel()} contiguous uint8 (got {cleaned.numel()} {cleaned.dtype})")
        if counts.dtype != torch.int32 or counts.numel() != 3 * B or not counts.is_contiguous():
            raise ValueError(f"filter_small_regions: out counts must hold {3 * B} contiguous int32 (got {counts.numel()} {counts.dtype})")
        counts = counts.view(B, 3)
    ops.check(ops.lib().excel_filter_small_regions(
        ops._p(lab, torch.uint8), ops._p(comp, torch.int32), ops._p(area, torch.int32), B, H, W,
        ops._p(plan.table, torch.int32) if plan is not None else None, C.byref(plan.info) if plan is not None else None,
        ops._p(thr, torch.int32), thr_all, nc, ops._p(cleaned, torch.uint8), ops._p(counts, torch.int32), ops._stream()),
        "excel_filter_small_regions")
    return cleaned, counts


# ------------------------------------------------------------------ the same contracts in numpy
def components_numpy(label, connectivity=8):
    """One [H,W] map -> (comp, area) int32 [H,W], label_components' contract.  Union-find over the row runs of the map: runs are
    numbered in raster order of their first pixel, the smaller number always becomes the parent, so a component's root run starts at
    the component's first pixel."""
    connectivity = check_connectivity(connectivity)
    lab = np.ascontiguousarray(label)
    if lab.ndim != 2 or lab.size == 0:
        raise ValueError(f"components_numpy: need one non-empty [H,W] map (got {lab.shape})")
    H, W = lab.shape
    head = np.ones((H, W), bool)
    head[:, 1:] = lab[:, 1:] != lab[:, :-1]
    run_of = np.cumsum(head.reshape(-1)) - 1                                  # run number of every pixel
    start = np.flatnonzero(head.reshape(-1))                                  # linear index of every run's first pixel
    length = np.diff(np.append(start, H * W))
    row, c0 = start // W, start % W
    c1 = c0 + length                                                          # exclusive
    value = lab.reshape(-1)[start]
    first = np.searchsorted(row, np.arange(H + 1))                            # runs of row r: first[r] .. first[r + 1]
    parent = list(range(len(start)))

    def find(x):
        r = x
        while parent[r] != r:
            r = parent[r]
        while parent[x] != r:
            parent[x], x = r, parent[x]
        return r
    d = 1 if connectivity == 8 else 0
    c0l, c1l, vl = c0.tolist(), c1.tolist(), value.tolist()
    for r in range(1, H):
        i, j, ie, je = int(first[r - 1]), int(first[r]), int(first[r]), int(first[r + 1])
        while i < ie and j < je:
            if vl[i] == vl[j] and c0l[i] < c1l[j] + d and c0l[j] < c1l[i] + d:
                a, b = find(i), find(j)
                if a != b:
                    parent[max(a, b)] = min(a, b)
            if c1l[i] < c1l[j]:                                                # the run that ends first cannot touch anything further
                i += 1
            elif c1l[j] < c1l[i]:
                j += 1
            else:                                                              # both end here: with d = 1 each may still touch the other's successor
                if d and i + 1 < ie and vl[i + 1] == vl[j] and c0l[i + 1] < c1l[j] + d:
                    a, b = find(i + 1), find(j)
                    if a != b:
                        parent[max(a, b)] = min(a, b)
                if d and j + 1 < je and vl[j + 1] == vl[i] and c0l[j + 1] < c1l[i] + d:
                    a, b = find(i), find(j + 1)
                    if a != b:
                        parent[max(a, b)] = min(a, b)
                i += 1
                j += 1
    root = np.asarray([find(x) for x in range(len(start))], np.int64)
    run_area = np.bincount(root, weights=length, minlength=len(start)).astype(np.int64)
    comp = start[root][run_of].astype(np.int32).reshape(H, W)
    area = run_area[root][run_of].astype(np.int32).reshape(H, W)
    return comp, area


def clean_numpy(label, min_area, num_classes, connectivity=8):
    """One [H,W] uint8 map -> (cleaned uint8 [H,W], counts int64 [3]): filter_small_regions(label_components(...)) restated exactly.
    min_area: pixels, an integer >= 1 (min_area_rule)."""
    if int(min_area) != min_area or int(min_area) < 1:
        raise ValueError(f"clean_numpy: min_area = {min_area!r} must be an integer >= 1 (min_area_rule)")
    lab = np.ascontiguousarray(label).astype(np.uint8)
    comp, area = components_numpy(lab, connectivity)
    H, W = lab.shape
    cls = lab < int(num_classes)
    gone = cls & (area < int(min_area))
    rootpix = comp == np.arange(H * W, dtype=np.int64).reshape(H, W)
    out = lab.copy()
    out[gone] = IGNORE
    return out, np.asarray([int((cls & rootpix).sum()), int((gone & rootpix).sum()), int(gone.sum())], np.int64)


# ------------------------------------------------------------------ what the programs report
def coverage(kept_hist, plain_hist):
    """Kept pixels over labelled pixels: both confusion matrices count the pixels with a valid ground truth and a class label, so their
    sums are the scored pixels after and before the cleaning.  NaN when nothing was labelled."""
    k = float(np.asarray(kept_hist.detach().cpu().numpy() if hasattr(kept_hist, "detach") else kept_hist, np.float64).sum())
    p = float(np.asarray(plain_hist.detach().cpu().numpy() if hasattr(plain_hist, "detach") else plain_hist, np.float64).sum())
    return k / p if p > 0 else float("nan")


def region_stats(counts):
    """[N,3] count rows (refused rows of -1 left out) -> dict of the totals and the per-image mean / max of regions and regions removed."""
    c = np.asarray(counts, np.int64).reshape(-1, 3)
    c = c[(c >= 0).all(1)]
    if c.shape[0] == 0:
        return dict(images=0, regions_mean=float("nan"), regions_max=0, removed_mean=float("nan"), removed_max=0, pixels_removed=0)
    return dict(images=int(c.shape[0]), regions_mean=float(c[:, 0].mean()), regions_max=int(c[:, 0].max()),
                removed_mean=float(c[:, 1].mean()), removed_max=int(c[:, 1].max()), pixels_removed=int(c[:, 2].sum()))


def format_clean_summary(stats, cover=None):
    """The two summary lines of the log: coverage (when there was ground truth), then regions and regions removed per image."""
    lines = []
    if cover is not None:
        lines.append(f"clean coverage (kept pixels over labelled pixels): {cover * 100:.3f} %")
    lines.append(f"clean regions per image: mean {stats['regions_mean']:.1f}, max {stats['regions_max']}; removed: mean "
                 f"{stats['removed_mean']:.1f}, max {stats['removed_max']}; pixels set to {IGNORE}: {stats['pixels_removed']} "
                 f"over {stats['images']} images")
    return "\n".join(lines)


def clean_json(min_region, connectivity, stats, score=None, cover=None):
    """The `clean` block of --json_out."""
    nn = lambda x: None if x is None or x != x else float(x)
    block = dict(min_region=float(min_region), connectivity=int(connectivity), images=stats["images"], regions_mean=nn(stats["regions_mean"]),
                 regions_max=stats["regions_max"], regions_removed_mean=nn(stats["removed_mean"]), regions_removed_max=stats["removed_max"],
                 pixels_removed=stats["pixels_removed"])
    if score is not None:
        block.update(miou=nn(score["miou"]), pAcc=nn(score["pAcc"]), coverage=nn(cover))
    return block


# ------------------------------------------------------------------ the programs' flags (tools/infer_lam.py, tools/eval_labels.py)
def _flag_value(text):
    try:
        v = float(text)
    except ValueError:
        raise ValueError(f"--clean_min_region: {text!r} is not a number (pixels, e.g. 64, or a fraction of the image area, e.g. 0.001)")
    return int(v) if v >= 1 and v == int(v) else v


def add_flags(parser):
    parser.add_argument("--clean_min_region", default=None, type=str,
                        help="relabel every connected region of the label maps below this size as 255: an integer >= 1 is pixels, a value in "
                             "(0, 1) a fraction of the image area (absent: off - no launch, no output)")
    parser.add_argument("--clean_connectivity", default=8, type=int, help="neighbourhood of a region: 8 (default) or 4")
    parser.add_argument("--clean_label_dir", default=None, type=str, help="write the cleaned label maps here as palette PNGs")


def resolve(args, program="infer_lam"):
    """The three flags -> dict(min_region=, connectivity=, label_dir=) or None (off), checked before anything is built; the refusals
    name the flag that excludes them."""
    raw = getattr(args, "clean_min_region", None)
    conn = getattr(args, "clean_connectivity", 8)
    out_dir = getattr(args, "clean_label_dir", None)
    if raw is None:
        if out_dir is not None:
            raise ValueError("--clean_label_dir needs --clean_min_region: there are no cleaned maps to write")
        if conn != 8:
            raise ValueError("--clean_connectivity needs --clean_min_region: nothing is cleaned")
        return None
    value = _flag_value(raw) if isinstance(raw, str) else raw
    min_area_rule(value, 1, 1)                                 # the value itself: image sizes come later
    try:
        conn = check_connectivity(conn)
    except ValueError as e:
        raise ValueError(f"--{e}")
    if program == "infer_lam":
        if getattr(args, "api_path", False):
            raise ValueError("--clean_min_region runs on the batched loop: --api_path true is the reference's per-image call sequence, "
                             "which has no cleaning")
        if getattr(args, "unlabeled", False) and out_dir is None:
            raise ValueError("--clean_min_region with --unlabeled true scores nothing: give --clean_label_dir, the cleaned maps are its only output")
    return dict(min_region=value, connectivity=conn, label_dir=out_dir)
