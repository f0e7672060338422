"""Score a directory of label PNGs against the ground truth - mirror of tools/infer_seg_coco_from_crf_pred.py:39-76 (validate_from_png).

    python -m excel_amd.tools.eval_labels --pred_dir DIR --data_folder VOC2012/ --list_folder lists/ --infer_set train_aug

reads `<pred_dir>/<name>.png` (what `infer_lam --save_label true` writes, or any palette / grey label PNG) and the ground truth
(`<data_folder>/SegmentationClassAug/<name>.png`; with --dataset_name ms_coco `<data_folder>/SegmentationClass/<infer_set>/<name[13:]>.png`,
:61), accumulates the [nc,nc] confusion matrix and prints the table infer_lam prints.  Differences from the reference, as in infer_lam:
the files are decoded in a thread pool, the matrix is accumulated on the device (ops.confusion_accumulate), ranks take names r, r+R, ...
and exchange their matrices once.  Without a GPU the matrix is computed with numpy (np.bincount, the arithmetic of utils/evaluate.py:9-20):
file handling is the point of this program, not compute.  A missing prediction and a prediction whose size differs from the ground truth
are errors that name the file.  `--per_image_scores PATH` also writes every image's own scores (utils/image_scores.py: a CSV in list
order and PATH.npz with the per-class counts; ops.image_scores on the device, np.bincount without one).  `--boundary_scores true` adds
the Boundary IoU of the directory (a boundary_score table in the log, extra columns and arrays in --per_image_scores' files):
ops.boundary_scores on the device, image_scores.boundary_counts_numpy without one.  `--clean_min_region VALUE` (with --clean_connectivity
8|4) cleans the maps of --pred_dir first - every connected class region below VALUE (pixels, or a fraction of the image area) becomes 255:
utils/components.label_components + filter_small_regions on the device, components.clean_numpy without one -, scores the cleaned maps as
a second table (clean_label_score, with the coverage and the region counts) and, with `--clean_label_dir DIR`, writes them there as
palette PNGs.  The first table is unchanged.  This is the route for CRF labels and for labels from elsewhere.  `--fill_ignore inf|PIXELS`
gives 255 pixels the value of the nearest class pixel of their image (utils/label_fill.fill_nearest_label on the device, fill_numpy
without one; exact squared Euclidean distance, ties to the first pixel in raster order, at most PIXELS away): with --clean_min_region
the pixels the cleaning removed (the map before the cleaning is the mask: a 255 it already had stays), without it every 255 of the
predictions.  The filled maps are scored as one more table (fill_label_score, with holes, filled, largest distance and coverage) and,
with `--fill_label_dir DIR`, written there.  Same tables and files with and without a GPU.  `--snap_superpixels STEP` (with
--snap_compactness, --snap_iters, --snap_min_share, --snap_label_dir) snaps the maps of --pred_dir to superpixels of their images first:
it reads `<data_folder>/JPEGImages/<name>.jpg` (a missing image, or one whose size differs from the label map, is an error that names the
file), over-segments it (utils/superpixels.slic_superpixels on the device, slic_numpy without one) and gives every superpixel the
majority class of the labels inside it; the snapped maps are scored as one more table (snap_label_score, with the superpixels, the
snapped ones and the pixels changed) and written to --snap_label_dir.  With it the cleaning and the fill work on the snapped maps
(snap -> clean -> fill).
"""
import argparse
import concurrent.futures as cf
import logging
import os
import time

import numpy as np
import torch

from .infer_lam import VOC_CLASSES, format_scores_table, gather_hists, shard_indices


def get_parser():
    p = argparse.ArgumentParser()
    p.add_argument("--pred_dir", required=True, type=str, help="directory of <name>.png label maps")
    p.add_argument("--data_folder", required=True, type=str, help="VOC2012 root (SegmentationClassAug/) or COCO root (SegmentationClass/<split>/)")
    p.add_argument("--list_folder", required=True, type=str, help="directory with <infer_set>.txt")
    p.add_argument("--infer_set", default="train_aug", type=str)
    p.add_argument("--dataset_name", default="pascal_voc", choices=["pascal_voc", "ms_coco"])
    p.add_argument("--num_classes", default=None, type=int, help="default: 21 (pascal_voc) / 81 (ms_coco), or the lines of --class_names + 1; at most 256")
    p.add_argument("--class_names", default=None, type=str, help="one foreground class name per line: the rows of the table (infer_lam --class_names)")
    p.add_argument("--num_workers", default=8, type=int, help="PNG decode threads")
    p.add_argument("--batch_size", default=64, type=int, help="images decoded per device accumulation")
    from ..utils import image_scores
    image_scores.add_flags(p)
    image_scores.add_boundary_flags(p)
    from ..utils import components
    components.add_flags(p)
    from ..utils import label_fill
    label_fill.add_flags(p)
    from ..utils import superpixels
    superpixels.add_flags(p)
    p.add_argument("--local_rank", default=int(os.environ.get("LOCAL_RANK", 0)), type=int)
    p.add_argument("--backend", default="nccl")
    return p


def label_paths(args, name):
    """(prediction, ground truth) of one list entry (infer_seg_coco_from_crf_pred.py:59-61)."""
    if "coco" in args.dataset_name:
        gt = os.path.join(args.data_folder, "SegmentationClass", args.infer_set, name[13:] + ".png")
    else:
        gt = os.path.join(args.data_folder, "SegmentationClassAug", name + ".png")
    return os.path.join(args.pred_dir, name + ".png"), gt


def _load_pair(args, name):
    from PIL import Image
    pred_path, gt_path = label_paths(args, name)
    if not os.path.isfile(pred_path):
        raise FileNotFoundError(f"eval_labels: no prediction for {name!r}: {pred_path} is missing")
    gt = np.asarray(Image.open(gt_path))
    pred = np.asarray(Image.open(pred_path))
    if pred.shape != gt.shape or pred.ndim != 2:
        raise ValueError(f"eval_labels: {pred_path} is {pred.shape}, the ground truth {gt_path} is {gt.shape}")
    return np.ascontiguousarray(gt, np.uint8).reshape(-1), np.ascontiguousarray(pred, np.uint8).reshape(-1), gt.shape


def _load_image(args, name, hw):
    """The decoded uint8 [H,W,3] image of one list entry, <data_folder>/JPEGImages/<name>.jpg, for --snap_superpixels."""
    from PIL import Image
    path = os.path.join(args.data_folder, "JPEGImages", name + ".jpg")
    if not os.path.isfile(path):
        raise FileNotFoundError(f"eval_labels: --snap_superpixels needs the image of {name!r}: {path} is missing")
    img = np.ascontiguousarray(np.asarray(Image.open(path).convert("RGB")), np.uint8)
    if img.shape[:2] != tuple(hw):
        raise ValueError(f"eval_labels: {path} is {img.shape[:2]}, the label map of {name!r} is {tuple(hw)}")
    return img


def _save_index_png(path, label):
    """One [H,W] uint8 map as a palette PNG (the VOC colour map; index 255 is the ignore colour)."""
    from PIL import Image
    from ..utils.imutils import colormap
    im = Image.fromarray(np.ascontiguousarray(label, np.uint8))          # mode L; the palette makes it P with the same indices
    im.putpalette(np.asarray(colormap(256), np.uint8).reshape(-1).tolist())
    im.save(path)


def _hist_numpy(gt, pred, nc):
    """_fast_hist (utils/evaluate.py:9-20): rows = ground truth, columns = prediction, labels >= nc (255 = ignore) dropped."""
    gt, pred = gt.astype(np.int64), pred.astype(np.int64)
    m = (gt < nc) & (pred < nc)
    return np.bincount(nc * gt[m] + pred[m], minlength=nc * nc).reshape(nc, nc)


def validate(args):
    """-> {"score": scores_from_hist of the gathered matrix, "hist": [nc,nc] int64 (CPU tensor), "images": scored on this rank,
    "seconds"}: the layout of infer_seg_voc.validate (+ "image_scores" with --per_image_scores)."""
    from ..utils import components, evaluate, image_scores, label_fill, superpixels
    image_scores.refuse(args)
    clean = components.resolve(args, program="eval_labels")
    fill = label_fill.resolve(args, program="eval_labels")
    snap = superpixels.resolve(args, program="eval_labels")
    names_fg = None
    if getattr(args, "class_names", None):
        from .infer_lam import _read_names
        names_fg = _read_names(args.class_names, "--class_names")
        if args.num_classes and args.num_classes != len(names_fg) + 1:
            raise ValueError(f"--num_classes {args.num_classes} contradicts --class_names: {len(names_fg)} names + background")
    nc = args.num_classes or (len(names_fg) + 1 if names_fg else (81 if "coco" in args.dataset_name else 21))
    if not 1 <= nc <= 256:
        raise ValueError(f"--num_classes {nc}: uint8 label maps hold at most 256 classes")
    if snap is not None and nc > 255:
        raise ValueError(f"--snap_superpixels: --num_classes {nc} leaves no value that does not vote (at most 255)")
    world, rank = int(os.environ.get("WORLD_SIZE", 1)), int(os.environ.get("RANK", 0))
    on_gpu = torch.cuda.is_available()
    device = torch.device("cuda", args.local_rank) if on_gpu else torch.device("cpu")
    if on_gpu:
        torch.cuda.set_device(args.local_rank)
    if world > 1 and not torch.distributed.is_initialized():
        torch.distributed.init_process_group(backend=args.backend if on_gpu else "gloo")
    with open(os.path.join(args.list_folder, args.infer_set) + ".txt") as f:
        names = [x.split()[0] for x in f.read().split("\n") if x.strip()]
    idx = shard_indices(len(names), rank, world)
    mine = [names[i] for i in idx]
    boundary = image_scores.boundary_of(args)
    scores = image_scores.ImageScoreLog(nc, boundary=boundary) if image_scores.wanted(args) else None
    hist = torch.zeros((nc, nc), dtype=torch.int64, device=device)
    hist_clean, clean_rows = (torch.zeros_like(hist) if clean is not None else None), []
    if clean is not None and clean["label_dir"]:
        os.makedirs(clean["label_dir"], exist_ok=True)
    hist_fill, fill_rows = (torch.zeros_like(hist) if fill is not None else None), []
    hist_snap, snap_rows, snap_pixels = (torch.zeros_like(hist) if snap is not None else None), [], 0
    if snap is not None and snap["label_dir"]:
        os.makedirs(snap["label_dir"], exist_ok=True)
    if fill is not None and fill["label_dir"]:
        os.makedirs(fill["label_dir"], exist_ok=True)
    t0 = time.time()
    with cf.ThreadPoolExecutor(max_workers=max(1, int(args.num_workers))) as pool:
        for s in range(0, len(mine), args.batch_size):
            pairs = list(pool.map(lambda n: _load_pair(args, n), mine[s:s + args.batch_size]))       # raises the first error, in order
            gt = np.concatenate([p[0] for p in pairs])
            pred = np.concatenate([p[1] for p in pairs])
            hws = [p[2] for p in pairs]
            if on_gpu:
                from .. import ops
                gt_d, pred_d = torch.from_numpy(gt).to(device), torch.from_numpy(pred).to(device)
                hist = ops.confusion_accumulate(gt_d, pred_d, nc, hist)
                if scores is not None:                                                           # the batch as one ragged plan, behind a ticket
                    from ..pipeline import ScoreTicket
                    hws = [p[2] for p in pairs]
                    scores.defer(ScoreTicket().launch("main", gt_d, pred_d, nc, plan=ops.RaggedPlan(hws, device), boundary=boundary), idx[s:s + len(pairs)],
                                 mine[s:s + len(pairs)], hws)
            else:
                hist += torch.from_numpy(_hist_numpy(gt, pred, nc))
                if scores is not None:
                    for j, p in enumerate(pairs):
                        scores.put(idx[s + j], mine[s + j], p[2], "main", image_scores.counts_numpy(p[0], p[1], nc))
                        if boundary is not None:
                            scores.put(idx[s + j], mine[s + j], p[2], "main_bd", image_scores.boundary_counts_numpy(
                                p[0].reshape(p[2]), p[1].reshape(p[2]), nc, image_scores.checked_radius(mine[s + j], p[2][0], p[2][1], boundary)))
            src, src_d = pred, (pred_d if on_gpu else None)      # what the cleaning and the fill work on: the predictions, or the snapped maps
            if snap is not None:                                 # the snapped maps of the batch: the images decoded, segmented, voted on
                imgs = list(pool.map(lambda nh: _load_image(args, *nh), zip(mine[s:s + len(pairs)], hws)))
                if on_gpu:
                    plan = ops.RaggedPlan(hws, device)
                    hwc_d = torch.from_numpy(np.concatenate([im.reshape(-1) for im in imgs])).to(device)
                    sp_d, _, cent = superpixels.slic_superpixels(hwc_d, snap["step"], snap["compactness"], snap["iters"], plan=plan)
                    src_d, counts_d = superpixels.snap_labels(pred_d, sp_d, snap["step"], nc, snap["min_share"], plan=plan, cent=cent)
                    hist_snap = ops.confusion_accumulate(gt_d, src_d, nc, hist_snap)
                    src, counts = src_d.cpu().numpy(), counts_d.cpu().numpy()
                else:
                    done = superpixels.snap_batch_numpy(imgs, [p[1].reshape(p[2]) for p in pairs], snap["step"], nc, snap["compactness"],
                                                        snap["iters"], snap["min_share"])
                    src = np.concatenate([d[2].reshape(-1) for d in done])
                    counts = np.stack([d[3] for d in done])
                    hist_snap += torch.from_numpy(_hist_numpy(gt, src, nc))
                snap_rows.extend(np.asarray(counts, np.int64).reshape(-1, 3).tolist())
                snap_pixels += int(src.size)
                if snap["label_dir"]:
                    off = 0
                    for n, (h, w) in zip(mine[s:s + len(pairs)], hws):
                        _save_index_png(os.path.join(snap["label_dir"], n + ".png"), src[off:off + h * w].reshape(h, w))
                        off += h * w
            offs = np.concatenate([[0], np.cumsum([h * w for h, w in hws])])
            if clean is not None:                                # the cleaned maps of the batch: scored into a matrix of their own, written
                hws = [p[2] for p in pairs]
                thr = [components.min_area_rule(clean["min_region"], h, w) for h, w in hws]
                if on_gpu:
                    plan = ops.RaggedPlan(hws, device)
                    comp, area = components.label_components(src_d, plan=plan, connectivity=clean["connectivity"])
                    cleaned_d, counts_d = components.filter_small_regions(src_d, comp, area, thr, nc, plan=plan)
                    hist_clean = ops.confusion_accumulate(gt_d, cleaned_d, nc, hist_clean)
                    cleaned, counts = cleaned_d.cpu().numpy(), counts_d.cpu().numpy()
                else:
                    done = [components.clean_numpy(src[offs[j]:offs[j + 1]].reshape(p[2]), t, nc, clean["connectivity"])
                            for j, (p, t) in enumerate(zip(pairs, thr))]
                    cleaned = np.concatenate([d[0].reshape(-1) for d in done])
                    counts = np.stack([d[1] for d in done])
                    hist_clean += torch.from_numpy(_hist_numpy(gt, cleaned, nc))
                clean_rows.extend(np.asarray(counts, np.int64).reshape(-1, 3).tolist())
                if clean["label_dir"]:
                    off = 0
                    for n, (h, w) in zip(mine[s:s + len(pairs)], hws):
                        _save_index_png(os.path.join(clean["label_dir"], n + ".png"), cleaned[off:off + h * w].reshape(h, w))
                        off += h * w
            if fill is not None:                                 # the filled maps: what the cleaning removed, or every 255 of the predictions
                if on_gpu:
                    hole_d, mask_d = (cleaned_d, src_d) if clean is not None else (src_d, None)
                    filled_d, _, counts_d = label_fill.fill_nearest_label(hole_d, nc, plan=ops.RaggedPlan(hws, device), mask=mask_d, radius=fill["radius"])
                    hist_fill = ops.confusion_accumulate(gt_d, filled_d, nc, hist_fill)
                    filled, counts = filled_d.cpu().numpy(), counts_d.cpu().numpy()
                else:
                    hole, off, done = (cleaned if clean is not None else src), 0, []
                    for p in pairs:
                        n_pix = p[2][0] * p[2][1]
                        done.append(label_fill.fill_numpy(hole[off:off + n_pix].reshape(p[2]), nc, radius=fill["radius"],
                                                          mask=src[off:off + n_pix].reshape(p[2]) if clean is not None else None))
                        off += n_pix
                    filled = np.concatenate([d[0].reshape(-1) for d in done])
                    counts = np.stack([d[2] for d in done])
                    hist_fill += torch.from_numpy(_hist_numpy(gt, filled, nc))
                fill_rows.extend(np.asarray(counts, np.int64).reshape(-1, 3).tolist())
                if fill["label_dir"]:
                    off = 0
                    for n, (h, w) in zip(mine[s:s + len(pairs)], hws):
                        _save_index_png(os.path.join(fill["label_dir"], n + ".png"), filled[off:off + h * w].reshape(h, w))
                        off += h * w
    _, total = gather_hists(hist)
    total = total.cpu()
    score = evaluate.scores_from_hist(total)
    secs = time.time() - t0
    cats = VOC_CLASSES
    if "coco" in args.dataset_name:
        from ..datasets import coco
        cats = coco.class_list
    if names_fg:
        cats = [VOC_CLASSES[0]] + names_fg
    if scores is not None:
        merged = image_scores.finish(scores, args, cats, rank)
    if rank == 0:
        logging.info(f"label_score of {args.pred_dir}:")
        logging.info("\n" + format_scores_table(score, cats))
        logging.info(f"mIoU {score['miou'] * 100:.3f}  images {len(names)}  ({len(mine) / max(secs, 1e-9):.1f} img/s/rank)")
    out = {"score": score, "hist": total, "images": len(mine), "seconds": secs}
    if snap is not None:
        _, snap_total = gather_hists(hist_snap)
        snap_total = snap_total.cpu()
        parts = [(snap_rows, snap_pixels)]
        if world > 1:
            parts = [None] * world
            torch.distributed.all_gather_object(parts, (snap_rows, snap_pixels))
        counts = np.asarray([r for part in parts for r in part[0]], np.int64).reshape(-1, 3)
        out["snap"] = dict(score=evaluate.scores_from_hist(snap_total), hist=snap_total, coverage=components.coverage(snap_total, total),
                           counts=counts, stats=superpixels.snap_stats(counts, sum(part[1] for part in parts)),
                           **{k: snap[k] for k in ("step", "compactness", "iters", "min_share")})
        if rank == 0:
            logging.info(f"snap_label_score of {args.pred_dir} (--snap_superpixels {snap['step']}, compactness {snap['compactness']}, "
                         f"{snap['iters']} iterations, min share {snap['min_share']:g}):")
            logging.info("\n" + format_scores_table(out["snap"]["score"], cats))
            logging.info(superpixels.format_snap_summary(out["snap"]["stats"], out["snap"]["coverage"]))
            if snap["label_dir"]:
                logging.info(f"snapped label maps -> {snap['label_dir']}")
    if clean is not None:
        _, clean_total = gather_hists(hist_clean)
        clean_total = clean_total.cpu()
        parts = [clean_rows]
        if world > 1:
            parts = [None] * world
            torch.distributed.all_gather_object(parts, clean_rows)
        counts = np.asarray([r for part in parts for r in part], np.int64).reshape(-1, 3)
        out["clean"] = dict(score=evaluate.scores_from_hist(clean_total), hist=clean_total, coverage=components.coverage(clean_total, total),
                            counts=counts, stats=components.region_stats(counts), min_region=clean["min_region"],
                            connectivity=clean["connectivity"])
        if rank == 0:
            logging.info(f"clean_label_score of {args.pred_dir} (--clean_min_region {clean['min_region']:g}, connectivity {clean['connectivity']}):")
            logging.info("\n" + format_scores_table(out["clean"]["score"], cats))
            logging.info(components.format_clean_summary(out["clean"]["stats"], out["clean"]["coverage"]))
            if clean["label_dir"]:
                logging.info(f"cleaned label maps -> {clean['label_dir']}")
    if fill is not None:
        _, fill_total = gather_hists(hist_fill)
        fill_total = fill_total.cpu()
        parts = [fill_rows]
        if world > 1:
            parts = [None] * world
            torch.distributed.all_gather_object(parts, fill_rows)
        counts = np.asarray([r for part in parts for r in part], np.int64).reshape(-1, 3)
        out["fill"] = dict(score=evaluate.scores_from_hist(fill_total), hist=fill_total, coverage=components.coverage(fill_total, total),
                           counts=counts, stats=label_fill.fill_stats(counts), radius=fill["radius"])
        if rank == 0:
            logging.info(f"fill_label_score of {args.pred_dir} (--fill_ignore {'inf' if fill['radius'] is None else fill['radius']}):")
            logging.info("\n" + format_scores_table(out["fill"]["score"], cats))
            logging.info(label_fill.format_fill_summary(out["fill"]["stats"], out["fill"]["coverage"]))
            if fill["label_dir"]:
                logging.info(f"filled label maps -> {fill['label_dir']}")
    if scores is not None:
        out["image_scores"] = merged                           # the merged table (utils/image_scores.ImageScoreLog.merged)
    return out


if __name__ == "__main__":
    logging.basicConfig(level=logging.INFO, format="%(message)s")
    validate(get_parser().parse_args())
