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


def _split(flat, hws):
    """A flat numpy batch -> its [H,W] maps."""
    offs = np.concatenate([[0], np.cumsum([h * w for h, w in hws])])
    return [flat[offs[j]:offs[j + 1]].reshape(hw) for j, hw in enumerate(hws)]


# One batch of one stage -> (maps, counts [B,3]).  The maps of a batch are flat: a device tensor (the device arm, ops through the stage's
# utils module) or a numpy array (the numpy arm, its restatement); what comes back is of the same kind.
def _snap_batch(snap, src, imgs, hws, nc):
    from ..utils import superpixels
    if torch.is_tensor(src):
        from .. import ops
        plan = ops.RaggedPlan(hws, src.device)
        hwc_d = torch.from_numpy(np.concatenate([im.reshape(-1) for im in imgs])).to(src.device)
        sp_d, _, cent = superpixels.slic_superpixels(hwc_d, snap["step"], snap["compactness"], snap["iters"], plan=plan)
        return superpixels.snap_labels(src, sp_d, snap["step"], nc, snap["min_share"], plan=plan, cent=cent)
    done = superpixels.snap_batch_numpy(imgs, _split(src, hws), snap["step"], nc, snap["compactness"], snap["iters"], snap["min_share"])
    return np.concatenate([d[2].reshape(-1) for d in done]), np.stack([d[3] for d in done])


def _clean_batch(clean, src, hws, nc):
    from ..utils import components
    thr = [components.min_area_rule(clean["min_region"], h, w) for h, w in hws]
    if torch.is_tensor(src):
        from .. import ops
        plan = ops.RaggedPlan(hws, src.device)
        comp, area = components.label_components(src, plan=plan, connectivity=clean["connectivity"])
        return components.filter_small_regions(src, comp, area, thr, nc, plan=plan)
    done = [components.clean_numpy(m, t, nc, clean["connectivity"]) for m, t in zip(_split(src, hws), thr)]
    return np.concatenate([d[0].reshape(-1) for d in done]), np.stack([d[1] for d in done])


def _fill_batch(fill, hole, mask, hws, nc):
    """mask: the map in which a 255 is to stay, or None: every 255 of `hole` is a hole."""
    from ..utils import label_fill
    if torch.is_tensor(hole):
        from .. import ops
        filled_d, _, counts_d = label_fill.fill_nearest_label(hole, nc, plan=ops.RaggedPlan(hws, hole.device), mask=mask, radius=fill["radius"])
        return filled_d, counts_d
    masks = _split(mask, hws) if mask is not None else [None] * len(hws)
    done = [label_fill.fill_numpy(h, nc, radius=fill["radius"], mask=m) for h, m in zip(_split(hole, hws), masks)]
    return np.concatenate([d[0].reshape(-1) for d in done]), np.stack([d[2] for d in done])


def validate(args):
    """-> {"score": scores_from_hist of the gathered matrix, "hist": [nc,nc] int64 (CPU tensor), "images": scored on this rank,
    "seconds"}: the layout of infer_seg_voc.validate (+ "image_scores" with --per_image_scores, + one entry per label stage that is on)."""
    from ..utils import components, evaluate, image_scores, label_stages
    image_scores.refuse(args)
    on = {name: label_stages.STAGES[name].resolve(args, program="eval_labels") for name in ("clean", "fill", "snap")}
    clean, fill, snap = on["clean"], on["fill"], on["snap"]
    stages = {name: on[name] for name in label_stages.EVAL_LABELS_ORDER if on[name] is not None}     # those that run, in the order of the report
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
    stage_hist, stage_rows, pixels = {name: torch.zeros_like(hist) for name in stages}, {name: [] for name in stages}, 0
    for resolved in stages.values():
        if resolved["label_dir"]:
            os.makedirs(resolved["label_dir"], exist_ok=True)

    def scored(name, maps, counts):
        """The shared end of a stage's batch: its maps into the stage's matrix, its rows kept, its PNGs written -> the maps as they came."""
        if on_gpu:
            from .. import ops
            stage_hist[name] = ops.confusion_accumulate(gt_d, maps, nc, stage_hist[name])
            host, counts = maps.cpu().numpy(), counts.cpu().numpy()
        else:
            host = maps
            stage_hist[name] += torch.from_numpy(_hist_numpy(gt, host, nc))
        stage_rows[name].extend(np.asarray(counts, np.int64).reshape(-1, 3).tolist())
        if stages[name]["label_dir"]:
            for n, m in zip(batch, _split(host, hws)):
                _save_index_png(os.path.join(stages[name]["label_dir"], n + ".png"), m)
        return maps

    t0 = time.time()
    with cf.ThreadPoolExecutor(max_workers=max(1, int(args.num_workers))) as pool:
        for s in range(0, len(mine), args.batch_size):
            batch = mine[s:s + args.batch_size]
            pairs = list(pool.map(lambda n: _load_pair(args, n), batch))                             # raises the first error, in order
            gt = np.concatenate([p[0] for p in pairs])
            pred = np.concatenate([p[1] for p in pairs])
            hws = [p[2] for p in pairs]
            if on_gpu:
                from .. import ops
                gt_d, pred_d = torch.from_numpy(gt).to(device), torch.from_numpy(pred).to(device)
                hist = ops.confusion_accumulate(gt_d, pred_d, nc, hist)
                if scores is not None:                                                           # the batch as one ragged plan, behind a ticket
                    from ..pipeline import ScoreTicket
                    scores.defer(ScoreTicket().launch("main", gt_d, pred_d, nc, plan=ops.RaggedPlan(hws, device), boundary=boundary), idx[s:s + len(pairs)],
                                 batch, hws)
            else:
                hist += torch.from_numpy(_hist_numpy(gt, pred, nc))
                if scores is not None:
                    for j, p in enumerate(pairs):
                        scores.put(idx[s + j], batch[j], p[2], "main", image_scores.counts_numpy(p[0], p[1], nc))
                        if boundary is not None:
                            scores.put(idx[s + j], batch[j], p[2], "main_bd", image_scores.boundary_counts_numpy(
                                p[0].reshape(p[2]), p[1].reshape(p[2]), nc, image_scores.checked_radius(batch[j], p[2][0], p[2][1], boundary)))
            # the chain snap -> clean -> fill (label_stages.CHAIN_ORDER), every stage on the maps of the one in front of it
            src = pred_d if on_gpu else pred                     # what the cleaning and the fill work on: the predictions, or the snapped maps
            pixels += int(pred.size)
            if snap is not None:                                 # the images decoded, segmented, voted on
                imgs = list(pool.map(lambda nh: _load_image(args, *nh), zip(batch, hws)))
                src = scored("snap", *_snap_batch(snap, src, imgs, hws, nc))
            if clean is not None:
                cleaned = scored("clean", *_clean_batch(clean, src, hws, nc))
            if fill is not None:                                 # what the cleaning removed (its input is the mask: a 255 it had stays), or every 255
                hole, mask = (cleaned, src) if clean is not None else (src, None)
                scored("fill", *_fill_batch(fill, hole, mask, hws, nc))
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
    for name, resolved in stages.items():                      # every rank gathers in this order
        stage = label_stages.STAGES[name]
        _, set_total = gather_hists(stage_hist[name])
        set_total = set_total.cpu()
        parts = [(stage_rows[name], pixels)]
        if world > 1:
            parts = [None] * world
            torch.distributed.all_gather_object(parts, (stage_rows[name], pixels))
        counts = np.asarray([r for part in parts for r in part[0]], np.int64).reshape(-1, 3)
        more = (sum(part[1] for part in parts),) if name == "snap" else ()       # the share of pixels the vote changed
        out[name] = dict(score=evaluate.scores_from_hist(set_total), hist=set_total, coverage=components.coverage(set_total, total),
                         counts=counts, stats=stage.stats(counts, *more), **label_stages.pipeline_value(stage, resolved))
        if rank == 0:
            logging.info(label_stages.title(stage, resolved, of=args.pred_dir))
            logging.info("\n" + format_scores_table(out[name]["score"], cats))
            logging.info(stage.summary(out[name]["stats"], out[name]["coverage"]))
            if resolved["label_dir"]:
                logging.info(f"{stage.noun} label maps -> {resolved['label_dir']}")
    if scores is not None:
        out["image_scores"] = merged                           # the merged table (utils/image_scores.ImageScoreLog.merged)
    return out


if __name__ == "__main__":
    logging.basicConfig(level=logging.INFO, format="%(message)s")
    validate(get_parser().parse_args())
