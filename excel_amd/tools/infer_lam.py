"""Training-free LAM evaluation harness - mirror of tools/infer_lam.py (build_validation :63-128, validate :130-176).

Differences from the reference, all deliberate:
  * batches of B > 1 images run through the device-resident TrainingFreePipeline (the reference is batch 1 with
    per-class host round trips) - with `--training_free false` on ragged batches through OptimisedLamPipeline (the decoder-driven
    flip-TTA LAMs, labels bit-identical to the per-image sequence); `--api_path` runs the reference's per-image call sequence instead.  Real data (`--data_folder`:
    every image has its own size, and the path refines and scores at that size, :74,:94) and `--ragged true` synthetic data run
    as RAGGED batches: a background decode pool (`--num_workers` threads; `--decode processes` = the reference's DataLoader worker
    processes, :167) fills a pinned staging ring, a copy stream moves the batches to the device ahead of the compute stream, the device resizes every image to the network size and runs the size-dependent half (up-sampling, PAR, arg-max) over packed
    planes through a tile map - one launch per stage for any mix of sizes (pipeline.run_batch_ragged);
  * ranks take images r, r+R, ... exactly like :166, accumulate a device-side [nc,nc] int64 confusion matrix and
    exchange it ONCE with an all_gather over RCCL (the reference scores each shard separately and never aggregates);
  * weights: `--model` is a CLIP checkpoint path or a model name found under --clip_root / $EXCEL_CLIP_ROOT / ~/.cache/clip
    (clip.load, model/model_excel.py:25); the class + background prompts are encoded with the checkpoint's text tower
    (model/model_excel.py:31-33; needs CLIP's BPE merges file: --bpe_path / $EXCEL_BPE_VOCAB).  `--model_path` = the trained
    decoder checkpoint, required only with `--training_free false` (the reference loads and then ignores it otherwise, :150-152);
  * `--save_cam true` writes the CAM overlay images of :97-111 (jet-coloured CAM blended over the photo, JPEG quality 75): per present
    class into --cs_cam_dir with --save_cls_specific_cam true (the reference's default), else the max over the classes into --cam_dir.
    The blend runs on the device right after each step (ops.cam_overlay_ragged, one launch per batch; the per-image path uses
    ops.cam_overlay); only the overlay bytes come back, into pinned memory, and a small thread pool encodes the files while the next
    batches run.  Deliberate differences: per-class file names use the data set's own class list (the reference's voc.class_list[idx+1],
    :111, fails on COCO classes >= 20), and an image without a present class writes no max overlay (the reference's torch.max raises).
    Directories follow :242-267 (cam_output_dirs); --refine_with_aff only picks the aff_lam / seeds_lam tag there, as in the reference;
  * `--save_label true` writes the pseudo-label map of every image as a palette PNG `<label_dir>/<name>.png` (the imsave of :95, commented
    out in the reference; live at tools/training_free_attr.py:225): the labels the run scores, encoded on the device on the step's
    stream (ops.png_encode_labels_ragged) with the VOC colour map, so the directory can stand in for a SegmentationClassAug directory
    (255 = ignore) and `python -m excel_amd.tools.eval_labels` scores it.  Only file bytes come back; every rank writes its own shard;
  * `--crf_post true --crf_inline true` runs the DenseCRF stage (:179-237) inside the main loop instead of over logits records: right
    after each ragged step, on its stream, ops.dcrf_lam_ragged refines the step's cams where they lie - every image over its own k + 1
    planes, the whole batch in one chain of launches per --crf_ws_gb group - and the labels go into a device-side confusion matrix
    that is gathered once like the main one.  No records, no second decode, no crf_proc pass; labels bit-identical to the record path.
    `--crf_label_dir DIR` writes the CRF labels as palette PNGs through the device encoder (like --save_label);
    --segs_crf_rgb_dir keeps its colour-coded files.  `--infer_set` names with "test" keep the record path (the reference scores
    against image[:,:,0] there, :213-214);
  * `--overflow_guard` (default auto = rerun on the batched GPU loop when the run's GEMM mode is f16x2 / f16x3, else off): those modes
    hold activations in IEEE half and turn a value beyond 65 504 into NaNs on purpose.  Every batched step counts the non-finite
    values of its attribute maps, affinity and random-walk result per image on the device (pipeline guard="skip"; no host wait in the
    loop), keeps flagged images out of the confusion matrices, and after the loop exactly those images run once more in exact fp32
    through the same consumers - their files are overwritten by name.  `raise` stops at the first flagged image instead; `off` is the
    unguarded loop.  The second pass is rank-local (no collective); the report is validate.last_guard;
  * `--cam_scales "1.0,0.5,0.75,1.5"` and `--cam_flip true` (training-free regime; defaults "1.0" / false = the plain step): the flip and
    multi-scale LAM fuse of utils/camutils.py:8-63 and the switched-off :82.  One model pass per scale over [x; mirror x], each network
    input made straight from the decoded pixels; ops.lam_tta_fuse brings every scale's maps to the patch grid of --resize_size, takes
    the maximum with the mirrored half, sums and min-max normalises - the `attr` the random walk reads.  The affinity is that of the
    plain scale-1.0 pass (:79).  Everything behind it (labels, score, --save_cam / --save_label / --crf_inline, the overflow guard) is
    unchanged; --api_path true runs the same arithmetic per image (camutils.tta_attr_map);
  * `--conf_label true` adds the two-threshold pseudo labels of utils/affutils.py:101-158 (refine_cams_with_bkg_v2, which the reference
    carries but never calls): from the step's cams, at half resolution, one PAR pass over the planes of both background scores
    (--conf_high_thre 0.7 / --conf_low_thre 0.25, the reference's --high_thre / --low_thre defaults), and a pixel that only the strict
    pass calls background becomes 255.  Right after each ragged step, on its stream (pipeline.run_batch_ragged(conf=)); the labels are
    written as palette PNGs `<conf_label_dir>/<name>.png` by the device encoder and scored into a second device-side confusion matrix
    that is gathered once like the main one: the log shows `conf_label_score` (over the kept pixels) and the coverage (kept / scored
    pixels).  The overflow guard covers it; --api_path true runs the same arithmetic per image (affutils.conf_labels_image);
  * `--tags clip` (training-free regime, batched loop; default `labels` = cls_labels_onehot.npy): the present classes of every image are
    predicted on the device right after the scale-1.0 forward, from CLIP's own image embedding (row 0 of x_raw, the class token the
    reference puts back at clip/clip_surgery_model.py:442-446) and the class + background prompts (ops.clip_tags: softmax over all prompts
    at --tag_scale 100, a class within --tag_thre 0.2 of the image's best one, at most --tag_max 6, the best always kept); the reference
    never tags images itself (its tools carry an unused --tag_threshold 0.2).  The pipeline is built with smax = --tag_max; the rows come
    back behind a ticket (no wait in the loop) for `--save_tags PATH` (the format of cls_labels_onehot.npy: a later --tags labels run
    reads it; one all_gather_object, rank 0 writes) and, where image-level labels exist, the third table `tag_score` (per class and micro
    precision / recall / F1, mean utils/evaluate.multilabel_score).  `--unlabeled true` reads a plain folder of images
    (datasets/images.ImageListDataset: no SegmentationClassAug, nothing scored, so one of --save_label / --conf_label / --save_tags is
    required).  --save_cam and the CRF stages size host-side work from the class list and are refused with --tags clip: --save_tags
    first, then --tags labels.  The default --tag_thre is provisional (tag quality is unmeasured);
  * `--per_image_scores PATH`: the reference scores at batch 1 with the labels on the host, so one print in its loop shows an image's
    own numbers; the batched, device-resident loops here only ever had the summed matrix.  With the flag every scored matrix (main,
    --conf_label's, --crf_inline's) also gets ops.image_scores on the same arrays - per image and class the ground-truth area, the
    predicted area and the intersection - behind a ticket (no wait in the loop; the per-image path calls the op with B = 1); after the
    loop one all_gather_object, rank 0 writes PATH (CSV, data-set order) and PATH.npz (the raw counts) and logs the image-averaged
    mIoU and the --per_image_worst 20 weakest images (utils/image_scores.py).  With --overflow_guard rerun the second pass's rows
    replace those of the flagged images (zero after the first pass).  Refused with --unlabeled true;
  * `--boundary_scores true` (--boundary_ratio 0.02, --boundary_px 0): region IoU is dominated by object interiors, while PAR, the
    DenseCRF stages and --conf_label all work at the contours.  With the flag every scored set (main, conf, crf) also gets
    ops.boundary_scores - the same counts restricted to the band within 2 % of the image diagonal of each map's own contours (Boundary
    IoU, Cheng et al., CVPR 2021) - in the same tickets; the log gets a boundary_score table per set, --json_out a `boundary` block
    and --per_image_scores' files `radius` / `biou` columns and `bcounts_<set>` arrays.  Works with or without --per_image_scores;
    refused with --unlabeled true; off by default (no launch, no column);
  * `--bkg_sweep "0.5,0.7,0.85,1.0,1.2,1.5,2.0"` / `--bkg_scale 1.0`: the reference writes the background channel torch.pow(1 - max, 1.)
    (utils/affutils.py:161-174) and its tools carry a --bkg_thre nothing reads; the strength of the background is the one knob of the
    CAM-to-label step.  PAR is linear per channel, so the labels of a background scaled by `a` are `a * b0 >= F` on the PAR output the
    step already has: with --bkg_sweep one more launch per ragged step (utils/bkg_sweep.sweep_ragged) counts the labels of every scale
    against the ground truth, the totals are summed over the ranks once, and rank 0 logs a bkg_sweep_score table (pAcc, mIoU, background
    IoU, foreground mIoU per scale) and the best scale; --json_out gains a `bkg_sweep` block.  --bkg_scale labels at one scale instead
    of 1.0: scores, PNGs and per-image scores take those labels (the conf labels and the CRF stages are built from the cams and do not
    change).  Ragged batches on the batched loop only; --bkg_sweep is refused with --unlabeled true, both with --api_path true; off by
    default (no launch).  The exponent of that pow is not swept: it is not linear under PAR;
  * `--margin_sweep "0,0.05,0.1,0.2,0.3"` / `--margin_min T` (`--margin_label_dir DIR`): the margin of a pixel is the winning PAR plane
    minus the runner-up (utils/margin.py), a confidence the step's PAR output already holds.  With --margin_sweep one more launch per
    ragged step counts, per threshold, the pixels with margin >= t (coverage: no ground truth needed, so --unlabeled true is allowed)
    and their counts against the ground truth; the ranks' counts are summed once and rank 0 logs a margin_sweep_score table,
    --json_out gains a `margin_sweep` block.  --margin_min makes a further label set (255 where the margin is below T) by the cleaned
    set's route: PNGs, a margin_label_score table and its coverage, a `margin` block, the margin_* columns of --per_image_scores.
    The values are illustrations: no default is chosen, nothing has been measured on real data.  Ragged batches on the batched loop
    only; off by default (no launch, no key, no column);
  * `--clean_min_region VALUE` (`--clean_connectivity 8|4`, `--clean_label_dir DIR`): the arg-max leaves islands of a few pixels and
    pin-holes; the reference has no remedy.  Behind the arg-max of every ragged step, utils/components.label_components labels the
    connected regions of the step's main label map (equal raw value, 8- or 4-neighbours) and filter_small_regions turns every class
    region below VALUE - pixels, or with 0 < VALUE < 1 a fraction of the image's own area - into 255.  The cleaned maps go to
    `<clean_label_dir>/<name>.png` through the device encoder, their kept pixels into a second device-side confusion matrix: the log
    gains a clean_label_score table, the coverage (kept over labelled pixels) and the regions / regions removed per image, --json_out a
    `clean` block, --per_image_scores the clean_* columns plus regions, regions_removed and pixels_removed.  The main labels, scores and
    PNGs are untouched.  Ragged batches on the batched loop only (refused with --api_path true); with --unlabeled true nothing is
    scored and --clean_label_dir is required; off by default (no launch, no key, no column).  The conf and crf label sets are not
    cleaned here: their PNGs can go through eval_labels --clean_min_region;
  * `--fill_ignore inf|PIXELS` (`--fill_label_dir DIR`; needs --clean_min_region): the other half of the cleaning.  Behind the filter,
    utils/label_fill.fill_nearest_label gives every pixel the cleaning turned into 255 the value of the nearest class pixel of its image
    (exact squared Euclidean distance, ties to the first pixel in raster order, at most PIXELS away), so a pin-hole inside an object
    becomes object again; an ignore pixel the main map already had would stay.  The filled maps are one more scored label set, by the
    cleaned set's route: `<fill_label_dir>/<name>.png`, a fill_label_score table, one summary line (holes, filled, largest distance,
    coverage), a `fill` block in --json_out, fill_* columns plus holes, filled and max_fill_dist in --per_image_scores.  The main, conf,
    crf and clean outputs are untouched.  Refused without --clean_min_region, with --api_path true, and with --unlabeled true unless
    --fill_label_dir is given; off by default (no launch, no key, no column).  Conf and crf PNGs go through eval_labels --fill_ignore;
  * `--snap_superpixels STEP` (`--snap_compactness 10`, `--snap_iters 5`, `--snap_min_share 0`, `--snap_label_dir DIR`): the one stage
    behind the arg-max that looks at the image again.  utils/superpixels.slic_superpixels over-segments the step's decoded images into
    superpixels of grid step STEP (2..64; an integer SLIC on a fixed grid, csrc/superpixels.hip) and snap_labels gives every superpixel
    the majority class of the main labels inside it - only where that class holds at least --snap_min_share of the votes -, so contours
    move onto colour edges and speckle is voted away instead of ignored.  The snapped maps are one more scored label set:
    `<snap_label_dir>/<name>.png`, a snap_label_score table, one summary line (superpixels with a vote, snapped, pixels changed and
    their share), a `snap` block in --json_out, snap_* columns plus superpixels, snapped and pixels_changed in --per_image_scores, a
    boundary_score table with --boundary_scores.  With it --clean_min_region and --fill_ignore work on the snapped maps (snap -> clean
    -> fill); the main labels, scores and PNGs are untouched.  Superpixels are not made connected.  Refused with --api_path true, and
    with --unlabeled true unless --snap_label_dir is given; off by default (0: no launch, no key, no column);
  * `--synthetic N` (no --data_folder) feeds seeded synthetic samples; seeded random weights are used ONLY in that mode and only
    when no checkpoint can be resolved (logged).  `--data_folder` without a resolvable checkpoint is an error.
Launch: python -m torch.distributed.run --nproc-per-node R -m excel_amd.tools.infer_lam --synthetic 64 ...
"""
import argparse
import logging
import os
import time

import numpy as np
import torch
import torch.distributed as dist

VOC_CLASSES = ["_background_", "aeroplane", "bicycle", "bird", "boat", "bottle", "bus", "car", "cat", "chair", "cow",
               "diningtable", "dog", "horse", "motorbike", "person", "pottedplant", "sheep", "sofa", "train", "tvmonitor"]


def _bool(x):
    return x.lower() in ["true", "1", "yes"]


OVERFLOW_GUARD_POLICIES = ("auto", "off", "raise", "rerun")
F16_GEMM_MODES = ("f16x2", "f16x3")          # activations in IEEE half: range 65 504, overflow -> NaN (include/excel_hip.h, modes 2 and 3)


def resolve_overflow_guard(policy, gemm_mode, on_gpu, batched):
    """--overflow_guard -> the policy the loop runs with ("off" | "raise" | "rerun").  auto = rerun when the loop is the batched one on
    a GPU and the handle's mode (after the start-up check) is an f16 mode, else off: bf16x3 has the fp32 exponent range, f32 is exact.
    An explicit raise / rerun on the per-image loop is an error: that loop has no guard."""
    if policy not in OVERFLOW_GUARD_POLICIES:
        raise ValueError(f"--overflow_guard must be one of {OVERFLOW_GUARD_POLICIES} (got {policy!r})")
    if policy == "auto":
        return "rerun" if (batched and on_gpu and gemm_mode in F16_GEMM_MODES) else "off"
    if policy != "off" and not batched:
        raise ValueError(f"--overflow_guard {policy} needs the batched loop: the per-image loop (--api_path true, or --training_free false "
                         "on uniform synthetic batches) has no overflow guard - use --overflow_guard off or auto there")
    return policy


def tta_sizes(S, scales):
    """--cam_scales at --resize_size S -> [(S_s, g_s), ...], scale 1.0 first (pipeline.tta_sizes: the rule and what it refuses)."""
    from ..pipeline import tta_sizes as sizes
    return sizes(S, scales)


def resolve_tta(args):
    """--cam_scales / --cam_flip -> (tta_scales, tta_flip) for TrainingFreePipeline / camutils.tta_attr_map; (None, False) = the plain
    step (the defaults "1.0" / false).  Checked here, before a model is built: the scales against --resize_size (tta_sizes), and the
    regime - --training_free false has its own flip (cure_attr_map_flip) and no multi-scale fuse."""
    from .infer_seg_voc import parse_scales
    scales = parse_scales(flag_defaults(args).cam_scales or "1.0")
    flip = bool(args.cam_flip)
    if not flip and scales == (1.0,):
        return None, False
    if not args.training_free:
        raise ValueError(f"--cam_scales {','.join(str(x) for x in scales)} / --cam_flip {str(flip).lower()} belong to the training-free regime: "
                         "--training_free false already runs its own flip (cure_attr_map_flip) - drop the two flags there")
    tta_sizes(args.resize_size, scales)
    return scales, flip


def resolve_conf(args):
    """--conf_label / --conf_high_thre / --conf_low_thre -> (high_thre, low_thre) for run_batch_ragged(conf=), or None (the default:
    the plain step).  Checked here, before a model is built (pipeline.check_conf: a threshold outside (0, 1), low_thre >= high_thre)."""
    if not flag_defaults(args).conf_label:
        return None
    from ..pipeline import check_conf
    try:
        return check_conf((args.conf_high_thre, args.conf_low_thre))
    except ValueError as e:
        raise ValueError(f"--conf_high_thre / --conf_low_thre: {e}") from None


TAG_SOURCES = ("labels", "clip")


def resolve_tags(args, have_dataset=False):
    """--tags / --tag_thre / --tag_max / --tag_scale / --unlabeled / --save_tags -> the `tagger` of TrainingFreePipeline
    (dict(thre=, kmax=, scale=)) for --tags clip, or None (--tags labels, the default: the image-level labels of cls_labels_onehot.npy).
    Checked here, before a device or a model is touched (args.num_classes must be settled: resolve_vocabulary runs first); every refusal
    names its flag.  `have_dataset`: the caller supplies the data set itself (validate(dataset=)), so --unlabeled needs no --data_folder."""
    flag_defaults(args)
    if args.tags not in TAG_SOURCES:
        raise ValueError(f"--tags must be one of {TAG_SOURCES} (got {args.tags!r})")
    if args.unlabeled:
        if not args.data_folder and not have_dataset:
            raise ValueError("--unlabeled true reads a folder of images (--data_folder with JPEGImages/, --list_folder with <infer_set>.txt): "
                             "--synthetic samples always carry their labels")
        if not args.list_folder and not have_dataset:
            raise ValueError("--unlabeled true needs --list_folder: the image ids come from <list_folder>/<infer_set>.txt")
        if args.crf_post:
            raise ValueError("--unlabeled true has no ground truth to score: --crf_post scores the DenseCRF labels against it - drop one of the two")
        if args.api_path:
            raise ValueError("--unlabeled true runs on the batched loop: --api_path true scores every image against its ground truth")
        if not (args.save_label or args.conf_label or args.save_tags or getattr(args, "clean_label_dir", None)
                or getattr(args, "fill_label_dir", None) or getattr(args, "snap_label_dir", None)):
            raise ValueError("--unlabeled true scores nothing, so the run must write something: give at least one of --save_label true, "
                             "--conf_label true, --save_tags PATH")
    if args.save_tags and args.tags != "clip":
        raise ValueError("--save_tags writes the predicted tags: it needs --tags clip")
    if args.tags == "labels":
        return None
    if not args.training_free:
        raise ValueError("--tags clip belongs to the training-free regime: --training_free false has no tagger (OptimisedLamPipeline)")
    if args.api_path:
        raise ValueError("--tags clip runs on the batched loop: --api_path true is the reference's per-image call sequence, which reads the "
                         "image-level labels")
    for flag in ("save_cam", "crf_post", "crf_inline"):
        if getattr(args, flag):
            raise ValueError(f"--tags clip cannot feed --{flag} true yet: that stage sizes its work from the host copy of the class list "
                             "when the step is enqueued, and predicted tags exist on the device only.  Take the two-run route: first "
                             f"--tags clip --save_tags <list_folder>/cls_labels_onehot.npy, then --tags labels --{flag} true")
    F = int(args.num_classes) - 1
    if not 1 <= int(args.tag_max) <= F:
        raise ValueError(f"--tag_max {args.tag_max} is outside [1, {F}] (num_classes - 1 foreground classes)")
    if not 0.0 <= float(args.tag_thre) <= 1.0:
        raise ValueError(f"--tag_thre {args.tag_thre} is outside [0, 1]: the threshold is relative to the best foreground score")
    if not float(args.tag_scale) > 0.0:
        raise ValueError(f"--tag_scale {args.tag_scale} must be positive (CLIP's logit scale is 100)")
    return dict(thre=float(args.tag_thre), kmax=int(args.tag_max), scale=float(args.tag_scale))


def tag_report(rows, truth, num_fg):
    """The predicted tags of a run -> its report.  rows = {name: one-hot [F]} (what --save_tags writes), truth = {name: one-hot [F]} of the
    image-level labels for the images that have them (may be empty).  -> {"images", "tags_per_image": histogram list (index = number of
    tags), "scored": images with labels, and for those "counts" {tp, fp, fn, tn} (they add up to scored x F), "per_class_counts" [F][3]
    (tp, fp, fn), "score" (evaluate.tag_scores) and "image_f1" (mean of evaluate.multilabel_score per image); None without labels}."""
    from ..utils import evaluate
    F = int(num_fg)
    hist = np.zeros(F + 1, np.int64)
    for r in rows.values():
        hist[int((np.asarray(r) != 0).sum())] += 1
    out = {"images": len(rows), "tags_per_image": [int(v) for v in hist[:int(np.flatnonzero(hist).max()) + 1]] if len(rows) else [],
           "scored": 0, "counts": None, "per_class_counts": None, "score": None, "image_f1": None}
    names = sorted(n for n in rows if n in truth)
    if not names:
        return out
    P = np.stack([np.asarray(rows[n]) != 0 for n in names])
    T = np.stack([np.asarray(truth[n]) != 0 for n in names])
    pc = np.stack([(P & T).sum(0), (P & ~T).sum(0), (~P & T).sum(0)], 1).astype(np.int64)
    tp, fp, fn = (int(v) for v in pc.sum(0))
    out.update(scored=len(names), counts={"tp": tp, "fp": fp, "fn": fn, "tn": len(names) * F - tp - fp - fn},
               per_class_counts=[[int(v) for v in row] for row in pc], score=evaluate.tag_scores(pc),
               image_f1=float(np.mean([evaluate.multilabel_score(T[i], P[i]) for i in range(len(names))])))
    return out


def save_tags_file(path, rows):
    """--save_tags: {name: one-hot float32 [F]} in exactly the format of cls_labels_onehot.npy (datasets/voc.load_cls_label_list reads it
    back), written next to its place and moved there in one step."""
    d = os.path.dirname(os.path.abspath(path))
    os.makedirs(d, exist_ok=True)
    tmp = os.path.join(d, f".{os.path.basename(path)}.{os.getpid()}.tmp")
    try:
        with open(tmp, "wb") as f:
            np.save(f, {str(n): np.asarray(rows[n], np.float32) for n in sorted(rows)}, allow_pickle=True)
        os.replace(tmp, path)
    finally:
        if os.path.exists(tmp):
            os.remove(tmp)


def _handle_gemm_mode(model):
    """The GEMM mode of the model's ViT handle, or None (no model: a stub pipeline)."""
    try:
        return model.encoder.visual.handle().gemm_mode()
    except AttributeError:
        return None


class _StoreGiven(argparse.Action):
    """store, and note in <dest>_given that the flag was on the command line (a default cannot contradict a vocabulary file)"""

    def __call__(self, parser, namespace, values, option_string=None):
        setattr(namespace, self.dest, values)
        setattr(namespace, self.dest + "_given", True)


MAX_FG_CLASSES = 254       # uint8 label maps: keys 1..254, 0 = background, 255 = ignore
MAX_TEXT_ROWS = 512        # excel_patch_text_cam


def _read_names(path, what):
    with open(path) as f:
        names = [x.strip() for x in f.read().split("\n")]
    while names and not names[-1]:
        names.pop()                                                                         # trailing newline(s)
    if not names:
        raise ValueError(f"{what} {path}: no names")
    for i, n in enumerate(names):
        if not n:
            raise ValueError(f"{what} {path}: line {i + 1} is empty")
    seen = {}
    for i, n in enumerate(names):
        if n in seen:
            raise ValueError(f"{what} {path}: {n!r} appears on lines {seen[n] + 1} and {i + 1}")
        seen[n] = i
    return names


def load_attr_bank(path):
    """--attr_bank: the reference's torch-saved pair [bank [C,K], flag] or an .npz with `bank` (and `flag`) -> bank [C,K] float32 tensor"""
    if not os.path.isfile(path):
        raise FileNotFoundError(f"--attr_bank {path}: no such file")
    if path.endswith(".npz"):
        z = np.load(path)
        if "bank" not in z:
            raise ValueError(f"--attr_bank {path}: no array named `bank`")
        bank = torch.from_numpy(np.asarray(z["bank"], np.float32))
    else:
        obj = torch.load(path, map_location="cpu")
        bank = torch.as_tensor(obj[0] if isinstance(obj, (list, tuple)) else obj).float()
    if bank.ndim != 2:
        raise ValueError(f"--attr_bank {path}: the bank must be [C,K], got {tuple(bank.shape)}")
    return bank


def resolve_vocabulary(args):
    """--class_names / --bkg_names / --attr_bank -> args.vocab = {"fg", "bkg", "bank"} (None entries where not given), args.num_classes
    settled.  Runs before any model is built and refuses: duplicate or empty names, more than 254 foreground classes, more than 512
    prompts, a --num_classes that contradicts the file, num_classes > 255, and real data (--data_folder) with --class_names but no
    --attr_bank - a vocabulary is never silently paired with another data set's bank."""
    from ..pipeline import check_num_classes
    fg = bkg = bank = None
    path = flag_defaults(args).class_names
    if path:
        fg = _read_names(path, "--class_names")
        if len(fg) > MAX_FG_CLASSES:
            raise ValueError(f"--class_names {path}: {len(fg)} foreground classes; the uint8 label maps hold at most {MAX_FG_CLASSES} "
                             "(keys 1..254, 255 = ignore)")
        if args.num_classes_given and args.num_classes != len(fg) + 1:
            raise ValueError(f"--num_classes {args.num_classes} contradicts --class_names {path}: {len(fg)} names + background = {len(fg) + 1}")
        args.num_classes = len(fg) + 1
        if args.bkg_names:
            bkg = _read_names(args.bkg_names, "--bkg_names")
        else:
            from ..datasets.clip_text import BACKGROUND_CATEGORY
            bkg = list(BACKGROUND_CATEGORY)
        both = set(fg) & set(bkg)
        if both:
            raise ValueError(f"--class_names / --bkg_names: {sorted(both)[0]!r} is in both lists")
        if len(fg) + len(bkg) > MAX_TEXT_ROWS:
            raise ValueError(f"{len(fg)} class names + {len(bkg)} background names = {len(fg) + len(bkg)} prompts; the CAM kernel takes at most "
                             f"{MAX_TEXT_ROWS}")
    elif args.bkg_names:
        raise ValueError("--bkg_names needs --class_names")
    check_num_classes(args.num_classes)
    if args.attr_bank:
        bank = load_attr_bank(args.attr_bank)
    elif fg is not None and args.data_folder:
        raise ValueError("--data_folder with --class_names needs --attr_bank: the shipped banks belong to the VOC and COCO vocabularies")
    args.vocab = {"fg": fg, "bkg": bkg, "bank": bank}
    return args.vocab


def get_parser():
    p = argparse.ArgumentParser()
    # flags kept from the reference (tools/infer_lam.py:30-60)
    p.add_argument("--model_path", default=None, type=str)
    p.add_argument("--model", default="ExCEL_ViT-B/16", type=str)
    p.add_argument("--dataset_name", default="pascal_voc", type=str)
    p.add_argument("--attr_json", default=None, type=str)
    p.add_argument("--num_attri", default=112, type=int)
    p.add_argument("--embedding_dim", default=256, type=int)
    p.add_argument("--in_channels", default=768, type=int)
    p.add_argument("--resize_size", default=448, type=int)
    p.add_argument("--infer_set", default="train", type=str)
    p.add_argument("--training_free", default=True, type=_bool)
    p.add_argument("--refine_with_aff", default=True, type=_bool, help="only names the output tag (aff_lam / seeds_lam, :242-246)")
    p.add_argument("--save_cls_specific_cam", default=True, type=_bool, help="with --save_cam: one overlay per present class (:104-111)")
    p.add_argument("--save_cam", default=False, type=_bool, help="write the CAM overlay images (:97-111)")
    p.add_argument("--cam_device_jpeg", default=False, type=_bool,
                   help="with --save_cam on the batched path: encode the overlay JPEGs on the device (the same bytes; --api_path true keeps the host encoder)")
    p.add_argument("--cam_dir", default=None, type=str, help="max-overlay directory (default: cam_output_dirs)")
    p.add_argument("--cs_cam_dir", default=None, type=str, help="per-class overlay directory (default: cam_output_dirs)")
    p.add_argument("--save_label", default=False, type=_bool, help="write the pseudo-label maps as palette PNGs <label_dir>/<name>.png (:95)")
    p.add_argument("--label_dir", default=None, type=str, help="label PNG directory (default: label_output_dir, next to the CAM directories)")
    p.add_argument("--conf_label", default=False, type=_bool,
                   help="also write two-threshold pseudo labels with an ignore band (utils/affutils.py:101-158) as palette PNGs <conf_label_dir>/<name>.png")
    p.add_argument("--conf_high_thre", default=0.7, type=float, help="--conf_label: background score of the strict pass (the reference's --high_thre)")
    p.add_argument("--conf_low_thre", default=0.25, type=float, help="--conf_label: background score of the lenient pass (the reference's --low_thre)")
    p.add_argument("--conf_label_dir", default=None, type=str, help="confident-label PNG directory (default: conf_label_output_dir, next to the label directory)")
    p.add_argument("--data_folder", default=None, type=str, help="VOC2012 root (JPEGImages/, SegmentationClassAug/): real data instead of --synthetic")
    p.add_argument("--list_folder", default=None, type=str, help="directory with <infer_set>.txt and cls_labels_onehot.npy")
    p.add_argument("--u8_input", default=False, type=_bool, help="feed decoded uint8 HWC images and normalise on the device")
    p.add_argument("--crf_post", default=False, type=_bool, help="write the per-image logits records (:116-119, api path) and run the DenseCRF stage over them (:179-237)")
    p.add_argument("--logits_dir", default="./logits", type=str)
    p.add_argument("--segs_crf_rgb_dir", default=None, type=str, help="colour-coded CRF label images (tools/infer_lam.py:228); default: not written")
    p.add_argument("--crf_inline", default=False, type=_bool,
                   help="with --crf_post: run the DenseCRF stage inside the main loop on the step's cams (no logits records, no crf_proc pass)")
    p.add_argument("--crf_ws_gb", default=16.0, type=float, help="--crf_inline: workspace budget of the DenseCRF stage in GiB; a batch is cut into groups that fit")
    p.add_argument("--crf_label_dir", default=None, type=str, help="--crf_inline: write the CRF labels as palette PNGs <dir>/<name>.png (device encoder)")
    p.add_argument("--num_classes", default=21, type=int, action=_StoreGiven,
                   help="default: 21, or with --class_names its lines + 1 (a contradicting value is refused)")
    p.add_argument("--class_names", default=None, type=str,
                   help="a vocabulary of your own: text file with one FOREGROUND class name per line (up to 254); prompts, score tables, "
                        "overlay names follow it.  With --data_folder it needs --attr_bank")
    p.add_argument("--bkg_names", default=None, type=str, help="with --class_names: one background prompt per line (default: the VOC background list)")
    p.add_argument("--attr_bank", default=None, type=str,
                   help="attribute bank file: the reference's .pth pair [bank, flag] or this package's .npz with `bank` [C,K] and `flag`")
    p.add_argument("--ignore_index", default=255, type=int)
    p.add_argument("--local_rank", default=int(os.environ.get("LOCAL_RANK", 0)), type=int)
    p.add_argument("--backend", default="nccl")
    # additions
    p.add_argument("--batch_size", default=32, type=int)
    p.add_argument("--synthetic", default=64, type=int, help="number of seeded synthetic samples")
    p.add_argument("--seed", default=1234, type=int)
    p.add_argument("--api_path", default=False, type=_bool, help="per-image reference call sequence instead of the batched pipeline")
    p.add_argument("--ragged", default=False, type=_bool, help="synthetic samples with VOC-like, per-image sizes (uint8 images), fed as ragged batches like real data")
    p.add_argument("--num_workers", default=-1, type=int,
                   help="background decoders of the ragged path (the reference's DataLoader uses 2 worker processes, :167); -1 = from the CPUs "
                        "this rank may really use (affinity and the container's cgroup quota, shared by the ranks of the node): at most 16")
    p.add_argument("--decode", default="threads", choices=["threads", "processes"],
                   help="threads: a decode thread pool in this process (Pillow releases the GIL; default); processes: forked DataLoader "
                        "workers like the reference - after such workers exit, host-side GPU event waits of this process were measured "
                        "at ~350 ms each on ROCm 7.2, so the default avoids fork")
    p.add_argument("--clip_root", default=None, type=str, help="directory holding the published CLIP archive (ViT-B-16.pt); default $EXCEL_CLIP_ROOT, ~/.cache/clip")
    p.add_argument("--bpe_path", default=None, type=str, help="CLIP's bpe_simple_vocab_16e6.txt.gz (default $EXCEL_BPE_VOCAB)")
    p.add_argument("--gemm_mode", default=None, type=str, help="auto (default: f16x2 when every GEMM weight is fp16-valued - every published CLIP archive -, else bf16x3) | bf16x3 | f16x3 | f16x2 | f32")
    p.add_argument("--gemm_check", default=True, type=_bool,
                   help="before the loop, run the first few images in the chosen fast mode AND in exact fp32 and compare the CAMs; above "
                        "--gemm_check_tol the run moves down the ladder bf16x3 -> f16x3 (f16x2 on fp16-valued weights) -> f32 (ill-conditioned weights; "
                        "ExCEL_model.check_numerics)")
    p.add_argument("--gemm_check_tol", default=5e-4, type=float)
    p.add_argument("--overflow_guard", default="auto", choices=list(OVERFLOW_GUARD_POLICIES),
                   help="the f16 GEMM modes (f16x2 / f16x3) turn an activation beyond 65 504 into NaNs: rerun = count the non-finite values "
                        "per image on the device in every batched step, keep flagged images out of the scores and run exactly those again in "
                        "exact fp32 after the loop; raise = stop at the first flagged image; off = no check; auto = rerun on the batched GPU "
                        "loop in an f16 mode, else off (bf16x3 has the fp32 exponent range, f32 is exact)")
    p.add_argument("--cam_scales", default="1.0", type=str,
                   help="training-free regime: fuse the LAMs of these scales of --resize_size, e.g. \"1.0,0.5,0.75,1.5\" (must hold 1.0; each "
                        "scale is one more model pass; fused at the patch grid in front of the random walk)")
    p.add_argument("--cam_flip", default=False, type=_bool,
                   help="training-free regime: every scale also runs the mirrored image, the two LAMs are fused by their maximum")
    p.add_argument("--tags", default="labels", choices=list(TAG_SOURCES),
                   help="where the present classes of an image come from: labels = cls_labels_onehot.npy (default); clip = predicted on the "
                        "device from CLIP's image embedding and the class / background prompts (training-free regime, batched loop)")
    p.add_argument("--tag_thre", default=0.2, type=float,
                   help="--tags clip: a class is tagged when its score reaches this fraction of the image's best class score (the best is always kept)")
    p.add_argument("--tag_max", default=6, type=int, help="--tags clip: at most this many tags per image (the pipeline's smax)")
    p.add_argument("--tag_scale", default=100.0, type=float, help="--tags clip: the logit scale in front of the softmax over all prompts")
    p.add_argument("--save_tags", default=None, type=str,
                   help="--tags clip: write the predicted tags here in the format of cls_labels_onehot.npy (a later --tags labels run reads them)")
    p.add_argument("--unlabeled", default=False, type=_bool,
                   help="a folder of images without ground truth: --data_folder/JPEGImages/<id>.jpg for the ids of --list_folder/<infer_set>.txt; "
                        "nothing is scored, so give --save_label, --conf_label or --save_tags")
    p.add_argument("--cpu_affinity", default="auto", choices=["auto", "off"],
                   help="auto: with several ranks on the node every rank pins itself (decode pool included) to its own share of the host cores")
    from ..utils import image_scores
    image_scores.add_flags(p)
    image_scores.add_boundary_flags(p)
    from ..utils import bkg_sweep
    bkg_sweep.add_flags(p)
    from ..utils import margin as margin_flags
    margin_flags.add_flags(p)
    from ..utils import components
    components.add_flags(p)
    from ..utils import label_fill
    label_fill.add_flags(p)
    from ..utils import superpixels
    superpixels.add_flags(p)
    p.add_argument("--json_out", default=None, type=str, help="rank 0 writes a one-line JSON record of the run here (rate, ranks, per-rank mass)")
    p.set_defaults(ragged_batches=False, run_token=None, vocab=None, num_classes_given=False)      # what the program sets itself
    return p


def flag_defaults(args, parser=None):
    """Tests and other programs call in with namespaces of their own: every flag of the parser (default: get_parser()) that `args`
    lacks gets the parser's default, in place, so the code below reads args.flag.  -> args"""
    for k, v in vars((parser or get_parser()).parse_args([])).items():
        if not hasattr(args, k):
            setattr(args, k, v)
    return args


# ------------------------------------------------------------------ CAM overlay images (tools/infer_lam.py:97-111, :242-267)
DEFAULT_CAM_ROOT = "lam_cams"       # stands in for the part before "checkpoints/" when there is no --model_path


def cam_output_dirs(model_path, infer_set, training_free=True, refine_with_aff=True):
    """The reference's output locations (:242-267): base = <model_path before "checkpoints/">/<infer_set>, then
    <infer_set>_<ckpt>_<tag>_img (max overlays) and <infer_set>_<ckpt>_<tag>_class_specific_img (per-class overlays).  A model path
    without "checkpoints/" uses the checkpoint's own directory (infer_seg_voc.output_dirs' rule); no model path uses
    ./lam_cams/<infer_set>/<infer_set>_none_<tag>_..."""
    tag = ("lam_training_free" if training_free else "lam_optimized") + ("/aff_lam" if refine_with_aff else "/seeds_lam")
    if not model_path:
        root, ckpt = DEFAULT_CAM_ROOT, "none"
    elif "checkpoints/" in model_path:
        root, ckpt = model_path.split("checkpoints/")[0], model_path.split("checkpoints/")[-1]
    else:
        root, ckpt = os.path.dirname(os.path.abspath(model_path)), os.path.basename(model_path)
    ckpt = ckpt.replace(".pth", "")
    base = os.path.normpath(os.path.join(root, infer_set))
    return {"tag": tag, "cam_dir": os.path.join(base, f"{infer_set}_{ckpt}_{tag}_img"),
            "cs_cam_dir": os.path.join(base, f"{infer_set}_{ckpt}_{tag}_class_specific_img")}


def label_output_dir(model_path, infer_set, training_free=True, refine_with_aff=True):
    """Where --save_label writes without --label_dir: next to cam_output_dirs' directories, <infer_set>_<ckpt>_<tag>_label."""
    return cam_output_dirs(model_path, infer_set, training_free, refine_with_aff)["cam_dir"][:-len("_img")] + "_label"


def conf_label_output_dir(model_path, infer_set, training_free=True, refine_with_aff=True):
    """Where --conf_label writes without --conf_label_dir: <infer_set>_<ckpt>_<tag>_conf_label, next to label_output_dir's directory."""
    return label_output_dir(model_path, infer_set, training_free, refine_with_aff)[:-len("_label")] + "_conf_label"


LABEL_WRITERS = 2        # threads that only open / write / close the device-encoded files


def default_cam_writers(local_world=1):
    """JPEG encoder threads per rank: a quarter of this rank's CPU share (at least 1).  The decode pool gives these up (build_validation)."""
    return max(1, host_cpu_budget() // max(local_world, 1) // 4)


def class_names(args):
    """The data set's own class list (index 0 = background); with --class_names, the file's."""
    vocab = flag_defaults(args).vocab
    if vocab and vocab.get("fg"):
        return [VOC_CLASSES[0]] + list(vocab["fg"])
    if "coco" in args.dataset_name:
        from ..datasets import coco
        return coco.class_list
    return VOC_CLASSES


class _CamSaver:
    """--save_cam: device overlays of a batch / an image -> JPEG files through imutils.CamOverlayWriter (host encoder), or with
    device_jpeg=True through ops.jpeg_encode_rgb_ragged and imutils.CamJpegWriter: the files are encoded on the device into a grow-only
    arena, only its bytes cross, threads only write.  The first arena has the raw size of the overlays (the bound); once a batch has
    landed, the arena is budgeted by the largest file / raw ratio seen (plus a quarter), and an overlay that does not fit is encoded on
    the host by the writer - the same bytes either way."""

    def __init__(self, args, writers, device_jpeg=False):
        from ..utils import imutils
        self.per_class = bool(flag_defaults(args).save_cls_specific_cam)
        self.mode = "per_class" if self.per_class else "max"
        dirs = cam_output_dirs(args.model_path, args.infer_set, bool(args.training_free), bool(args.refine_with_aff))
        self.dir = (args.cs_cam_dir or dirs["cs_cam_dir"]) if self.per_class else (args.cam_dir or dirs["cam_dir"])
        os.makedirs(self.dir, exist_ok=True)
        self.names = class_names(args)
        self.device_jpeg = bool(device_jpeg)
        self.writer = imutils.CamJpegWriter(LABEL_WRITERS) if self.device_jpeg else imutils.CamOverlayWriter(writers)
        self._arena = self._ws = None
        self.batches = self.copied = 0       # batches with overlays; bytes they sent to the host

    def _encode(self, out, items):
        from .. import ops
        paths, geo = [it[0] for it in items], [it[1:] for it in items]
        hw = [(H, W) for _, H, W in geo]
        budget = ops.jpeg_rgb_arena_bytes(hw)
        if self.writer.ratio is not None:
            raw = sum(3 * H * W for H, W in hw)
            budget = min(budget, len(hw) * (ops.JPEG_HEADER_BYTES + 2) + int(raw * min(1.0, 1.25 * self.writer.ratio + 0.02)))
        if self._arena is None or self._arena.numel() < budget:
            self._arena = torch.empty(budget, dtype=torch.uint8, device=out.device)
        ws_need = ops.jpeg_rgb_workspace_bytes(hw)
        if self._ws is None or self._ws.numel() < ws_need:
            self._ws = torch.empty(ws_need, dtype=torch.uint8, device=out.device)
        from ..utils import imutils
        data, table = ops.jpeg_encode_rgb_ragged(out, geo, imutils.CAM_JPEG_QUALITY, out=self._arena[:budget], ws=self._ws)
        self.writer.submit(data, table, paths, geo, out)

    def _items(self, name, present, H, W, off):
        if not self.per_class:
            return [(os.path.join(self.dir, name + ".jpg"), int(off), H, W)] if len(present) else []
        return [(os.path.join(self.dir, f"{name}_{self.names[int(c) + 1].replace('/', '_')}.jpg"), int(off) + 3 * j * H * W, H, W) for j, c in enumerate(present)]

    def ragged(self, names, plan, images, cams, Cmax, cls_host):
        from .. import ops
        present = [np.flatnonzero(row != 0) for row in cls_host]              # cls_compact's order
        out, off = ops.cam_overlay_ragged(images, cams, plan, Cmax, [len(p) for p in present], self.mode)
        items = []
        for b, name in enumerate(names):
            items += self._items(str(name), present[b], int(plan.hw[b, 0]), int(plan.hw[b, 1]), off[b])
        if not items:
            return
        self.batches += 1
        if self.device_jpeg:
            self._encode(out, items)
            self.copied = self.writer.copied
        else:
            self.writer.submit(out, items)
            self.copied += int(out.numel())

    def image(self, name, hwc, normed, cls_lst):
        from .. import ops
        out = ops.cam_overlay(hwc, normed, self.mode)
        if out is not None:
            H, W = int(normed.shape[1]), int(normed.shape[2])
            self.writer.submit(out.view(-1), self._items(str(name), np.asarray(cls_lst.cpu() if hasattr(cls_lst, "cpu") else cls_lst), H, W, 0))

    def barrier(self):
        self.writer.barrier()

    def close(self):
        return self.writer.close()


class _LabelSaver:
    """--save_label: the step's labels -> PNG files, encoded on the device (ops.png_encode_labels_ragged), written by imutils.LabelPngWriter.
    The arena and the row records live in grow-only buffers: the copy into the writer's pinned ring is queued on the same stream in
    front of the next step's encoder, so one arena is enough."""

    def __init__(self, args, directory=None):
        from ..utils import imutils
        self.dir = directory or flag_defaults(args).label_dir or label_output_dir(args.model_path, args.infer_set, bool(args.training_free),
                                                                   bool(args.refine_with_aff))
        os.makedirs(self.dir, exist_ok=True)
        self.writer = imutils.LabelPngWriter(LABEL_WRITERS)
        self._arena = self._ws = None

    def ragged(self, names, plan, labels_flat):
        from .. import ops
        if not labels_flat.is_cuda:
            raise RuntimeError("--save_label encodes on the device: it needs GPU labels")
        need = ops.png_labels_arena_bytes(plan.hw)
        if self._arena is None or self._arena.numel() < need:
            self._arena = torch.empty(need, dtype=torch.uint8, device=labels_flat.device)
        ws_need = int(ops.lib().excel_png_labels_workspace_bytes(plan.B, int(plan.hw[:, 0].max())))
        if self._ws is None or self._ws.numel() < ws_need:
            self._ws = torch.empty(ws_need, dtype=torch.uint8, device=labels_flat.device)
        data, table = ops.png_encode_labels_ragged(labels_flat, plan, out=self._arena, ws=self._ws)
        self.writer.submit(data, table, [os.path.join(self.dir, str(n) + ".png") for n in names])

    def uniform(self, names, labels):
        """labels [B,H,W] uint8 (device): the same entry over a plan of equal sizes."""
        from .. import ops
        B, H, W = labels.shape
        self.ragged(names, ops.RaggedPlan([(H, W)] * B, labels.device), labels.contiguous().view(-1))

    def barrier(self):
        self.writer.barrier()

    def close(self):
        return self.writer.close()


CRF_PARAMS = dict(iter_max=10, pos_w=3, pos_xy_std=1, bi_w=4, bi_xy_std=67, bi_rgb_std=3)     # tools/infer_lam.py:191-198
CRF_RGB_WRITERS = 2      # threads that colour-code and save the --segs_crf_rgb_dir images


def crf_inline_wanted(args):
    """--crf_post true --crf_inline true, except for a test split (the reference scores against image[:,:,0] there, :213-214)."""
    return bool(flag_defaults(args).crf_post) and bool(args.crf_inline) and "test" not in str(args.infer_set)


def _save_crf_rgb(path, lab):
    from PIL import Image
    from ..utils import imutils
    Image.fromarray(imutils.encode_cmap(lab)).save(path)                                    # :228


class _CrfInline:
    """--crf_inline: the DenseCRF stage of :179-237 on the step's own cams, right after the step and on its stream.  Labels go into a
    device-side confusion matrix (`hist`), into palette PNGs (--crf_label_dir, device encoder) and, from one device-to-host copy of the
    batch's labels made only then, into the colour-coded files of --segs_crf_rgb_dir (a small thread pool)."""

    def __init__(self, args, device):
        self.nc = flag_defaults(args).num_classes
        self.hist = torch.zeros((self.nc, self.nc), dtype=torch.int64, device=device)
        self.budget = int(float(args.crf_ws_gb) * 2 ** 30)
        self.groups, self.calls, self.peak_ws = 0, 0, 0
        self.lab = self.pool = None
        self.futures = []
        from ..utils import image_scores as _scores
        self.image_scores = _scores.wanted(args)         # --per_image_scores / --boundary_scores: a ScoreTicket ("crf") per call
        self.boundary = _scores.boundary_of(args)
        self.last_score_ticket = None
        if args.crf_label_dir:
            self.lab = _LabelSaver(args, args.crf_label_dir)
        self.rgb_dir = args.segs_crf_rgb_dir
        if self.rgb_dir:
            from concurrent.futures import ThreadPoolExecutor
            os.makedirs(self.rgb_dir, exist_ok=True)
            self.pool = ThreadPoolExecutor(CRF_RGB_WRITERS)

    def _rgb(self, names, plan, labels_flat):
        host = labels_flat.cpu().numpy()                                                    # the one copy, only when the files are asked for
        self.futures = [f for f in self.futures if not f.done() or f.result() is not None]  # (a finished writer's error is raised here)
        for b, name in enumerate(names):
            H, W, o = int(plan.hw[b, 0]), int(plan.hw[b, 1]), int(plan.loff[b])
            self.futures.append(self.pool.submit(_save_crf_rgb, os.path.join(self.rgb_dir, str(name) + ".png"), host[o:o + H * W].reshape(H, W)))

    def ragged(self, names, plan, images, cams, Cmax, nchan, nchan_host, cls_idx, gts_packed, skip=None):
        """`skip`: the step's per-image overflow flags (device int32 [B]) - flagged images stay out of `hist` - or None."""
        from .. import ops
        P = CRF_PARAMS
        labels, _ = ops.dcrf_lam_ragged(images, plan, cams, Cmax, nchan, nchan_host, cls_idx, P["iter_max"], P["pos_w"], P["pos_xy_std"],
                                        P["bi_w"], P["bi_xy_std"], P["bi_rgb_std"], want_labels=True, want_q=False, budget_bytes=self.budget)
        self.calls += 1
        self.groups += int(getattr(ops.dcrf_lam_ragged, "last_groups", 1))
        self.peak_ws = max(self.peak_ws, int(getattr(ops.dcrf_lam_ragged, "last_workspace_bytes", 0)))
        if gts_packed is not None and skip is not None:
            self.hist = ops.confusion_accumulate_masked(gts_packed, labels, self.nc, skip, self.hist, plan=plan)
        elif gts_packed is not None:
            self.hist = ops.confusion_accumulate(gts_packed, labels, self.nc, self.hist)    # :233
        if self.image_scores and gts_packed is not None:
            from ..pipeline import ScoreTicket
            self.last_score_ticket = ScoreTicket().launch("crf", gts_packed, labels, self.nc, skip=skip, plan=plan, boundary=self.boundary)
        if self.lab is not None:
            self.lab.ragged(names, plan, labels)
        if self.pool is not None:
            self._rgb(names, plan, labels)
        return labels

    def image(self, name, hwc, normed, cls_lst, gt):
        """The per-image path (--api_path true): :221-226 on the image's own normed maps, without a record."""
        from .. import ops
        P = CRF_PARAMS
        if hwc.dtype != torch.uint8:
            raise ValueError("--crf_inline needs the decoded uint8 images (--data_folder, --ragged true or --u8_input true)")
        q = ops.dcrf_inference(hwc, normed, P["iter_max"], P["pos_w"], P["pos_xy_std"], P["bi_w"], P["bi_xy_std"], P["bi_rgb_std"])   # :221
        keys = torch.nn.functional.pad(torch.as_tensor(cls_lst, device=q.device).to(torch.int64).view(-1) + 1, (1, 0))     # :225
        labels = keys[q.argmax(0)].to(torch.uint8)                                          # :222, :226
        self.calls += 1
        self.groups += 1
        self.hist = ops.confusion_accumulate(gt.to(torch.uint8), labels, self.nc, self.hist)                                  # :233
        if self.image_scores:
            from ..pipeline import ScoreTicket
            self.last_score_ticket = ScoreTicket().launch("crf", gt.to(torch.uint8)[None], labels[None], self.nc, boundary=self.boundary)
        plan = None
        if self.lab is not None:
            self.lab.uniform([name], labels[None])
        if self.pool is not None:
            plan = ops.RaggedPlan([tuple(labels.shape)], None)
            self._rgb([name], plan, labels.view(-1))
        return labels

    def barrier(self):
        """Every file queued so far is on disk (a writer's error is raised)."""
        for f in self.futures:
            f.result()
        self.futures = []
        if self.lab is not None:
            self.lab.barrier()

    def close(self):
        err = None
        if self.pool is not None:
            self.pool.shutdown(wait=True)
            for f in self.futures:
                err = err or f.exception()
        if self.lab is not None:
            self.lab.close()
        if err is not None:
            raise err


# ------------------------------------------------------------------ sharding + the one collective
def shard_indices(n, rank, world):
    """Subset(np.arange(i, len, n_gpus)) (tools/infer_lam.py:166)."""
    return np.arange(rank, n, world)


def host_cpu_budget():
    """CPUs this process may really use: the affinity mask capped by the container's cgroup-v2 quota (`cpu.max`; the GPU boxes of this
    project report 256 logical CPUs and grant 16)."""
    n = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 1)
    try:
        q, per = open("/sys/fs/cgroup/cpu.max").read().split()
        if q != "max":
            n = min(n, max(1, int(int(q) / int(per))))
    except (OSError, ValueError):
        pass
    return n


def default_decode_workers(local_world=1):
    """Decode threads per rank: this rank's share of the CPU budget minus the launching thread, between 2 and 16 (measured: 16 threads are
    best for one rank on 16 granted CPUs, 8 per rank for 8 ranks)."""
    return max(2, min(16, host_cpu_budget() // max(local_world, 1) - (1 if local_world > 1 else 0)))


def pin_rank_to_cores(local_rank, local_world):
    """Give local rank r of R its own contiguous share of the CPUs this process may run on (os.sched_setaffinity): the decode pool and
    the launch thread of a rank then stay off the other ranks' cores (8 ranks x 16 decode threads + 8 launch threads on one host,
    BASELINE configs[3]).  -> the core set, or None when there are fewer cores than ranks / the platform has no affinity call."""
    if not hasattr(os, "sched_setaffinity") or local_world <= 1:
        return None
    cores = sorted(os.sched_getaffinity(0))
    if len(cores) < local_world:
        return None
    per = len(cores) // local_world
    mine = set(cores[local_rank * per:(local_rank + 1) * per])
    os.sched_setaffinity(0, mine)
    return mine


def gather_hists(hist, group=None):
    """all_gather of the per-rank [nc,nc] int64 confusion matrices -> ([R,nc,nc], summed [nc,nc]).
    One small message per rank (3.5 KB VOC / 52 KB COCO): latency-bound, issued once per evaluation.
    With a process group the collective always runs - also over a single rank (RCCL on one GPU: the same call path as N > 1, which is
    what the 1-GPU hardware tests and `bench.py --gpus 1` exercise); without one the matrix is returned as it is."""
    if not (dist.is_available() and dist.is_initialized()):
        return hist[None], hist
    world = dist.get_world_size(group)
    parts = [torch.empty_like(hist) for _ in range(world)]
    dist.all_gather(parts, hist.contiguous(), group=group)
    stacked = torch.stack(parts, 0)
    return stacked, stacked.sum(0)


def format_scores_table(score, cat_list, metric_names=("confusion", "precision", "recall", "iou")):
    """The table of utils/pyutils.py:37-58 (format_tabs_multi_metircs) without the texttable dependency."""
    rows = [["Class"] + list(metric_names)]
    vals = np.array([list(score[m].values()) for m in metric_names], np.float64)
    for i in range(vals.shape[1]):
        rows.append([cat_list[i] if i < len(cat_list) else str(i)] + [f"{v:.4f}" for v in vals[:, i]])
    rows.append(["average_metrics"] + [f"{v:.4f}" for v in vals.mean(1)])
    widths = [max(len(r[c]) for r in rows) for c in range(len(rows[0]))]
    line = "+" + "+".join("-" * (w + 2) for w in widths) + "+"
    out = [line]
    for i, r in enumerate(rows):
        out.append("|" + "|".join(" " + r[c].ljust(widths[c]) + " " for c in range(len(r))) + "|")
        if i == 0 or i == len(rows) - 2:
            out.append(line)
    out.append(line)
    return "\n".join(out)


# ------------------------------------------------------------------ the loop
def _check_present_classes(batches, smax):
    """The compacted class list of an image has `smax` slots (the kernels clamp to it): an image with MORE present classes than the data
    set's max_k() promised would silently lose the extra ones - refuse it instead, on the host, from the batch's own one-hot rows."""
    for rb in batches:
        k = rb.cls.sum(1)
        if int(k.max()) > smax:
            b = int(k.argmax())
            raise RuntimeError(f"{rb.names[b]}: {int(k[b])} present classes, the pipeline was built for at most {smax} (dataset.max_k()): "
                               "build the pipeline with a larger smax")
        yield rb


def build_validation(model=None, par=None, dataset=None, indices=None, device="cuda", args=None, pipe=None):
    """-> (hist [nc,nc] int64 on device, images processed, seconds).  Mirrors :63-128.  Everything the run depends on is resolved here,
    once, into `run`, for one of the two loops below; the run's `report` is published in build_validation.last_* on the way out."""
    from types import SimpleNamespace
    from ..pipeline import OptimisedLamPipeline, TrainingFreePipeline
    flag_defaults(args)
    # the optimised-LAM regime runs batched on ragged batches; uniform synthetic batches keep its per-image call sequence
    per_image = args.api_path or (not args.training_free and not args.ragged_batches)
    ragged = bool(args.ragged_batches) and not per_image
    on_gpu = torch.device(device).type == "cuda"
    # the overflow guard of the f16 modes: resolved from the mode the handle is in NOW (after the start-up check)
    mode = _handle_gemm_mode(model if pipe is None else getattr(pipe, "model", None))
    policy = resolve_overflow_guard(args.overflow_guard, mode, on_gpu, not per_image)
    tta_scales, tta_flip = resolve_tta(args)
    conf = resolve_conf(args)
    tagger = resolve_tags(args, have_dataset=True)
    from ..utils import image_scores
    image_scores.refuse(args, unlabeled=bool(args.unlabeled))
    want_scores, boundary = image_scores.wanted(args), image_scores.boundary_of(args)
    from ..utils import bkg_sweep
    sweep, bkg_scale = bkg_sweep.resolve(args)
    if (sweep is not None or bkg_scale != 1.0) and not ragged:
        raise ValueError(f"{'--bkg_sweep' if sweep is not None else '--bkg_scale'} runs behind the ragged step: ragged batches (--data_folder or "
                         "--ragged true) on the batched loop")
    bkg_kw = {**({"bkg_sweep": sweep} if sweep is not None else {}), **({"bkg_scale": bkg_scale} if bkg_scale != 1.0 else {})}
    # the label stages that are on: name -> resolved flags (utils/label_stages.py); each runs behind the ragged step
    from ..utils import label_stages
    from ..utils import margin as margin_mod
    stages, asked = {}, {}                                   # asked: pipeline keyword -> (the flag that asks for it, its value)
    for name in label_stages.INFER_LAM_ORDER:
        stage = label_stages.STAGES[name]
        resolved = stage.resolve(args, ragged=ragged)
        if resolved is None:
            continue
        if not ragged:
            raise ValueError(f"{stage.flag} runs behind the ragged step: ragged batches (--data_folder or --ragged true) on the batched loop")
        stages[name], asked[stage.kwarg] = resolved, (stage.flag, label_stages.pipeline_value(stage, resolved))
    msweep = margin_mod.resolve(args, ragged=ragged)[0]
    if msweep is not None:
        asked["margin_sweep"] = ("--margin_sweep", msweep)
    bkg_kw = {**bkg_kw, **{k: want for k, (_, want) in asked.items()}}
    if pipe is None:
        kw = dict(num_classes=args.num_classes, dilations=par.dilations, num_iter=par.num_iter, caa_thre=0.79,
                  smax=dataset.max_k() if tagger is None else tagger["kmax"], guard="skip" if policy in ("raise", "rerun") else None,
                  image_scores=want_scores, **({"boundary": boundary} if boundary is not None else {}), **bkg_kw)
        if args.training_free:
            pipe = TrainingFreePipeline(model, tta_scales=tta_scales, tta_flip=tta_flip, tagger=tagger, **kw)
        elif ragged:
            pipe = OptimisedLamPipeline(model, **kw)
    elif policy != "off" and getattr(pipe, "guard", None) is None:
        # a caller's pipeline keeps the guard it was built with: without one there are no flags to act on
        logging.warning(f"--overflow_guard {policy}: the supplied pipeline was built without a guard - running unguarded")
        policy = "off"
    if want_scores and pipe is not None and not per_image and not getattr(pipe, "image_scores", False):
        raise ValueError("--per_image_scores: the supplied pipeline was built without image_scores=True")
    if boundary is not None and pipe is not None and not per_image and getattr(pipe, "boundary", None) != boundary:
        raise ValueError(f"--boundary_scores: the supplied pipeline was built with boundary={getattr(pipe, 'boundary', None)!r}, the flags ask for {boundary!r}")
    for k, (flag, want) in asked.items():
        if pipe is not None and getattr(pipe, k, None) != want:
            raise ValueError(f"{flag}: the supplied pipeline was built with {k}={getattr(pipe, k, None)!r}, the flags ask for {want!r}")
    for k, want in (("bkg_sweep", sweep), ("bkg_scale", bkg_scale)):
        if (sweep is not None or bkg_scale != 1.0) and pipe is not None and getattr(pipe, k, None if k == "bkg_sweep" else 1.0) != want:
            raise ValueError(f"--{k}: the supplied pipeline was built with {k}={getattr(pipe, k, None)!r}, the flags ask for {want!r}")
    report = dict(guard={"policy": policy, "mode": mode, "checked": 0, "flagged": [], "rerun": 0, "nonfinite_in_f32": []},
                  crf_hist=None, crf_stats=None, cam_stats=None, conf_hist=None, tags=None, image_scores=None, bkg_sweep=None,
                  **{name: None for name in label_stages.STAGES})
    local_world = int(os.environ.get("LOCAL_WORLD_SIZE", os.environ.get("WORLD_SIZE", 1)))
    run = SimpleNamespace(model=model, par=par, dataset=dataset, indices=indices, device=device, args=args, pipe=pipe, S=args.resize_size,
                          on_gpu=on_gpu, ragged=ragged, tta=(tta_scales, tta_flip), conf=conf, tagger=tagger, guard=report["guard"], report=report, sweep=sweep, stages=stages, msweep=msweep,
                          local_world=local_world, writers=default_cam_writers(local_world) if args.save_cam else 0,
                          hist=torch.zeros((args.num_classes, args.num_classes), dtype=torch.int64, device=device), t0=time.time(),
                          consumers={})       # cam, lab, crf, conf_lab: those that exist, in the order the re-run barrier and the close take them
    # --per_image_scores: the rank's table of per-image counts, one set per matrix the run scores (utils/image_scores.py)
    run.scores = report["image_scores"] = image_scores.ImageScoreLog(
        args.num_classes, ["main"] + (["conf"] if conf is not None else []) + (["crf"] if crf_inline_wanted(args) else [])
        + ([] if args.unlabeled else list(stages)), boundary=boundary,
        rows=[label_stages.STAGES[name].rows.key for name in stages if label_stages.STAGES[name].rows is not None]) if want_scores else None
    try:
        for wanted, needs in ((args.save_cam, "--save_cam needs the decoded images"), (conf is not None, "--conf_label runs behind the ragged step"),
                              (crf_inline_wanted(args), "--crf_inline needs the decoded images")):
            if wanted and not (ragged or per_image):
                raise ValueError(f"{needs}: ragged batches (--data_folder or --ragged true) or the per-image path "
                                 "(--api_path true / --training_free false)")
        if args.save_cam:
            run.consumers["cam"] = _CamSaver(args, run.writers, device_jpeg=bool(args.cam_device_jpeg) and ragged)
        if args.save_label:
            run.consumers["lab"] = _LabelSaver(args)
        if crf_inline_wanted(args):
            run.consumers["crf"] = _CrfInline(args, device)
        if conf is not None:
            run.consumers["conf_lab"] = _LabelSaver(args, args.conf_label_dir or conf_label_output_dir(
                args.model_path, args.infer_set, bool(args.training_free), bool(args.refine_with_aff)))
        for name, resolved in stages.items():
            if resolved["label_dir"]:
                run.consumers[name + "_lab"] = _LabelSaver(args, resolved["label_dir"])
        out = (_per_image_loop if per_image else _batched_loop)(run)
    except BaseException:
        _close_consumers(run, failed=True)
        raise
    else:
        _close_consumers(run, failed=False)      # every file on disk (and a writer's error raised) before the scores are reported
    finally:
        build_validation.last_guard, build_validation.last_crf_hist, build_validation.last_crf_stats, build_validation.last_cam_stats, \
            build_validation.last_conf_hist = (report[k] for k in ("guard", "crf_hist", "crf_stats", "cam_stats", "conf_hist"))
        for k in ("tags", "image_scores", "bkg_sweep", *label_stages.STAGES):
            setattr(build_validation, "last_" + k, report[k])
    return out


def _close_consumers(run, failed):
    """Every consumer is closed once, on every path, and the overlay statistics are recorded.  After a loop that ran through, the first
    writer's error is raised and only a clean close hands out the CRF stage's matrix; after one that `failed`, the loop's own exception stays."""
    first = None
    for c in run.consumers.values():
        try:
            c.close()
        except Exception as e:
            first = first or e
    cam, crf = run.consumers.get("cam"), run.consumers.get("crf")
    if cam is not None:
        run.report["cam_stats"] = dict(device_jpeg=cam.device_jpeg, files=getattr(cam.writer, "files", 0), batches=cam.batches,
                                       bytes_to_host=cam.copied, host_fallbacks=getattr(cam.writer, "fallbacks", 0))
    if first is not None and not failed:
        raise first
    if crf is not None and not failed:
        run.report["crf_hist"] = crf.hist
        run.report["crf_stats"] = dict(calls=crf.calls, groups=crf.groups, peak_workspace_bytes=crf.peak_ws)


def _per_image_loop(run):
    """The reference's call sequence, image by image (--api_path true, and --training_free false on uniform synthetic batches)."""
    from ..utils import evaluate
    from ..utils.affutils import refine_cams_with_aff, refine_cams_with_bkg_weclip
    from .. import ops
    args, model, par, dataset, indices, device, S = run.args, run.model, run.par, run.dataset, run.indices, run.device, run.S
    training_free, tta, conf, hist = args.training_free, run.tta, run.conf, run.hist
    cam, lab, crf, conf_lab = (run.consumers.get(k) for k in ("cam", "lab", "crf", "conf_lab"))
    from ..pipeline import ScoreTicket
    scores = run.scores
    boundary = scores.boundary if scores is not None else None
    nimg, hist_conf = 0, None
    for s in range(0, len(indices)):
        names, imgs, gts, cls = dataset.batch(indices[s:s + 1])
        inputs = torch.from_numpy(imgs).to(device, non_blocking=True)
        if cam is not None and inputs.dtype != torch.uint8:
            raise ValueError("--save_cam needs the decoded uint8 images (--data_folder, --ragged true or --u8_input true)")
        decoded = inputs
        if inputs.dtype == torch.uint8:                                                     # decoded images: normalise on the device
            inputs = ops.normalize_img_u8(inputs)                                           # datasets/voc.py:115-116
        full = inputs                                                                       # (what --cam_scales resizes the other scales from)
        if inputs.shape[-2:] != (S, S):
            inputs = ops.bilinear_resize(inputs, S, S, align_corners=False)                 # :74
        cls_labels = torch.from_numpy(cls).to(device, non_blocking=True)
        gt_dev = torch.from_numpy(gts).to(device, non_blocking=True)
        if training_free:
            _, _, attr_maps_raw, attn_weights, attn_pred = model(inputs)                    # :79
            if tta[0] is not None:                                                          # :82, the same fuse as the batched step
                from ..utils.camutils import tta_attr_map
                attr_maps_raw = tta_attr_map(model, inputs, tta[0], tta[1], source=full)
        else:
            # optimised-LAM regime (:84-85, :91): needs the caller's decoder as model.feature_head
            from ..utils.camutils import cure_attr_map_flip
            _, _, _, attn_weights, attn_pred = model(inputs, n_attn_out=6)                  # :79
            if attn_pred is None:
                raise RuntimeError("--training_free false needs model.feature_head (the learned decoder, SURVEY 8f #2)")
            attr_maps_raw = cure_attr_map_flip(model, inputs)                               # :85
        for i, attr_map in enumerate(attr_maps_raw):                                        # :88
            rec = ([int(indices[s + i])], [names[i]], [gts.shape[-2:]])                     # what --per_image_scores files the counts under
            seg_attn = None if training_free else attn_pred[i][None]                        # :91-92
            refined, cls_lst = refine_cams_with_aff(attr_map, attn_weights[:, i], cls_labels[i], size=inputs.shape[2:],
                                                    seg_attn=seg_attn, caa_thre=0.79)       # :93
            labels, normed = refine_cams_with_bkg_weclip(refined, inputs[i], cls_lst, par, gts.shape[-2:])   # :94
            if crf is not None:                                                             # :179-237 without a record
                crf.image(str(names[i]), decoded[i], normed, cls_lst, gt_dev[i])
                if scores is not None:
                    scores.defer(crf.last_score_ticket, *rec)
            elif args.crf_post:                                                             # :116-119 record for the CRF stage
                from ..utils import imutils
                imutils.save_logits(args.logits_dir, str(names[i]), normed, cls_lst, run_token=args.run_token)
            if cam is not None:                                                             # :97-111
                cam.image(names[i], decoded[i], normed, cls_lst)
            hist = evaluate.hist_from_labels([gt_dev[i]], [labels[0]], args.num_classes, device, hist)
            if scores is not None:                                                          # the op with B = 1, behind a ticket: no wait here
                scores.defer(ScoreTicket().launch("main", gt_dev[i].to(torch.uint8)[None], labels[:1].to(torch.uint8), args.num_classes, boundary=boundary), *rec)
            if lab is not None:                                                             # :95 (uint8 as hist_from_labels scores them)
                lab.uniform([names[i]], labels[:1].to(torch.uint8))
            if conf is not None:                                                            # affutils.py:101-158 on the image's own cams
                from ..utils.affutils import conf_labels_image
                kept = conf_labels_image(par, inputs[i], normed, cls_lst, conf[0], conf[1])
                hist_conf = ops.confusion_accumulate(gt_dev[i].to(torch.uint8), kept, args.num_classes, hist_conf)
                if scores is not None:
                    scores.defer(ScoreTicket().launch("conf", gt_dev[i].to(torch.uint8)[None], kept[None], args.num_classes, boundary=boundary), *rec)
                conf_lab.uniform([names[i]], kept[None])
        nimg += len(imgs)
    torch.cuda.synchronize()
    if scores is not None:
        scores.poll(True)
    run.report["conf_hist"] = hist_conf
    return hist, nimg, time.time() - run.t0


def _batched_loop(run):
    """The batched loop of build_validation: one pass over `indices`, and with the overflow guard's `rerun` policy a second pass in exact
    fp32 over the images the first one flagged - the same loop body (`steps`) and the same consumers both times."""
    from collections import deque
    from .. import ops
    args, dataset, indices, device, pipe, S, on_gpu = run.args, run.dataset, run.indices, run.device, run.pipe, run.S, run.on_gpu
    ragged, guard, conf, tagger = run.ragged, run.guard, run.conf, run.tagger
    truth_known = bool(getattr(dataset, "has_cls_labels", True))      # the samples' one-hot rows are image-level labels (not placeholders)
    step_cls = [None]           # the host one-hot rows of the step enqueued last
    step_hw = [None]            # ... and its label sizes [(H, W)] (--per_image_scores)
    scores = run.scores
    cam, lab, crf, conf_lab = (run.consumers.get(k) for k in ("cam", "lab", "crf", "conf_lab"))
    policy = guard["policy"]
    pipe.hist = run.hist
    if conf is not None:
        pipe.hist_conf = torch.zeros_like(run.hist)
    if run.sweep is not None:                                # --bkg_sweep: the pipeline adds every step's counts per scale (both passes of the guard)
        pipe.sweep_totals = torch.zeros((len(run.sweep), 3, args.num_classes), dtype=torch.int64, device=device)
    # the label stages that are on (utils/label_stages.py): the matrix of each, the PNG writers of those with a label directory, and
    # per set of per-image rows: the queue of (pinned counts, event, dataset indices, names, sizes) and the rows read, index: (name, row)
    from ..utils.label_stages import STAGES
    for name in run.stages:
        setattr(pipe, "hist_" + name, torch.zeros_like(run.hist))
    stage_labs = [(name, run.consumers[name + "_lab"]) for name in run.stages if name + "_lab" in run.consumers]
    row_sets = {name: (deque(), {}) for name in run.stages if STAGES[name].rows is not None}
    row_pix = {}                                             # index: the pixels of the image (the share of pixels the snap changed)
    if run.msweep is not None:                               # --margin_sweep: the pipeline adds every step's counts per threshold (both passes of the guard)
        pipe.margin_kept = torch.zeros((len(run.msweep) + 1,), dtype=torch.int64, device=device)
        pipe.margin_totals = None if args.unlabeled else torch.zeros((len(run.msweep), 3, args.num_classes), dtype=torch.int64, device=device)
    if ragged:
        # every sample at its own size: decode in background workers, everything else on the device, one launch per stage
        from ..datasets.loader import DeviceFeeder, ragged_batches, threaded_batches
        from ..utils import imutils
        keep = bool(args.crf_post) and crf is None           # the record path of the CRF stage; --crf_inline needs no copies
        nw = int(args.num_workers)
        if nw < 0:                                           # the JPEG encoders of --save_cam share this rank's CPUs
            nw = max(2, default_decode_workers(run.local_world) - run.writers)

    def feed_of(idxs):
        if args.decode == "processes" and nw > 0:                           # the reference's mechanism (DataLoader worker processes, :167)
            batches = ragged_batches(dataset, idxs, args.batch_size, num_workers=nw, pin_memory=False)
        else:                                                               # default: a thread pool (datasets/loader.threaded_batches)
            batches = threaded_batches(dataset, idxs, args.batch_size, num_threads=max(nw, 1))
        if tagger is None:                                    # (predicted tags are capped at smax by the tagger itself)
            batches = _check_present_classes(batches, pipe.smax)
        if on_gpu:
            return DeviceFeeder(batches, device)              # H2D on a copy stream, a few batches ahead

        def on_host(rb):                                      # (control-flow tests: a stub pipeline on CPU tensors)
            plan = ops.RaggedPlan(rb.hw, None)
            plan.cls_host = rb.cls.numpy().copy()             # what DeviceFeeder attaches
            return rb.names, plan, rb.images, rb.cls, rb.labels
        return map(on_host, batches)

    def ragged_step(names, plan, images, cls_t, labels_t):
        step_cls[0] = getattr(plan, "cls_host", None)
        step_hw[0] = plan.hw
        if conf is None:
            out = pipe.run_batch_ragged(images, plan, cls_t, labels_t, S=S, return_intermediates=keep)
        else:                                                                           # affutils.py:101-158, same stream, step's own cams
            plan.conf_half = ops.conf_half_plan(plan, names=names)                      # (an image too small to halve is refused by name; the step reuses the plan)
            main, kept, *rest = pipe.run_batch_ragged(images, plan, cls_t, labels_t, S=S, return_intermediates=keep, conf=conf)
            out = (main, rest[0]) if keep else main
            conf_lab.ragged(names, plan, kept)
        if cam is not None:                                                             # :97-111, same stream, step's own cams
            cam.ragged(names, plan, images, pipe.last_cams, pipe.smax + 1, plan.cls_host)
        if crf is not None:                                                             # :179-237, same stream, step's own cams
            nchan_host = np.minimum((plan.cls_host != 0).sum(1), pipe.smax).astype(np.int32) + 1
            skip = pipe.last_flags if getattr(pipe, "guard", None) == "skip" else None  # flagged images stay out of the CRF scores too
            crf.ragged(names, plan, images, pipe.last_cams, pipe.smax + 1, pipe.last_nchan, nchan_host, pipe.last_cls_idx, labels_t, skip)
        if lab is not None:                                                             # :95, same stream, the labels just scored
            lab.ragged(names, plan, out[0] if keep else out)
        for name, stage_lab in stage_labs:                                              # same stream, the maps each stage left of this step
            stage_lab.ragged(names, plan, getattr(pipe, f"last_{name}_labels"))
        if keep:                                                                        # :116-119 record for the CRF stage
            inter = out[1]
            cls_idx, ncls = inter["cls_idx"].cpu().numpy(), inter["ncls"].cpu().numpy()
            for b, name in enumerate(names):
                k = min(int(ncls[b]), pipe.smax)            # (ncls <= smax is enforced below; the record stays consistent anyway)
                imutils.save_logits(args.logits_dir, name, plan.planes(inter["cams"], b, pipe.smax + 1)[:k + 1], cls_idx[b, :k].astype(np.int64),
                                    run_token=args.run_token)

    def uniform_step(idxs):
        names, imgs, gts, cls = dataset.batch(idxs)
        step_cls[0] = cls
        step_hw[0] = [gts.shape[-2:]] * len(names)
        inputs = torch.from_numpy(imgs).to(device, non_blocking=True)
        if inputs.dtype == torch.uint8:                                                     # decoded images: normalise on the device
            inputs = ops.normalize_img_u8(inputs)                                           # datasets/voc.py:115-116
        if inputs.shape[-2:] != (S, S):
            inputs = ops.bilinear_resize(inputs, S, S, align_corners=False)                 # :74
        cls_labels = torch.from_numpy(cls).to(device, non_blocking=True)
        gt_dev = torch.from_numpy(gts).to(device, non_blocking=True)
        labels = pipe.run_batch(inputs, cls_labels, gt_dev)
        if lab is not None:                                                                 # :95
            lab.uniform(names, labels)
        return names

    def steps(idxs):
        """One pass over `idxs`: every step is enqueued, then its names are yielded."""
        if ragged:
            for names, plan, images, cls_t, labels_t in feed_of(idxs):
                ragged_step(names, plan, images, cls_t, labels_t)
                yield names
        else:
            for s in range(0, len(idxs), args.batch_size):
                yield uniform_step(idxs[s:s + args.batch_size])

    pending = deque()           # (ticket, names, dataset indices) of the steps whose flags have not been read

    def enqueue(names, idxs):
        pending.append((pipe.last_guard, [str(n) for n in names], [int(i) for i in idxs]))

    def score_enqueue(names, idxs):
        """--per_image_scores: the step's tickets (the pipeline's main / conf counts, the CRF stage's) go to the table; a later row of an
        image (the fp32 second pass) replaces the earlier one, which the guard's skip flags left zero."""
        scores.defer(pipe.last_score_ticket, idxs, names, step_hw[0])
        if crf is not None:
            scores.defer(crf.last_score_ticket, idxs, names, step_hw[0])

    def take(wait, found, first_pass=True):
        """Read the tickets that are ready (all of them with `wait`), oldest first: flagged images -> found[dataset index] = name."""
        while pending and (wait or pending[0][0].ready()):
            ticket, names, idxs = pending.popleft()
            flags = np.asarray(ticket.flags()).reshape(-1)
            bad = [b for b in range(len(names)) if flags[b] != 0]
            for b in bad:
                found[idxs[b]] = names[b]
            if first_pass:
                guard["checked"] += len(names)
                guard["flagged"] = [found[i] for i in sorted(found)]
                if bad and policy == "raise":
                    raise RuntimeError(f"--overflow_guard raise: non-finite attribute maps / affinity in GEMM mode {guard['mode']} (an activation "
                                       f"beyond the IEEE-half range 65 504) for {', '.join(names[b] for b in bad)}: run these images in f32 "
                                       "(--overflow_guard rerun, or --gemm_mode f32)")

    # --tags clip: the predicted rows come back behind the step's tag ticket, like the guard's flags; a later row of an image (the
    # fp32 second pass) replaces the earlier one
    tag_pending, tag_rows, tag_truth = deque(), {}, {}

    def tag_enqueue(names):
        ticket = getattr(pipe, "last_tag_ticket", None)
        if ticket is None:
            raise RuntimeError("--tags clip: the pipeline left no last_tag_ticket (it was built without a tagger)")
        tag_pending.append((ticket, [str(n) for n in names], step_cls[0] if truth_known else None))

    def tag_take(wait):
        while tag_pending and (wait or tag_pending[0][0].ready()):
            ticket, names, truth = tag_pending.popleft()
            onehot = np.asarray(ticket.tags()[0])
            for b, n in enumerate(names):
                tag_rows[n] = np.array(onehot[b], np.float32)
                if truth is not None:
                    tag_truth[n] = np.array(truth[b], np.float32)

    def clean_enqueue(names, idxs):
        """The filter's (the fill's, the vote's) per-image counts of the step just enqueued, on their way to the host behind an event (no
        wait here)."""
        for which in row_sets:
            dev = getattr(pipe, f"last_{which}_counts")
            host = torch.empty(dev.shape, dtype=torch.int32, pin_memory=on_gpu)
            host.copy_(dev, non_blocking=True)
            ev = None
            if on_gpu:
                ev = torch.cuda.Event()
                ev.record()
            row_sets[which][0].append((host, ev, [int(i) for i in idxs], [str(n) for n in names], [tuple(int(x) for x in hw) for hw in step_hw[0]]))
        clean_take(False)

    def clean_take(wait):
        """A later row of an image (the fp32 second pass) replaces the earlier one."""
        for which, (pending, rows_of) in row_sets.items():
            while pending and (wait or pending[0][1] is None or pending[0][1].query()):
                host, ev, idxs, names, hws = pending.popleft()
                if ev is not None:
                    ev.synchronize()
                rows = host.numpy()
                for b, i in enumerate(idxs):
                    rows_of[i] = (names[b], rows[b].astype(np.int64))
                    row_pix[i] = hws[b][0] * hws[b][1]
                if scores is not None:
                    scores.put_rows(STAGES[which].rows.key, idxs, names, hws, rows)

    nimg, pos, flagged = 0, 0, {}
    for names in steps(indices):
        if row_sets:
            clean_enqueue(names, indices[pos:pos + len(names)])
        if policy != "off":
            enqueue(names, indices[pos:pos + len(names)])
            take(False, flagged)                              # never a wait inside the loop
        if tagger is not None:
            tag_enqueue(names)
            tag_take(False)
        if scores is not None:
            score_enqueue(names, indices[pos:pos + len(names)])
        pos += len(names)
        nimg += len(names)
    if policy != "off":
        take(True, flagged)
    if flagged:
        logging.warning(f"overflow guard ({guard['mode']}): {len(flagged)} of {guard['checked']} images left the IEEE-half range (non-finite "
                        f"maps): {', '.join(guard['flagged'])}" + (" - running them again in exact fp32" if policy == "rerun" else ""))
    if policy == "rerun" and flagged:
        # every file of the first pass on disk before a flagged image's file is written again: the good one must be the last
        if on_gpu:
            torch.cuda.synchronize()
        for c in run.consumers.values():
            c.barrier()
        order, still = sorted(flagged), {}
        found_guard, pipe.guard = pipe.guard, "observe"       # count again, score everything: fp32's own result is final
        try:
            with pipe.exact_mode():
                pos = 0
                for names in steps(np.asarray(order, dtype=np.asarray(indices).dtype)):
                    enqueue(names, order[pos:pos + len(names)])
                    if row_sets:
                        clean_enqueue(names, order[pos:pos + len(names)])
                    if tagger is not None:
                        tag_enqueue(names)                    # the fp32 row replaces the first pass's
                    if scores is not None:
                        score_enqueue(names, order[pos:pos + len(names)])
                    pos += len(names)
                    guard["rerun"] += len(names)
                take(True, still, first_pass=False)           # (also: the fp32 forwards are done before the mode goes back)
                if on_gpu:
                    torch.cuda.synchronize()
        finally:
            pipe.guard = found_guard
        guard["nonfinite_in_f32"] = [still[i] for i in sorted(still)]
        if still:
            logging.warning(f"overflow guard: {len(still)} images are non-finite in exact fp32 too (kept as fp32 computes them): "
                            f"{', '.join(guard['nonfinite_in_f32'])}")
    if on_gpu:
        torch.cuda.synchronize()
    if conf is not None:
        run.report["conf_hist"] = pipe.hist_conf
    if run.sweep is not None:
        run.report["bkg_sweep"] = pipe.sweep_totals
    clean_take(True)
    for name, (_, rows_of) in row_sets.items():
        run.report[name] = dict(hist=getattr(pipe, "hist_" + name), rows=rows_of)
    if "snap" in row_sets:
        run.report["snap"]["pixels"] = int(sum(row_pix.values()))
    if run.msweep is not None or "margin" in run.stages:      # the sweep's counts travel with the cut's matrix
        run.report["margin"] = dict(totals=pipe.margin_totals, kept=pipe.margin_kept, hist=pipe.hist_margin)
    if scores is not None:
        scores.poll(True)
    if tagger is not None:
        tag_take(True)
        run.report["tags"] = dict(rows=tag_rows, truth=tag_truth, **tag_report(tag_rows, tag_truth, args.num_classes - 1))
    return pipe.hist, nimg, time.time() - run.t0


def resolve_model_inputs(args):
    """What ExCEL_model is built from (tools/infer_lam.py:144-162, model/model_excel.py:25-34) -> keyword arguments:
      state_dict          the CLIP checkpoint --model denotes (path, or model name under --clip_root / $EXCEL_CLIP_ROOT / ~/.cache/clip)
      tokenizer           CLIP's BPE tokenizer (the class/background prompts are encoded by the checkpoint's text tower)
      decoder_state_dict  --model_path (trained head, `module.` prefixes stripped, positional embedding skipped: :153-160)
                          when --training_free false
    Seeded random weights + random unit-norm text features are returned ONLY for --synthetic runs without a resolvable
    checkpoint; real data without weights raises."""
    from .. import clip
    from . import synthetic
    kw = {}
    ckpt = clip.clip.find_checkpoint(flag_defaults(args).model, args.clip_root)
    if ckpt is not None:
        sd = clip.clip.read_checkpoint(ckpt)
        kw["state_dict"] = sd
        if not any(k in sd for k in ("text_projection", "visual.proj")) and "proj" not in sd:
            raise RuntimeError(f"{ckpt}: not a CLIP checkpoint (no visual.proj / text_projection)")
        if "text_projection" not in sd:
            raise RuntimeError(f"{ckpt}: the checkpoint has no text tower (text_projection ...): the class / background prompts of "
                               "model/model_excel.py:31-33 cannot be encoded")
        from ..clip import bpe
        kw["tokenizer"] = bpe.BPETokenizer(args.bpe_path)         # raises FileNotFoundError with the remedy
        logging.info(f"CLIP weights: {ckpt}")
    elif args.data_folder:
        raise RuntimeError(f"--data_folder given but no CLIP checkpoint found for --model {args.model!r}: pass a checkpoint path, or put "
                           "the published archive (ViT-B-16.pt) under --clip_root / $EXCEL_CLIP_ROOT / ~/.cache/clip. "
                           "Refusing to score real data with random weights.")
    else:
        vocab = args.vocab or {}
        T = synthetic.text_rows(args.num_classes, len(vocab["bkg"]) if vocab.get("bkg") else None, custom=bool(vocab.get("fg")))
        kw["state_dict"] = synthetic.make_vit_state_dict(seed=0)
        kw["text_features"] = synthetic.make_text_features(T)
        logging.warning("SYNTHETIC run: seeded random ViT-B/16 weights and random text features (no CLIP checkpoint resolved); "
                        "the mIoU below is a throughput / plumbing check, not a result")
    if not args.training_free:
        if not args.model_path or not os.path.isfile(args.model_path):
            raise RuntimeError("--training_free false needs --model_path (the trained decoder checkpoint, tools/infer_lam.py:150-160)")
        trained = torch.load(args.model_path, map_location="cpu")
        dec = {}
        for k, v in trained.items():                                                        # :153-160
            k = k.replace("module.", "")
            if "encoder.visual.positional_embedding" not in k and k.startswith(("decoder_fts_fuse.", "decoder.")):
                dec[k] = v
        if not dec:
            raise RuntimeError(f"{args.model_path}: no decoder_fts_fuse.* / decoder.* tensors")
        kw["decoder_state_dict"] = dec
    return kw


def crf_proc(args, rank=0, world=1, device="cuda"):
    """tools/infer_lam.py:179-237: DenseCRF (iter 10, pos_xy_std 1, pos_w 3, bi_xy_std 67, bi_rgb_std 3, bi_w 4, :191-198) over the logits
    records of the main loop, label = pad(keys_gt + 1)[argmax] (:225-226), colour-coded PNG (:228), scores against the ground truth
    (:233).  The reference fans the images out over CPU processes (joblib); here every rank takes names r, r+R, ... through the
    device-side mean field (excel_dcrf_inference) and the confusion matrices are all-gathered like the main loop's.
    -> (score dict, summed hist)"""
    from PIL import Image
    from ..utils import evaluate, imutils
    from ..utils.dcrf import DenseCRF
    from .. import ops
    flag_defaults(args)
    with open(os.path.join(args.list_folder, args.infer_set) + ".txt") as f:
        name_list = [x for x in f.read().split("\n") if x]                                  # :182-184
    images_path = os.path.join(args.data_folder, "JPEGImages")
    labels_path = os.path.join(args.data_folder, "SegmentationClassAug")
    post = DenseCRF(iter_max=10, pos_xy_std=1, pos_w=3, bi_xy_std=67, bi_rgb_std=3, bi_w=4)  # :191-198
    hist = torch.zeros((args.num_classes, args.num_classes), dtype=torch.int64, device=device)
    for i in shard_indices(len(name_list), rank, world):
        name = name_list[i]
        rec = os.path.join(args.logits_dir, name + ".npy")
        # records carry the token of the run that wrote them (validate() draws one and shares it with every rank): no dependence on
        # file-system time stamps or clocks.  A caller that runs build_validation + crf_proc without a token accepts any record.
        if not os.path.isfile(rec) or (args.run_token is not None and imutils.logits_run_token(rec) != args.run_token):
            raise RuntimeError(f"crf_proc: {rec} was not written by this run (missing or stale): the CRF stage scores the records of the "
                               "main loop (tools/infer_lam.py:116-119), never those of an earlier one")
        lams, keys = imutils.load_logits(rec)                                               # :203-206
        image = np.asarray(Image.open(os.path.join(images_path, name + ".jpg")).convert("RGB")).astype(np.uint8)   # :209-210, :220
        if "test" in args.infer_set:
            label = image[:, :, 0]                                                          # :213-214
        else:
            label = np.array(Image.open(os.path.join(labels_path, name + ".png")))          # :216
        prob = post(torch.from_numpy(image).to(device), torch.from_numpy(np.asarray(lams, np.float32)).to(device))   # :221
        pred = prob.argmax(0)                                                               # :222
        keys_t = torch.from_numpy(np.pad(np.asarray(keys) + 1, (1, 0), mode="constant")).to(device)   # :225
        pred_crf = keys_t[pred].to(torch.uint8)                                             # :226
        if args.segs_crf_rgb_dir:
            os.makedirs(args.segs_crf_rgb_dir, exist_ok=True)
            Image.fromarray(imutils.encode_cmap(pred_crf.cpu().numpy())).save(os.path.join(args.segs_crf_rgb_dir, name + ".png"))   # :228
        hist = ops.confusion_accumulate(torch.from_numpy(np.array(label, dtype=np.uint8)).to(device), pred_crf, args.num_classes, hist)
    _, total = gather_hists(hist)
    return evaluate.scores_from_hist(total), total                                          # :233


def _tags_json(tags, tagger):
    """validate.last_tags without the rows, as plain JSON types (the --json_out record of a --tags clip run)."""
    out = {k: tags[k] for k in ("images", "tags_per_image", "scored", "counts", "image_f1")}
    out.update(thre=tagger["thre"], kmax=tagger["kmax"], scale=tagger["scale"], micro=None, per_class=None)
    if tags["score"] is not None:
        sc = tags["score"]
        out["micro"] = sc["micro"]
        out["per_class"] = {m: [float(v) for v in sc[m].values()] for m in ("precision", "recall", "f1")}
    return out


def _gemm_self_check(model, dataset, idx, args, device, world):
    """ExCEL_model.check_numerics (the one implementation of the bf16x3 -> f16x3 -> f32 ladder) on the first (up to 4) samples of this
    rank's shard, resized like the loop resizes them (:74).  With several ranks every rung's verdict is shared (all-reduce MAX of the
    difference): every rank runs the same mode, and a rank whose shard is EMPTY (fewer images than ranks) still joins every collective
    with a difference of 0 instead of leaving the others waiting."""
    from .. import ops
    S = flag_defaults(args).resize_size
    take = [int(i) for i in idx[:4]]
    inputs = None
    if take:
        first = dataset[take[0]][1]
        if first.dtype == np.uint8:                                                         # decoded images of their own sizes
            from ..datasets.loader import pack_samples
            rb = pack_samples([dataset[i] for i in take])
            inputs = ops.normalize_resize_u8_ragged(rb.images.to(device), ops.RaggedPlan(rb.hw, device), S)
        else:
            _, imgs, _, _ = dataset.batch(take)
            inputs = torch.from_numpy(imgs).to(device)
            if inputs.shape[-2:] != (S, S):
                inputs = ops.bilinear_resize(inputs, S, S, align_corners=False)

    def share(diff):
        if world > 1 and dist.is_initialized():
            t = torch.tensor([diff], dtype=torch.float64, device=device)
            dist.all_reduce(t, op=dist.ReduceOp.MAX)
            return float(t.item())
        return diff

    tol = float(args.gemm_check_tol)
    out = model.check_numerics(inputs, tol=tol, fallback=True, reduce=share)
    before, after, ladder = out["mode_before"], out["mode_after"], out["ladder"]
    if after != before:
        logging.warning(f"gemm self-check: CAMs of the {before} mode differ from exact fp32 by {ladder[0][1]:.2e} (> {tol:.1e}) on these weights: "
                        f"the run continues in {after} ({', '.join(f'{m} {d:.2e}' for m, d in ladder)})")
    elif ladder:
        logging.info(f"gemm self-check: {before} vs exact fp32 CAM max-abs difference {ladder[0][1]:.2e} (tolerance {tol:.1e})")
    return out


def validate(args=None, dataset=None, pipe=None):
    """tools/infer_lam.py:130-176.  `dataset` / `pipe` are injection points for the multi-rank control-flow tests (a stub pipeline on
    CPU tensors over gloo): with `pipe` given no model is built and the device is pipe.device; the product path passes neither."""
    from ..utils import evaluate
    from ..utils.PAR import PAR
    from . import synthetic
    world = int(os.environ.get("WORLD_SIZE", 1))
    rank = int(os.environ.get("RANK", 0))
    flag_defaults(args)
    # what this call reports: every attribute starts over, None where a stage does not run
    validate.last_gemm_check = validate.last_model = validate.last_guard = validate.last_per_rank = validate.last_cat_list = None
    validate.last_conf = validate.last_crf = validate.last_tags = validate.last_image_scores = validate.last_bkg_sweep = None
    from ..utils import bkg_sweep, components, image_scores, label_stages
    from ..utils import margin as margin_mod
    for name in label_stages.STAGES:
        setattr(validate, "last_" + name, None)
    image_scores.refuse(args, unlabeled=bool(args.unlabeled))                                # ... and per-image scores of nothing
    sweep, _ = bkg_sweep.resolve(args)                                                       # ... and a sweep nobody can score or run
    stages = {name: label_stages.STAGES[name].resolve(args) for name in label_stages.INFER_LAM_ORDER}   # ... and a label stage nobody can run or see
    stages = {name: resolved for name, resolved in stages.items() if resolved is not None}
    msweep, mcut = margin_mod.resolve(args)[0], stages.get("margin")                         # ... and a margin sweep likewise
    tta = resolve_tta(args)                                                                  # a bad flag combination stops here
    conf = resolve_conf(args)                                                                # ... and a bad pair of thresholds
    vocab = resolve_vocabulary(args)                                                         # ... and a vocabulary that cannot be served
    tagger = resolve_tags(args, have_dataset=dataset is not None)                            # ... and tags nobody can supply
    if pipe is None:
        torch.cuda.set_device(args.local_rank)
        device = torch.device("cuda", args.local_rank)
    else:
        device = torch.device(pipe.device)
    if world > 1 and not dist.is_initialized():
        dist.init_process_group(backend=args.backend)                                       # :133
    local_world = int(os.environ.get("LOCAL_WORLD_SIZE", world))
    if pipe is None and args.cpu_affinity == "auto" and local_world > 1:
        cores = pin_rank_to_cores(int(os.environ.get("LOCAL_RANK", args.local_rank)), local_world)
        if cores and rank == 0:
            logging.info(f"rank 0 pinned to {len(cores)} of the host's cores (every rank takes its own share; --cpu_affinity off disables)")
    # one token per evaluation, the same on every rank (rank 0 draws it): stamps the CRF records this run writes
    import uuid
    tok = [uuid.uuid4().hex]
    if world > 1:
        dist.broadcast_object_list(tok, src=0)
    args.run_token = tok[0]
    if dataset is not None:
        args.ragged_batches = True
    elif args.unlabeled:
        # a plain folder of images: no SegmentationClassAug, and image-level labels only where --tags labels asks for them
        from ..datasets import images, voc
        have = bool(args.list_folder) and os.path.isfile(os.path.join(args.list_folder, "cls_labels_onehot.npy"))
        if tagger is None and not have:
            raise FileNotFoundError(f"--tags labels reads {os.path.join(str(args.list_folder), 'cls_labels_onehot.npy')}: no such file "
                                    "(--tags clip predicts the tags, --save_tags writes such a file)")
        dataset = images.ImageListDataset(args.data_folder, args.list_folder, split=args.infer_set, num_fg=args.num_classes - 1,
                                          label_list=voc.load_cls_label_list(args.list_folder) if have else None)
        args.ragged_batches = True
    elif args.data_folder:
        # :156-163: every image has its own size.  The reference's harness always builds the VOC data set (:132); a COCO tree
        # (--dataset_name ms_coco, BASELINE configs[4]) gets the COCO reader of datasets/coco.py here
        if "coco" in args.dataset_name:
            from ..datasets import coco
            dataset = coco.CocoSegDataset(root_dir=args.data_folder, name_list_dir=args.list_folder, split=args.infer_set, stage="val",
                                          cls_labels_optional=tagger is not None)
        else:
            from ..datasets import voc
            dataset = voc.VOC12SegDataset(root_dir=args.data_folder, name_list_dir=args.list_folder, split=args.infer_set, stage="val",
                                          cls_labels_optional=tagger is not None, num_fg=args.num_classes - 1)
        args.ragged_batches = True
    else:
        args.ragged_batches = bool(args.ragged)
        dataset = synthetic.SyntheticSegDataset(args.synthetic, (args.resize_size, args.resize_size), num_classes=args.num_classes,
                                                seed=args.seed, u8_images=args.u8_input, ragged=args.ragged_batches)
    model = None
    if pipe is None:
        from ..model.model_excel import ExCEL_model
        model = ExCEL_model(clip_model=args.model, embedding_dim=args.embedding_dim, in_channels=args.in_channels,
                            dataset_name=args.dataset_name, num_classes=args.num_classes, num_atrr_clusters=args.num_attri,
                            json_file=args.attr_json, img_size=args.resize_size, mode=args.infer_set, device=device,
                            gemm_mode=args.gemm_mode, class_names=vocab["fg"], bkg_names=vocab["bkg"],
                            attr_bank=vocab["bank"], **resolve_model_inputs(args))
    # everything built so far (torch, the weights, the data set index) lives for the whole run: move it out of the cyclic collector's
    # reach, or every full collection walks it again - 40-70 ms of host time each (measured in bench.py, where one landed in a timed step)
    import gc
    gc.collect()
    gc.freeze()
    par = PAR(num_iter=20, dilations=[1, 2, 4, 8, 12, 24])                                  # :168
    idx = shard_indices(len(dataset), rank, world)                                          # :166
    if model is not None and args.gemm_check:                                # every rank joins, also one with an empty shard
        validate.last_gemm_check = _gemm_self_check(model, dataset, idx, args, device, world)
    hist, nimg, secs = build_validation(model, par, dataset, idx, device, args, pipe=pipe)
    validate.last_model = model                                                             # handle for callers / tests
    validate.last_guard = build_validation.last_guard                                       # the overflow guard's report (rank-local)
    per_rank, total = gather_hists(hist)
    validate.last_per_rank = per_rank
    score = None if args.unlabeled else evaluate.scores_from_hist(total)                    # (no ground truth: nothing to score)
    if sweep is not None:
        # --bkg_sweep: the ranks' totals summed once, like the matrix (a flagged image is in them once: skipped, then counted in fp32)
        _, sweep_total = gather_hists(build_validation.last_bkg_sweep)
        sweep_scores = bkg_sweep.scores_from_totals(sweep_total)
        validate.last_bkg_sweep = dict(scales=sweep, totals=sweep_total, scores=sweep_scores, best_scale=bkg_sweep.best_scale(sweep_scores, sweep)[1])
    def gathered_set(name):
        """One more scored label set: its matrix summed over the ranks once, the per-image rows of its stage - if it has any - gathered
        once (every rank joins, also one whose shard is empty)."""
        mine = getattr(build_validation, "last_" + name) or {}
        _, set_total = gather_hists(mine["hist"] if mine.get("hist") is not None else torch.zeros_like(hist))
        got = dict(score=None if args.unlabeled else evaluate.scores_from_hist(set_total), hist=set_total,
                   coverage=None if args.unlabeled else components.coverage(set_total, total))
        if label_stages.STAGES[name].rows is None:
            return got
        parts = [mine.get("rows", {})]
        if world > 1:
            parts = [None] * world
            dist.all_gather_object(parts, mine.get("rows", {}))
        rows = {}
        for part in parts:
            rows.update(part)
        order = sorted(rows)
        counts = np.stack([rows[i][1] for i in order]) if order else np.zeros((0, 3), np.int64)
        return dict(**got, names=[rows[i][0] for i in order], counts=counts)
    said = {}                                           # per stage that is on, what the log and the record say of it: score, stats, coverage
    for name, resolved in stages.items():
        stage = label_stages.STAGES[name]
        if stage.rows is None:                                                              # margin: below, behind its sweep
            continue
        got, more = gathered_set(name), ()
        if name == "snap":                                                                  # the share of pixels the vote changed
            pixels = torch.tensor([int((build_validation.last_snap or {}).get("pixels", 0))], dtype=torch.int64, device=hist.device)
            if world > 1:
                dist.all_reduce(pixels)
            more = (int(pixels.item()),)
        said[name] = dict(**label_stages.pipeline_value(stage, resolved), stats=stage.stats(got["counts"], *more), **got)
        setattr(validate, "last_" + name, said[name])
    if msweep is not None or mcut is not None:
        # --margin_sweep / --margin_min: the ranks' counts summed once, like the matrix (a flagged image is in them once: skipped, then
        # counted in fp32); every rank joins, also one whose shard is empty
        mine = build_validation.last_margin or {}
        m = validate.last_margin = dict(thresholds=msweep, margin_min=None if mcut is None else mcut["min"])
        if msweep is not None:
            kept = mine.get("kept")
            _, m["kept"] = gather_hists(kept if kept is not None else torch.zeros((len(msweep) + 1,), dtype=torch.int64, device=hist.device))
            m["coverage"] = margin_mod.coverage_from_kept(m["kept"])
            m["totals"] = m["scores"] = None
            if not args.unlabeled:
                tot = mine.get("totals")
                _, m["totals"] = gather_hists(tot if tot is not None else torch.zeros((len(msweep), 3, args.num_classes), dtype=torch.int64, device=hist.device))
                m["scores"] = bkg_sweep.scores_from_totals(m["totals"])
        if mcut is not None:
            got = gathered_set("margin") if not args.unlabeled else dict(hist=None, score=None, coverage=None)   # (no matrix without ground truth)
            m.update(hist=got["hist"], score=got["score"], label_coverage=got["coverage"])
            said["margin"] = dict(score=got["score"], stats=None, coverage=got["coverage"])
    tags = None
    if tagger is not None:
        # the predicted rows of every rank, once: every rank joins, also one whose shard is empty
        mine = build_validation.last_tags or {"rows": {}, "truth": {}}
        parts = [{"rows": mine["rows"], "truth": mine["truth"]}]
        if world > 1:
            parts = [None] * world
            dist.all_gather_object(parts, {"rows": mine["rows"], "truth": mine["truth"]})
        rows, truth = {}, {}
        for part in parts:
            rows.update(part["rows"])
            truth.update(part["truth"])
        tags = validate.last_tags = dict(rows=rows, **tag_report(rows, truth, args.num_classes - 1))
        if args.save_tags and rank == 0:
            save_tags_file(args.save_tags, rows)
    cat_list = VOC_CLASSES                                                                  # :123
    if "voc" not in args.dataset_name:
        from ..datasets import coco
        cat_list = coco.class_list
    if vocab["fg"]:
        cat_list = class_names(args)
    validate.last_cat_list = cat_list
    if rank == 0:
        if score is not None:
            logging.info(f"Training_free:{args.training_free}, LAM_score:")
            logging.info("\n" + format_scores_table(score, cat_list))
            logging.info(f"mIoU {score['miou'] * 100:.3f}  images {int(nimg) * world}  ({nimg / secs:.1f} img/s/rank)")
        else:
            logging.info(f"--unlabeled true: no ground truth, nothing scored  images {int(nimg) * world}  ({nimg / secs:.1f} img/s/rank)")
        if sweep is not None:
            logging.info("bkg_sweep_score:")
            logging.info("\n" + bkg_sweep.format_sweep_table(sweep_scores, sweep, cat_list))
            jb, sb = bkg_sweep.best_scale(sweep_scores, sweep)
            logging.info(f"bkg_sweep best scale {sb:g}: mIoU {sweep_scores[jb]['miou'] * 100:.3f} (labels written and scored at --bkg_scale {args.bkg_scale:g})")
        def log_set(name):
            stage, resolved, c = label_stages.STAGES[name], stages[name], said[name]
            if c["score"] is not None:
                logging.info(label_stages.title(stage, resolved))
                logging.info("\n" + format_scores_table(c["score"], cat_list))
            summary = stage.summary(c["stats"], c["coverage"])
            if summary:
                logging.info(summary)
            if resolved["label_dir"]:
                logging.info(f"{stage.noun} label maps -> {resolved['label_dir']}")
        for name in stages:
            if name != "margin":
                log_set(name)
        if msweep is not None:                              # the sweep's table stands in front of the cut's
            logging.info("margin_sweep_score (kept: arg-max margin >= the threshold; coverage over all pixels):")
            logging.info("\n" + margin_mod.format_margin_table(msweep, validate.last_margin["kept"], validate.last_margin["scores"], cat_list))
        if mcut is not None:
            log_set("margin")
        if tags is not None:
            logging.info(f"tags (--tags clip, thre {tagger['thre']}, at most {tagger['kmax']}, scale {tagger['scale']}): {tags['images']} images, "
                         f"tags per image {dict((k, v) for k, v in enumerate(tags['tags_per_image']) if v)}"
                         + (f", written to {args.save_tags}" if args.save_tags else ""))
            if tags["score"] is not None:
                logging.info("tag_score:")
                logging.info("\n" + format_scores_table(tags["score"], cat_list[1:], metric_names=("precision", "recall", "f1")))
                m = tags["score"]["micro"]
                logging.info(f"tag_score micro precision {m['precision']:.4f} recall {m['recall']:.4f} f1 {m['f1']:.4f}  "
                             f"mean image F1 (multilabel_score) {tags['image_f1']:.4f}  over {tags['scored']} images with labels")
        if args.json_out:
            # one self-checking record per run (tools_dev/scale.sh): wall time, rate and every rank's scored-pixel mass
            import json
            with open(args.json_out, "w") as f:
                json.dump({"world": world, "rccl_ranks": int(dist.get_world_size()) if world > 1 else 1, "images_rank0": int(nimg),
                           "images_total": int(len(dataset)), "seconds_rank0": round(secs, 3), "images_per_s_rank0": round(nimg / secs, 2),
                           "images_per_s_job": round(len(dataset) / secs, 2), "miou": float(score["miou"]) if score is not None else None,
                           "per_rank_hist_mass": [int(x) for x in per_rank.reshape(per_rank.shape[0], -1).sum(1).tolist()],
                           "hist_total": [[int(v) for v in row] for row in total.cpu().tolist()],       # the gathered confusion matrix itself
                           "batch_size": args.batch_size, "ragged": bool(args.ragged_batches), "resize_size": args.resize_size,
                           "cam_scales": [float(x) for x in (tta[0] or (1.0,))], "cam_flip": bool(tta[1]),
                           **({"tags": _tags_json(tags, tagger)} if tags is not None else {}),
                           **({"bkg_sweep": bkg_sweep.sweep_json(sweep_scores, sweep)} if sweep is not None else {}),
                           **({"margin_sweep": margin_mod.margin_json(msweep, validate.last_margin["kept"], validate.last_margin["scores"])}
                              if msweep is not None else {}),
                           **{name: label_stages.STAGES[name].json(stages[name], said[name]["stats"], said[name]["score"], said[name]["coverage"])
                              for name in label_stages.INFER_LAM_JSON_ORDER if name in stages}}, f)
    if image_scores.wanted(args):                                                           # one all_gather_object, rank 0 writes
        validate.last_image_scores = image_scores.finish(build_validation.last_image_scores, args, cat_list, rank, what="LAM_score")
        if rank == 0 and args.json_out and image_scores.boundary_of(args) is not None:       # the record above gains its `boundary` block
            import json
            with open(args.json_out) as f:
                record = json.load(f)
            record["boundary"] = image_scores.boundary_json(validate.last_image_scores, image_scores.boundary_of(args))
            with open(args.json_out, "w") as f:
                json.dump(record, f)
    if conf is not None:
        conf_hist = build_validation.last_conf_hist
        if conf_hist is None:                                                               # a rank with an empty shard still joins the gather
            conf_hist = torch.zeros_like(hist)
        _, conf_total = gather_hists(conf_hist)                                             # once, like the main matrix
        conf_score = evaluate.scores_from_hist(conf_total)
        coverage = float(conf_total.sum().item()) / max(float(total.sum().item()), 1.0)
        validate.last_conf = (conf_score, conf_total, coverage)
        if rank == 0:
            logging.info("conf_label_score:")
            logging.info("\n" + format_scores_table(conf_score, cat_list))
            logging.info(f"conf_label coverage {coverage * 100:.3f} % of the scored pixels kept "
                         f"(high_thre {args.conf_high_thre}, low_thre {args.conf_low_thre})")
    inline_hist = build_validation.last_crf_hist
    if args.crf_post and args.crf_inline and inline_hist is None and rank == 0:
        logging.info(f"--crf_inline: the {args.infer_set} split keeps the record path of the CRF stage (scored against image[:,:,0], :213-214)")
    if inline_hist is not None or (args.crf_post and args.data_folder):                     # :173-174
        if inline_hist is not None:                                                         # scored in the loop: one gather, like the main histogram
            _, crf_total = gather_hists(inline_hist)
            crf_score = evaluate.scores_from_hist(crf_total)
            st = build_validation.last_crf_stats
            if rank == 0:
                logging.info(f"crf inline: {st['groups']} groups over {st['calls']} batches, peak workspace {st['peak_workspace_bytes'] / 2 ** 20:.1f} MiB")
        else:
            crf_score, crf_total = crf_proc(args, rank, world, device)
        validate.last_crf = (crf_score, crf_total)
        if rank == 0:
            logging.info("crf_seg_score:")
            logging.info("\n" + format_scores_table(crf_score, cat_list))
    return score, total


if __name__ == "__main__":
    logging.basicConfig(level=logging.INFO, format="%(message)s")
    validate(get_parser().parse_args())
