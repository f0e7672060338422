"""Multi-scale / flip segmentation inference with the decoder head: mirror of tools/infer_seg_voc.py:47-101 (`_validate`).

  per image batch:  resize to (S,S) -> cat(x, flip(x)) -> model(.)[0] = seg logits -> bilinear to the input size
                    scale 1.0: the un-flipped half alone (:69); other scales: (seg + flip(seg_flipped)) / 2 (:79)
                    mean over scales (:82) -> bilinear to the label size (:84) -> arg-max (:85) -> confusion matrix
All tensor work runs in libexcel_hip.so (ViT, decoder head, excel_seg_scale_accumulate, excel_bilinear_resize,
excel_argmax_label, excel_confusion_accumulate); torch is used for device memory and the flip/cat copies.

The evaluation PROGRAM (`python -m excel_amd.tools.infer_seg_voc`, get_parser / validate below; tools/infer_seg_coco.py's twin is
excel_amd.tools.infer_seg_coco) runs the same chain over RAGGED batches: decode threads and a copy stream feed packed uint8 images
(datasets/loader), the device resizes every image to each scale (excel_normalize_resize_u8_ragged), the decoder runs on image + flip
(ExCEL_model.seg_logits), and one launch fuses all scales at every image's own size and takes the arg-max (excel_seg_msc_fuse_ragged;
COCO: excel_seg_resize_argmax_ragged after a fuse at 0.2x).  The confusion matrix stays on the device; ranks take images r, r+R, ...
and all-gather it once.  `--batch_size 1` runs the same code with the reference's batch of one.

Deliberate differences from the reference:
  * the DenseCRF stage (crf_proc, :103-174) runs INLINE on the fused logits that are still on the device, for the whole batch at once
    (--crf_batched true, the default: excel_seg_softmax_resize_ragged + excel_dcrf_inference_ragged over groups of images that fit
    --crf_ws_gb of workspace, one confusion update and one device-to-host copy of the batch's labels, the PNGs written by a small
    thread pool while the next batch runs) or image by image (--crf_batched false: excel_seg_softmax_resize + excel_dcrf_inference
    per image); both give the same files and histograms, bit for bit.  No `{"msc_seg": ...}` records are written and no `logits/`
    directory is created (the reference writes ~15 MB per VOC image and reads them back);
  * output paths follow :223-240 (`<model_path before "checkpoints/">/<infer_set>/<infer_set>_<ckpt>_segs/...`); a --model_path
    without a `checkpoints/` component uses the checkpoint's own directory in place of the part before it;
  * --scales takes a comma-separated list ("0.7,1.0,1.2,1.5");
  * --per_image_scores PATH (not for --infer_set test): every image's own scores of the raw and, with --crf_post, the CRF labels
    (excel_image_scores next to each confusion update, read behind tickets; utils/image_scores.py writes PATH and PATH.npz);
  * --boundary_scores true (not for --infer_set test): the Boundary IoU of the raw and the CRF labels (excel_boundary_scores in the
    same tickets; a boundary_score table per set, and extra columns / arrays in --per_image_scores' files).
"""
import argparse
import logging
import os
import time

import numpy as np
import torch

from .. import ops
from .infer_lam import _bool, flag_defaults


@torch.no_grad()
def multi_scale_seg(model, inputs, resize_size, scales=(1.0, 0.5, 0.75, 1.5), flip_first=False):
    """inputs [B,3,h,w] -> msc_seg [B,nc,h,w] (the tensor the reference stores as {"msc_seg": ...}, :89).
    flip_first=True: the variant of tools/test_msc_flip_voc.py:89-107, where scale 1.0 is flip-averaged as well."""
    if model._dec is None:
        raise RuntimeError("multi_scale_seg needs the decoder head: build ExCEL_model with decoder_state_dict=")
    B, _, h, w = inputs.shape
    todo = [1.0] + [s for s in scales if s != 1.0]                    # :63-70 first, then :72-80
    acc = None
    for i, sc in enumerate(todo):
        S = resize_size if sc == 1.0 else int(resize_size * sc)       # :64 / :74
        x = ops.bilinear_resize(inputs, S, S, align_corners=False)    # :65 / :75
        segs = model(torch.cat([x, x.flip(-1)], dim=0))[0]            # :66-67 / :76-77
        acc = ops.seg_scale_accumulate(segs, acc, h, w, flip_mean=(sc != 1.0 or flip_first), init=(i == 0),
                                       scale=(1.0 / len(todo)) if i == len(todo) - 1 else 1.0)     # :68-70 / :78-80, :82
    return acc


@torch.no_grad()
def seg_labels(msc_seg, label_hw):
    """:84-85 -> uint8 labels [B,H,W] on the device."""
    H, W = int(label_hw[0]), int(label_hw[1])
    resized = ops.bilinear_resize(msc_seg, H, W, align_corners=False)
    return ops.argmax_label(resized)


@torch.no_grad()
def validate_seg(model, batches, num_classes, resize_size, scales=(1.0, 0.5, 0.75, 1.5)):
    """batches: iterable of (inputs [B,3,h,w] device f32, labels [B,H,W] uint8 device).  -> scores dict (evaluate.scores layout)."""
    from ..utils import evaluate
    hist = None
    for inputs, labels in batches:
        pred = seg_labels(multi_scale_seg(model, inputs, resize_size, scales), labels.shape[-2:])
        hist = ops.confusion_accumulate(labels, pred, num_classes, hist)
    return evaluate.scores_from_hist(hist), hist


# ------------------------------------------------------------------ the evaluation program (tools/infer_seg_voc.py:23-45, :176-240)
def parse_scales(x):
    """"0.7,1.0,1.2,1.5" (or a sequence) -> tuple of floats."""
    if isinstance(x, str):
        x = [v for v in x.replace(" ", "").strip("[]()").split(",") if v]
    return tuple(float(v) for v in x)


def get_parser():
    """The reference's flags and defaults (tools/infer_seg_voc.py:23-45) plus the ones infer_lam has."""
    p = argparse.ArgumentParser()
    p.add_argument("--model_path", default=None, type=str, help="trained decoder checkpoint (scripts/train_voc.py model_iter_N.pth or the reference's)")
    p.add_argument("--model", default="ExCEL_ViT-B/16", type=str)
    p.add_argument("--dataset_name", default="pascal_voc", type=str)
    p.add_argument("--attr_json", default=None, type=str)
    p.add_argument("--num_attri", default=112, type=int)
    p.add_argument("--embedding_dim", default=256, type=int)
    p.add_argument("--in_channels", default=768, type=int)
    p.add_argument("--crf_post", default=False, type=_bool)
    p.add_argument("--resize_size", default=320, type=int)
    p.add_argument("--scales", default="0.7,1.0,1.2,1.5", type=parse_scales, help="comma-separated multi-scale factors")
    p.add_argument("--infer_set", default="val", type=str)
    p.add_argument("--data_folder", default=None, type=str)
    p.add_argument("--test_data_folder", default=None, type=str)
    p.add_argument("--list_folder", default="datasets/voc", type=str)
    p.add_argument("--num_classes", default=21, type=int)
    p.add_argument("--ignore_index", default=255, type=int)
    # what infer_lam has
    p.add_argument("--batch_size", default=16, type=int)
    p.add_argument("--num_workers", default=-1, type=int, help="decode threads; -1 = from the CPUs this rank may use (at most 16)")
    p.add_argument("--clip_root", default=None, type=str)
    p.add_argument("--bpe_path", default=None, type=str)
    p.add_argument("--gemm_mode", default=None, type=str)
    p.add_argument("--gemm_check", default=True, type=_bool)
    p.add_argument("--gemm_check_tol", default=5e-4, type=float)
    p.add_argument("--crf_batched", default=True, type=_bool, help="run the DenseCRF stage over the whole batch (false: image by image)")
    p.add_argument("--crf_ws_gb", default=16.0, type=float, help="workspace budget of the batched DenseCRF stage; a batch is cut into groups that fit")
    from ..utils import image_scores
    image_scores.add_flags(p)
    image_scores.add_boundary_flags(p)
    p.add_argument("--local_rank", default=int(os.environ.get("LOCAL_RANK", 0)), type=int)
    p.add_argument("--backend", default="nccl")
    return p


def scale_sizes(resize_size, scales):
    """The reference's scale order and input sizes: scale 1.0 first at resize_size (:63-64), then every other scale at
    int(resize_size * s) (:72-74).  -> [(S, s), ...]"""
    return [(int(resize_size), 1.0)] + [(int(resize_size * s), float(s)) for s in scales if s != 1.0]


def output_dirs(model_path, infer_set, crf_post=False):
    """Output locations of :223-240.  base = <model_path before "checkpoints/">/<infer_set>; without a "checkpoints/" component the
    checkpoint's own directory stands in for the part before it."""
    if "checkpoints/" in model_path:
        root = model_path.split("checkpoints/")[0]
        ckpt = model_path.split("checkpoints/")[-1]
    else:
        root = os.path.dirname(os.path.abspath(model_path))
        ckpt = os.path.basename(model_path)
    ckpt = ckpt.replace(".pth", "")
    base = os.path.normpath(os.path.join(root, infer_set))
    segs = os.path.join(base, f"{infer_set}_{ckpt}_segs")
    crf = "crf" if crf_post else "no_crf"
    return {"base": base, "segs": segs, "seg_preds": os.path.join(segs, "seg_preds"), "seg_preds_rgb": os.path.join(segs, "seg_preds_rgb"),
            "log": os.path.join(segs, "results.log"),
            "test": os.path.join(base, f"{infer_set}_{ckpt}_segs_{crf}", "results", "VOC2012", "Segmentation", "comp6_test_cls")}


class SegVariant:
    """What differs between tools/infer_seg_voc.py and tools/infer_seg_coco.py."""
    name = "voc"
    fuse_factor = None           # COCO: fuse at (int(0.2 h), int(0.2 w)), :63-64
    flip_first = False           # COCO: scale 1.0 flip-averaged as well, :73
    test_set = True              # only VOC has the test-server branch

    @staticmethod
    def dataset(args, stage):
        from ..datasets import voc
        return voc.VOC12SegDataset(root_dir=args.data_folder, name_list_dir=args.list_folder, split=args.infer_set, stage=stage,
                                   ignore_index=args.ignore_index)

    @staticmethod
    def class_list():
        from ..datasets import voc
        return voc.class_list

    def fuse_size(self, h, w):
        if self.fuse_factor is None:
            return int(h), int(w)
        fh, fw = int(self.fuse_factor * h), int(self.fuse_factor * w)
        if fh < 1 or fw < 1:
            raise ValueError(f"image of {h} x {w}: the {self.fuse_factor}x fuse size ({fh} x {fw}) is empty")
        return fh, fw


VOC = SegVariant()

log = logging.getLogger("excel_amd.infer_seg")        # results.log receives this logger's records (INFO and up)
log.setLevel(logging.INFO)

CRF_PARAMS = dict(iter_max=10, pos_xy_std=1, pos_w=3, bi_xy_std=67, bi_rgb_std=3, bi_w=4)      # :112-119
CRF_WRITERS = 4                  # threads that encode the batched CRF stage's PNGs


def _write_crf_files(dirs, name, lab_np, test):
    """The files crf_proc writes for one image (:153-162)."""
    from ..utils import imutils
    _save_png(os.path.join(dirs["seg_preds"], name + ".png"), lab_np)
    _save_png(os.path.join(dirs["seg_preds_rgb"], name + ".png"), imutils.encode_cmap(lab_np).astype(np.uint8))
    if test:
        imutils.convert_test_seg2RGB(lab_np, os.path.join(dirs["test"], name + ".png"))


def _crf_batch(post, images, plan, planes, fplan, nc, budget):
    """crf_proc :134-152 for a whole ragged batch: softmax of the fused logits at every image's size, mean field, arg-max ->
    tight uint8 labels on the device (ops.dcrf_inference_ragged; the bits of the per-image chain)."""
    prob = ops.seg_softmax_resize_ragged(planes, fplan, plan, nc)
    lab, _ = ops.dcrf_inference_ragged(images, plan, prob, nc, post.iter_max, post.pos_w, post.pos_xy_std, post.bi_w, post.bi_xy_std,
                                       post.bi_rgb_std, want_labels=True, budget_bytes=budget)
    return lab


@torch.no_grad()
def evaluate_batches(model, feed, args, variant=VOC, test=False, dirs=None, scores=None, indices=None):
    """The loop of _validate (:58-91) and crf_proc (:103-174) over ragged batches `feed` = (names, plan, images u8, cls, labels u8)
    device tuples (datasets/loader.DeviceFeeder).  -> dict(hist, hist_crf (None without --crf_post), images).  With --crf_batched the
    CRF files of a batch are written by a thread pool while the next batch runs; it is joined, and a failed write raised, before this
    returns.  `scores` (--per_image_scores: an utils/image_scores.ImageScoreLog) receives the per-image counts of both matrices behind
    tickets, filed under `indices` - the data-set indices `feed` runs through, in its order."""
    from concurrent.futures import ThreadPoolExecutor
    from ..utils import imutils
    from ..utils.dcrf import DenseCRF
    from ..pipeline import ScoreTicket
    nc = int(args.num_classes)
    boundary = scores.boundary if scores is not None else None
    crf = bool(args.crf_post)
    batched = crf and bool(args.crf_batched)
    budget = int(float(args.crf_ws_gb) * 2 ** 30)
    sizes = scale_sizes(args.resize_size, parse_scales(args.scales))
    flips = [s != 1.0 or variant.flip_first for _, s in sizes]
    post = DenseCRF(**CRF_PARAMS) if crf else None
    hist = hist_crf = None
    nimg = 0
    writers = ThreadPoolExecutor(max_workers=CRF_WRITERS) if batched else None
    pending = []
    try:
        for names, plan, images, _cls, labels in feed:
            dev = images.device
            if hist is None:
                hist = torch.zeros((nc, nc), dtype=torch.int64, device=dev)
                hist_crf = torch.zeros((nc, nc), dtype=torch.int64, device=dev) if crf else None
            segs = []
            for S, _ in sizes:                                                                   # :63-80
                x = ops.normalize_resize_u8_ragged(images, plan, S)
                segs.append(model.seg_logits(torch.cat([x, x.flip(-1)], dim=0)))
            if variant.fuse_factor is None:                                                       # VOC: fuse at the label size
                fplan = plan
                planes, pred = ops.seg_msc_fuse_ragged(segs, flips, plan, want_planes=crf, want_labels=True, label_hw=plan.hw)
            else:                                                                                 # COCO: fuse small, arg-max at the label size
                fplan = ops.RaggedPlan([variant.fuse_size(h, w) for h, w in plan.hw], dev)
                planes, _ = ops.seg_msc_fuse_ragged(segs, flips, fplan, want_planes=True)
                pred = ops.seg_resize_argmax_ragged(planes, fplan, plan, nc)
            if scores is not None:
                rec = ([int(i) for i in indices[nimg:nimg + len(names)]], names, plan.hw)
            if not test:
                hist = ops.confusion_accumulate(labels, pred, nc, hist)                          # :86-87, :97
                if scores is not None:
                    scores.defer(ScoreTicket().launch("main", labels, pred, nc, plan=plan, boundary=boundary), *rec)
            if batched:
                lab = _crf_batch(post, images, plan, planes, fplan, nc, budget)
                if not test:
                    hist_crf = ops.confusion_accumulate(labels, lab, nc, hist_crf)
                    if scores is not None:
                        scores.defer(ScoreTicket().launch("crf", labels, lab, nc, plan=plan, boundary=boundary), *rec)
                lab_host = lab.cpu().numpy()                                                      # the batch's one device-to-host copy
            for b, name in enumerate(names):
                H, W = int(plan.hw[b, 0]), int(plan.hw[b, 1])
                if batched:
                    lo = int(plan.loff[b])
                    pending.append(writers.submit(_write_crf_files, dirs, name, lab_host[lo:lo + H * W].reshape(H, W), test))
                elif crf:                                                                         # crf_proc :134-152, inline
                    prob = ops.seg_softmax_resize(planes, fplan, b, nc, H, W)
                    lo = int(plan.loff[b])
                    q = post(images[3 * lo:3 * (lo + H * W)].view(H, W, 3), prob)
                    lab = ops.argmax_label(q[None])[0]
                    if not test:
                        hist_crf = ops.confusion_accumulate(plan.label(labels, b), lab, nc, hist_crf)
                        if scores is not None:
                            scores.defer(ScoreTicket().launch("crf", plan.label(labels, b)[None], lab[None], nc, boundary=boundary), rec[0][b:b + 1], [name], [(H, W)])
                    lab_np = lab.cpu().numpy()
                    _save_png(os.path.join(dirs["seg_preds"], name + ".png"), lab_np)
                    _save_png(os.path.join(dirs["seg_preds_rgb"], name + ".png"), imutils.encode_cmap(lab_np).astype(np.uint8))
                    if test:
                        imutils.convert_test_seg2RGB(lab_np, os.path.join(dirs["test"], name + ".png"))
                elif test:                                                                        # :92-95
                    imutils.convert_test_seg2RGB(plan.label(pred, b).cpu().numpy(), os.path.join(dirs["test"], name + ".png"))
            while len(pending) > 8 * CRF_WRITERS:                                                 # bounds the label maps waiting on the host
                pending.pop(0).result()
            nimg += len(names)
        for f in pending:
            f.result()
    finally:
        if writers is not None:
            writers.shutdown(wait=True)
    return {"hist": hist, "hist_crf": hist_crf, "images": nimg}


def _save_png(path, arr):
    from PIL import Image
    os.makedirs(os.path.dirname(path), exist_ok=True)
    Image.fromarray(arr).save(path)


def build_model(args, device):
    """ExCEL_model with the trained head of --model_path, loaded like infer_lam --training_free false (module. prefixes stripped, the
    positional embedding skipped, decoder_fts_fuse.* / decoder.* kept: tools/infer_seg_voc.py:196-205)."""
    from ..model.model_excel import ExCEL_model
    from . import infer_lam
    if not args.model_path:
        raise RuntimeError("--model_path (the trained decoder checkpoint) is required")
    ns = argparse.Namespace(**vars(args))
    ns.training_free = False
    kw = infer_lam.resolve_model_inputs(ns)
    return ExCEL_model(clip_model=args.model, embedding_dim=args.embedding_dim, in_channels=args.in_channels, dataset_name=args.dataset_name,
                       num_classes=args.num_classes, num_atrr_clusters=args.num_attri, json_file=args.attr_json, img_size=args.resize_size,
                       mode=args.infer_set, device=device, gemm_mode=args.gemm_mode, **kw)


def validate(args, model=None, variant=VOC):
    """tools/infer_seg_voc.py validate + _validate + crf_proc (:176-220).  `model`: an ExCEL_model with its decoder head (built from
    --model / --model_path when None).  -> dict(score, crf_score, hist, hist_crf, dirs, images, seconds); scores are None for the
    test set."""
    import torch.distributed as dist
    from ..datasets.loader import DeviceFeeder, threaded_batches
    from ..utils import evaluate
    from . import infer_lam
    from ..utils import image_scores
    flag_defaults(args, get_parser())
    image_scores.refuse(args, test_split=args.infer_set == "test")
    world = int(os.environ.get("WORLD_SIZE", 1))
    rank = int(os.environ.get("RANK", 0))
    torch.cuda.set_device(args.local_rank)
    device = torch.device("cuda", args.local_rank)
    if world > 1 and not dist.is_initialized():
        dist.init_process_group(backend=args.backend)
    test = args.infer_set == "test"
    if test and not variant.test_set:
        raise ValueError(f"{variant.name}: no test-set branch (the reference has none)")
    if test:
        args.data_folder = args.test_data_folder                                              # :236
    if not args.data_folder:
        raise RuntimeError("--data_folder (--test_data_folder for --infer_set test) is required")
    dirs = output_dirs(args.model_path or os.path.join(os.getcwd(), "model.pth"), args.infer_set, args.crf_post)
    handler = None
    if rank == 0:
        os.makedirs(dirs["segs"], exist_ok=True)
        handler = logging.FileHandler(dirs["log"])
        log.addHandler(handler)
    try:
        dataset = variant.dataset(args, "test" if test else "val")
        if model is None:
            model = build_model(args, device)
        idx = infer_lam.shard_indices(len(dataset), rank, world)                              # one image per r, r+R, ...
        if args.gemm_check:
            infer_lam._gemm_self_check(model, dataset, idx, args, device, world)
        nw = int(args.num_workers)
        if nw < 0:
            nw = infer_lam.default_decode_workers(int(os.environ.get("LOCAL_WORLD_SIZE", world)))
        t0 = time.time()
        feed = DeviceFeeder(threaded_batches(dataset, idx, args.batch_size, num_threads=max(nw, 1)), device)
        scores = image_scores.ImageScoreLog(int(args.num_classes), ["main"] + (["crf"] if args.crf_post else []),
                                            boundary=image_scores.boundary_of(args)) if image_scores.wanted(args) else None
        out = evaluate_batches(model, feed, args, variant, test=test, dirs=dirs, scores=scores, indices=idx)
        torch.cuda.synchronize()
        secs = time.time() - t0
        nc = int(args.num_classes)
        hist = out["hist"] if out["hist"] is not None else torch.zeros((nc, nc), dtype=torch.int64, device=device)
        hist_crf = out["hist_crf"]
        if args.crf_post and hist_crf is None:
            hist_crf = torch.zeros((nc, nc), dtype=torch.int64, device=device)
        res = {"score": None, "crf_score": None, "hist": None, "hist_crf": None, "dirs": dirs, "images": out["images"], "seconds": secs,
               "image_scores": None}
        if not test:
            _, res["hist"] = infer_lam.gather_hists(hist)                                     # the one collective of the run
            res["score"] = evaluate.scores_from_hist(res["hist"])
            if args.crf_post:
                _, res["hist_crf"] = infer_lam.gather_hists(hist_crf)
                res["crf_score"] = evaluate.scores_from_hist(res["hist_crf"])
            if scores is not None:                                                            # one all_gather_object, rank 0 writes
                res["image_scores"] = image_scores.finish(scores, args, variant.class_list(), rank, what="raw_seg_score")
            if rank == 0:
                cats = variant.class_list()
                log.info("raw_seg_score:")
                log.info("\n" + infer_lam.format_scores_table(res["score"], cats))
                if args.crf_post:
                    log.info("crf_seg_score:")
                    log.info("\n" + infer_lam.format_scores_table(res["crf_score"], cats))
        if rank == 0:
            log.info(f"{variant.name} {args.infer_set}: {out['images'] * world} images, {secs:.2f} s on rank 0"
                         + (f", mIoU {res['score']['miou'] * 100:.2f}" if res["score"] else "")
                         + (f", CRF mIoU {res['crf_score']['miou'] * 100:.2f}" if res["crf_score"] else ""))
        return res
    finally:
        if handler is not None:
            log.removeHandler(handler)
            handler.close()


if __name__ == "__main__":
    logging.basicConfig(level=logging.INFO, format="%(message)s")
    validate(get_parser().parse_args())
