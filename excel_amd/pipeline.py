"""Batched, fully device-resident training-free pipeline over the same HIP kernels the per-image API uses.

One `run_batch` = tools/infer_lam.py:74-114 for B images at once:
    ViT surgery forward (+ fused affinity mean) -> patch-text CAM -> box-masked attention random walk
    -> min-max + cv2-style up-sampling + background -> PAR x20 -> arg-max -> confusion accumulate.
No host round trip happens inside a step (the reference makes ~2k+5 per image).
"""
import contextlib

import torch

from . import ops
from .utils.label_stages import STAGES

GUARD_MODES = (None, "skip", "observe")
TTA_MAX_SCALES = ops.TTA_MAX_SCALES
TTA_MAX_GRID = ops.TTA_MAX_GRID


def _check_tta_scales(scales):
    scales = [float(s) for s in scales]
    if 1.0 not in scales:
        raise ValueError(f"cam scales {scales}: scale 1.0 must be one of them (it supplies the affinity of the random walk)")
    if len(scales) > TTA_MAX_SCALES:
        raise ValueError(f"cam scales {scales}: {len(scales)} scales, at most {TTA_MAX_SCALES}")
    return scales


def tta_sizes(S, scales):
    """The network sizes of a multi-scale pass at resize size S -> [(S_s, g_s), ...], scale 1.0 FIRST wherever the caller listed it (its
    un-flipped half supplies the affinity and the image PAR reads), the others in the caller's order.  S_s = S for 1.0, else
    int(s * S) // 16 * 16 (camutils.multi_scale_lam's rule); g_s = S_s // 16.  Refused, naming the scale: a list without 1.0, more than
    8 scales, S_s < 16, g_s > 48 (the largest grid the ViT's attention kernels are tested at) and two scales with the same S_s."""
    scales = _check_tta_scales(scales)
    out, seen = [], {}
    for s in [1.0] + [s for s in scales if s != 1.0] + [1.0] * (scales.count(1.0) - 1):
        S_s = int(S) if s == 1.0 else int(s * S) // 16 * 16
        if S_s < 16:
            raise ValueError(f"cam scale {s}: network size {S_s} at resize size {S} is below one 16-pixel patch")
        if S_s // 16 > TTA_MAX_GRID:
            raise ValueError(f"cam scale {s}: grid {S_s // 16} at resize size {S} is above {TTA_MAX_GRID}")
        if S_s in seen:
            raise ValueError(f"cam scale {s}: rounds to the same network size {S_s} as scale {seen[S_s]} at resize size {S}")
        seen[S_s] = s
        out.append((S_s, S_s // 16))
    return out


def _refuse_tta(who, tta_scales, tta_flip):
    if tta_flip or (tta_scales is not None and tuple(float(x) for x in tta_scales) != (1.0,)):
        raise ValueError(f"{who} has no flip / multi-scale fuse (tta_scales={tta_scales}, tta_flip={tta_flip}): the option belongs to the "
                         "training-free regime (TrainingFreePipeline.run_batch / run_batch_ragged)")


def check_conf(conf):
    """conf = (high_thre, low_thre) of the two-threshold labels (utils/affutils.py:101-158) -> the pair as floats, or None.  Refused,
    naming the value: a threshold outside (0, 1) and low_thre >= high_thre (the band between the two passes would be empty)."""
    if conf is None:
        return None
    high, low = (float(x) for x in conf)
    for name, v in (("high_thre", high), ("low_thre", low)):
        if not 0.0 < v < 1.0:
            raise ValueError(f"{name} {v} is outside (0, 1): the background score competes with min-max normalised cams")
    if low >= high:
        raise ValueError(f"low_thre {low} must be below high_thre {high}: the strict pass takes the high score")
    return high, low


def conf_labels_ragged(imgs, cams, plan, half_plan, smax, nchan, cls_idx, high_thre, low_thre, dilations=ops.PAR_DILATIONS, num_iter=20,
                       w1=0.3, w2=0.01, img_box=None, ignore_index=255, buf=None, keep=False):
    """refine_cams_with_bkg_v2 (utils/affutils.py:101-158) over a ragged batch, two launches around one PAR:
        ops.conf_planes_ragged   cams (smax + 1 pitched planes per image on `plan`) -> both softmaxes on `half_plan`   (:115-141)
        ops.par_forward_ragged   ONE pass over the 2 (k_b + 1) planes of every image: planes do not interact, the two   (:93)
                                 groups share the affinities of the guide
        ops.conf_merge_ragged    per group resize + arg-max + keys, the merge and img_box                               (:94-96, :146-156)
    imgs [B,3,h,w]: what PAR resizes per image to the half plan (align_corners=True, the identity at equal sizes).
    buf(name, numel, dtype, device) supplies step buffers (the pipeline's _buf); keep=True asks for fresh zero-filled tensors.
    -> (tight uint8 labels on `plan`, planes, PAR output)"""
    dev = cams.device
    C2 = 2 * (smax + 1)
    n = C2 * half_plan.total_pix
    fresh = keep or buf is None
    planes, nchan2 = ops.conf_planes_ragged(cams, plan, half_plan, smax, nchan, high_thre, low_thre,
                                            out=torch.zeros(n, device=dev) if fresh else buf("conf_planes", n, torch.float32, dev))
    ws = None if buf is None else buf("par_ws", ops.lib().excel_par_ragged_workspace_bytes(half_plan.total_pix, C2), torch.uint8, dev)
    par_out = ops.par_forward_ragged(imgs, planes, half_plan, C2, dilations, num_iter, nchan=nchan2, w1=w1, w2=w2, ws=ws,
                                     out=None if fresh else buf("conf_par_out", n, torch.float32, dev))
    labels = ops.conf_merge_ragged(par_out, half_plan, plan, smax, nchan, cls_idx, img_box=img_box, ignore_index=ignore_index)
    return labels, planes, par_out


class GuardTicket:
    """The per-image non-finite counts of one guarded step on their way to the host: a pinned int32 [B] the step's stream copies
    into, and the event recorded behind that copy.  ready() never blocks; flags() waits for the event."""

    def __init__(self, host, event):
        self._host, self._event = host, event

    def ready(self):
        return self._event.query()

    def flags(self):
        self._event.synchronize()
        return self._host.numpy()


class TagTicket:
    """The predicted tags of one step on their way to the host (the GuardTicket pattern): pinned float32 [B,F] copies of the one-hot
    rows and the scores, and the event recorded behind them on the step's stream.  ready() never blocks; tags() waits for the event."""

    def __init__(self, onehot, scores, event):
        self._onehot, self._scores, self._event = onehot, scores, event

    def ready(self):
        return self._event.query()

    def tags(self):
        """-> (onehot [B,F], scores [B,F]) as numpy arrays"""
        self._event.synchronize()
        return self._onehot.numpy(), self._scores.numpy()


class ScoreTicket:
    """The per-image score counts of one step on their way to the host (the GuardTicket pattern): per matrix the step scored - "main"
    (self.hist), "seg" (self.hist_seg), otherwise "<set>" for self.hist_<set> - a pinned int32 [B,3,nc] copy of ops.image_scores' result,
    and the event recorded behind the last copy on the step's stream.  ready() never blocks; counts() waits for the event."""

    def __init__(self):
        self._parts, self._event = {}, None

    def launch(self, which, gts, labels, num_classes, skip=None, plan=None, out=None, boundary=None, out_bd=None):
        """ops.image_scores over (gts, labels) on the current stream, its copy to pinned memory and the event behind it -> self.
        boundary = None | dict(ratio=, px=): also ops.boundary_scores on the same arrays and stream - every image's radius by the host
        rule utils/image_scores.boundary_radius of its own size (uniform maps must then be [B,H,W]) -, filed under which + "_bd"."""
        dev = ops.image_scores(gts, labels, num_classes, skip=skip, plan=plan, out=out)
        host = torch.empty(dev.shape, dtype=torch.int32, pin_memory=True)
        host.copy_(dev, non_blocking=True)
        if boundary is not None:
            from .utils.image_scores import boundary_radius, check_boundary
            bd = check_boundary(boundary)
            hws = plan.hw if plan is not None else [gts.shape[-2:]] * int(gts.shape[0])
            radii = [boundary_radius(int(h), int(w), **bd) for h, w in hws]
            dev_bd = ops.boundary_scores(gts, labels, num_classes, radii if len(set(radii)) > 1 else radii[0], skip=skip, plan=plan, out=out_bd)
            host_bd = torch.empty(dev_bd.shape, dtype=torch.int32, pin_memory=True)
            host_bd.copy_(dev_bd, non_blocking=True)
            self._parts[which + "_bd"] = host_bd
        self._event = torch.cuda.Event()
        self._event.record()
        self._parts[which] = host
        return self

    def ready(self):
        return self._event is None or self._event.query()

    def counts(self):
        """-> {"main": int32 [B,3,nc], ...} as numpy arrays: the matrices this step scored"""
        if self._event is not None:
            self._event.synchronize()
        return {k: v.numpy() for k, v in self._parts.items()}


def check_tagger(tagger, smax, num_classes):
    """tagger = dict(thre=, kmax=, scale=) of the predicted image tags (ops.clip_tags; defaults 0.2 / smax / 100.0) -> the complete dict,
    or None.  Refused, naming `tagger`: an unknown key, thre outside [0, 1], scale <= 0, kmax outside [1, num_classes - 1] and
    kmax != smax - the compacted class list has smax slots, and the tagger is what caps the number of present classes."""
    if tagger is None:
        return None
    if not isinstance(tagger, dict) or set(tagger) - {"thre", "kmax", "scale"}:
        raise ValueError(f"tagger must be a dict with the keys thre, kmax, scale (got {tagger!r})")
    out = dict(thre=float(tagger.get("thre", 0.2)), kmax=int(tagger.get("kmax", smax)), scale=float(tagger.get("scale", 100.0)))
    if not 0.0 <= out["thre"] <= 1.0:
        raise ValueError(f"tagger: thre {out['thre']} is outside [0, 1] (it is relative to the best foreground score)")
    if not out["scale"] > 0.0:
        raise ValueError(f"tagger: scale {out['scale']} must be positive (CLIP's logit scale is 100)")
    if not 1 <= out["kmax"] <= int(num_classes) - 1:
        raise ValueError(f"tagger: kmax {out['kmax']} is outside [1, {int(num_classes) - 1}] (num_classes - 1 foreground classes)")
    if out["kmax"] != int(smax):
        raise ValueError(f"tagger: kmax {out['kmax']} must equal smax {smax}: the compacted class list has smax slots and the tagger is "
                         "what caps the number of present classes")
    return out


def _refuse_tagger(who, tagger):
    if tagger is not None:
        raise ValueError(f"{who} has no predicted image tags (tagger={tagger!r}): the option belongs to the training-free regime "
                         "(TrainingFreePipeline.run_batch / run_batch_ragged)")


MAX_NUM_CLASSES = 255      # background + 254 foreground classes


def check_num_classes(num_classes):
    """The label maps are uint8 with 255 as the ignore value, and a present class c is written as the key c + 1: the largest
    vocabulary is 254 foreground classes plus background."""
    if not 1 <= int(num_classes) <= MAX_NUM_CLASSES:
        raise ValueError(f"num_classes = {num_classes}: the label maps are uint8 with 255 as the ignore value, so at most "
                         f"{MAX_NUM_CLASSES} classes (254 foreground + background) fit")


def _check_clean(clean):
    """clean= of the pipelines -> dict(min_region=, connectivity=) checked by utils/components.py, or None."""
    if clean is None:
        return None
    from .utils import components as cc
    if not isinstance(clean, dict) or "min_region" not in clean or set(clean) - {"min_region", "connectivity"}:
        raise ValueError(f"clean must be dict(min_region=, connectivity=8) (got {clean!r})")
    cc.min_area_rule(clean["min_region"], 1, 1)
    v = clean["min_region"]
    return dict(min_region=int(v) if v >= 1 else float(v), connectivity=cc.check_connectivity(clean.get("connectivity", 8)))


def _check_fill(fill, clean):
    """fill= of the pipelines -> dict(radius=None | int) checked by utils/label_fill.py, or None.  It fills what the cleaning removed."""
    if fill is None:
        return None
    from .utils import label_fill as lf
    if not isinstance(fill, dict) or set(fill) - {"radius"}:
        raise ValueError(f"fill must be dict(radius=None | pixels) (got {fill!r})")
    radius = fill.get("radius")
    radius = None if radius is None or (isinstance(radius, str) and radius == "inf") else radius
    lf.radius_rule(radius)
    if clean is None:
        raise ValueError(f"fill needs clean (fill={fill!r}): the main arg-max map has no 255 pixel, there is nothing to fill")
    return dict(radius=None if radius is None else int(radius))


def _check_snap(snap):
    """snap= of the pipelines -> dict(step=, compactness=, iters=, min_share=) checked by utils/superpixels.py, or None."""
    if snap is None:
        return None
    from .utils import superpixels as sx
    if not isinstance(snap, dict) or "step" not in snap or set(snap) - {"step", "compactness", "iters", "min_share"}:
        raise ValueError(f"snap must be dict(step=, compactness=10, iters=5, min_share=0.0) (got {snap!r})")
    step, compactness, iters = sx.check_params(snap["step"], snap.get("compactness", sx.DEFAULTS["compactness"]),
                                               snap.get("iters", sx.DEFAULTS["iters"]))
    share = snap.get("min_share", sx.DEFAULTS["min_share"])
    sx.share_rule(share)
    return dict(step=step, compactness=compactness, iters=iters, min_share=float(share))


class TrainingFreePipeline:
    def __init__(self, model, num_classes=21, dilations=ops.PAR_DILATIONS, num_iter=20, caa_thre=0.79, smax=6, guard=None,
                 tta_scales=None, tta_flip=False, tagger=None, image_scores=False, boundary=None, bkg_sweep=None, bkg_scale=1.0, clean=None, fill=None, snap=None, margin_sweep=None, margin_min=None):
        """`smax` = the largest number of present classes of any image that will be fed (known from the host-side
        image-level labels; VOC train_aug: 6).  run_batch* do not check it: an image with more present classes is processed with
        its first `smax` classes in ascending order and the others are dropped (include/excel_hip.h, excel_cls_compact;
        tests/test_gpu_many_classes.py) - a caller that must not lose classes checks the one-hot rows itself, like tools/infer_lam.
        `guard` = the overflow guard of the f16 GEMM modes (an activation beyond 65 504 turns an image's maps into NaNs there):
          None       today's step, launch for launch;
          "skip"     run_batch / run_batch_ragged count the non-finite values per image in what they hand to the random walk (attr, the
                     affinity) and in its result, score only the images without one (ops.confusion_accumulate_masked) and leave the
                     counts in `last_flags` (device int32 [B], until the next step on the stream) and `last_guard` (a GuardTicket);
          "observe"  the same counts and ticket, every image scored (the exact-fp32 second pass, see exact_mode).
        `tta_scales` / `tta_flip` = test-time augmentation of the LAMs (utils/camutils.py:8-63), off by default (None / False, also for
        the single scale (1.0,) without flip: today's step, launch for launch).  With it, run_batch / run_batch_ragged run the model once
        per scale of `tta_scales` (tta_sizes: 1.0 must be among them) on [x; mirror x] (tta_flip) and ops.lam_tta_fuse fuses the maps at
        the patch grid of scale 1.0 into the `attr` the random walk reads; the affinity is that of the un-mirrored scale-1.0 pass.
        `tagger` = dict(thre=, kmax=, scale=) (check_tagger; kmax must equal smax), off by default (None: today's step, launch for
        launch).  With it, run_batch / run_batch_ragged ignore the values of `cls_labels` (None is accepted): right after the scale-1.0
        forward, model.image_tags predicts the one-hot rows on the device (ops.clip_tags over CLIP's image embedding and the text rows)
        and those go to ops.cls_compact.  They stay in `last_tags` = (onehot, scores) (device [B,F], until the next step) and travel to
        the host behind `last_tag_ticket` (a TagTicket) - no synchronisation.  Everything behind cls_compact is untouched.
        `image_scores` = per-image scores, off by default (False: today's step, launch for launch).  With it, every matrix run_batch /
        run_batch_ragged score (hist, hist_conf, a ValidationPipeline's hist_seg) also gets ops.image_scores on the same arrays - with the
        step's guard flags as `skip` when guard == "skip" - and the counts travel to the host behind `last_score_ticket` (a ScoreTicket:
        counts() -> {"main": ..., "conf": ..., "seg": ...}, int32 [B,3,nc] each) - no synchronisation.
        `boundary` = None | dict(ratio=, px=): Boundary IoU counts, off by default (no launch).  With it - it requires image_scores=True -
        every set that gets ops.image_scores also gets ops.boundary_scores on the same arrays and stream, every image's radius from the
        host rule utils/image_scores.boundary_radius; the rows travel in the same ticket under "<set>_bd".
        `bkg_scale` = the factor on the background plane of the arg-max (utils/bkg_sweep.py), 1.0 by default (today's step, launch for
        launch).  With another value run_batch_ragged takes its labels from bkg_sweep.sweep_ragged at that scale - PAR is linear per
        channel, so they are the labels PAR of the scaled background would have given - and everything behind them (confusion, per-image
        and boundary scores, what the caller saves) reads those; the conf labels and a CRF stage are built from the cams and do not change.
        `bkg_sweep` = a tuple of scales (bkg_sweep.check_scales), None by default (no launch).  With it and ground truth, one more launch
        per ragged step adds the step's counts at every scale into `sweep_totals` (int64 [K,3,nc]: ground-truth area, predicted area and
        intersection per class - bkg_sweep.scores_from_totals), with the guard's flags as `skip` exactly when the confusion matrix gets
        them.  Both are for run_batch_ragged; the uniform and multi-stream paths refuse them.
        `clean` = dict(min_region=, connectivity=8) (utils/components.py), None by default (no launch).  With it run_batch_ragged labels
        the connected regions of the step's main label map - whatever bkg_scale produced it - and turns every class region below
        min_region (pixels, or a fraction of each image's area: components.min_area_rule) into 255: the cleaned maps stay in
        `last_clean_labels` (flat uint8 like the labels) and the per-image counts (regions, regions removed, pixels removed) in
        `last_clean_counts` (int32 [B,3]) on the device until the next step; with ground truth the kept pixels go into `hist_clean`,
        and with image_scores the step's ScoreTicket gets a set named "clean".  The returned labels are untouched; the uniform and
        multi-stream paths refuse the option.
        `fill` = dict(radius=None | pixels) (utils/label_fill.py), None by default (no launch); it needs `clean`.  Behind the cleaning,
        every pixel the cleaning turned into 255 takes the value of the nearest class pixel of its image (within `radius`, None =
        unlimited; the main labels are the mask, so a 255 they already had stays): the filled maps stay in `last_fill_labels`, the
        squared distances in `last_fill_dist2` (int32, like the labels) and the per-image counts (holes, filled, largest squared
        distance) in `last_fill_counts` (int32 [B,3]) until the next step; with ground truth the filled maps go into `hist_fill`, and
        with image_scores the step's ScoreTicket gets a set named "fill".  The main and cleaned outputs are untouched.
        `snap` = dict(step=, compactness=10, iters=5, min_share=0.0) (utils/superpixels.py), None by default (no launch).  With it
        run_batch_ragged over-segments the step's decoded images into superpixels of grid step `step` (integer SLIC) and gives every
        superpixel the majority class of the main arg-max labels inside it (only where that class holds at least `min_share` of the
        votes): the snapped maps stay in `last_snap_labels` (flat uint8 like the labels), the superpixel index of every pixel in
        `last_snap_sp` (int32) and the per-image counts (superpixels with a vote, snapped, pixels changed) in `last_snap_counts`
        (int32 [B,3]) until the next step; with ground truth the snapped maps go into `hist_snap`, and with image_scores the step's
        ScoreTicket gets a set named "snap".  With snap, `clean` and `fill` take the snapped map as their input and mask: the order is
        snap -> clean -> fill.  The returned labels are untouched; the uniform and multi-stream paths refuse the option.
        `margin_sweep` = a tuple of arg-max margin thresholds (utils/margin.check_thresholds), `margin_min` = one such value; both None by
        default (no launch).  With either, run_batch_ragged runs ONE margin.margin_ragged launch behind the arg-max, on the step's PAR
        output with bkg_scale: margin_sweep adds the step's pixel counts per threshold into `margin_kept` (int64 [K+1], no ground truth
        needed; coverage = margin.coverage_from_kept) and, with ground truth, the counts of the kept pixels into `margin_totals` (int64
        [K,3,nc], bkg_sweep.scores_from_totals), with the guard's flags as `skip` exactly when the confusion matrix gets them;
        margin_min leaves the labels with 255 where the margin is below it in `last_margin_labels` (flat uint8 like the labels, until
        the next step) and, with ground truth, their kept pixels in `hist_margin`; with image_scores the step's ScoreTicket gets a set
        named "margin".  The returned labels, hist and the snap -> clean -> fill chain are untouched; the uniform and multi-stream
        paths refuse both."""
        self.clean = _check_clean(clean)
        self.fill = _check_fill(fill, self.clean)
        self.snap = _check_snap(snap)
        from .utils import margin as _mrg
        self.margin_sweep = _mrg.check_thresholds(margin_sweep) if margin_sweep is not None else None
        self.margin_min = _mrg.check_min(margin_min) if margin_min is not None else None
        for stage in STAGES.values():                   # what every label stage leaves behind (utils/label_stages.py)
            setattr(self, "hist_" + stage.name, None)
            setattr(self, f"last_{stage.name}_labels", None)
            if stage.rows is not None:
                setattr(self, f"last_{stage.name}_counts", None)
        self.last_fill_dist2 = self.last_snap_sp = None
        self.margin_totals = self.margin_kept = None
        from .utils import bkg_sweep as _bkg
        self.bkg_sweep = _bkg.check_scales(bkg_sweep) if bkg_sweep is not None else None
        self.bkg_scale = _bkg.check_scale(bkg_scale)
        self.sweep_totals = None
        self.image_scores = bool(image_scores)
        from .utils.image_scores import check_boundary
        self.boundary = check_boundary(boundary)
        if self.boundary is not None and not self.image_scores:
            raise ValueError("boundary= needs image_scores=True: the boundary counts travel in the step's ScoreTicket")
        self.last_score_ticket = None
        if guard not in GUARD_MODES:
            raise ValueError(f"guard must be one of {GUARD_MODES} (got {guard!r})")
        self.guard = guard
        self.last_flags = self.last_guard = None
        self.tta_flip = bool(tta_flip)
        self.tta_scales = tuple(float(x) for x in tta_scales) if tta_scales is not None else (1.0,)
        self.tta = self.tta_flip or self.tta_scales != (1.0,)
        if self.tta:
            _check_tta_scales(self.tta_scales)
        self.model = model
        check_num_classes(num_classes)
        self.num_classes = num_classes
        self.dilations = tuple(dilations)
        self.num_iter = num_iter
        self.caa_thre = caa_thre
        self.smax = smax
        self.tagger = check_tagger(tagger, smax, num_classes)
        self.last_tags = self.last_tag_ticket = None
        self.hist = None
        self.hist_conf = None               # the confident labels' matrix (run_batch_ragged(conf=)): counts the kept pixels only
        self.last_conf_labels = None
        self._bufs = {}

    @property
    def device(self):
        """Where the model lives (tools/infer_lam.validate reads it from a caller-supplied pipeline)."""
        return torch.device(getattr(self.model, "device", "cuda"))

    def reset(self):
        self.drain()
        self.hist = None
        self.hist_conf = None
        for name in STAGES:
            setattr(self, "hist_" + name, None)
        self.sweep_totals = None
        self.margin_totals = self.margin_kept = None

    def _buf(self, name, numel, dtype=torch.float32, device=None):
        """Step-persistent scratch (cams, PAR output, PAR workspace): one grow-only flat buffer per (name, launch stream), so a step
        allocates nothing and launches no fill kernels.  Only buffers nobody outside the step keeps are taken from here.
        The buffers are NOT initialised and the producers skip what nobody reads: pad columns (W_b <= x < Wp_b) and the planes of
        unused channels (c >= nchan[b]) of the step's cams / PAR output hold garbage.  The step's own consumers clamp to W_b - 1 and
        nchan[b]; a new consumer (saving cams, a CRF stage) must do the same or ask for `return_intermediates=True`, which switches to
        fresh zero-filled tensors."""
        key = (name, torch.cuda.current_stream().cuda_stream)
        b = self._bufs.get(key)
        if b is None or b.numel() < numel or b.dtype != dtype:
            self._bufs.pop(key, None)
            b = None
            b = self._bufs[key] = torch.empty(int(numel), dtype=dtype, device=device)
        return b[:int(numel)]

    # ------------------------------------------------------------------ overflow guard
    def _guard_count(self, *tensors):
        """guard set: per-image non-finite counts over `tensors` ([B, ...] each; the first launch writes, the rest add), then the copy to
        pinned memory and the event of the step's ticket - all on the step's stream, no synchronisation.  -> the device counts or None."""
        if self.guard is None:
            return None
        B = tensors[0].shape[0]
        flags = self._buf("guard", B, torch.int32, tensors[0].device)
        for i, t in enumerate(tensors):
            ops.nonfinite_count(t, out=flags, init=(i == 0))
        host = torch.empty((B,), dtype=torch.int32, pin_memory=True)
        host.copy_(flags, non_blocking=True)
        ev = torch.cuda.Event()
        ev.record()
        self.last_flags, self.last_guard = flags, GuardTicket(host, ev)
        return flags

    # ------------------------------------------------------------------ predicted image tags
    def _tags(self, cls_labels):
        """Without a tagger: the caller's one-hot rows.  With one: the rows model.image_tags predicts from the forward that has just run
        (the un-mirrored scale-1.0 pass), kept in last_tags, plus their pinned copy and event (last_tag_ticket) on the step's stream."""
        if self.tagger is None:
            return cls_labels
        onehot, scores = self.model.image_tags(**self.tagger)
        self.last_tags = (onehot, scores)
        h1 = torch.empty(onehot.shape, dtype=torch.float32, pin_memory=True)
        h2 = torch.empty(scores.shape, dtype=torch.float32, pin_memory=True)
        h1.copy_(onehot, non_blocking=True)
        h2.copy_(scores, non_blocking=True)
        ev = torch.cuda.Event()
        ev.record()
        self.last_tag_ticket = TagTicket(h1, h2, ev)
        return onehot

    def _no_tagger(self, what):
        if self.tagger is not None:
            raise ValueError(f"{what} has no predicted image tags (tagger={self.tagger!r}): use run_batch or run_batch_ragged, or build "
                             "the pipeline without tagger")

    def _score(self, gts, labels, flags, plan=None, into="hist"):
        """-> the confusion matrix `into` (self.hist, self.hist_conf, a label stage's self.hist_<name>) with this step's pixels added.
        The score set of the per-image counts is "main" for hist, else what follows "hist_"."""
        hist = getattr(self, into)
        if self.image_scores:
            self._image_scores("main" if into == "hist" else into[len("hist_"):], gts, labels, flags if self.guard == "skip" else None, plan)
        if self.guard == "skip":
            return ops.confusion_accumulate_masked(gts, labels, self.num_classes, flags, hist, plan=plan)
        return ops.confusion_accumulate(gts, labels, self.num_classes, hist)                       # evaluate.py:9-20

    def _image_scores(self, which, gts, labels, skip=None, plan=None):
        """image_scores set: the per-image counts of one scored matrix, added to the step's ScoreTicket (on the step's stream)."""
        B = plan.B if plan is not None else int(gts.shape[0])
        out = self._buf("image_scores_" + which, B * 3 * self.num_classes, torch.int32, gts.device)
        out_bd = self._buf("boundary_scores_" + which, B * 3 * self.num_classes, torch.int32, gts.device) if self.boundary is not None else None
        self.last_score_ticket.launch(which, gts, labels, self.num_classes, skip=skip, plan=plan, out=out, boundary=self.boundary, out_bd=out_bd)

    def _no_image_scores(self, what):
        if self.image_scores:
            raise ValueError(f"{what} has no per-image scores (image_scores=True): its sub-batches run on streams of their own - use "
                             "run_batch or run_batch_ragged, or build the pipeline without image_scores")

    def _no_bkg(self, what):
        if self.bkg_sweep is not None:
            raise ValueError(f"{what} has no background sweep (bkg_sweep={self.bkg_sweep}): it runs behind the ragged step - use "
                             "run_batch_ragged, or build the pipeline without bkg_sweep")
        if self.bkg_scale != 1.0:
            raise ValueError(f"{what} has no background scale (bkg_scale={self.bkg_scale}): it runs behind the ragged step - use "
                             "run_batch_ragged, or build the pipeline with bkg_scale=1.0")

    def _no_margin(self, what):
        if self.margin_sweep is not None:
            raise ValueError(f"{what} has no margin sweep (margin_sweep={self.margin_sweep}): it runs behind the ragged step - use "
                             "run_batch_ragged, or build the pipeline without margin_sweep")
        if self.margin_min is not None:
            raise ValueError(f"{what} has no margin labels (margin_min={self.margin_min}): they are made behind the ragged step - use "
                             "run_batch_ragged, or build the pipeline without margin_min")

    def _margin(self, par_out, plan, C, nchan, idx, gts_packed, flags):
        """margin_sweep / margin_min set: one launch over the step's PAR output - the counts per threshold, the labels cut at margin_min -
        and the score of those labels (all on the step's stream, no synchronisation)."""
        from .utils.margin import margin_ragged
        sweep = self.margin_sweep or ()
        out = self._buf("margin_labels", plan.total_label_pix, torch.uint8, par_out.device) if self.margin_min is not None else None
        counted = bool(sweep) and gts_packed is not None
        totals, kept, self.last_margin_labels, _ = margin_ragged(
            par_out, plan, C, sweep, nchan=nchan, cls_idx=idx, gts=gts_packed if counted else None, num_classes=self.num_classes,
            skip=flags if self.guard == "skip" else None, totals=self.margin_totals if counted else None,
            kept=(self.margin_kept if self.margin_kept is not None else True) if sweep else None,
            label_thre=self.margin_min, labels_out=out, bkg_scale=self.bkg_scale)
        if counted:
            self.margin_totals = totals
        if sweep:
            self.margin_kept = kept
        if self.margin_min is not None and gts_packed is not None:
            self.hist_margin = self._score(gts_packed, self.last_margin_labels, flags, plan=plan, into="hist_margin")

    def _no_clean(self, what):
        if self.clean is not None:
            raise ValueError(f"{what} has no label cleaning (clean={self.clean}): it runs behind the ragged step - use run_batch_ragged, "
                             "or build the pipeline without clean")
        if self.snap is not None:
            raise ValueError(f"{what} has no superpixel snap (snap={self.snap}): it runs behind the ragged step - use run_batch_ragged, "
                             "or build the pipeline without snap")

    def _snap(self, labels, hwc_packed, plan, gts_packed, flags):
        """snap set: superpixels of the step's decoded images, the majority vote of the main labels inside each, the score of the
        snapped maps (all on the step's stream, no synchronisation; the centre offsets are host integers, cached on the plan)."""
        from .utils import superpixels as sx
        if hwc_packed is None:
            raise ValueError("snap needs the step's decoded images (hwc_packed)")
        dev, n, k = labels.device, plan.total_label_pix, self.snap
        cache = plan.__dict__.setdefault("_snap_cent", {})
        cent = cache.get(k["step"])
        if cent is None:
            cent = cache[k["step"]] = sx.centre_table([(int(h), int(w)) for h, w in plan.hw], k["step"], dev)
        sp, _, _ = sx.slic_superpixels(hwc_packed, k["step"], k["compactness"], k["iters"], plan=plan, cent=cent,
                                       out=(self._buf("snap_sp", n, torch.int32, dev), self._buf("snap_centres", 5 * cent[1], torch.int32, dev)))
        self.last_snap_sp = sp
        self.last_snap_labels, self.last_snap_counts = sx.snap_labels(
            labels, sp, k["step"], self.num_classes, k["min_share"], plan=plan, cent=cent,
            out=(self._buf("snap_labels", n, torch.uint8, dev), self._buf("snap_counts", 3 * plan.B, torch.int32, dev)))
        if gts_packed is not None:
            self.hist_snap = self._score(gts_packed, self.last_snap_labels, flags, plan=plan, into="hist_snap")

    def _clean(self, labels, plan, gts_packed, flags):
        """clean set: label the step's main map, filter it, score the kept pixels (all on the step's stream, no synchronisation)."""
        from .utils import components as cc
        dev = labels.device
        value = self.clean["min_region"]
        if value >= 1:
            thr = int(value)
        else:                                                 # a fraction of every image's own area: host integers, cached on the plan
            cache = plan.__dict__.setdefault("_clean_thr", {})
            thr = cache.get(value)
            if thr is None:
                host = [cc.min_area_rule(value, int(h), int(w)) for h, w in plan.hw]
                thr = cache[value] = torch.tensor(host, dtype=torch.int32).to(dev, non_blocking=True)
        n = plan.total_label_pix
        comp, area = cc.label_components(labels, plan=plan, connectivity=self.clean["connectivity"],
                                         out=(self._buf("cc_comp", n, torch.int32, dev), self._buf("cc_area", n, torch.int32, dev)))
        self.last_clean_labels, self.last_clean_counts = cc.filter_small_regions(labels, comp, area, thr, self.num_classes, plan=plan)
        if gts_packed is not None:
            self.hist_clean = self._score(gts_packed, self.last_clean_labels, flags, plan=plan, into="hist_clean")

    def _fill(self, labels, plan, gts_packed, flags):
        """fill set: what _clean removed takes the nearest class of its image, the step's main labels as the mask; score the filled maps
        (all on the step's stream, no synchronisation)."""
        from .utils import label_fill as lf
        dev, n = labels.device, plan.total_label_pix
        self.last_fill_labels, self.last_fill_dist2, self.last_fill_counts = lf.fill_nearest_label(
            self.last_clean_labels, self.num_classes, plan=plan, mask=labels, radius=self.fill["radius"],
            out=(self._buf("fill_labels", n, torch.uint8, dev), self._buf("fill_dist2", n, torch.int32, dev),
                 self._buf("fill_counts", 3 * plan.B, torch.int32, dev)))
        if gts_packed is not None:
            self.hist_fill = self._score(gts_packed, self.last_fill_labels, flags, plan=plan, into="hist_fill")

    def _no_guard(self, what):
        if self.guard is not None:
            raise ValueError(f"{what} has no overflow guard (guard={self.guard!r}): it is a bench / training path - use run_batch or "
                             "run_batch_ragged, or build the pipeline with guard=None")

    @contextlib.contextmanager
    def exact_mode(self):
        """Switch the model's ViT handle to exact fp32 ("f32") for the block and restore the mode it found (the second pass over the
        images the guard flagged).  Switching re-splits the weights and synchronises the device: not for use inside a timed loop."""
        h = self.model.encoder.visual.handle()
        before = h.gemm_mode()
        h.set_gemm_mode("f32")
        try:
            yield self
        finally:
            h.set_gemm_mode(before)

    # ------------------------------------------------------------------ flip / multi-scale LAMs (utils/camutils.py:8-63)
    # The step's own `attr` is the model's maps of one pass.  With tta_scales / tta_flip it is the fuse of one pass per scale over
    # [x; mirror x]: every scale's maps go to the patch grid of scale 1.0, max with the mirrored half, sum, min-max - one op
    # (ops.lam_tta_fuse) whose output is the [B,P,F] the random walk and the box mask read.  The reference's own fuse resizes to
    # pixel size (camutils.multi_scale_lam); the step fuses at the grid because everything downstream of `attr` works there and
    # cam_upsample_bkg does the one up-sampling to the label size afterwards.
    def _no_tta(self, what):
        if self.tta:
            raise ValueError(f"{what} has no flip / multi-scale fuse (tta_scales={self.tta_scales}, tta_flip={self.tta_flip}): use "
                             "run_batch or run_batch_ragged, or build the pipeline without tta_scales / tta_flip")

    def _tta_uniform_input(self, inputs, S_s):
        """[B,3,S,S] f32 -> the network input of one scale, [x_s; mirror x_s] with tta_flip (camutils.py:50-51)."""
        x = inputs if S_s == inputs.shape[-1] else ops.bilinear_resize(inputs, S_s, S_s, align_corners=False)
        return torch.cat([x, x.flip(-1)], 0) if self.tta_flip else x

    def _tta_ragged_input(self, hwc_packed, plan, S_s, name):
        """The packed uint8 images -> the network input of one scale, straight from the decoded pixels (no float image is resized twice)."""
        nb = plan.B * (2 if self.tta_flip else 1)
        out = self._buf(name, nb * 3 * S_s * S_s, device=hwc_packed.device).view(nb, 3, S_s, S_s)
        if self.tta_flip:
            return ops.normalize_resize_u8_ragged_mirror(hwc_packed, plan, S_s, out=out)           # camutils.py:15
        return ops.normalize_resize_u8_ragged(hwc_packed, plan, S_s, out=out)

    def _tta_maps(self, x, P1):
        """model.attr_maps over x [n,3,S_s,S_s], cut into image groups of about the token count of the scale-1.0 pass (a 1.5x scale has
        2.25x the tokens and 5x the attention scores per image).  The ViT is batch-invariant bit for bit: the grouping changes nothing."""
        n, P_s = x.shape[0], (x.shape[-1] // 16) ** 2
        step = max(1, min(n, n * P1 // P_s))
        if step >= n:
            return self.model.attr_maps(x)
        return torch.cat([self.model.attr_maps(x[lo:lo + step]) for lo in range(0, n, step)], 0)

    def _tta_attr(self, S, make_input, cls_labels=None):
        """One model pass per scale (tta_sizes(S, tta_scales): 1.0 first) over make_input(S_s) = [B or 2B, 3, S_s, S_s], then the fuse.
        Scale 1.0's un-mirrored half runs as the plain step does and supplies the affinity (tools/infer_lam.py:79 before :82); every
        other pass asks the tower for the maps alone; with a tagger that pass also supplies the tags (_tags).
        -> (attr [B,P,F], attn_weights of scale 1.0, the step's one-hot rows)"""
        g = S // 16
        maps, grids, attn_w = [], [], None
        for S_s, g_s in tta_sizes(S, self.tta_scales):
            x = make_input(S_s)
            B = x.shape[0] // 2 if self.tta_flip else x.shape[0]
            if attn_w is None:
                _, _, m, attn_w, _ = self.model(x[:B])                                              # infer_lam.py:79
                cls_labels = self._tags(cls_labels)
                if self.tta_flip:
                    m = torch.cat([m, self._tta_maps(x[B:], g * g)], 0)
            else:
                m = self._tta_maps(x, g * g)
            maps.append(m)
            grids.append(g_s)
        return ops.lam_tta_fuse(maps, grids, g, self.tta_flip), attn_w, cls_labels

    @torch.no_grad()
    def run_batch(self, inputs, cls_labels, gts=None, label_hw=None, return_intermediates=False):
        """inputs [B,3,S,S] f32 (normalised, already at the network size), cls_labels [B,F] f32 one-hot (ignored, and may be None, when the
        pipeline has a tagger), gts [B,H,W] uint8 (255 = ignore) or None.  Returns labels [B,H,W] uint8 (device)."""
        self._no_bkg("run_batch")
        self._no_clean("run_batch")
        self._no_margin("run_batch")
        B, _, S, _ = inputs.shape
        g = S // 16
        H, W = (gts.shape[-2:] if gts is not None else (label_hw or (S, S)))
        if self.image_scores:
            self.last_score_ticket = ScoreTicket()
        if self.tta:
            attr, attn_w, cls_labels = self._tta_attr(S, lambda S_s: self._tta_uniform_input(inputs, S_s), cls_labels)
        else:
            _, _, attr, attn_w, _ = self.model(inputs)                                              # infer_lam.py:79
            cls_labels = self._tags(cls_labels)
        idx, ncls, nchan = ops.cls_compact(cls_labels, self.smax, want_nchan=True)                  # affutils.py:203
        refined = ops.refine_cams_with_aff_batched(attr, attn_w.w_aff, idx, ncls, g, self.caa_thre)  # infer_lam.py:93
        flags = self._guard_count(attr, attn_w.w_aff, refined)
        C = self.smax + 1
        if return_intermediates:            # the caller keeps these: fresh tensors, unused channels zeroed
            cams = ops.cam_upsample_bkg(refined, ncls, g, H, W)                                     # affutils.py:164-166
            par_out = ops.par_forward(inputs, cams, self.dilations, self.num_iter, nchan=nchan)    # affutils.py:84
        else:
            dev = inputs.device
            cams = ops.cam_upsample_bkg(refined, ncls, g, H, W, out=self._buf("cams", B * C * H * W, device=dev).view(B, C, H, W),
                                        zero_unused=False)
            ws = self._buf("par_ws", ops.lib().excel_par_workspace_bytes(B, C, H, W, len(self.dilations)), torch.uint8, dev)
            par_out = ops.par_forward(inputs, cams, self.dilations, self.num_iter, nchan=nchan, ws=ws,
                                      out=self._buf("par_out", B * C * H * W, device=dev).view(B, C, H, W))
        labels = ops.argmax_label(par_out, nchan, idx)                                              # affutils.py:86-87
        if gts is not None:
            self.hist = self._score(gts, labels, flags)
        if return_intermediates:
            return labels, dict(attr=attr, w_aff=attn_w.w_aff, refined=refined, cams=cams, par_out=par_out,
                                cls_idx=idx, ncls=ncls)
        return labels

    # ------------------------------------------------------------------ ragged batches: every image at its OWN label size
    # The reference resizes the input to S x S but refines and scores at the image's original size (tools/infer_lam.py:74,94:
    # labels.shape[-2:]), batch 1.  Here the size-uniform half (ViT, CAM, random walk) runs as one batch as before, and the
    # size-dependent half (input resize, up-sampling, PAR, arg-max) runs over packed, pitched planes through a tile map
    # (ops.RaggedPlan; include/excel_hip.h "ragged batches"): one launch per stage whatever the mix of sizes.
    @torch.no_grad()
    def run_batch_ragged(self, hwc_packed, plan, cls_labels, gts_packed=None, S=448, return_intermediates=False, conf=None):
        """hwc_packed: the decoded uint8 [H_b,W_b,3] images back to back (device); plan = ops.RaggedPlan of their sizes;
        cls_labels [B,F] f32 one-hot (ignored, and may be None, when the pipeline has a tagger); gts_packed: the uint8 [H_b,W_b]
        ground-truth maps back to back (255 = ignore) or None.
        Returns the labels as one flat uint8 tensor (image b = plan.label(labels, b)).
        Without `return_intermediates` the cams / PAR output live in uninitialised step buffers (see _buf: pad columns and unused
        channels are undefined); with it they are fresh tensors whose unused parts are zero.
        `self.last_cams` is the step's cams (smax + 1 pitched planes per image) until the next step on the same stream overwrites it:
        a consumer queued on that stream right after the step (the --save_cam overlay) reads them without a copy.
        `conf` = (high_thre, low_thre) (check_conf) adds the two-threshold labels of utils/affutils.py:101-158 from those cams, on the same
        stream right after the main labels: the return value becomes (labels, conf_labels[, intermediates]), conf_labels a flat uint8
        tensor like labels with ignore_index 255 in the band; they stay in `self.last_conf_labels` until the next step and, with ground
        truth, go into `self.hist_conf` (which therefore counts the kept pixels: coverage = hist_conf.sum() / hist.sum())."""
        dev = hwc_packed.device
        B = plan.B
        g = S // 16
        if self.image_scores:
            self.last_score_ticket = ScoreTicket()
        if self.tta:
            first = []                      # the scale-1.0 input: its un-mirrored half is what PAR reads

            def make(S_s):
                x = self._tta_ragged_input(hwc_packed, plan, S_s, "inputs" if not first else "tta_inputs")
                first.append(x)
                return x
            attr, attn_w, cls_labels = self._tta_attr(S, make, cls_labels)
            inputs = first[0][:B]
        else:
            inputs = ops.normalize_resize_u8_ragged(hwc_packed, plan, S, out=self._buf("inputs", B * 3 * S * S, device=dev).view(B, 3, S, S))  # voc.py:115, infer_lam.py:74
            _, _, attr, attn_w, _ = self.model(inputs)                                              # infer_lam.py:79
            cls_labels = self._tags(cls_labels)
        idx, ncls, nchan = ops.cls_compact(cls_labels, self.smax, want_nchan=True)                  # affutils.py:203
        refined = ops.refine_cams_with_aff_batched(attr, attn_w.w_aff, idx, ncls, g, self.caa_thre)  # infer_lam.py:93
        flags = self._guard_count(attr, attn_w.w_aff, refined)
        return self._ragged_back_half(inputs, plan, g, refined, idx, ncls, nchan, gts_packed, return_intermediates,
                                      dict(attr=attr, w_aff=attn_w.w_aff), flags, conf=conf, hwc=hwc_packed)

    def _ragged_back_half(self, inputs, plan, g, refined, idx, ncls, nchan, gts_packed, return_intermediates, inter, flags=None, conf=None, hwc=None):
        """Up-sampling + background, PAR, arg-max and confusion of a ragged step (tools/infer_lam.py:94), shared by every regime.
        inputs [B,3,S,S] = the network input PAR reads; `inter` = the regime's own intermediates (attr, w_aff); `flags` = the guard's
        per-image counts (None without a guard); `conf` = run_batch_ragged's (high_thre, low_thre) or None; `hwc` = the step's decoded
        images (what snap= segments)."""
        conf = check_conf(conf)
        dev = inputs.device
        C = self.smax + 1
        keep = return_intermediates
        cams = ops.cam_upsample_bkg_ragged(refined, ncls, g, plan, zero_unused=keep,
                                           out=None if keep else self._buf("cams", C * plan.total_pix, device=dev))   # affutils.py:164-166
        self.last_cams = cams
        self.last_nchan, self.last_cls_idx = nchan, idx       # the step's class counts (k_b + 1) and compacted class lists, for the same consumers
        ws = self._buf("par_ws", ops.lib().excel_par_ragged_workspace_bytes(plan.total_pix, C), torch.uint8, dev)
        par_out = ops.par_forward_ragged(inputs, cams, plan, C, self.dilations, self.num_iter, nchan=nchan, ws=ws,
                                         out=None if keep else self._buf("par_out", C * plan.total_pix, device=dev))   # affutils.py:84
        if self.bkg_scale == 1.0:
            labels = ops.argmax_label_ragged(par_out, plan, C, nchan, idx)                          # affutils.py:86-87
        else:                                                 # the same arg-max with the background plane scaled (utils/bkg_sweep.py)
            from .utils.bkg_sweep import sweep_ragged
            labels = sweep_ragged(par_out, plan, C, (self.bkg_scale,), nchan=nchan, cls_idx=idx, label_sel=0)[1]
        if gts_packed is not None:
            self.hist = self._score(gts_packed, labels, flags, plan=plan)
            if self.bkg_sweep is not None:                    # the step's counts at every scale of the sweep, from the same planes
                from .utils.bkg_sweep import sweep_ragged
                self.sweep_totals = sweep_ragged(par_out, plan, C, self.bkg_sweep, nchan=nchan, cls_idx=idx, gts=gts_packed,
                                                 num_classes=self.num_classes, skip=flags if self.guard == "skip" else None,
                                                 totals=self.sweep_totals)[0]
        if self.margin_sweep is not None or self.margin_min is not None:
            self._margin(par_out, plan, C, nchan, idx, gts_packed, flags)
        chain = labels                                        # what clean and fill work on: the main labels, or the snapped ones
        if self.snap is not None:
            self._snap(labels, hwc, plan, gts_packed, flags)
            chain = self.last_snap_labels
        if self.clean is not None:
            self._clean(chain, plan, gts_packed, flags)
            if self.fill is not None:
                self._fill(chain, plan, gts_packed, flags)
        if conf is None:
            if return_intermediates:
                return labels, dict(inputs=inputs.clone(), refined=refined, cams=cams, par_out=par_out, cls_idx=idx, ncls=ncls, **inter)
            return labels
        # the two-threshold labels (affutils.py:101-158) from the step's cams: half plan, one PAR over both groups, merge
        half = getattr(plan, "conf_half", None)
        if half is None:
            half = plan.conf_half = ops.conf_half_plan(plan)
        conf_labels, conf_planes, conf_par_out = conf_labels_ragged(inputs, cams, plan, half, self.smax, nchan, idx, conf[0], conf[1],
                                                                    self.dilations, self.num_iter, buf=self._buf, keep=keep)
        self.last_conf_labels = conf_labels
        if gts_packed is not None:
            self.hist_conf = self._score(gts_packed, conf_labels, flags, plan=plan, into="hist_conf")
        if return_intermediates:
            return labels, conf_labels, dict(inputs=inputs.clone(), refined=refined, cams=cams, par_out=par_out, cls_idx=idx, ncls=ncls,
                                             conf_planes=conf_planes, conf_par_out=conf_par_out, conf_plan=half, **inter)
        return labels, conf_labels

    # ------------------------------------------------------------------ concurrent sub-batches
    # Every kernel of the path leaves part of the chip idle in its last round of workgroups (e.g. the N=768 GEMMs of a
    # 32-image batch are 594 tiles for 256 CUs: 2.3 rounds).  run_batch_split runs the batch as `nsplit` independent
    # sub-batches, each on its own stream with its own workspaces: the tail of one sub-batch's kernel is filled by the
    # other's.  Same kernels, per-image results bit-identical to run_batch (images are independent).  Measured at B=32,
    # nsplit=2: +6 % before the GEMM tile selection became round-aware (gemm_bf16x3.hip), +1 % after; nsplit=4: no gain.
    @torch.no_grad()
    def run_batch_split(self, inputs, cls_labels, gts=None, label_hw=None, nsplit=2):
        """Same contract as run_batch; the returned labels and self.hist are complete only after drain()."""
        self._no_guard("run_batch_split")
        self._no_tta("run_batch_split")
        self._no_tagger("run_batch_split")
        self._no_image_scores("run_batch_split")
        self._no_bkg("run_batch_split")
        self._no_clean("run_batch_split")
        self._no_margin("run_batch_split")
        B, _, S, _ = inputs.shape
        nsplit = max(1, min(nsplit, B))
        if nsplit == 1:
            return self.run_batch(inputs, cls_labels, gts, label_hw)
        if len(getattr(self, "_sub", ())) != nsplit:
            self._sub = [dict(stream=torch.cuda.Stream(), hist=None) for _ in range(nsplit)]
        cur = torch.cuda.current_stream()
        H, W = (gts.shape[-2:] if gts is not None else (label_hw or (S, S)))
        labels = torch.empty((B, H, W), dtype=torch.uint8, device=inputs.device)
        step = -(-B // nsplit)
        for i, sub in enumerate(self._sub):
            lo, hi = i * step, min(B, (i + 1) * step)
            if lo >= hi:
                continue
            st = sub["stream"]
            st.wait_stream(cur)
            with torch.cuda.stream(st):
                for t in (inputs, cls_labels, labels) + ((gts,) if gts is not None else ()):
                    t.record_stream(st)
                main_hist, self.hist = self.hist, sub["hist"]
                try:
                    part = self.run_batch(inputs[lo:hi], cls_labels[lo:hi], None if gts is None else gts[lo:hi], (H, W))
                    sub["hist"] = self.hist
                finally:
                    self.hist = main_hist
                labels[lo:hi].copy_(part)
        return labels

    # ------------------------------------------------------------------ two-stream software pipeline
    # Stage A (ViT + CAM + random walk + up-sampling: matrix-core bound) and stage B (PAR + argmax + confusion:
    # HBM bound) use different hardware resources.  run_batch_overlapped enqueues stage A of batch i on stream A and
    # its stage B on stream B behind an event, so stage B of batch i overlaps stage A of batch i+1.  Results are
    # identical to run_batch (same kernels, same order per batch); only the issue order across batches changes.
    def _streams(self):
        if not hasattr(self, "_sa"):
            self._sa = torch.cuda.Stream()
            self._sb = torch.cuda.Stream()
            self._sb_done = None
        return self._sa, self._sb

    @torch.no_grad()
    def run_batch_overlapped(self, inputs, cls_labels, gts=None, label_hw=None):
        self._no_guard("run_batch_overlapped")
        self._no_tta("run_batch_overlapped")
        self._no_tagger("run_batch_overlapped")
        self._no_image_scores("run_batch_overlapped")
        self._no_bkg("run_batch_overlapped")
        self._no_clean("run_batch_overlapped")
        self._no_margin("run_batch_overlapped")
        sa, sb = self._streams()
        cur = torch.cuda.current_stream()
        B, _, S, _ = inputs.shape
        g = S // 16
        H, W = (gts.shape[-2:] if gts is not None else (label_hw or (S, S)))
        sa.wait_stream(cur)
        with torch.cuda.stream(sa):
            # the caller may free / reuse these right after the call: the caching allocator must know stream A reads them
            inputs.record_stream(sa)
            cls_labels.record_stream(sa)
            _, _, attr, attn_w, _ = self.model(inputs)
            idx, ncls, nchan = ops.cls_compact(cls_labels, self.smax, want_nchan=True)
            refined = ops.refine_cams_with_aff_batched(attr, attn_w.w_aff, idx, ncls, g, self.caa_thre)
            cams = ops.cam_upsample_bkg(refined, ncls, g, H, W)
            ready = torch.cuda.Event()
            ready.record(sa)
        with torch.cuda.stream(sb):
            sb.wait_event(ready)
            for t in (cams, nchan, idx, inputs) + ((gts,) if gts is not None else ()):
                t.record_stream(sb)
            par_out = ops.par_forward(inputs, cams, self.dilations, self.num_iter, nchan=nchan)
            labels = ops.argmax_label(par_out, nchan, idx)
            if gts is not None:
                self.hist = ops.confusion_accumulate(gts, labels, self.num_classes, self.hist)
        return labels

    def drain(self):
        """Make the caller's stream wait for the pipeline's side streams and fold the sub-batch histograms into
        self.hist (call before reading hist / labels of run_batch_split / run_batch_overlapped)."""
        cur = torch.cuda.current_stream()
        if hasattr(self, "_sa"):
            cur.wait_stream(self._sa)
            cur.wait_stream(self._sb)
        for sub in getattr(self, "_sub", ()):
            cur.wait_stream(sub["stream"])
            if sub["hist"] is not None:
                self.hist = sub["hist"] if self.hist is None else self.hist + sub["hist"]
                sub["hist"] = None


class OptimisedLamPipeline(TrainingFreePipeline):
    """The optimised-LAM regime (tools/infer_lam.py:79-94 with training_free=False: flip-TTA LAMs through the LVC branch and a
    seg_attn-gated affinity, both driven by the trained decoder head) for a ragged batch of B images at once, on the training-free
    pipeline's ragged back half.  Per image, labels are bit-identical to the reference's per-image call sequence:

        model(x, n_attn_out=6)                      -> per-layer maps of x, attn_fts(x), attn_pred = affinity over image x alone
        cure_attr_map_flip(model, x)                -> ex_feats = attn_fts([x; flip x]), ex_attn = affinity over that pair,
                                                       LVC-branch CAMs of [x; flip x], flip-max + min-max (camutils.py:8-30)
        refine_cams_with_aff(seg_attn=attn_pred)    -> gated affinity (affutils.py:182-195), random walk at caa_thre
        refine_cams_with_bkg_weclip                 -> up-sampling, PAR, arg-max at the image's own size

    The per-image sequence runs 5 image-forwards (x with the maps; [x; flip x] for ex_feats; [x; flip x] through the LVC branch).
    Here it is 4 full-batch forwards per image: attn_fts(x) of the first forward is reused as the x half of ex_feats (the tower's
    flags are those of model(x) in both calls, the per-layer maps are side outputs: the decoder input is the same bits), the flipped
    half comes from a feature-only forward of flip x.  The whole-batch means of excel_feature_affinity are replaced by the grouped
    entry (one image for attn_pred, the pair (x_b, flip x_b) for ex_attn), which is what the reference's batch-1 harness computes."""

    def __init__(self, model, num_classes=21, dilations=ops.PAR_DILATIONS, num_iter=20, caa_thre=0.79, smax=6, attn_layers=6, guard=None,
                 tta_scales=None, tta_flip=False, tagger=None, image_scores=False, boundary=None, bkg_sweep=None, bkg_scale=1.0, clean=None, fill=None, snap=None, margin_sweep=None, margin_min=None):
        check_num_classes(num_classes)
        _refuse_tta("OptimisedLamPipeline", tta_scales, tta_flip)
        _refuse_tagger("OptimisedLamPipeline", tagger)
        if getattr(model, "_dec", None) is None:
            raise ValueError("OptimisedLamPipeline needs the trained decoder head: build ExCEL_model(..., decoder_state_dict=) "
                             "(--training_free false --model_path)")
        super().__init__(model, num_classes=num_classes, dilations=dilations, num_iter=num_iter, caa_thre=caa_thre, smax=smax, guard=guard,
                         image_scores=image_scores, boundary=boundary, bkg_sweep=bkg_sweep, bkg_scale=bkg_scale, clean=clean, fill=fill, snap=snap, margin_sweep=margin_sweep, margin_min=margin_min)
        self.attn_layers = attn_layers

    def _tower(self, imgs, n_attn_out=0):
        """model.forward's tower call (model_excel.py:55-58 flags with a decoder head): maps, aliased feats, w_aff and x_raw as there."""
        return self.model.encoder.encode_image(imgs, True, None, want_w_aff=True, aff_layers=6, n_attn_out=n_attn_out, want_feats=True,
                                               feats_as_reference=True, want_raw=True, want_features=False)

    @torch.no_grad()
    def run_batch_ragged(self, hwc_packed, plan, cls_labels, gts_packed=None, S=448, return_intermediates=False, conf=None):
        """Same contract as TrainingFreePipeline.run_batch_ragged (flat uint8 labels, self.hist, self.last_cams, intermediates);
        `attr` of the intermediates is the flip-TTA LAM [B,P,F], `w_aff` the seg_attn-gated affinity [B,P,P]."""
        dev = hwc_packed.device
        B = plan.B
        g = S // 16
        if self.image_scores:
            self.last_score_ticket = ScoreTicket()
        model = self.model
        dec = model._dec
        inputs2 = ops.normalize_resize_u8_ragged_mirror(hwc_packed, plan, S,
                                                        out=self._buf("inputs2", 2 * B * 3 * S * S, device=dev).view(2 * B, 3, S, S))  # camutils.py:15
        inputs = inputs2[:B]
        # x: per-layer maps + decoder features (infer_lam.py:79 with n_attn_out=6)
        r = self._tower(inputs, n_attn_out=6)
        fts_x, _ = dec.forward(r["feats"], want_seg=False)                                          # model_excel.py:60-68
        attn_pred = ops.feature_affinity_grouped(fts_x, "sigmoid", group=1)                          # :70-76, batch 1 per image
        w_aff = ops.attn_select_mean(r["attn"], attn_pred, self.attn_layers)                         # affutils.py:182-195
        del r
        # flip x: decoder features only (the flipped half of camutils.py:17)
        r = self._tower(inputs2[B:])
        fts_f, _ = dec.forward(r["feats"], want_seg=False)
        del r
        ex_feats = torch.cat([fts_x, fts_f], 0)
        del fts_f
        ex_attn = ops.feature_affinity_grouped(ex_feats, "mask_softmax", group=2, member_stride=B)   # clip_surgery_model.py:128-137 per pair
        del ex_feats
        h = model.encoder.visual.handle()
        r = h.forward(inputs2, want_w_aff=False, want_raw=True, want_features=False, ex_attn=ex_attn)  # camutils.py:18
        del ex_attn
        maps = ops.patch_text_cam(r["x_raw"], model._text_rows, num_fg=model.num_classes - 1, mode=h.gemm_mode())[1]   # model_excel.py:52
        del r
        attr = ops.flip_max_normalize(maps, g)                                                      # camutils.py:21-26
        del maps
        idx, ncls, nchan = ops.cls_compact(cls_labels, self.smax, want_nchan=True)                  # affutils.py:203
        refined = ops.refine_cams_with_aff_batched(attr, w_aff, idx, ncls, g, self.caa_thre)         # infer_lam.py:93
        flags = self._guard_count(attr, w_aff, refined)
        return self._ragged_back_half(inputs, plan, g, refined, idx, ncls, nchan, gts_packed, return_intermediates,
                                      dict(attr=attr, w_aff=w_aff, attn_pred=attn_pred), flags, conf=conf, hwc=hwc_packed)


class ValidationPipeline(TrainingFreePipeline):
    """The in-training validation pass (engine/validatation_engine.py:19-37) for a ragged batch of B images at once, on the training-free
    pipeline's ragged back half.  Per image, both confusion matrices equal the reference's per-image call sequence bit for bit:

        model(x, n_attn_out=6)                      -> attr maps, per-layer maps, attn_fts, seg logits, attn_pred = affinity of x alone
        refine_cams_with_aff(seg_attn=attn_pred)    -> gated affinity (affutils.py:182-195), random walk at caa_thre 0.75 (:33)
        refine_cams_with_bkg_weclip                 -> up-sampling, PAR, arg-max at the image's own size   -> `self.hist`     (:34-36)
        bilinear(seg, label size) + argmax(1)       -> seg prediction at the image's own size             -> `self.hist_seg` (:27, :37)

    One tower forward per batch with model(x, n_attn_out=6)'s flags.  The model's own attn_pred takes its mean over the whole batch tensor
    (= the reference only at batch 1); here it is the grouped entry with group 1, the per-image affinity.  The seg logits [B,nc,g,g] go to
    every image's label size and through the arg-max in one launch (ops.seg_resize_argmax_uniform); no host round trip inside a batch."""

    def __init__(self, model, num_classes=21, dilations=ops.PAR_DILATIONS, num_iter=20, caa_thre=0.75, smax=6, attn_layers=6, guard=None,
                 tta_scales=None, tta_flip=False, tagger=None, image_scores=False, boundary=None, bkg_sweep=None, bkg_scale=1.0, clean=None, fill=None, snap=None, margin_sweep=None, margin_min=None):
        check_num_classes(num_classes)
        _refuse_tta("ValidationPipeline", tta_scales, tta_flip)
        _refuse_tagger("ValidationPipeline", tagger)
        if getattr(model, "_dec", None) is None:
            raise ValueError("ValidationPipeline needs the decoder head: build ExCEL_model(..., decoder_state_dict=)")
        if guard is not None:
            raise ValueError(f"ValidationPipeline has no overflow guard (guard={guard!r}): the in-training validation pass scores two "
                             "histograms per step and is out of the guard's scope")
        super().__init__(model, num_classes=num_classes, dilations=dilations, num_iter=num_iter, caa_thre=caa_thre, smax=smax,
                         image_scores=image_scores, boundary=boundary, bkg_sweep=bkg_sweep, bkg_scale=bkg_scale, clean=clean, fill=fill, snap=snap, margin_sweep=margin_sweep, margin_min=margin_min)
        self.attn_layers = attn_layers
        self.hist_seg = None

    def reset(self):
        super().reset()
        self.hist_seg = None

    @torch.no_grad()
    def run_batch_ragged(self, hwc_packed, plan, cls_labels, gts_packed=None, S=320, return_intermediates=False, conf=None):
        """Same contract as TrainingFreePipeline.run_batch_ragged (flat uint8 pseudo labels, self.hist, self.last_cams, intermediates);
        with ground truth it also accumulates the seg prediction's confusion matrix into self.hist_seg.  The intermediates add
        attn_pred [B,P,P], seg [B,nc,g,g] and seg_labels (flat uint8, image b = plan.label(seg_labels, b))."""
        dev = hwc_packed.device
        B = plan.B
        g = S // 16
        if self.image_scores:
            self.last_score_ticket = ScoreTicket()
        model = self.model
        h = model.encoder.visual.handle()
        inputs = ops.normalize_resize_u8_ragged(hwc_packed, plan, S, out=self._buf("inputs", B * 3 * S * S, device=dev).view(B, 3, S, S))  # :20
        r = model.encoder.encode_image(inputs, True, None, want_w_aff=True, aff_layers=6, n_attn_out=6, want_feats=True,
                                       feats_as_reference=True, want_raw=True, want_features=False)                   # :25 (model_excel.py:55-58)
        attr = ops.patch_text_cam(r["x_raw"], model._text_rows, num_fg=model.num_classes - 1, mode=h.gemm_mode())[1]  # model_excel.py:58
        fts, seg = model._dec.forward(r["feats"])                                                   # model_excel.py:60-68
        attn_pred = ops.feature_affinity_grouped(fts, "sigmoid", group=1)                            # :70-76, batch 1 per image
        del fts
        w_aff = ops.attn_select_mean(r["attn"], attn_pred, self.attn_layers)                         # affutils.py:182-195
        del r
        seg_labels = ops.seg_resize_argmax_uniform(seg, plan)                                        # :27, :37
        if gts_packed is not None:
            if self.image_scores:
                self._image_scores("seg", gts_packed, seg_labels, None, plan)
            self.hist_seg = ops.confusion_accumulate(gts_packed, seg_labels, self.num_classes, self.hist_seg)
        idx, ncls, nchan = ops.cls_compact(cls_labels, self.smax, want_nchan=True)                  # affutils.py:203
        refined = ops.refine_cams_with_aff_batched(attr, w_aff, idx, ncls, g, self.caa_thre)         # :33
        return self._ragged_back_half(inputs, plan, g, refined, idx, ncls, nchan, gts_packed, return_intermediates,
                                      dict(attr=attr, w_aff=w_aff, attn_pred=attn_pred, seg=seg, seg_labels=seg_labels), conf=conf, hwc=hwc_packed)   # :34-36
