"""Decoder training: mirror of scripts/train_voc.py.  `train(args)` is the program (data, loop, logging, checkpoints, validation);
DecoderTrainer.train_step is one iteration, the loop body of :172-220:

  frozen CLIP surgery forward + CAMs (the hot path)      -> attr_maps_raw, attention            :186
  decoder head in training mode                          -> segs, fts_diver, attn_pred          :186 (model/model_excel.py:60-76)
  pseudo labels: refine_cams_with_aff (+ seg_attn after `lvc_iter`) + refine_cams_with_bkg_weclip on the DE-normalised image  :188-199
  seg loss on the up-sampled logits + affinity ("diver") loss on attn_pred, w_diver = 0.1                                       :202-215
  backward of the head, gradient all-reduce over RCCL (DistributedDataParallel's mean), PolyWarmupAdamW step                    :217-219

All tensor work runs in libexcel_hip.so; torch carries device memory and the one collective.  The data path of `train`: decode
threads read the VOC tree (datasets/voc.VOC12ClsDataset) and draw each sample's augmentation parameters on the host, a copy stream
stages the ragged batch and the transform's table (datasets/loader.DeviceFeeder), and ops.train_augment applies the reference's
training transform on the device.  The validation pass every --eval_iters runs on ragged batches split across the ranks
(engine/validatation_engine.build_validation_ragged: its own decode threads and copy stream, the same confusion matrices as the reference's
per-image loop, which --val_api_path true runs instead).  With --save_visual true, rank 0 renders the reference's TensorBoard grids
(:233-246: input batch, CAM heat-map, affinity and patch-grid pseudo labels, ground truth, prediction) every --log_iters iterations in
one launch (ops.train_panels) and writes them as <visual_dir>/iter_<N>/<panel>.png; train(tb_writer=...) hands the same grids to any
object with add_image (utils/tbutils.py).  No TensorBoard event files are written.

Stopping and continuing a run (the reference ships save_train / resume_train, utils/pyutils.py:114-181, without wiring them in; the
state file's keys step / model_state_dict / optimizer_state_dict / lr are theirs, see utils/train_state.py):
  --save_state_iters N   rank 0 writes <work_dir>/checkpoints/train_state_iter_<n>.pth after every N-th iteration: head weights, AdamW
                         moments, the iteration count and the settings the continuation depends on.  Independent of --eval_iters,
                         --save_ckpt and --save_ckpt_from; model_iter_<n>.pth files are written as without it.
  --keep_states K        only the K newest state files stay (default 2)
  --iters_per_run N      this process runs at most N iterations, writes the state at its last one (after that iteration's validation and
                         checkpoint, if due) and returns: a run cut into job-sized pieces.  The stopping point is a function of the
                         iteration count alone, so every rank stops at the same iteration.
  --resume PATH|auto     continue from a state file; `auto`: the newest one under <work_dir>/checkpoints, from scratch when there is
                         none - one command line serves the first job and every later one.
Everything random in the loop is a function of (seed, iteration): the epoch's shuffle and each sample's augmentation draws
(datasets/loader.epoch_shard, datasets/voc.py), the dropout seed, the learning rate and the lvc_iter / seg_aff_iter switches.  A resumed
run therefore continues BIT FOR BIT: losses.txt, every model_iter_<n>.pth and the validation tables equal those of the uninterrupted
run (tests/test_gpu_train_resume.py).  What must match between the pieces is the state's `run` dictionary (train_state.run_config: seed,
number of ranks, --spg, size of the training list, crop size, schedule and loss settings, the variant's thresholds and switches); a
difference is refused before anything is written.  What only reports or paces (eval_iters, log_iters, num_workers, val_batch_size, the
visual flags) may differ.  On resume losses.txt is cut back to the state's iteration and appended to; the ETA of the log line is computed
from the iterations done in this process and its running means restart at the resume point - neither is part of the exactness claim.
The returned history / tables / ckpts / val_seconds cover this process's iterations only.
Deliberately not built: (1) stopping on a signal or on wall-clock time - ranks would decide at different iterations and the first to stop
leaves the others waiting in the gradient all-reduce, and a stop flag agreed by a collective every iteration would change the existing
step; (2) loading torch-format optimizer state written by the reference's save_train; (3) resuming onto another number of ranks or
another --spg - the data order depends on both, check_resume_compat refuses it.

  python -m excel_amd.scripts.train_voc --data_folder VOC2012 --list_folder datasets/voc --model ViT-B-16.pt --bpe_path ... \
      [--crop_size 320 --spg 4 --max_iters 30000] [--save_state_iters 2000 --iters_per_run 10000 --resume auto]
  python -m torch.distributed.run --nproc-per-node R -m excel_amd.scripts.train_voc ...       (R ranks, gradients all-reduced)
"""
import argparse
import datetime
import logging
import os
import time

import numpy as np
import torch
import torch.distributed as dist

from .. import clip as xclip
from .. import ops
from ..utils import imutils
from ..utils.affutils import refine_cams_with_aff, refine_cams_with_bkg_weclip
from ..utils.camutils import cure_attr_map


def poly_warmup_lr(base_lr, step, warmup_iter, max_iter, warmup_ratio, power):
    """PolyWarmupAdamW's schedule (utils/optimizer.py:52-64); `step` = optimizer.global_step before the update."""
    if step < warmup_iter:
        return base_lr * (1 - (1 - step / warmup_iter) * (1 - warmup_ratio))
    if step < max_iter:
        return base_lr * (1 - step / max_iter) ** power
    return base_lr * (1 - (max_iter - 1) / max_iter) ** power if max_iter > 0 else base_lr     # the reference stops updating lr past max_iter


def allreduce_mean_(flat, group=None):
    """DistributedDataParallel's gradient averaging as one collective on the flat gradient buffer."""
    if dist.is_available() and dist.is_initialized() and dist.get_world_size(group) > 1:
        dist.all_reduce(flat, op=dist.ReduceOp.SUM, group=group)
        flat.div_(dist.get_world_size(group))
    return flat


class DecoderTrainer:
    def __init__(self, model, par, lr=1e-4, wt_decay=1e-2, betas=(0.9, 0.999), warmup_iters=50, max_iters=30000, warmup_lr=1e-6, power=1, caa_thre=0.79,
                 w_diver=0.1, radius=8, ignore_index=255, lvc_iter=14000, seg_aff_iter=24000, dropout_p=0.1, seed=0,
                 bkg_thre=0.5, high_thre=0.7, low_thre=0.25):
        """Defaults = scripts/train_voc.py:36-80.  The head's parameters sit in param group 3 (model_excel.py:40-45): lr x 10.
        `seg_aff_iter` None: the affinity target stays the pseudo labels at every iteration (scripts/train_coco.py:206)."""
        if model._dec is None:
            raise RuntimeError("DecoderTrainer needs a model built with decoder_state_dict= (initial head weights)")
        self.model, self.par = model, par
        self.base_lr = lr * 10                                         # engine/optimizer_engine.py: groups 2, 3 use args.lr * 10
        self.wt_decay, self.betas = wt_decay, betas
        self.warmup_iters, self.max_iters, self.warmup_lr, self.power = warmup_iters, max_iters, warmup_lr, power
        self.w_diver, self.radius, self.ignore_index, self.lvc_iter = w_diver, radius, ignore_index, lvc_iter
        self.caa_thre = caa_thre                                       # 0.79 VOC (train_voc.py:195), 0.88 COCO (train_coco.py:193)
        self.seg_aff_iter, self.dropout_p, self.seed = seg_aff_iter, dropout_p, seed
        self.bkg_thre, self.high_thre, self.low_thre = bkg_thre, high_thre, low_thre       # lam_to_label of the pseu_mid panel (:211)
        self.global_step = 0

    def state_dict(self):
        """-> dict(global_step, model = the head's weights (model.state_dict(), CPU), optimizer = DecoderHandle.optimizer_state(), None
        before the first step): with the trainer's settings, all the next train_step depends on."""
        return dict(global_step=int(self.global_step), model={k: v.detach().cpu() for k, v in self.model.state_dict().items()},
                    optimizer=self.model._dec.optimizer_state())

    def load_state_dict(self, state):
        """state_dict()'s inverse, in place: head weights (ExCEL_model.load_decoder_state_dict), AdamW moments, global_step.  Refusals
        (ValueError naming the key) come before anything is changed."""
        dec = self.model._dec
        if state["optimizer"] is not None:        # checked first: load_weights below already copies
            dec.check_optimizer_state(state["optimizer"])
        self.model.load_decoder_state_dict(state["model"])
        if state["optimizer"] is None:
            dec._adam = None
        else:
            dec.load_optimizer_state(state["optimizer"])
        self.global_step = int(state["global_step"])

    @torch.no_grad()
    def pseudo_labels(self, inputs, cls_labels, attr_maps_raw, attn_weights, attn_pred, n_iter):
        """:188-199 -> aff_pseudos [B,H,W] uint8 (PAR guide = denormalize_img2(inputs), :181)."""
        guide = imutils.denormalize_img2(inputs)
        out = []
        for i, attr_map in enumerate(attr_maps_raw):
            seg_attn = attn_pred[i][None] if n_iter >= self.lvc_iter else None                                        # :194
            refined, cls_lst = refine_cams_with_aff(attr_map, attn_weights[:, i, ...], cls_labels[i], size=inputs.shape[2:],
                                                    seg_attn=seg_attn, caa_thre=self.caa_thre)                     # :195
            lab, _ = refine_cams_with_bkg_weclip(refined, guide[i], cls_lst, self.par, size=inputs.shape[2:])     # :196
            out.append(lab)
        return torch.cat(out, dim=0).to(torch.uint8)                                                               # :198

    def train_step(self, inputs, cls_labels, n_iter=None, want_visual=False):
        """inputs [B,3,S,S] normalised, cls_labels [B,F] -> dict(seg_loss, diver_loss, lr, aff_pseudos).  want_visual: the dict also
        carries what the progress panels show (:204, :211, :234-239): attr_maps_raw [B,P,F] (the cured one from lvc_iter on), seg_pred
        uint8 [B,S,S] and pseu_mid uint8 [B,g,g]; without it nothing extra is queued."""
        n_iter = self.global_step if n_iter is None else n_iter
        model, dec = self.model, self.model._dec
        with torch.no_grad():
            image_features, attn_weights, all_feats = xclip.generate_clip_fts(
                inputs, model.encoder, return_weights=True, n_attn_out=6 if n_iter >= self.lvc_iter else 0, want_feats=True,
                feats_as_reference=True)                                                                             # model_excel.py:56
            attr_maps_raw = ops.clip_feature_surgery(image_features, model._text_rows, num_fg=model.num_classes - 1, want_full=False)[1]
            segs, attn_pred, ctx = dec.forward_train(all_feats, dropout_p=self.dropout_p,
                                                     dropout_seed=self.seed * 1000003 + self.global_step)            # :60-76 (Dropout2d active: model.train())
            if n_iter >= self.lvc_iter:
                # fts_diver = attn_fts.clone().detach() of THIS train-mode forward (:186-189): the post-Dropout2d features
                attr_maps_raw = cure_attr_map(model, inputs, ex_feats=dec.train_attn_fts(ctx))
            aff_pseudos = self.pseudo_labels(inputs, cls_labels, attr_maps_raw, attn_weights, attn_pred, n_iter)
            aff_src = None
            if self.seg_aff_iter is not None and n_iter >= self.seg_aff_iter:                                        # :204, :210
                aff_src = ops.argmax_label(ops.bilinear_resize(segs, inputs.shape[2], inputs.shape[3], align_corners=False))
            losses, d_seg, d_ap = ops.train_losses(segs, attn_pred, aff_pseudos, radius=self.radius, ignore_index=self.ignore_index,
                                                   w_seg=1.0, w_diver=self.w_diver, aff_labels_u8=aff_src)           # :202-215
            dec.backward(ctx, d_seg, d_ap)                                                                           # :218
            allreduce_mean_(dec.grad_flat)
            lr = poly_warmup_lr(self.base_lr, self.global_step, self.warmup_iters, self.max_iters, self.warmup_lr, self.power)
            dec.adamw_step(lr, self.global_step + 1, betas=self.betas, eps=1e-8, weight_decay=self.wt_decay)         # :219
            self.global_step += 1
            visual = {}
            if want_visual:
                B, P, F_ = attr_maps_raw.shape
                g = inputs.shape[2] // 16
                seg_pred = aff_src if aff_src is not None else ops.argmax_label(
                    ops.bilinear_resize(segs, inputs.shape[2], inputs.shape[3], align_corners=False))                # :202-204
                pseu_mid = ops.lam_to_label(attr_maps_raw.permute(0, 2, 1).reshape(B, F_, g, g), cls_labels, img_box=None, ignore_mid=False,
                                            bkg_thre=self.bkg_thre, high_thre=self.high_thre, low_thre=self.low_thre,
                                            ignore_index=self.ignore_index)[1]                                      # :211
                visual = dict(attr_maps_raw=attr_maps_raw, seg_pred=seg_pred, pseu_mid=pseu_mid)
        l = losses.tolist()
        return dict(seg_loss=l[0], diver_loss=l[1], lr=lr, aff_pseudos=aff_pseudos, **visual)


KEEP_STATES_DEFAULT = 2


def get_parser():
    """scripts/train_voc.py:30-83 where the arguments apply, plus the model arguments of tools/infer_lam.py."""
    from ..tools.infer_lam import _bool
    p = argparse.ArgumentParser()
    p.add_argument("--model", default="ExCEL_ViT-B/16", type=str, help="CLIP checkpoint path or name (see tools/infer_lam.py)")
    p.add_argument("--dataset_name", default="pascal_voc", type=str)
    p.add_argument("--attr_json", default=None, type=str)
    p.add_argument("--num_attri", default=112, type=int)
    p.add_argument("--embedding_dim", default=256, type=int)
    p.add_argument("--in_channels", default=768, type=int)
    p.add_argument("--radius", default=8, type=int)
    p.add_argument("--w_seg", default=1.0, type=float)
    p.add_argument("--w_diver", default=0.1, type=float)
    p.add_argument("--max_iters", default=30000, type=int)
    p.add_argument("--log_iters", default=200, type=int)
    p.add_argument("--eval_iters", default=2000, type=int)
    p.add_argument("--warmup_iters", default=50, type=int)
    p.add_argument("--ignore_index", default=255, type=int)
    p.add_argument("--save_ckpt", default=True, type=_bool)
    p.add_argument("--seed", default=0, type=int)
    p.add_argument("--work_dir", default="w_outputs", type=str)
    p.add_argument("--data_folder", default="/data/Datasets/VOC/VOC2012/", type=str)
    p.add_argument("--list_folder", default="datasets/voc", type=str)
    p.add_argument("--num_classes", default=21, type=int)
    p.add_argument("--crop_size", default=320, type=int)
    p.add_argument("--train_set", default="train_aug", type=str)
    p.add_argument("--val_set", default="train", type=str)
    p.add_argument("--spg", default=4, type=int, help="samples per GPU")
    p.add_argument("--lr", default=1e-4, type=float)
    p.add_argument("--warmup_lr", default=1e-6, type=float)
    p.add_argument("--wt_decay", default=1e-2, type=float)
    p.add_argument("--power", default=1, type=float)
    p.add_argument("--bkg_thre", default=0.5, type=float)
    p.add_argument("--high_thre", default=0.7, type=float)
    p.add_argument("--low_thre", default=0.25, type=float)
    p.add_argument("--save_visual", default=False, type=_bool,
                   help="rank 0 writes the training-progress image grids as PNG files every --log_iters iterations")
    p.add_argument("--visual_dir", default=None, type=str, help="where --save_visual writes (default <work_dir>/visual)")
    p.add_argument("--local_rank", default=int(os.environ.get("LOCAL_RANK", 0)), type=int)
    p.add_argument("--num_workers", default=8, type=int, help="decode threads per rank")
    p.add_argument("--backend", default="nccl")
    p.add_argument("--val_batch_size", default=16, type=int, help="images per ragged batch of the validation pass")
    p.add_argument("--val_api_path", default=False, type=_bool,
                   help="validate with the reference's per-image loop (build_validation) on every rank instead of the batched pass split "
                        "across ranks (build_validation_ragged)")
    # stopping and continuing (utils/train_state.py); all off by default
    p.add_argument("--save_state_iters", default=0, type=int,
                   help="rank 0 writes <work_dir>/checkpoints/train_state_iter_<n>.pth (weights, AdamW moments, iteration) after every "
                        "N-th iteration; 0: never")
    p.add_argument("--keep_states", default=KEEP_STATES_DEFAULT, type=int, help="state files kept; older ones are deleted after each write")
    p.add_argument("--iters_per_run", default=0, type=int,
                   help="stop after N iterations of this process and write the state there (continue with --resume); 0: no limit")
    p.add_argument("--resume", default=None, type=str,
                   help="a train_state_iter_<n>.pth to continue from, or `auto`: the newest under <work_dir>/checkpoints, from scratch "
                        "when there is none")
    # model arguments of tools/infer_lam.py
    p.add_argument("--clip_root", default=None, type=str)
    p.add_argument("--bpe_path", default=None, type=str)
    p.add_argument("--gemm_mode", default=None, type=str)
    return p


def _fmt_td(seconds):
    return str(datetime.timedelta(seconds=int(seconds)))


def _val_batches(dataset, device):
    """The reference's val loader (batch 1, normalize_img + HWC->CHW): the package's VOC12SegDataset yields uint8 images, normalised
    here on the device by ops.normalize_img_u8."""
    for i in range(len(dataset)):
        name, image, label, cls = dataset[i]
        img = ops.normalize_img_u8(torch.from_numpy(np.array(image))[None].to(device))
        yield [name], img, torch.from_numpy(np.array(label))[None], torch.from_numpy(np.array(cls))[None]


def build_model(args, device):
    """ExCEL_model(mode="train") at the head's initial weights (model/init_head.py), the tower from --model like tools/infer_lam.py."""
    from ..model import ExCEL_model, init_decoder_state_dict
    from ..tools.infer_lam import resolve_model_inputs
    args.training_free = True                       # resolve_model_inputs: no trained head is loaded, training starts from init
    kw = resolve_model_inputs(args)
    n_layers = sum(1 for k in kw["state_dict"] if k.startswith("visual.transformer.resblocks.") and k.endswith(".ln_1.weight")) or 12
    dec = init_decoder_state_dict(num_classes=args.num_classes, in_channels=args.in_channels, embedding_dim=args.embedding_dim,
                                  crop_size=args.crop_size, seed=args.seed, index=n_layers)
    return ExCEL_model(clip_model=args.model, embedding_dim=args.embedding_dim, in_channels=args.in_channels, dataset_name=args.dataset_name,
                       num_classes=args.num_classes, num_atrr_clusters=args.num_attri, json_file=args.attr_json, img_size=args.crop_size,
                       mode="train", device=device, gemm_mode=args.gemm_mode, decoder_state_dict=dec, **kw)


class TrainVariant:
    """What differs between scripts/train_voc.py and scripts/train_coco.py (the COCO program: scripts/train_coco.py here)."""
    name = "voc"
    caa_thre = 0.79              # refine_cams_with_aff threshold (:195)
    lvc_iter = 14000             # cure_attr_map(ex_feats=fts_diver) + seg_attn from this iteration on (:188, :194)
    seg_aff_iter = 24000         # affinity target = seg arg-max from this iteration on (:210); None: never

    @staticmethod
    def datasets(args):
        """-> (train dataset with sample(idx, epoch), val dataset with __getitem__ -> (name, image, label, cls))."""
        from ..datasets import voc
        train = voc.VOC12ClsDataset(root_dir=args.data_folder, name_list_dir=args.list_folder, split=args.train_set, stage="train",
                                    aug=True, rescale_range=(0.5, 2.0), crop_size=args.crop_size, img_fliplr=True,
                                    ignore_index=args.ignore_index, num_classes=args.num_classes, seed=args.seed)
        val = voc.VOC12SegDataset(root_dir=args.data_folder, name_list_dir=args.list_folder, split=args.val_set, stage="val",
                                  ignore_index=args.ignore_index)
        return train, val

    @staticmethod
    def augment(images, plan, labels, args):
        """the training transform of a staged batch (DeviceFeeder with aug_crop_size) -> inputs [B,3,S,S]"""
        return ops.train_augment(images, plan, labels, None, args.crop_size, aug_plan=plan.aug)[0]

    @staticmethod
    def augment_with_gt(images, plan, labels, args):
        """augment() plus the augmented ground-truth label map uint8 [B,S,S] the seg_gt panel shows (None: the data has none)"""
        inputs, gt = ops.train_augment(images, plan, labels, None, args.crop_size, aug_plan=plan.aug)[:2]
        return inputs, gt

    @staticmethod
    def class_list(args):
        from ..datasets import voc
        return voc.class_list if args.num_classes == 21 else None

    @staticmethod
    def first_ckpt_iter(args):
        return 2                 # `(n_iter + 1) >= 2` (:253)


VOC = TrainVariant()


def train(args, model=None, variant=VOC, tb_writer=None):
    """scripts/train_voc.py:train (scripts/train_coco.py:train with variant=train_coco.COCO).  `model`: an ExCEL_model with a decoder
    head (tests inject a small one); default: built from --model with the head at its initial weights.  `tb_writer`: any object with
    add_image(tag, chw_uint8, global_step=); rank 0 hands it the reference's six grids (:240-246) every --log_iters iterations.
    -> dict(history=[per-iteration losses], tables=[validation tables], ckpts=[paths], val_seconds=[wall seconds of each validation pass],
    and with --save_visual true visuals=[directories written]), all of this process's iterations.  With any of --save_state_iters,
    --keep_states, --iters_per_run, --resume (module docstring) also states=[state files written] and resumed_from=the state continued
    from (None: `--resume auto` found none, or no --resume)."""
    from ..datasets import loader
    from ..engine.validatation_engine import build_validation, build_validation_ragged
    from ..utils import train_state
    from ..utils.PAR import PAR
    world = int(os.environ.get("WORLD_SIZE", 1))
    rank = int(os.environ.get("RANK", 0))
    torch.cuda.set_device(args.local_rank)
    device = torch.device("cuda", args.local_rank)
    if world > 1 and not dist.is_initialized():
        dist.init_process_group(backend=args.backend)
    time0 = time.time()
    ckpt_dir = os.path.join(args.work_dir, "checkpoints")
    if rank == 0:
        os.makedirs(ckpt_dir, exist_ok=True)
    logging.info("Total gpus: %d, samples per gpu: %d..." % (world, args.spg))
    train_dataset, val_dataset = variant.datasets(args)
    # stopping and continuing: which state to continue from is settled, and a state of another run refused, before anything is built or written
    save_every, keep_states = getattr(args, "save_state_iters", 0), getattr(args, "keep_states", KEEP_STATES_DEFAULT)
    per_run, resume = getattr(args, "iters_per_run", 0), getattr(args, "resume", None)
    stateful = save_every > 0 or per_run > 0 or resume is not None or keep_states != KEEP_STATES_DEFAULT
    start, state, resumed_from, run_cfg, states = 0, None, None, None, []
    if stateful:
        if save_every < 0 or per_run < 0 or keep_states < 1:
            raise ValueError("--save_state_iters and --iters_per_run must be >= 0, --keep_states >= 1")
        run_cfg = train_state.run_config(args, variant, world, len(train_dataset))
        if resume is not None:
            resumed_from = train_state.find_latest_state(ckpt_dir) if resume == "auto" else resume
        if resumed_from is not None:
            state = train_state.load_train_state(resumed_from)              # every rank reads the file
            train_state.check_resume_compat(state["run"], run_cfg)
            start = int(state["step"])
    stop_at = min(args.max_iters, start + per_run) if per_run > 0 else args.max_iters
    if model is None:
        model = build_model(args, device)
    par = PAR(num_iter=20, dilations=[1, 2, 4, 8, 12, 24])
    trainer = DecoderTrainer(model, par, lr=args.lr, wt_decay=args.wt_decay, warmup_iters=args.warmup_iters, max_iters=args.max_iters,
                             warmup_lr=args.warmup_lr, power=args.power, caa_thre=variant.caa_thre, w_diver=args.w_diver,
                             radius=args.radius, ignore_index=args.ignore_index, lvc_iter=variant.lvc_iter,
                             seg_aff_iter=variant.seg_aff_iter, seed=args.seed, bkg_thre=args.bkg_thre, high_thre=args.high_thre,
                             low_thre=args.low_thre)
    history, tables, ckpts, meter, val_seconds = [], [], [], [], []

    def result(visuals):
        res = dict(history=history, tables=tables, ckpts=ckpts, val_seconds=val_seconds)
        if args.save_visual:            # a run without the flag returns what it always did
            res["visuals"] = visuals
        if stateful:                    # likewise
            res["states"], res["resumed_from"] = states, resumed_from
        return res

    start_epoch = start_batch = 0
    if state is not None:
        trainer.load_state_dict(dict(global_step=start, model=state["model_state_dict"], optimizer=state["optimizer_state_dict"]))
        logging.info("Resuming from %s: continuing after iteration %d of %d" % (resumed_from, start, args.max_iters))
        if start >= args.max_iters:     # the run had finished
            return result([])
        start_epoch, start_batch = loader.resume_position(start, len(train_dataset), world, args.spg)
    loss_log = None
    if rank == 0:
        log_path = os.path.join(args.work_dir, "losses.txt")
        if state is not None:           # lines of iterations after the state (a process that got further) are written again
            train_state.truncate_loss_log(log_path, start)
        loss_log = open(log_path, "w" if state is None else "a")
    batches = loader.train_batches(train_dataset, args.spg, rank=rank, world=world, seed=args.seed, start_epoch=start_epoch,
                                   num_threads=args.num_workers, start_batch=start_batch)
    feeder = loader.DeviceFeeder(batches, device, aug_crop_size=args.crop_size)
    class_list = variant.class_list(args)
    first_ckpt = variant.first_ckpt_iter(args)
    visual_dir = args.visual_dir or os.path.join(args.work_dir, "visual")
    show = rank == 0 and (args.save_visual or tb_writer is not None)
    png_writer = None
    it = iter(feeder)
    try:
        for n_iter in range(start, stop_at):
            names, plan, images, cls, labels = next(it)
            visual = show and (n_iter + 1) % args.log_iters == 0
            if visual:
                inputs, seg_gt = variant.augment_with_gt(images, plan, labels, args)
                out = trainer.train_step(inputs, cls, n_iter, want_visual=True)
            else:                       # every other iteration: exactly the calls of a run without the panels
                inputs = variant.augment(images, plan, labels, args)
                out = trainer.train_step(inputs, cls, n_iter)
            rec = dict(iter=n_iter + 1, seg_loss=out["seg_loss"], diver_loss=out["diver_loss"], lr=out["lr"])
            history.append(rec)
            meter.append((out["seg_loss"], out["diver_loss"]))
            if loss_log is not None:
                loss_log.write("%d %.9g %.9g %.9g\n" % (n_iter + 1, out["seg_loss"], out["diver_loss"], out["lr"]))
                loss_log.flush()
            if (n_iter + 1) % args.log_iters == 0 and rank == 0:                                                   # :226-233
                elapsed = time.time() - time0
                eta = elapsed / (n_iter + 1 - start) * (args.max_iters - n_iter - 1)      # the pace of this process's iterations
                m = np.mean(np.asarray(meter), axis=0)
                meter = []
                logging.info("Iter: %d; Elasped: %s; ETA: %s; LR: %.3e; seg_loss: %.4f, diver_loss: %.4f"
                             % (n_iter + 1, _fmt_td(elapsed), _fmt_td(eta), out["lr"], m[0], m[1]))
                if visual:                                                                                          # :233-246
                    from ..utils import tbutils
                    panels = tbutils.render_panels(inputs, cls, out, seg_gt=seg_gt)
                    if tb_writer is not None:
                        tbutils.log_panels(tb_writer, panels, n_iter + 1)
                    if args.save_visual:
                        if png_writer is None:
                            png_writer = tbutils.PanelWriter()
                        png_writer.submit(os.path.join(visual_dir, "iter_%d" % (n_iter + 1)), panels.host())    # one device-to-host copy
            if (n_iter + 1) % args.eval_iters == 0:                                                                 # :245-253
                if rank == 0:
                    logging.info("Validating...")
                    if args.save_ckpt and (n_iter + 1) >= first_ckpt:
                        path = os.path.join(ckpt_dir, "model_iter_%d.pth" % (n_iter + 1))
                        torch.save({k: v.detach().cpu() for k, v in model.state_dict().items()}, path)
                        ckpts.append(path)
                # the reference resizes to a fixed 320 (engine/validatation_engine.py:20) = its default crop; here: the crop size
                t_val = time.time()
                if args.val_api_path:       # the reference's loop: every rank validates the whole list, one image at a time
                    table = build_validation(model=model, par=par, val_loader=_val_batches(val_dataset, device), device=device,
                                             num_classes=args.num_classes, resize_size=args.crop_size, class_list=class_list)[0]
                else:                       # ragged batches, images r, r+R, ... on rank r, the matrices all-gathered once
                    table = build_validation_ragged(model=model, par=par, dataset=val_dataset, device=device, num_classes=args.num_classes,
                                                    resize_size=args.crop_size, class_list=class_list, batch_size=args.val_batch_size,
                                                    num_workers=args.num_workers, rank=rank, world=world, group=None)[0]
                torch.cuda.synchronize(device)
                val_seconds.append(time.time() - t_val)
                tables.append(table)
                if rank == 0:
                    logging.info("\n" + table)
                    logging.info("Validation: %d images in %.2f s (%s)" % (len(val_dataset), val_seconds[-1],
                                                                           "per image" if args.val_api_path else f"{world} rank(s), batches of {args.val_batch_size}"))
            # the full state: every --save_state_iters iterations, and where --iters_per_run stops an unfinished run
            due = (save_every > 0 and (n_iter + 1) % save_every == 0) or (n_iter + 1 == stop_at and stop_at < args.max_iters)
            if stateful and due and rank == 0:
                st = trainer.state_dict()
                states.append(train_state.save_train_state(train_state.state_path(ckpt_dir, n_iter + 1), n_iter + 1, st["model"],
                                                           st["optimizer"], out["lr"], run_cfg))
                train_state.prune_states(ckpt_dir, keep_states)
                logging.info("Training state of iteration %d: %s" % (n_iter + 1, states[-1]))
    finally:
        it.close()                      # records the last batch's event, then DeviceFeeder.close waits for it and stops the stager
        feeder.close()
        if loss_log is not None:
            loss_log.close()
        visuals = png_writer.close() if png_writer is not None else []         # joins the writer thread, re-raises its first error
    return result(visuals)


if __name__ == "__main__":
    logging.basicConfig(level=logging.INFO, format="%(asctime)s %(message)s")
    train(get_parser().parse_args())
