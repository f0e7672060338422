"""Full-state checkpoints of the decoder training programs (scripts/train_voc.py, scripts/train_coco.py --save_state_iters / --resume).

The file is <work_dir>/checkpoints/train_state_iter_<N>.pth, written after iteration N.  Its top-level keys are those of the reference's
save_train / resume_train (utils/pyutils.py:114-181):

  step                  N: iterations done, = DecoderTrainer.global_step = the optimizer's step count
  model_state_dict      the head's weights with the keys of model_iter_N.pth ("decoder_fts_fuse.*", "decoder.*"), CPU float32
  optimizer_state_dict  {"exp_avg": {name: tensor}, "exp_avg_sq": {name: tensor}} keyed by ops.DecoderHandle's parameter names
                        (DecoderHandle.optimizer_state()).  NOT torch's index-keyed optimizer format ({"state": {0: ...}, "param_groups"}):
                        the optimizer here is one kernel per parameter, there are no param groups to index, and a name-keyed table can be
                        checked key by key on load.  A file written by the reference's save_train therefore does not load here.
  lr                    the learning rate of iteration N (a record; the schedule is a function of `step`)

plus two keys of this package:

  format_version        1
  run                   everything that determines how the run continues (run_config): a resume with another value of any of them is
                        refused (check_resume_compat), because the continuation would no longer be the run that was interrupted

The file holds tensors, numbers, strings, None and dictionaries only: torch.load(path, map_location="cpu", weights_only=True) reads it.
This module is CPU torch only: no GPU, no HIP library.
"""
import os
import re

import torch

FORMAT_VERSION = 1
_NAME = re.compile(r"train_state_iter_(\d+)\.pth")

# the order check_resume_compat reports in
RUN_KEYS = ("seed", "world", "spg", "n_train", "crop_size", "max_iters", "warmup_iters", "lr", "warmup_lr", "power", "wt_decay", "w_diver",
            "radius", "num_classes", "train_set", "name", "caa_thre", "lvc_iter", "seg_aff_iter")


def run_config(args, variant, world, n_train):
    """The `run` dictionary of a state file: the flags and variant settings the data order, the schedule, the losses and the pseudo
    labels depend on.  Flags that only change what is reported or how fast (eval_iters, log_iters, num_workers, val_batch_size, the
    visual flags, work_dir ...) are not in it and may differ between the pieces of a run."""
    def num(x):
        return None if x is None else (int(x) if isinstance(x, int) else float(x))
    return dict(seed=int(args.seed), world=int(world), spg=int(args.spg), n_train=int(n_train), crop_size=int(args.crop_size),
                max_iters=int(args.max_iters), warmup_iters=int(args.warmup_iters), lr=float(args.lr), warmup_lr=float(args.warmup_lr),
                power=float(args.power), wt_decay=float(args.wt_decay), w_diver=float(args.w_diver), radius=int(args.radius),
                num_classes=int(args.num_classes), train_set=str(args.train_set), name=str(variant.name), caa_thre=float(variant.caa_thre),
                lvc_iter=num(variant.lvc_iter), seg_aff_iter=num(variant.seg_aff_iter))


def state_path(ckpt_dir, step):
    return os.path.join(ckpt_dir, "train_state_iter_%d.pth" % int(step))


def save_train_state(path, step, model_state_dict, optimizer_state_dict, lr, run):
    """Write one state file atomically: a temporary name in the same directory, flush + fsync, then os.replace.  Whatever goes wrong,
    `path` keeps what it held (or stays absent) and the temporary file is removed.  -> path"""
    obj = {"step": int(step),
           "model_state_dict": {k: v.detach().cpu() for k, v in model_state_dict.items()},
           "optimizer_state_dict": optimizer_state_dict,
           "lr": float(lr), "format_version": FORMAT_VERSION, "run": dict(run)}
    d, base = os.path.split(path)
    tmp = os.path.join(d, ".%s.tmp%d" % (base, os.getpid()))
    try:
        with open(tmp, "wb") as f:
            torch.save(obj, f)
            f.flush()
            os.fsync(f.fileno())
        os.replace(tmp, path)
    except BaseException:
        try:
            os.remove(tmp)
        except OSError:
            pass
        raise
    return path


def load_train_state(path):
    """-> the dictionary save_train_state wrote (CPU tensors).  FileNotFoundError for a missing file, ValueError for another layout."""
    if not os.path.isfile(path):
        raise FileNotFoundError(f"--resume: no training state at {path}")
    st = torch.load(path, map_location="cpu", weights_only=True)
    need = ("step", "model_state_dict", "optimizer_state_dict", "lr", "format_version", "run")
    missing = [k for k in need if not isinstance(st, dict) or k not in st]
    if missing:
        raise ValueError(f"{path} is not a training state of this package: no {missing[0]!r} (files of the reference's save_train hold "
                         "torch's optimizer format and cannot be resumed here)")
    if st["format_version"] != FORMAT_VERSION:
        raise ValueError(f"{path}: format_version {st['format_version']}, this package reads {FORMAT_VERSION}")
    return st


def _states(ckpt_dir):
    """[(iteration, path)] of the state files in ckpt_dir, oldest first; temporary files and other names are not state files."""
    try:
        names = os.listdir(ckpt_dir)
    except (FileNotFoundError, NotADirectoryError):
        return []
    found = [(int(m.group(1)), os.path.join(ckpt_dir, nm)) for nm in names for m in [_NAME.fullmatch(nm)] if m]
    return sorted(found)


def find_latest_state(ckpt_dir):
    """The state file of the highest iteration (by number: iter_10 is newer than iter_9), or None."""
    found = _states(ckpt_dir)
    return found[-1][1] if found else None


def prune_states(ckpt_dir, keep):
    """Delete all but the `keep` newest state files (model_iter_*.pth and everything else stays).  -> the paths deleted"""
    found = _states(ckpt_dir)
    gone = [p for _, p in (found[:-keep] if keep > 0 else found)]
    for p in gone:
        os.remove(p)
    return gone


def check_resume_compat(saved_run, current_run):
    """ValueError naming the first key (in RUN_KEYS order) on which the run that wrote the state and this one differ, with both values."""
    keys = list(RUN_KEYS) + sorted((set(saved_run) | set(current_run)) - set(RUN_KEYS))
    absent = object()
    for k in keys:
        a, b = saved_run.get(k, absent), current_run.get(k, absent)
        if a is absent or b is absent or type(a) is not type(b) or a != b:
            fmt = lambda v: "absent" if v is absent else repr(v)
            raise ValueError(f"cannot resume: {k} was {fmt(a)} in the run that wrote the state and is {fmt(b)} now "
                             "(the continuation would not be the interrupted run)")


def truncate_loss_log(path, step):
    """losses.txt ("<iteration> <seg_loss> <diver_loss> <lr>" per line) cut back to the iterations <= step: a process that got further
    than its last state file leaves later lines (and maybe half a line), which the resumed run writes again.  Earlier lines stay byte
    for byte; a missing file is created empty.  -> the number of lines kept"""
    try:
        with open(path, "rb") as f:
            lines = f.read().splitlines(keepends=True)
    except FileNotFoundError:
        open(path, "wb").close()
        return 0
    keep = 0
    for ln in lines:
        head = ln.split(None, 1)
        if not ln.endswith(b"\n") or not head or not head[0].isdigit() or int(head[0]) > step:
            break
        keep += 1
    if keep < len(lines):
        tmp = path + ".tmp%d" % os.getpid()
        try:
            with open(tmp, "wb") as f:
                f.writelines(lines[:keep])
                f.flush()
                os.fsync(f.fileno())
            os.replace(tmp, path)
        except BaseException:
            try:
                os.remove(tmp)
            except OSError:
                pass
            raise
    return keep
