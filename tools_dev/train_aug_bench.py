"""Training augmentation on the device against the host (Pillow + numpy) path, on one GPU box.  One JSON line per measurement.

  (a) ops.train_augment for spg 4 and 32 VOC-sized images (500 x 375 / 375 x 500 / 500 x 333 mix), ms per batch and HBM bytes
  (b) the reference's host transform (Pillow BILINEAR / NEAREST, flip, pad, crop with the retry rule, normalize_img, HWC->CHW) for the
      same batch on a pool of 16 threads
  (c) ms per training iteration (ViT-B/16 with seeded synthetic weights, spg 4): the GPU step alone, device augmentation + step, and
      host augmentation + H2D + step (serial), at crop_size 320 and 448

  python tools_dev/train_aug_bench.py [--reps 20]
"""
import argparse
import json
import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import _train_aug_ref as R  # noqa: E402  (the host restatement of the reference's transform)
from excel_amd import ops  # noqa: E402
from excel_amd.datasets.loader import pack_samples  # noqa: E402

HBM_GBS = 8000.0          # MI355X HBM3E peak, GB/s


def voc_batch(n, rng):
    sizes = [(375, 500), (500, 375), (333, 500)]
    ims, labs, hw = [], [], []
    for i in range(n):
        h, w = sizes[i % 3]
        ims.append(rng.integers(0, 256, (h, w, 3), dtype=np.uint8))
        labs.append(rng.integers(0, 21, (h, w), dtype=np.uint8))
        hw.append((h, w))
    return ims, labs, hw


def timed(fn, reps, sync=True):
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        if sync:
            torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ts)), float(np.min(ts))


def device_aug(ims, labs, params, S):
    rb = pack_samples([(str(i), im, lab, np.zeros(20, np.float32)) for i, (im, lab) in enumerate(zip(ims, labs))])
    plan = ops.RaggedPlan(rb.hw, "cuda")
    images, labels = rb.images.cuda(), rb.labels.cuda()
    aug = ops.TrainAugPlan(rb.hw, params, S, "cuda")
    return (lambda: ops.train_augment(images, plan, labels, None, S, aug_plan=aug)), aug


def host_aug(pool, ims, labs, params, S):
    outs = list(pool.map(lambda b: R.transform(ims[b], labs[b], params[b], S)["img_ref"], range(len(ims))))
    return np.stack(outs)


def aug_bytes(aug, hw, S):
    """HBM bytes of one call: source image + label read once, the horizontal pass' rows written and read back, the outputs written."""
    info = aug.info
    src = sum(4 * h * w for h, w in hw)
    mid = int(info.workspace_bytes)                # upper bound: the pass writes only the crop's columns / rows
    out = len(hw) * S * S * (12 + 1)
    return src + 2 * mid + out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--skip_step", action="store_true")
    args = ap.parse_args()
    rng = np.random.default_rng(0)
    pool = ThreadPoolExecutor(max_workers=args.threads)
    for S in (320, 448):
        for spg in (4, 32):
            ims, labs, hw = voc_batch(spg, rng)
            params = R.draw_params(rng, hw, S)
            fn, aug = device_aug(ims, labs, params, S)
            med, best = timed(fn, args.reps)
            nbytes = aug_bytes(aug, hw, S)
            hmed, hbest = timed(lambda: host_aug(pool, ims, labs, params, S), max(3, args.reps // 4), sync=False)
            print(json.dumps({"what": "augment", "crop_size": S, "spg": spg, "device_ms_median": round(med, 4), "device_ms_min": round(best, 4),
                              "hbm_bytes": nbytes, "hbm_floor_ms": round(nbytes / HBM_GBS / 1e6, 5),
                              "host_ms_median_%dthreads" % args.threads: round(hmed, 3), "host_ms_min": round(hbest, 3)}), flush=True)
    if args.skip_step:
        return
    from excel_amd.model import ExCEL_model, init_decoder_state_dict
    from excel_amd.scripts.train_voc import DecoderTrainer
    from excel_amd.tools import synthetic
    from excel_amd.utils.PAR import PAR
    sd = synthetic.make_vit_state_dict(seed=0)
    for S in (320, 448):
        model = ExCEL_model(clip_model="ExCEL_ViT-B/16", num_classes=21, img_size=S, mode="train", state_dict=sd,
                            text_features=synthetic.make_text_features(45), in_channels=768,
                            decoder_state_dict=init_decoder_state_dict(21, 768, 256, S, seed=0))
        tr = DecoderTrainer(model, PAR(num_iter=20, dilations=[1, 2, 4, 8, 12, 24]))
        ims, labs, hw = voc_batch(4, rng)
        params = R.draw_params(rng, hw, S)
        fn, _ = device_aug(ims, labs, params, S)
        cls = torch.zeros(4, 20, device="cuda")
        cls[:, [0, 14]] = 1
        x0 = fn()[0]
        step_ms = timed(lambda: tr.train_step(x0, cls), args.reps)[0]
        dev_ms = timed(lambda: tr.train_step(fn()[0], cls), args.reps)[0]
        host_ms = timed(lambda: tr.train_step(torch.from_numpy(host_aug(pool, ims, labs, params, S)).pin_memory().cuda(non_blocking=True), cls),
                        max(3, args.reps // 2))[0]
        print(json.dumps({"what": "iteration", "crop_size": S, "spg": 4, "step_only_ms": round(step_ms, 3), "device_aug_plus_step_ms": round(dev_ms, 3),
                          "host_aug_plus_step_ms_serial": round(host_ms, 3)}), flush=True)


if __name__ == "__main__":
    main()
