"""COCO training costs on one GPU box.  One JSON line per measurement.

  (a) ops.train_augment_image against ops.train_augment on the same COCO-sized batches (640 x 480 / 480 x 640 / 427 x 640 mix), spg 4
      and 32, crop 320: ms per batch (both are launch-bound: 3 launches against a memset + 4 launches)
  (b) host decode per sample on a pool of 16 threads: CocoClsDataset.sample (JPEG only) against the reference's read of the JPEG and
      the label PNG (CocoDataset.__getitem__), on a temporary tree of COCO-sized files
  (c) ms per training iteration at COCO's shape: ViT-B/16 with seeded synthetic weights, T = 103 text rows, 81 classes, spg 4, crop 320,
      images with 1, 6 and 18 present classes, before (n_iter 0) and after (n_iter 30000) the LVC switch; device augmentation included

  python tools_dev/train_coco_bench.py [--reps 20]
"""
import argparse
import json
import os
import sys
import tempfile
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import _coco_aug_ref as R  # noqa: E402
from excel_amd import ops  # noqa: E402
from excel_amd.datasets.loader import pack_samples  # noqa: E402

SIZES = [(480, 640), (640, 480), (427, 640)]


def coco_batch(n, rng):
    hw = [SIZES[i % 3] for i in range(n)]
    ims = [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for h, w in hw]
    labs = [rng.integers(0, 81, (h, w), dtype=np.uint8) for h, w in hw]
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


def staged(ims, labs, params, S):
    rb = pack_samples([(str(i), im, lab, np.zeros(80, np.float32)) for i, (im, lab) in enumerate(zip(ims, labs))])
    plan = ops.RaggedPlan(rb.hw, "cuda")
    images, labels = rb.images.cuda(), rb.labels.cuda()
    aug = ops.TrainAugPlan(rb.hw, params, S, "cuda")
    return (lambda: ops.train_augment_image(images, plan, None, S, aug_plan=aug),
            lambda: ops.train_augment(images, plan, labels, None, S, aug_plan=aug))


def bench_augment(args, rng):
    S = 320
    for spg in (4, 32):
        ims, labs, hw = coco_batch(spg, rng)
        params = R.params(rng, hw, S, distinct=True)
        img_only, labelled = staged(ims, labs, params, S)
        a = timed(img_only, args.reps)
        b = timed(labelled, args.reps)
        print(json.dumps({"what": "augment", "crop_size": S, "spg": spg, "image_only_ms_median": round(a[0], 4), "image_only_ms_min": round(a[1], 4),
                          "labelled_ms_median": round(b[0], 4), "labelled_ms_min": round(b[1], 4)}), flush=True)


def bench_decode(args, rng):
    from PIL import Image
    from excel_amd.datasets import coco
    n = 64
    with tempfile.TemporaryDirectory() as d:
        for sub in ("JPEGImages/train", "SegmentationClass/train"):
            os.makedirs(os.path.join(d, sub))
        names, onehot = [], {}
        for i in range(n):
            h, w = SIZES[i % 3]
            name = f"COCO_train2014_{i:012d}"
            yy, xx = np.mgrid[0:h, 0:w]
            base = 127 + 100 * np.sin(xx / (5.0 + i % 7)) * np.cos(yy / 6.0)
            im = np.clip(base[..., None] + rng.integers(-20, 20, (h, w, 3)), 0, 255).astype(np.uint8)
            Image.fromarray(im).save(os.path.join(d, "JPEGImages/train", name + ".jpg"), quality=90)
            lab = ((xx // 40 + yy // 40) % 5).astype(np.uint8)
            Image.fromarray(lab, mode="L").save(os.path.join(d, "SegmentationClass/train", name[15:] + ".png"))
            names.append(name)
            onehot[name] = np.zeros(80, np.float32)
        with open(os.path.join(d, "train.txt"), "w") as f:
            f.write("\n".join(names) + "\n")
        np.save(os.path.join(d, "cls_labels_onehot.npy"), onehot)
        cls_ds = coco.CocoClsDataset(d, d, "train", crop_size=320)
        ref_ds = coco.CocoDataset(d, d, "train", "train")
        with ThreadPoolExecutor(max_workers=args.threads) as pool:
            def run(fn):
                t0 = time.perf_counter()
                list(pool.map(fn, range(n)))
                return (time.perf_counter() - t0) * 1e3 / n
            res = {}
            for key, fn in (("image_only", cls_ds.sample), ("image_and_label_png", ref_ds.__getitem__)):
                run(fn)
                res[key] = float(np.median([run(fn) for _ in range(5)]))
        print(json.dumps({"what": "host_decode", "threads": args.threads, "samples": n, "ms_per_sample_image_only": round(res["image_only"], 4),
                          "ms_per_sample_with_label_png": round(res["image_and_label_png"], 4)}), flush=True)


def bench_iteration(args, rng):
    from excel_amd.model import ExCEL_model, init_decoder_state_dict
    from excel_amd.scripts.train_coco import COCO
    from excel_amd.scripts.train_voc import DecoderTrainer
    from excel_amd.tools import synthetic
    from excel_amd.utils.PAR import PAR
    S, spg = 320, 4
    model = ExCEL_model(clip_model="ExCEL_ViT-B/16", num_classes=81, img_size=S, mode="train", state_dict=synthetic.make_vit_state_dict(seed=0),
                        dataset_name="ms_coco", num_atrr_clusters=224, text_features=synthetic.make_text_features(103), in_channels=768,
                        decoder_state_dict=init_decoder_state_dict(81, 768, 256, S, seed=0))
    tr = DecoderTrainer(model, PAR(num_iter=20, dilations=[1, 2, 4, 8, 12, 24]), warmup_iters=200, max_iters=100000, caa_thre=COCO.caa_thre,
                        lvc_iter=COCO.lvc_iter, seg_aff_iter=COCO.seg_aff_iter)
    ims, labs, hw = coco_batch(spg, rng)
    params = R.params(rng, hw, S)
    img_only, _ = staged(ims, labs, params, S)
    for k in (1, 6, 18):
        cls = torch.zeros(spg, 80, device="cuda")
        for b in range(spg):
            cls[b, torch.from_numpy(rng.choice(80, k, replace=False))] = 1
        for n_iter in (0, 30000):
            ms = timed(lambda: tr.train_step(img_only()[0], cls, n_iter), args.reps)
            print(json.dumps({"what": "iteration", "crop_size": S, "spg": spg, "num_classes": 81, "text_rows": 103, "present_classes": k,
                              "n_iter": n_iter, "ms_median": round(ms[0], 3), "ms_min": round(ms[1], 3)}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--skip_step", action="store_true")
    args = ap.parse_args()
    rng = np.random.default_rng(0)
    bench_augment(args, rng)
    bench_decode(args, rng)
    if not args.skip_step:
        bench_iteration(args, rng)


if __name__ == "__main__":
    main()
