"""Wall time of the segmentation programs' DenseCRF stage on a synthetic tree of realistic image sizes.

    python tools_dev/crf_stage_time.py --variant voc  --images 64 --batch_size 16 --crf_batched true
    python tools_dev/crf_stage_time.py --variant coco --images 64 --batch_size 16 --crf_batched false
    python tools_dev/crf_stage_time.py --variant voc --pkg_root <checkout of another commit> --crf_batched absent

Writes VOC-like (about 500 x 375, 21 classes) or COCO-like (about 640 x 480, 81 classes) JPEGs and label PNGs into --work, builds the
tiny ViT + decoder head the tests use (the network is deliberately small: the run time is the CRF stage, the PNG writes and the decode),
runs `validate` with --crf_post true once to warm up (2 batches) and once timed, and prints one JSON line.  --pkg_root puts another
checkout (built) first on sys.path so that the same driver times a parent commit; `--crf_batched absent` leaves the flag out for
commits that do not have it.  --no_crf times the same run without the CRF stage (the floor)."""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np


def make_tree(work, variant, n, seed=0):
    from PIL import Image
    coco = variant == "coco"
    rng = np.random.default_rng(seed)
    root = os.path.join(work, "COCO" if coco else "VOC")
    img_dir = os.path.join(root, "JPEGImages", "val" if coco else "")
    lab_dir = os.path.join(root, "SegmentationClass" if coco else "SegmentationClassAug", "val" if coco else "")
    lists = os.path.join(work, "lists_" + variant)
    for d in (img_dir, lab_dir, lists):
        os.makedirs(d, exist_ok=True)
    nc = 81 if coco else 21
    base_h, base_w = (480, 640) if coco else (375, 500)
    names, onehot = [], {}
    for i in range(n):
        name = f"COCO_val2014_{i:012d}" if coco else f"2007_{i:06d}"
        h, w = (base_h, base_w) if i % 3 else (base_w, base_h - int(rng.integers(0, 40)))     # portrait every third image, ragged widths
        oh = np.zeros(nc - 1, np.float32)
        oh[i % (nc - 1)] = 1
        onehot[name] = oh
        names.append(name)
        if os.path.exists(os.path.join(img_dir, name + ".jpg")) and os.path.exists(os.path.join(lab_dir, (name[13:] if coco else name) + ".png")):
            continue                                                   # a tree from an earlier run of this driver: same seed, same files
        yy, xx = np.mgrid[0:h, 0:w]
        im = 127 + 90 * np.sin(xx / (17.0 + i % 7)) * np.cos(yy / 23.0)
        im = np.clip(im[..., None] + rng.integers(-25, 25, (h, w, 3)), 0, 255).astype(np.uint8)
        Image.fromarray(im).save(os.path.join(img_dir, name + ".jpg"), quality=90)
        lab = ((xx // 40 + yy // 40 + i) % nc).astype(np.uint8)
        Image.fromarray(lab, mode="L").save(os.path.join(lab_dir, (name[13:] if coco else name) + ".png"))
    with open(os.path.join(lists, "val.txt"), "w") as f:
        f.write("\n".join(names) + "\n")
    np.save(os.path.join(lists, "cls_labels_onehot.npy"), onehot)
    return root, lists, nc


def tiny_model(nc):
    from oracle.vit import VitConfig, make_vit_weights
    from excel_amd.model import ExCEL_model, init_decoder_state_dict
    cfg = VitConfig(width=128, layers=8, heads=2, patch=16, out_dim=64, input_resolution=64, n_surgery=5)
    kw = dict(width=128, layers=8, heads=2, patch=16, output_dim=64, input_resolution=64)
    rs = np.random.RandomState(3)
    text = rs.standard_normal((2 * nc - 1, 64)).astype(np.float32)
    text /= np.linalg.norm(text, axis=1, keepdims=True)
    dec = init_decoder_state_dict(num_classes=nc, in_channels=128, embedding_dim=32, crop_size=96, seed=0, index=8)
    return ExCEL_model(clip_model="tiny", num_classes=nc, img_size=64, mode="val", state_dict=make_vit_weights(cfg, seed=11), vit_cfg=kw,
                       text_attr=text.T.copy(), gemm_mode="f32", embedding_dim=32, in_channels=128, decoder_state_dict=dec)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--variant", choices=["voc", "coco"], default="voc")
    ap.add_argument("--images", type=int, default=64)
    ap.add_argument("--batch_size", type=int, default=16)
    ap.add_argument("--crf_batched", choices=["true", "false", "absent"], default="true")
    ap.add_argument("--crf_ws_gb", default=None)
    ap.add_argument("--no_crf", action="store_true")
    ap.add_argument("--pkg_root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    ap.add_argument("--work", default=os.path.join(tempfile.gettempdir(), "crf_stage_time"))
    ap.add_argument("--tag", default="")
    a = ap.parse_args()
    sys.path.insert(0, os.path.abspath(a.pkg_root))
    import torch
    from excel_amd.tools import infer_seg_coco, infer_seg_voc
    mod = infer_seg_coco if a.variant == "coco" else infer_seg_voc
    work = os.path.join(a.work, a.variant)
    root, lists, nc = make_tree(work, a.variant, a.images)
    model = tiny_model(nc)

    def run(list_dir, tag):
        argv = ["--data_folder", root, "--list_folder", list_dir, "--model_path", os.path.join(work, tag, "checkpoints", "model_iter_1.pth"),
                "--num_classes", str(nc), "--resize_size", "64", "--scales", "1.0,0.75,1.5", "--gemm_check", "false",
                "--batch_size", str(a.batch_size), "--crf_post", "false" if a.no_crf else "true"]
        if a.crf_batched != "absent":
            argv += ["--crf_batched", a.crf_batched]
        if a.crf_ws_gb is not None:
            argv += ["--crf_ws_gb", a.crf_ws_gb]
        t0 = time.time()
        res = mod.validate(mod.get_parser().parse_args(argv), model=model)
        torch.cuda.synchronize()
        return time.time() - t0, res

    warm = os.path.join(work, "lists_warm")
    os.makedirs(warm, exist_ok=True)
    names = open(os.path.join(lists, "val.txt")).read().split()
    with open(os.path.join(warm, "val.txt"), "w") as f:
        f.write("\n".join(names[:2 * a.batch_size]) + "\n")
    np.save(os.path.join(warm, "cls_labels_onehot.npy"), np.load(os.path.join(lists, "cls_labels_onehot.npy"), allow_pickle=True).item())
    run(warm, "warm")
    secs, res = run(lists, "timed")
    hist = res["hist_crf"] if res["hist_crf"] is not None else res["hist"]
    print(json.dumps({"tag": a.tag, "variant": a.variant, "images": res["images"], "batch_size": a.batch_size, "crf_batched": a.crf_batched,
                      "crf": not a.no_crf, "seconds": round(secs, 3), "images_per_s": round(res["images"] / secs, 2),
                      "hist_trace": int(hist.diagonal().sum()), "pkg_root": os.path.abspath(a.pkg_root)}))


if __name__ == "__main__":
    main()
