"""Dev: what the wide-vocabulary paths cost next to the narrow kernels they leave untouched.
   python tools_dev/wide_vocab_bench.py [--out profiles/wide_vocab_bench.json]
 - the fused patch-text CAM (excel_patch_text_cam, bf16x3 and f32) at (B, N, C) = (32, 785, 512) for T = 103 (narrow: COCO) and
   T = 175 / 288 (wide), as us per call and us per class row;
 - excel_confusion_accumulate on 32 x 448 x 448 labels at nc = 81 (narrow) and nc = 151 / 255 (wide: 3 / 8 bands of ground-truth rows).
Device events around 50 back-to-back calls, 5 windows per case with the cases interleaved, the median window reported (and min / max)."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from excel_amd import ops

REPS, WINDOWS = 50, 5


def window(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(REPS):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / REPS          # us per call


def measure(cases):
    for fn in cases.values():                        # warm-up: code objects, workspaces
        for _ in range(5):
            fn()
    torch.cuda.synchronize()
    t = {k: [] for k in cases}
    for _ in range(WINDOWS):
        for k, fn in cases.items():
            t[k].append(window(fn))
    return {k: {"us": float(np.median(v)), "us_min": float(min(v)), "us_max": float(max(v))} for k, v in t.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "wide_vocab_bench.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("wide_vocab_bench needs a GPU")
    rs = np.random.RandomState(0)
    B, N, C = 32, 785, 512
    x = torch.from_numpy(rs.standard_normal((B, N, C)).astype(np.float32)).cuda()
    cam = {}
    for T, F in ((103, 80), (175, 150), (288, 254)):
        t = rs.standard_normal((T, C)).astype(np.float32)
        t = torch.from_numpy(t / np.linalg.norm(t, axis=1, keepdims=True)).cuda()
        for mode in ("bf16x3", "f32"):
            cam[f"cam_{mode}_T{T}"] = (lambda t=t, F=F, mode=mode: ops.patch_text_cam(x, t, num_fg=F, mode=mode))
    out = {"shape": {"B": B, "N": N, "C": C}, "reps": REPS, "windows": WINDOWS, "cam": measure(cam)}
    for k, v in out["cam"].items():
        v["us_per_class_row"] = v["us"] / int(k.split("T")[-1])
    n = 32 * 448 * 448
    conf = {}
    for nc in (81, 151, 255):
        gt = torch.from_numpy(rs.randint(0, nc, n).astype(np.uint8)).cuda()
        pr = torch.from_numpy(rs.randint(0, nc, n).astype(np.uint8)).cuda()
        hist = torch.zeros((nc, nc), dtype=torch.int64, device="cuda")
        conf[f"confusion_nc{nc}"] = (lambda gt=gt, pr=pr, nc=nc, hist=hist: ops.confusion_accumulate(gt, pr, nc, hist))
    out["confusion"] = measure(conf)
    for k, v in out["confusion"].items():
        nc = int(k.split("nc")[-1])
        v["bands"] = 1 if nc * nc <= 8192 else -(-nc // (8192 // nc))
        v["pixels"] = n
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
