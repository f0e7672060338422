"""Dev: what the flip / multi-scale LAM fuse costs on one rank.
1. ops.lam_tta_fuse at B = 32, F = 20, g_out = 28, grids (28, 14, 21, 42) with flip, next to the chain of existing ops it equals
   (lam_scale_accumulate per scale, plane_minmax_normalize_, the permute to [B,P,F]): HIP events around every call, median of 20.
2. infer_lam --ragged true --synthetic N (B = 32, 448) with the fuse off, with --cam_flip true, and with the four scales + flip,
   alternating in one process after one warm-up run, RUNS times each; images over the wall time of the whole validate() call.
Appends one JSON line to profiles/lam_tta_bench.jsonl:
    python tools_dev/lam_tta_bench.py [--runs 3] [--n 2048]"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from excel_amd import ops
from excel_amd.tools import infer_lam

CONFIGS = {"off": [], "flip": ["--cam_flip", "true"], "scales4_flip": ["--cam_scales", "1.0,0.5,0.75,1.5", "--cam_flip", "true"]}


def _event_ms(fn, repeats=20, warm=3):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        out.append(e0.elapsed_time(e1))
    return dict(median_ms=round(statistics.median(out), 4), min_ms=round(min(out), 4), max_ms=round(max(out), 4), repeats=repeats)


def fuse_alone(B=32, F=20, g_out=28, grids=(28, 14, 21, 42)):
    gen = torch.Generator(device="cuda").manual_seed(1)
    maps = [4 * torch.rand((2 * B, g * g, F), device="cuda", generator=gen) for g in grids]
    out = torch.empty((B, g_out * g_out, F), device="cuda")

    def chain():
        acc = None
        for s, (m, g) in enumerate(zip(maps, grids)):
            acc = ops.lam_scale_accumulate(m, acc, g, g_out, g_out, init=(s == 0))
        return ops.plane_minmax_normalize_(acc).reshape(B, F, g_out * g_out).permute(0, 2, 1).contiguous()

    same = bool(torch.equal(ops.lam_tta_fuse(maps, grids, g_out, True), chain()))
    return dict(B=B, F=F, g_out=g_out, grids=list(grids), flip=True, same_bits_as_chain=same,
                lam_tta_fuse=_event_ms(lambda: ops.lam_tta_fuse(maps, grids, g_out, True, out=out)), chain_of_existing_ops=_event_ms(chain))


def one_run(n, flags):
    argv = ["--synthetic", str(n), "--ragged", "true", "--batch_size", "32"] + flags
    t0 = time.time()
    score, _ = infer_lam.validate(infer_lam.get_parser().parse_args(argv))
    secs = time.time() - t0
    return dict(seconds=round(secs, 3), images_per_s=round(n / secs, 1), miou=round(float(score["miou"]), 6))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", default=3, type=int)
    ap.add_argument("--n", default=2048, type=int)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "lam_tta_bench.jsonl"))
    a = ap.parse_args()
    rec = dict(tool="tools_dev/lam_tta_bench.py", images=a.n, runs=a.runs, device=torch.cuda.get_device_name(0), fuse_alone=fuse_alone())
    print(json.dumps(rec["fuse_alone"]), flush=True)
    print(json.dumps(dict(warm_up=one_run(a.n, []))), flush=True)
    runs = {k: [] for k in CONFIGS}
    for r in range(a.runs):
        for name, flags in CONFIGS.items():                  # back to back, alternating
            runs[name].append(one_run(a.n, flags))
            print(json.dumps(dict(config=name, run=r, **runs[name][-1])), flush=True)
    for name in CONFIGS:
        ips = [x["images_per_s"] for x in runs[name]]
        rec[name] = dict(images_per_s=ips, images_per_s_median=statistics.median(ips), seconds=[x["seconds"] for x in runs[name]],
                         miou=runs[name][-1]["miou"])
    with open(a.out, "a") as f:
        f.write(json.dumps(rec) + "\n")
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
