"""Dev: what --cam_device_jpeg buys on one rank.  infer_lam --save_cam true on the synthetic VOC-sized tree of DESIGN 8b
(--synthetic 1024 --ragged true, B = 32) with the flag off (the host encoder) and on, alternating in one process, RUNS times each;
then the encoder alone on one batch of overlays of those sizes, timed with events.  Appends one JSON line per mode to
profiles/cam_jpeg_bench.jsonl (median and range over the runs):
    python tools_dev/cam_jpeg_bench.py [--mode per_class|max] [--runs 3] [--n 1024]"""
import argparse
import json
import os
import shutil
import statistics
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from excel_amd import ops
from excel_amd.tools import infer_lam, synthetic


def one_run(n, mode, device_jpeg, out_dir):
    argv = ["--synthetic", str(n), "--ragged", "true", "--batch_size", "32", "--save_cam", "true", "--cam_device_jpeg", str(device_jpeg).lower()]
    argv += ["--cs_cam_dir", out_dir] if mode == "per_class" else ["--save_cls_specific_cam", "false", "--cam_dir", out_dir]
    t0 = time.time()
    infer_lam.validate(infer_lam.get_parser().parse_args(argv))
    secs = time.time() - t0
    st = dict(infer_lam.build_validation.last_cam_stats)
    st.update(seconds=round(secs, 3), images_per_s=round(n / secs, 1), file_bytes=sum(os.path.getsize(os.path.join(out_dir, f)) for f in os.listdir(out_dir)))
    return st


def encoder_alone(mode, iters=20):
    """one batch of 32 images' overlays at the synthetic tree's sizes: ms per ops.jpeg_encode_rgb_ragged call (events, warm)"""
    ds = synthetic.SyntheticSegDataset(32, seed=1234, ragged=True)
    items, flat, at = [], [], 0
    for i in range(32):
        img = np.ascontiguousarray(ds[i][1])               # the decoded image stands in for its overlays
        k = max(1, int(np.count_nonzero(ds[i][3]))) if mode == "per_class" else 1
        for _ in range(k):
            items.append((at, img.shape[0], img.shape[1]))
            flat.append(img.reshape(-1))
            at += img.size
    rgb = torch.from_numpy(np.concatenate(flat)).cuda()
    hw = [(h, w) for _, h, w in items]
    out = torch.empty(ops.jpeg_rgb_arena_bytes(hw), dtype=torch.uint8, device="cuda")
    ws = torch.empty(ops.jpeg_rgb_workspace_bytes(hw), dtype=torch.uint8, device="cuda")
    for _ in range(3):
        ops.jpeg_encode_rgb_ragged(rgb, items, 75, out=out, ws=ws)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        ops.jpeg_encode_rgb_ragged(rgb, items, 75, out=out, ws=ws)
    e1.record()
    torch.cuda.synchronize()
    return dict(overlays=len(items), raw_bytes=at, workspace_bytes=int(ws.numel()), ms_per_batch=round(e0.elapsed_time(e1) / iters, 4),
                content="the synthetic images themselves")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", default="per_class", choices=["per_class", "max"])
    ap.add_argument("--runs", default=3, type=int)
    ap.add_argument("--n", default=1024, type=int)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "cam_jpeg_bench.jsonl"))
    a = ap.parse_args()
    runs = {False: [], True: []}
    tmp = tempfile.mkdtemp(prefix="cam_jpeg_bench_")
    try:
        for r in range(a.runs):
            for flag in (False, True):                     # back to back, alternating
                d = os.path.join(tmp, f"{int(flag)}_{r}")
                runs[flag].append(one_run(a.n, a.mode, flag, d))
                print(json.dumps(dict(flag=flag, run=r, **runs[flag][-1])), flush=True)
                shutil.rmtree(d)
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    rec = dict(tool="tools_dev/cam_jpeg_bench.py", mode=a.mode, images=a.n, runs=a.runs, device=torch.cuda.get_device_name(0))
    for flag, key in ((False, "host_encoder"), (True, "device_encoder")):
        ips = [x["images_per_s"] for x in runs[flag]]
        last = runs[flag][-1]
        rec[key] = dict(images_per_s_median=statistics.median(ips), images_per_s_range=[min(ips), max(ips)], files=last["files"],
                        file_bytes=last["file_bytes"], bytes_to_host_per_batch=round(last["bytes_to_host"] / max(1, last["batches"])),
                        host_fallbacks=last["host_fallbacks"])
    rec["encoder_alone"] = encoder_alone(a.mode)
    with open(a.out, "a") as f:
        f.write(json.dumps(rec) + "\n")
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
