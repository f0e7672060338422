"""Cost of the connected-component cleaning (EXPERIMENTS.md, "Connected components"):  python tools_dev/components_bench.py ROOT OUT.json
ROOT = the tree to import excel_amd from.  One process, the model built once (seeded random ViT-B/16, bf16x3):
  * label_components + filter_small_regions on one ragged step of 32 VOC-sized maps (the sizes of the synthetic ragged set), at
    connectivity 4 and 8, on a constant map, a random 21-class map and a blob map - 100 calls between two device events, 5 alternating
    rounds (a call = the clearing fills + the five kernels + the Python wrappers) - beside the same step's arg-max plus confusion launches;
  * the kernels of one label_components call on the constant map (the union phase's worst case: every seam joins the same two trees),
    from the profiler's kernel records, per connectivity;
  * resident ragged steps at B = 32: plain, and with clean=dict(min_region=64), alternating;
  * infer_lam --synthetic 256 --ragged true with --clean_min_region off and on, alternating."""
import json
import logging
import os
import re
import sys
import time

root, out_path = os.path.abspath(sys.argv[1]), os.path.abspath(sys.argv[2])
sys.path.insert(0, root)
os.chdir(root)
import numpy as np
import torch

import excel_amd
from excel_amd import ops
from excel_amd.datasets.loader import pack_samples
from excel_amd.pipeline import TrainingFreePipeline
from excel_amd.tools import infer_lam, synthetic
from excel_amd.utils import components as cc

assert os.path.dirname(os.path.abspath(excel_amd.__file__)) == os.path.join(root, "excel_amd"), excel_amd.__file__
logging.basicConfig(level=logging.INFO, format="%(message)s")
rates = []


class Grab(logging.Handler):
    def emit(self, rec):
        m = re.search(r"\(([0-9.]+) img/s/rank\)", rec.getMessage())
        if m:
            rates.append(float(m.group(1)))


logging.getLogger().addHandler(Grab())
dev = torch.device("cuda", 0)
B, NIMG, NC = 32, 256, 21
base = ["--synthetic", str(NIMG), "--ragged", "true", "--batch_size", str(B), "--gemm_check", "false", "--num_workers", "12"]
parse = infer_lam.get_parser().parse_args
res = {"root": root, "build_id": ops.lib().excel_build_id().decode()}

infer_lam.validate(parse(base))                  # the program once: builds the model, warms every shape of the loop
model = infer_lam.validate.last_model
rates.clear()

ds = synthetic.SyntheticSegDataset(128, (448, 448), num_classes=NC, seed=1234, u8_images=False, ragged=True)
resident = []
for s0 in range(0, 128, B):
    rb = pack_samples([ds[i] for i in range(s0, s0 + B)])
    resident.append((rb.images.to(dev), ops.RaggedPlan(rb.hw, dev), rb.cls.to(dev), rb.labels.to(dev)))
plan = resident[0][1]
sizes = [(int(h), int(w)) for h, w in plan.hw]
res["sizes_first_last"] = [sizes[0], sizes[-1]]
res["pixels"] = plan.total_label_pix


# ---- the two ops beside the step's arg-max + confusion
def blob_map(h, w, rs):
    y, x = np.mgrid[:h, :w]
    m = np.zeros((h, w), np.uint8)
    for k in range(8):
        cy, cx, r = rs.randint(0, h), rs.randint(0, w), rs.randint(10, 90)
        m[(y - cy) ** 2 + (x - cx) ** 2 <= r * r] = 1 + k % 5
    sp = rs.rand(h, w) < 0.02
    m[sp] = rs.randint(0, NC, int(sp.sum())).astype(np.uint8)
    return m


rs = np.random.RandomState(0)
maps = {"constant": [np.zeros(s, np.uint8) for s in sizes], "random21": [rs.randint(0, NC, s).astype(np.uint8) for s in sizes],
        "blobs": [blob_map(h, w, rs) for h, w in sizes]}
C = 4
planes = torch.rand(C * plan.total_pix, device=dev)
nchan = torch.full((B,), C, dtype=torch.int32, device=dev)
gt = torch.from_numpy(np.concatenate([m.reshape(-1) for m in maps["blobs"]])).to(dev)
n = plan.total_label_pix
comp, area = torch.empty(n, dtype=torch.int32, device=dev), torch.empty(n, dtype=torch.int32, device=dev)
out = (torch.empty(n, dtype=torch.uint8, device=dev), torch.empty(3 * B, dtype=torch.int32, device=dev))
hist = torch.zeros((NC, NC), dtype=torch.int64, device=dev)


def timed(fns, calls=100, rounds=5):
    for f in fns.values():
        for _ in range(10):
            f()
    torch.cuda.synchronize()
    t = {k: [] for k in fns}
    for _ in range(rounds):
        for k, f in fns.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(calls):
                f()
            e1.record()
            e1.synchronize()
            t[k].append(round(e0.elapsed_time(e1) * 1e3 / calls, 2))
    return {k: {"us_per_call_rounds": v, "median_us": float(np.median(v))} for k, v in t.items()}


def argmax_confusion():
    lab = ops.argmax_label_ragged(planes, plan, C, nchan, None)
    ops.confusion_accumulate(gt, lab, NC, hist)


micro = {}
for name, ms in maps.items():
    lab = torch.from_numpy(np.concatenate([m.reshape(-1) for m in ms])).to(dev)
    fns = {"argmax_confusion": argmax_confusion}
    for conn in (4, 8):
        fns[f"label_{conn}"] = lambda conn=conn: cc.label_components(lab, plan=plan, connectivity=conn, out=(comp, area))
        fns[f"label_filter_{conn}"] = lambda conn=conn: cc.filter_small_regions(
            lab, *cc.label_components(lab, plan=plan, connectivity=conn, out=(comp, area)), 64, NC, plan=plan, out=out)
    micro[name] = timed(fns)
    torch.cuda.synchronize()
    micro[name]["regions_removed_pixels"] = out[1].view(B, 3).sum(0).tolist()
res["micro"] = micro

# ---- the kernels of one labelling of the constant map
kernels = {}
try:
    from torch.profiler import ProfilerActivity, profile
    lab = torch.from_numpy(np.concatenate([m.reshape(-1) for m in maps["constant"]])).to(dev)
    for conn in (4, 8):
        for _ in range(3):
            cc.label_components(lab, plan=plan, connectivity=conn, out=(comp, area))
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CUDA, ProfilerActivity.CPU]) as prof:
            for _ in range(20):
                cc.label_components(lab, plan=plan, connectivity=conn, out=(comp, area))
            torch.cuda.synchronize()
        per = {}
        for ev in prof.key_averages():
            m = re.search(r"cc_(tile|merge|flatten|broadcast)_kernel", ev.key)
            t_us = getattr(ev, "device_time_total", None)
            if t_us is None:
                t_us = getattr(ev, "cuda_time_total", 0.0)
            if m and ev.count:
                per[m.group(1)] = round(float(t_us) / ev.count, 2)
        kernels[str(conn)] = per
except Exception as e:                                        # the profiler is an observer: without it the phase split is "not measured"
    kernels = {"not_measured": repr(e)}
res["constant_map_kernel_us"] = kernels

# ---- resident steps
arms = {"off": TrainingFreePipeline(model, num_classes=NC, smax=ds.max_k()),
        "clean": TrainingFreePipeline(model, num_classes=NC, smax=ds.max_k(), clean=dict(min_region=64))}
for pipe in arms.values():
    for r in resident[:2]:
        pipe.run_batch_ragged(*r)
torch.cuda.synchronize()
resident_ms = {k: [] for k in arms}
for rep in range(7):
    for name, pipe in arms.items():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(2):
            for r in resident:
                pipe.run_batch_ragged(*r)
        torch.cuda.synchronize()
        resident_ms[name].append(round((time.perf_counter() - t0) * 1e3 / (2 * len(resident)), 3))
res["resident_ms_per_step"] = resident_ms
res["resident_median_ms"] = {k: float(np.median(v)) for k, v in resident_ms.items()}
assert torch.equal(arms["clean"].hist, arms["off"].hist), "the option changed the matrix"
res["resident_last_step_regions_removed_pixels"] = arms["clean"].last_clean_counts.sum(0).tolist()

# ---- the program's own loop
loop = {"off": [], "on": []}
for name in ("off", "on", "off", "on"):
    rates.clear()
    infer_lam.validate(parse(base + (["--clean_min_region", "64"] if name == "on" else [])), pipe=arms["clean" if name == "on" else "off"])
    loop[name].append({"img_per_s": rates[-1], "ms_per_step": round(B / rates[-1] * 1e3, 2)})
res["infer_lam_loop"] = loop

os.makedirs(os.path.dirname(out_path), exist_ok=True)
with open(out_path, "w") as f:
    json.dump(res, f, indent=1)
print(json.dumps(res))
