"""Cost of the superpixel snap (EXPERIMENTS.md, "Superpixel snap"):  python tools_dev/snap_bench.py ROOT OUT.json
ROOT = the tree to import excel_amd from.  One process, the model built once (seeded random ViT-B/16, bf16x3):
  * resident ragged steps at B = 32 (the synthetic ragged set's VOC-like sizes): a plain pipeline, snap=dict(step=16), and
    clean=dict(min_region=64) + fill=dict(radius=None) as the yardstick, alternating - 8 steps per timing, 7 rounds, a host clock
    around a synchronise;
  * the two entries alone (with the Python wrappers) on the last step's images and main labels at steps 8, 16 and 32, compactness 10,
    5 iterations - 50 calls between two device events, 5 rounds;
  * the four kernels of those calls apart, from the profiler's kernel records."""
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
from excel_amd.utils import superpixels as sx

assert os.path.dirname(os.path.abspath(excel_amd.__file__)) == os.path.join(root, "excel_amd"), excel_amd.__file__
logging.basicConfig(level=logging.WARNING, format="%(message)s")
dev = torch.device("cuda", 0)
B, NC = 32, 21
res = {"root": root, "build_id": ops.lib().excel_build_id().decode()}

infer_lam.validate(infer_lam.get_parser().parse_args(["--synthetic", str(B), "--ragged", "true", "--batch_size", str(B), "--gemm_check", "false",
                                                      "--num_workers", "12"]))          # builds the model, warms the step's shapes
model = infer_lam.validate.last_model
ds = synthetic.SyntheticSegDataset(128, (448, 448), num_classes=NC, seed=1234, u8_images=False, ragged=True)
resident = []
for s0 in range(0, 128, B):
    rb = pack_samples([ds[i] for i in range(s0, s0 + B)])
    resident.append((rb.images.to(dev), ops.RaggedPlan(rb.hw, dev), rb.cls.to(dev), rb.labels.to(dev)))
hwc, plan = resident[-1][0], resident[-1][1]
sizes = [(int(h), int(w)) for h, w in plan.hw]
res["pixels_last_step"] = plan.total_label_pix

# ---- resident steps
arms = {"plain": TrainingFreePipeline(model, num_classes=NC, smax=ds.max_k()),
        "snap16": TrainingFreePipeline(model, num_classes=NC, smax=ds.max_k(), snap=dict(step=16)),
        "clean_fill": TrainingFreePipeline(model, num_classes=NC, smax=ds.max_k(), clean=dict(min_region=64), fill=dict(radius=None))}
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
assert torch.equal(arms["plain"].hist, arms["snap16"].hist), "the snap changed the main labels"
res["last_step_superpixels_snapped_changed"] = arms["snap16"].last_snap_counts.sum(0).tolist()

# ---- the entries alone
labels = arms["plain"].run_batch_ragged(*resident[-1]).clone()
n = plan.total_label_pix
micro, kernels = {}, {}
from torch.profiler import ProfilerActivity, profile
for step in (8, 16, 32):
    cent = sx.centre_table(sizes, step, dev)
    out = (torch.empty(n, dtype=torch.int32, device=dev), torch.empty(5 * cent[1], dtype=torch.int32, device=dev))
    out2 = (torch.empty(n, dtype=torch.uint8, device=dev), torch.empty(3 * B, dtype=torch.int32, device=dev))
    slic = lambda: sx.slic_superpixels(hwc, step, 10, 5, plan=plan, cent=cent, out=out)
    snap = lambda: sx.snap_labels(labels, out[0], step, NC, 0.0, plan=plan, cent=cent, out=out2)
    row = {"centres": cent[1]}
    for name, fn in (("slic", slic), ("snap", snap)):
        for _ in range(5):
            fn()
        torch.cuda.synchronize()
        us = []
        for _ in range(5):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(50):
                fn()
            e1.record()
            e1.synchronize()
            us.append(round(e0.elapsed_time(e1) * 1e3 / 50, 2))
        row[name] = {"us_per_call_rounds": us, "median_us": float(np.median(us))}
    row["superpixels_snapped_changed"] = out2[1].view(B, 3).sum(0).tolist()
    micro[str(step)] = row
    try:
        with profile(activities=[ProfilerActivity.CUDA, ProfilerActivity.CPU]) as prof:
            for _ in range(10):
                slic()
                snap()
            torch.cuda.synchronize()
        per = {}
        for ev in prof.key_averages():
            m = re.search(r"(slic_init|slic_assign|slic_update|snap_vote)_kernel", ev.key)
            t_us = getattr(ev, "device_time_total", None)
            if t_us is None:
                t_us = getattr(ev, "cuda_time_total", 0.0)
            if m and ev.count:
                per[m.group(1)] = {"us_per_launch": round(float(t_us) / ev.count, 2), "launches_per_call": ev.count / 10}
        kernels[str(step)] = per
    except Exception as e:                                    # the profiler is an observer: without it the split is "not measured"
        kernels[str(step)] = {"not_measured": repr(e)}
res["entries_alone"] = micro
res["kernel_us"] = kernels

os.makedirs(os.path.dirname(out_path), exist_ok=True)
with open(out_path, "w") as f:
    json.dump(res, f, indent=1)
print(json.dumps(res))
