"""Cost of the nearest-label fill (EXPERIMENTS.md, "Nearest-label fill"):  python tools_dev/fill_bench.py ROOT OUT.json
ROOT = the tree to import excel_amd from: this one, or a checkout of the parent commit (which has no fill: it then times the `clean`
arm alone, the comparison point).  One process, the model built once (seeded random ViT-B/16, bf16x3):
  * resident ragged steps at B = 32 (the synthetic ragged set's VOC-like sizes): clean=dict(min_region=64) and, where the tree has it,
    the same with fill=dict(radius=None), alternating - 8 steps per timing, 7 rounds, a host clock around a synchronise;
  * the fill's two launches alone (with the clearing and the Python wrapper) on the last step's cleaned labels, on a cleaned blob map,
    on a map with 30 % holes, on a map with 1 % seeds and on maps with one seed each - 100 calls between two device events, 5 rounds;
  * the two kernels of those calls apart, from the profiler's kernel records."""
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
try:
    from excel_amd.utils import label_fill as lf
except ImportError:
    lf = None
logging.basicConfig(level=logging.WARNING, format="%(message)s")
dev = torch.device("cuda", 0)
B, NC = 32, 21
res = {"root": root, "build_id": ops.lib().excel_build_id().decode(), "has_fill": lf is not None}

infer_lam.validate(infer_lam.get_parser().parse_args(["--synthetic", str(B), "--ragged", "true", "--batch_size", str(B), "--gemm_check", "false",
                                                      "--num_workers", "12"]))          # builds the model, warms the step's shapes
model = infer_lam.validate.last_model
ds = synthetic.SyntheticSegDataset(128, (448, 448), num_classes=NC, seed=1234, u8_images=False, ragged=True)
resident = []
for s0 in range(0, 128, B):
    rb = pack_samples([ds[i] for i in range(s0, s0 + B)])
    resident.append((rb.images.to(dev), ops.RaggedPlan(rb.hw, dev), rb.cls.to(dev), rb.labels.to(dev)))
plan = resident[-1][1]
sizes = [(int(h), int(w)) for h, w in plan.hw]
res["pixels_last_step"] = plan.total_label_pix

# ---- resident steps
arms = {"clean": TrainingFreePipeline(model, num_classes=NC, smax=ds.max_k(), clean=dict(min_region=64))}
if lf is not None:
    arms["clean_fill"] = TrainingFreePipeline(model, num_classes=NC, smax=ds.max_k(), clean=dict(min_region=64), fill=dict(radius=None))
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
res["last_step_regions_removed_pixels"] = arms["clean"].last_clean_counts.sum(0).tolist()

if lf is not None:
    assert torch.equal(arms["clean"].hist, arms["clean_fill"].hist) and torch.equal(arms["clean"].hist_clean, arms["clean_fill"].hist_clean)
    res["last_step_holes_filled"] = arms["clean_fill"].last_fill_counts[:, :2].sum(0).tolist()
    res["last_step_max_dist2"] = int(arms["clean_fill"].last_fill_counts[:, 2].max())

    # ---- the fill alone
    def blob_map(h, w, rs):
        y, x = np.mgrid[:h, :w]
        m = np.zeros((h, w), np.uint8)
        for k in range(8):
            cy, cx, r = rs.randint(0, h), rs.randint(0, w), rs.randint(10, 90)
            m[(y - cy) ** 2 + (x - cx) ** 2 <= r * r] = 1 + k % 5
        sp = rs.rand(h, w) < 0.02
        m[sp] = rs.randint(0, NC, int(sp.sum())).astype(np.uint8)
        return m

    def holes_map(h, w, rs, share):
        m = rs.randint(0, NC, (h, w)).astype(np.uint8)
        m[rs.rand(h, w) < share] = 255
        return m

    def one_seed(h, w):
        m = np.full((h, w), 255, np.uint8)
        m[h // 2, w // 2] = 3
        return m

    rs = np.random.RandomState(0)
    flat = lambda ms: torch.from_numpy(np.concatenate([m.reshape(-1) for m in ms])).to(dev)
    blobs = flat([blob_map(h, w, rs) for h, w in sizes])
    blobs_clean = cc.filter_small_regions(blobs, *cc.label_components(blobs, plan=plan), 64, NC, plan=plan)[0]
    step_labels = arms["clean_fill"].run_batch_ragged(*resident[-1]).clone()
    cases = {"step (cleaned labels, main labels as mask)": (arms["clean_fill"].last_clean_labels.clone(), step_labels),
             "blobs + 2 % speckle, cleaned at 64 (blobs as mask)": (blobs_clean, blobs),
             "random classes, 30 % holes (no mask)": (flat([holes_map(h, w, rs, 0.30) for h, w in sizes]), None),
             "1 % seeds, 99 % holes (no mask)": (flat([holes_map(h, w, rs, 0.99) for h, w in sizes]), None),
             "one seed per image, at its centre (no mask)": (flat([one_seed(h, w) for h, w in sizes]), None)}
    n = plan.total_label_pix
    out = (torch.empty(n, dtype=torch.uint8, device=dev), torch.empty(n, dtype=torch.int32, device=dev), torch.empty(3 * B, dtype=torch.int32, device=dev))
    micro, kernels = {}, {}
    from torch.profiler import ProfilerActivity, profile
    for name, (lab, mask) in cases.items():
        fn = lambda: lf.fill_nearest_label(lab, NC, plan=plan, mask=mask, out=out)
        for _ in range(5):
            fn()
        torch.cuda.synchronize()
        calls = 100 if "seed" not in name else 10
        us = []
        for _ in range(5):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(calls):
                fn()
            e1.record()
            e1.synchronize()
            us.append(round(e0.elapsed_time(e1) * 1e3 / calls, 2))
        c = out[2].view(B, 3)
        micro[name] = {"us_per_call_rounds": us, "median_us": float(np.median(us)), "holes_filled": c[:, :2].sum(0).tolist(), "max_dist2": int(c[:, 2].max())}
        try:
            with profile(activities=[ProfilerActivity.CUDA, ProfilerActivity.CPU]) as prof:
                for _ in range(10):
                    fn()
                torch.cuda.synchronize()
            per = {}
            for ev in prof.key_averages():
                m = re.search(r"fill_(col|row)_kernel", ev.key)
                t_us = getattr(ev, "device_time_total", None)
                if t_us is None:
                    t_us = getattr(ev, "cuda_time_total", 0.0)
                if m and ev.count:
                    per[m.group(1)] = round(float(t_us) / ev.count, 2)
            kernels[name] = per
        except Exception as e:                                    # the profiler is an observer: without it the split is "not measured"
            kernels[name] = {"not_measured": repr(e)}
    res["fill_alone"] = micro
    res["fill_kernel_us"] = kernels

os.makedirs(os.path.dirname(out_path), exist_ok=True)
with open(out_path, "w") as f:
    json.dump(res, f, indent=1)
print(json.dumps(res))
