"""Cost of the arg-max margin launch (EXPERIMENTS.md, "Margin sweep"):  python tools_dev/margin_bench.py ROOT OUT.json
ROOT = the tree to import excel_amd from.  One process:
  * excel_margin_sweep_ragged beside the parent's excel_bkg_sweep_ragged on the same planes - the benchmark's ragged step in size (32
    images of VOC-like sizes, 7 planes per image, 1 - 3 present classes, 21 classes, K = 8), "coherent" fields (constant on 32- / 48-pixel
    cells plus 2 % noise) and "noise" fields (independent per pixel) - HIP events around each call, the median of 20 calls after 3
    warm-ups, the launches alternating; the margin launch also with each of its outputs alone, to see what the time is made of;
  * resident ragged steps at B = 32 (the model built once, seeded random ViT-B/16): a plain pipeline and one with margin_sweep +
    margin_min, alternating - 8 steps per timing, 7 rounds, a host clock around a synchronise."""
import json
import logging
import os
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
from excel_amd.utils.bkg_sweep import sweep_ragged
from excel_amd.utils.margin import coverage_from_kept, margin_ragged

assert os.path.dirname(os.path.abspath(excel_amd.__file__)) == os.path.join(root, "excel_amd"), excel_amd.__file__
logging.basicConfig(level=logging.WARNING, format="%(message)s")
dev = torch.device("cuda", 0)
B, NC, CMAX, K = 32, 21, 7, 8
THRESHOLDS = (0.0, 0.02, 0.05, 0.1, 0.15, 0.2, 0.3, 0.5)     # illustrations: no value has been measured on real data
SCALES = (0.5, 0.7, 0.85, 1.0, 1.2, 1.5, 2.0, 3.0)
MARGIN_MIN = 0.1
res = {"root": root, "build_id": ops.lib().excel_build_id().decode(), "thresholds": THRESHOLDS, "scales": SCALES, "margin_min": MARGIN_MIN}

# ---- the two launches on the same planes
rs = np.random.RandomState(7)
sizes = [synthetic.draw_voc_like_size(rs) for _ in range(B)]
plan = ops.RaggedPlan(sizes, dev)
nchan_h = (rs.choice([1, 2, 3], size=B, p=[0.6, 0.3, 0.1]) + 1).astype(np.int32)
cls_h = np.stack([np.sort(rs.choice(NC - 1, size=CMAX - 1, replace=False)) for _ in range(B)]).astype(np.int32)
res["pixels"], res["tiles"] = int(plan.total_label_pix), int(plan.total_tiles)


def cells(h, w, cell, lo, hi):
    g = rs.rand(h // cell + 1, w // cell + 1) * (hi - lo) + lo
    return np.kron(g, np.ones((cell, cell)))[:h, :w]


def fields(kind):
    planes, gts = [], []
    for b, (h, w) in enumerate(sizes):
        wp = (w + 3) // 4 * 4
        p = np.zeros((CMAX, h, wp), np.float32)
        if kind == "coherent":
            for c in range(CMAX):
                p[c, :, :w] = cells(h, w, 32 if c % 2 else 48, 0.0, 1.0) + 0.02 * rs.rand(h, w)
            g = cells(h, w, 48, 0, NC).astype(np.uint8)
        else:
            p[:, :, :w] = rs.rand(CMAX, h, w)
            g = rs.randint(0, NC, (h, w)).astype(np.uint8)
        g[rs.rand(h, w) < 0.03] = 255
        planes.append(p.reshape(-1))
        gts.append(g.reshape(-1))
    return torch.from_numpy(np.concatenate(planes)).to(dev), torch.from_numpy(np.concatenate(gts)).to(dev)


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3


nchan, cls = torch.from_numpy(nchan_h).to(dev), torch.from_numpy(cls_h).to(dev)
n = plan.total_label_pix
micro = {}
for kind in ("coherent", "noise"):
    planes, gts = fields(kind)
    t_s = torch.zeros((K, 3, NC), dtype=torch.int64, device=dev)
    t_m = torch.zeros((K, 3, NC), dtype=torch.int64, device=dev)
    k_m = torch.zeros((K + 1,), dtype=torch.int64, device=dev)
    lab = torch.empty(n, dtype=torch.uint8, device=dev)
    mar = torch.empty(n, dtype=torch.float32, device=dev)
    kw = dict(nchan=nchan, cls_idx=cls)
    arms = {
        "bkg_sweep_counts": lambda: sweep_ragged(planes, plan, CMAX, SCALES, gts=gts, num_classes=NC, totals=t_s, **kw),
        "margin_totals_kept": lambda: margin_ragged(planes, plan, CMAX, THRESHOLDS, gts=gts, num_classes=NC, totals=t_m, kept=k_m, **kw),
        "bkg_sweep_labels_only": lambda: sweep_ragged(planes, plan, CMAX, SCALES, label_sel=3, labels_out=lab, **kw),
        "margin_labels_only": lambda: margin_ragged(planes, plan, CMAX, (), label_thre=MARGIN_MIN, labels_out=lab, **kw),
        "margin_kept_only": lambda: margin_ragged(planes, plan, CMAX, THRESHOLDS, kept=k_m, **kw),
        "margin_totals_only": lambda: margin_ragged(planes, plan, CMAX, THRESHOLDS, gts=gts, num_classes=NC, totals=t_m, **kw),
        "margin_all_four": lambda: margin_ragged(planes, plan, CMAX, THRESHOLDS, gts=gts, num_classes=NC, totals=t_m, kept=k_m, label_thre=MARGIN_MIN,
                                                 labels_out=lab, margin_out=mar, **kw),
    }
    us = {k: [] for k in arms}
    for rep in range(23):                                     # 3 warm-ups, then 20 timed calls of every arm, alternating
        for name, fn in arms.items():
            t = timed(fn)
            if rep >= 3:
                us[name].append(round(t, 2))
    row = {k: {"median_us": float(np.median(v)), "min_us": float(np.min(v)), "max_us": float(np.max(v))} for k, v in us.items()}
    row["ratio_margin_over_sweep_counts"] = round(row["margin_totals_kept"]["median_us"] / row["bkg_sweep_counts"]["median_us"], 3)
    row["coverage"] = [round(c, 4) for c in coverage_from_kept(k_m)]         # (every call adds the same counts: the ratio stands)
    micro[kind] = row
    print(kind, json.dumps(row), flush=True)
res["launches_us"] = micro

# ---- resident steps
infer_lam.validate(infer_lam.get_parser().parse_args(["--synthetic", str(B), "--ragged", "true", "--batch_size", str(B), "--gemm_check", "false",
                                                      "--num_workers", "12"]))          # builds the model, warms the step's shapes
model = infer_lam.validate.last_model
ds = synthetic.SyntheticSegDataset(128, (448, 448), num_classes=NC, seed=1234, u8_images=False, ragged=True)
resident = []
for s0 in range(0, 128, B):
    rb = pack_samples([ds[i] for i in range(s0, s0 + B)])
    resident.append((rb.images.to(dev), ops.RaggedPlan(rb.hw, dev), rb.cls.to(dev), rb.labels.to(dev)))
pipes = {"plain": TrainingFreePipeline(model, num_classes=NC, smax=ds.max_k()),
         "margin": TrainingFreePipeline(model, num_classes=NC, smax=ds.max_k(), margin_sweep=THRESHOLDS, margin_min=MARGIN_MIN)}
for pipe in pipes.values():
    for r in resident[:2]:
        pipe.run_batch_ragged(*r)
torch.cuda.synchronize()
resident_ms = {k: [] for k in pipes}
for rep in range(7):
    for name, pipe in pipes.items():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(2):
            for r in resident:
                pipe.run_batch_ragged(*r)
        torch.cuda.synchronize()
        resident_ms[name].append(round((time.perf_counter() - t0) * 1e3 / (2 * len(resident)), 3))
res["resident_ms_per_step"] = resident_ms
res["resident_median_ms"] = {k: float(np.median(v)) for k, v in resident_ms.items()}
assert torch.equal(pipes["plain"].hist, pipes["margin"].hist), "the margin arguments changed the main labels"
res["resident_coverage"] = [round(c, 4) for c in coverage_from_kept(pipes["margin"].margin_kept)]

os.makedirs(os.path.dirname(out_path), exist_ok=True)
with open(out_path, "w") as f:
    json.dump(res, f, indent=1)
print(json.dumps(res))
