"""Cost of the boundary scores (EXPERIMENTS.md, "Boundary scores"):  python tools_dev/boundary_scores_bench.py ROOT parent|this OUT.json
ROOT = the tree to import excel_amd from (a checkout of the parent commit with `parent`: it has no flag, so only the plain arms run).
One process, the model built once (seeded random ViT-B/16, bf16x3):
  * `this`: ops.boundary_scores beside ops.image_scores on the same arrays - 32 uniform maps of 448 x 448, 21 classes, d = 13, a coherent
    pair (blocks of 60 pixels against themselves moved by (3, 5)) and a noise pair (independent random labels) - 200 calls between two
    device events, 7 alternating rounds (a call = the clearing fill + the kernel + the Python wrapper);
  * resident ragged steps at B = 32 with VOC-like sizes: plain, and with `this` image_scores=True and image_scores + boundary, alternating;
  * infer_lam --synthetic 256 --ragged true with the flag off and on, alternating."""
import json
import logging
import os
import re
import sys
import time

root, mode, out_path = os.path.abspath(sys.argv[1]), sys.argv[2], os.path.abspath(sys.argv[3])
sys.path.insert(0, root)
os.chdir(root)
import numpy as np
import torch

import excel_amd
from excel_amd import ops
from excel_amd.datasets.loader import pack_samples
from excel_amd.pipeline import TrainingFreePipeline
from excel_amd.tools import infer_lam, synthetic

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
B, NIMG = 32, 256
base = ["--synthetic", str(NIMG), "--ragged", "true", "--batch_size", str(B), "--gemm_check", "false", "--num_workers", "12"]
parse = infer_lam.get_parser().parse_args
res = {"mode": mode, "root": root, "build_id": ops.lib().excel_build_id().decode()}

infer_lam.validate(parse(base))                  # the program once: builds the model, warms every shape of the loop
model = infer_lam.validate.last_model
rates.clear()

# ---- the kernel beside image_scores_kernel
if mode == "this":
    nc, d, S = 21, 13, 448
    rs = np.random.RandomState(0)
    blocks = np.kron(rs.randint(0, nc, (B, S // 60 + 1, S // 60 + 1)), np.ones((1, 60, 60), np.int64))[:, :S, :S].astype(np.uint8)
    pairs = {"coherent": (blocks, np.roll(blocks, (3, 5), (1, 2))),
             "noise": (rs.randint(0, nc, (B, S, S)).astype(np.uint8), rs.randint(0, nc, (B, S, S)).astype(np.uint8))}
    micro = {}
    for cname, (g, p) in pairs.items():
        g, p = torch.from_numpy(g).to(dev), torch.from_numpy(p).to(dev)
        c1, c2 = (torch.empty(B * 3 * nc, dtype=torch.int32, device=dev) for _ in range(2))
        fns = {"boundary_scores": lambda: ops.boundary_scores(g, p, nc, d, out=c1),
               "image_scores": lambda: ops.image_scores(g.view(B, -1), p.view(B, -1), nc, out=c2)}
        for f in fns.values():
            for _ in range(20):
                f()
        torch.cuda.synchronize()
        t = {k: [] for k in fns}
        for rnd in range(7):
            for k, f in fns.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(200):
                    f()
                e1.record()
                e1.synchronize()
                t[k].append(round(e0.elapsed_time(e1) * 1e3 / 200, 2))
        band = c1.view(B, 3, nc)[:, 0].sum().item() / max(c2.view(B, 3, nc)[:, 0].sum().item(), 1)
        micro[cname] = {"band_share_of_gt": round(band, 4), **{k: {"us_per_call_rounds": v, "median_us": float(np.median(v))} for k, v in t.items()}}
    res["micro"] = micro

# ---- resident steps
ds = synthetic.SyntheticSegDataset(128, (448, 448), num_classes=21, seed=1234, u8_images=False, ragged=True)
resident = []
for s0 in range(0, 128, B):
    rb = pack_samples([ds[i] for i in range(s0, s0 + B)])
    resident.append((rb.images.to(dev), ops.RaggedPlan(rb.hw, dev), rb.cls.to(dev), rb.labels.to(dev)))
arms = {"off": TrainingFreePipeline(model, num_classes=21, smax=ds.max_k())}
if mode == "this":
    arms["image_scores"] = TrainingFreePipeline(model, num_classes=21, smax=ds.max_k(), image_scores=True)
    arms["boundary"] = TrainingFreePipeline(model, num_classes=21, smax=ds.max_k(), image_scores=True, boundary=dict(ratio=0.02, px=0))
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
if mode == "this":
    assert torch.equal(arms["boundary"].hist, arms["off"].hist), "the flag changed the matrix"
    assert sorted(arms["boundary"].last_score_ticket.counts()) == ["main", "main_bd"]

# ---- the program's own loop
loop = {"off": []}
order = ["off", "off"] if mode == "parent" else ["off", "on", "off", "on"]
if mode == "this":
    loop["on"] = []
for name in order:
    rates.clear()
    infer_lam.validate(parse(base + (["--boundary_scores", "true"] if name == "on" else [])), pipe=arms["boundary" if name == "on" else "off"])
    loop[name].append({"img_per_s": rates[-1], "ms_per_step": round(B / rates[-1] * 1e3, 2)})
res["infer_lam_loop"] = loop

os.makedirs(os.path.dirname(out_path), exist_ok=True)
with open(out_path, "w") as f:
    json.dump(res, f, indent=1)
print(json.dumps(res))
