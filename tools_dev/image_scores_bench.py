"""Cost of the per-image scores (EXPERIMENTS.md, "Per-image scores"):  python tools_dev/image_scores_bench.py ROOT parent|this OUT.json [AB_LIB]
ROOT = the tree to import excel_amd from (a checkout of the parent commit with `parent`: it has no flag, so only the plain arms run).
One process, the model built once (seeded random ViT-B/16, bf16x3): resident ragged steps at B = 32 with VOC-like sizes, then
infer_lam --synthetic 256 --ragged true; `this` alternates flag off / flag on inside the run and adds the launch time of
ops.image_scores next to ops.confusion_accumulate_masked on the label arrays of one step (200 calls between two device events, 7
alternating rounds; these calls can be bound by the Python wrapper - kernel durations come from a rocprofv3 --kernel-trace run over the
arrays this script leaves in step_labels.npz next to OUT.json).  AB_LIB: a shared library whose entry
`int imgscore_arm(gt, pred, B, per_image, table, max_pix, skip, nc, counts, stream)` launches an experimental arm of the kernel, timed
beside them and checked equal (the run-folding arm of EXPERIMENTS.md was image_scores_kernel compiled that way)."""
import ctypes as C
import json
import logging
import os
import re
import sys
import time

root, mode, out_path = os.path.abspath(sys.argv[1]), sys.argv[2], os.path.abspath(sys.argv[3])
ab_lib = os.path.abspath(sys.argv[4]) if len(sys.argv) > 4 else None
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

# the program once: builds the model, warms every shape of the loop
infer_lam.validate(parse(base))
model = infer_lam.validate.last_model
res["gemm_mode"] = model.encoder.visual.handle().gemm_mode()
rates.clear()

# ---- resident steps
ds = synthetic.SyntheticSegDataset(128, (448, 448), num_classes=21, seed=1234, u8_images=False, ragged=True)
resident = []
for s0 in range(0, 128, B):
    rb = pack_samples([ds[i] for i in range(s0, s0 + B)])
    resident.append((rb.images.to(dev), ops.RaggedPlan(rb.hw, dev), rb.cls.to(dev), rb.labels.to(dev)))
res["mpix_per_step"] = [round(int(r[1].total_label_pix) / 1e6, 3) for r in resident]
arms = {"off": TrainingFreePipeline(model, num_classes=21, smax=ds.max_k())}
if mode == "this":
    arms["on"] = TrainingFreePipeline(model, num_classes=21, smax=ds.max_k(), image_scores=True)
for pipe in arms.values():
    for r in resident[:2]:
        pipe.run_batch_ragged(*r)
torch.cuda.synchronize()
resident_ms = {k: [] for k in arms}
for rep in range(7):
    for name, pipe in arms.items():
        tickets = []
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(2):
            for r in resident:
                pipe.run_batch_ragged(*r)
                if name == "on":
                    tickets.append(pipe.last_score_ticket)
        torch.cuda.synchronize()
        resident_ms[name].append(round((time.perf_counter() - t0) * 1e3 / (2 * len(resident)), 3))
        if name == "on":
            assert all(t.ready() for t in tickets) and tickets[-1].counts()["main"].shape == (B, 3, 21)
res["resident_ms_per_step"] = resident_ms
if mode == "this":
    assert torch.equal(arms["on"].hist, arms["off"].hist), "the flag changed the matrix"

# ---- the program's own loop: infer_lam --synthetic --ragged, 256 images at batch 32
loop = {"off": []}
order = ["off", "off"] if mode == "parent" else ["off", "on", "off", "on"]
if mode == "this":
    loop["on"] = []
scratch = os.path.dirname(out_path)
os.makedirs(scratch, exist_ok=True)
for name in order:
    extra = ["--per_image_scores", os.path.join(scratch, "scratch_scores.csv")] if name == "on" else []
    rates.clear()
    infer_lam.validate(parse(base + extra), pipe=arms[name])
    loop[name].append({"img_per_s": rates[-1], "ms_per_step": round(B / rates[-1] * 1e3, 2)})
res["infer_lam_loop"] = loop

# ---- the kernel against the masked confusion kernel and the no-folding arm, on the label arrays of one step
if mode == "this":
    _, plan, _, gts = resident[0]
    labels = arms["off"].run_batch_ragged(*resident[0]).clone()
    nc = 21
    skip = torch.zeros(B, dtype=torch.int32, device=dev)
    hist = torch.zeros((nc, nc), dtype=torch.int64, device=dev)
    counts = torch.empty((B, 3, nc), dtype=torch.int32, device=dev)
    counts2 = torch.empty_like(counts)
    if ab_lib:
        arm = C.CDLL(ab_lib).imgscore_arm
        arm.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_longlong, C.c_void_p, C.c_longlong, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
        st = torch.cuda.current_stream().cuda_stream

        def run_arm(g, p, pl, out):
            assert arm(g.data_ptr(), p.data_ptr(), B, 0, pl.table.data_ptr(), int(pl.info.max_plane_pix), skip.data_ptr(), nc, out.data_ptr(), st) == 0

    # a second pair of label arrays: the ground truth against itself moved on by 500 pixels, one row of most images (the maps of a
    # good segmenter: long runs, errors at the boundaries only; the random network's labels of the first pair are noise)
    shifted = torch.roll(gts, 500)
    cases = {"step labels vs ground truth": (gts, labels), "ground truth vs shifted ground truth": (gts, shifted)}
    micro = {}
    for cname, (g, p) in cases.items():
        fns = {"image_scores": lambda: ops.image_scores(g, p, nc, skip=skip, plan=plan, out=counts.view(-1)),
               "confusion_accumulate_masked": lambda: ops.confusion_accumulate_masked(g, p, nc, skip, hist, plan=plan)}
        if ab_lib:
            fns["experimental_arm"] = lambda: run_arm(g, p, plan, counts2)
            fns["image_scores"]()
            fns["experimental_arm"]()
            assert torch.equal(counts, counts2), "the two arms disagree"
        t = {k: [] for k in fns}
        for k, f in fns.items():
            for _ in range(20):
                f()
        torch.cuda.synchronize()
        N = 200
        for rnd in range(7):
            for k, f in fns.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(N):
                    f()
                e1.record()
                e1.synchronize()
                t[k].append(round(e0.elapsed_time(e1) * 1e3 / N, 2))
        micro[cname] = {k: {"us_per_call_rounds": v, "median_us": float(np.median(v))} for k, v in t.items()}
    res["micro"] = micro
    np.savez(os.path.join(scratch, "step_labels.npz"), gts=gts.cpu().numpy(), labels=labels.cpu().numpy(), hw=plan.hw)
    res["micro_pixels"] = int(plan.total_label_pix)
    res["micro_note"] = "200 back-to-back calls between two device events, 7 alternating rounds; a call = memset + kernel for image_scores"

with open(out_path, "w") as f:
    json.dump(res, f, indent=1)
print(json.dumps(res))
