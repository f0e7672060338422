"""Measurements of the confident-label stage (infer_lam --conf_label, conf.hip) at the bench shapes: seeded random ViT-B/16, S = 448, two
resident ragged batches of 32 VOC-like images.  Step time with and without conf= (alternating, host clock around a synchronise), the
three new stages and the main PAR on their own (HIP events, alternating), ONE PAR over 2 (k + 1) planes against two over k + 1.
`python tools_dev/conf_label_bench.py [record.json]` on one MI355X; EXPERIMENTS.md "Confident labels"."""
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from excel_amd import ops  # noqa: E402
from excel_amd.datasets.loader import pack_samples  # noqa: E402
from excel_amd.model import ExCEL_model  # noqa: E402
from excel_amd.pipeline import TrainingFreePipeline  # noqa: E402
from excel_amd.tools import synthetic  # noqa: E402

dev = torch.device("cuda", 0)
B, S, NC = 32, 448, 21
CONF = (0.7, 0.25)
model = ExCEL_model(clip_model="ExCEL_ViT-B/16", num_classes=NC, img_size=S, mode="train", device=dev,
                    state_dict=synthetic.make_vit_state_dict(seed=0), text_features=synthetic.make_text_features(45))
ds = synthetic.SyntheticSegDataset(2 * B, (S, S), num_classes=NC, seed=1234, ragged=True)
batches = []
for lo in (0, B):
    rb = pack_samples([ds[i] for i in range(lo, lo + B)])
    batches.append((rb.images.to(dev), ops.RaggedPlan(rb.hw, dev), rb.cls.to(dev), rb.labels.to(dev)))
pipe = TrainingFreePipeline(model, num_classes=NC, smax=ds.max_k())
out = {"gemm_mode": model.encoder.visual.handle().gemm_mode(), "B": B, "S": S, "smax": pipe.smax,
       "mean_label_megapixels_per_image": sum(b[1].total_label_pix for b in batches) / 2 / B / 1e6}


def step(conf):
    for b in batches:
        pipe.run_batch_ragged(*b, S=S, conf=conf)


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


for conf in (None, CONF, None, CONF):       # warm-up of both variants
    step(conf)
torch.cuda.synchronize()
plain, with_conf = [], []
for _ in range(7):                          # alternate the two variants; each sample = 2 steps of 32 images
    plain.append(timed(lambda: step(None)) / 2)
    with_conf.append(timed(lambda: step(CONF)) / 2)
out["step_ms_plain"] = {"median": statistics.median(plain), "min": min(plain), "max": max(plain)}
out["step_ms_conf"] = {"median": statistics.median(with_conf), "min": min(with_conf), "max": max(with_conf)}
out["step_ms_added_median"] = statistics.median(with_conf) - statistics.median(plain)

# stages on their own, on the first batch's cams
images, plan, cls_t, gts = batches[0]
_, inter = pipe.run_batch_ragged(images, plan, cls_t, gts, S=S, return_intermediates=True)
inputs, cams, idx = inter["inputs"], inter["cams"], inter["cls_idx"]
nchan = inter["ncls"] + 1
C = pipe.smax + 1
half = ops.conf_half_plan(plan)
planes, nchan2 = ops.conf_planes_ragged(cams, plan, half, pipe.smax, nchan, *CONF)
n1 = C * half.total_pix
sep = [planes[:n1].clone(), planes[n1:2 * n1].clone()]      # timing only: any defined values of the right layout
ws_main = torch.empty(ops.lib().excel_par_ragged_workspace_bytes(plan.total_pix, C), dtype=torch.uint8, device=dev)
ws_f = torch.empty(ops.lib().excel_par_ragged_workspace_bytes(half.total_pix, 2 * C), dtype=torch.uint8, device=dev)
ws_s = torch.empty(ops.lib().excel_par_ragged_workspace_bytes(half.total_pix, C), dtype=torch.uint8, device=dev)
o_main, o_f, o_s = torch.empty_like(cams), torch.empty_like(planes), torch.empty_like(sep[0])
dil, it = pipe.dilations, pipe.num_iter
stages = {
    "conf_planes": lambda: ops.conf_planes_ragged(cams, plan, half, pipe.smax, nchan, *CONF, out=planes),
    "par_fused_2(k+1)": lambda: ops.par_forward_ragged(inputs, planes, half, 2 * C, dil, it, nchan=nchan2, ws=ws_f, out=o_f),
    "par_two_separate": lambda: [ops.par_forward_ragged(inputs, m, half, C, dil, it, nchan=nchan, ws=ws_s, out=o_s) for m in sep],
    "conf_merge": lambda: ops.conf_merge_ragged(o_f, half, plan, pipe.smax, nchan, idx),
    "par_main": lambda: ops.par_forward_ragged(inputs, cams, plan, C, dil, it, nchan=nchan, ws=ws_main, out=o_main),
}
samples = {k: [] for k in stages}
for rep in range(13):                       # 3 warm-up rounds, 10 timed; the stages alternate inside a round
    for name, fn in stages.items():
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        if rep >= 3:
            samples[name].append(e0.elapsed_time(e1))
out["stage_ms"] = {k: {"median": statistics.median(v), "min": min(v), "max": max(v)} for k, v in samples.items()}
m = {k: statistics.median(v) for k, v in samples.items()}
out["fused_over_separate"] = m["par_fused_2(k+1)"] / m["par_two_separate"]
out["fused_par_over_main_par"] = m["par_fused_2(k+1)"] / m["par_main"]
out["three_stages_ms"] = m["conf_planes"] + m["par_fused_2(k+1)"] + m["conf_merge"]
cov = float(pipe.hist_conf.sum()) / max(float(pipe.hist.sum()), 1.0) if pipe.hist_conf is not None else None
out["coverage_random_weights"] = cov
if len(sys.argv) > 1:
    with open(sys.argv[1], "w") as f:
        json.dump(out, f, indent=1)
print(json.dumps(out, indent=1))
