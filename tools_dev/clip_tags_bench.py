"""step time of run_batch at the benchmark's configuration (B = 32, 448 x 448, ViT-B/16, 45 prompts) with and without the tagger, and
the tagger's own launch timed with events"""
import json, sys, time, os
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np, torch
from excel_amd import ops
from excel_amd.model import ExCEL_model
from excel_amd.pipeline import TrainingFreePipeline
from excel_amd.tools import synthetic
B, S, NC = 32, 448, 21
sd = synthetic.make_vit_state_dict(seed=0)
model = ExCEL_model(clip_model="ExCEL_ViT-B/16", num_classes=NC, img_size=S, mode="train", device="cuda", state_dict=sd,
                    text_features=synthetic.make_text_features(45))
ds = synthetic.SyntheticSegDataset(2 * B, (S, S), num_classes=NC, seed=1234)
batches = []
for i in range(2):
    _, imgs, gts, cls = ds.batch(np.arange(i * B, (i + 1) * B))
    batches.append((torch.from_numpy(imgs).cuda(), torch.from_numpy(cls).cuda(), torch.from_numpy(gts).cuda()))
plain = TrainingFreePipeline(model, num_classes=NC, smax=6)
tagged = TrainingFreePipeline(model, num_classes=NC, smax=6, tagger=dict(thre=0.2, kmax=6, scale=100.0))
def timed(pipe, steps=20):
    for i in range(4):
        pipe.run_batch(*batches[i % 2])
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(steps):
        pipe.run_batch(*batches[i % 2])
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / steps
out = {"mode": model.encoder.visual.handle().gemm_mode()}
res = {"plain": [], "tagged": []}
for rep in range(3):                      # interleaved, so drift hits both alike
    res["plain"].append(round(timed(plain), 4))
    res["tagged"].append(round(timed(tagged), 4))
out["step_ms"] = res
x_raw = model.last_x_raw
e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
for _ in range(5):
    ops.clip_tags(x_raw, model._text_rows, NC - 1)
e0.record()
for _ in range(100):
    ops.clip_tags(x_raw, model._text_rows, NC - 1)
e1.record()
torch.cuda.synchronize()
out["clip_tags_us_per_call_back_to_back"] = round(e0.elapsed_time(e1) * 10, 3)
out["tags_per_image"] = tagged.last_tags[0].sum(1).cpu().tolist()
print(json.dumps(out))
