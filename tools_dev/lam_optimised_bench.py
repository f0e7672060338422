"""The optimised-LAM regime (`infer_lam --training_free false`) batched (OptimisedLamPipeline on ragged batches) against the per-image
call sequence (`--api_path true`), in one process on one box:

    python tools_dev/lam_optimised_bench.py [--n 512] [--batch_size 32] [--resize_size 448] [--out profiles/lam_optimised_bench.jsonl]

Both runs are `infer_lam --ragged true --synthetic N --batch_size B --resize_size S --training_free false --model_path <seeded head>`
(seeded ViT-B/16-shaped tower, the head of model/init_head.init_decoder_state_dict saved with torch.save); each is preceded by a short
warm-up run of the same configuration.  One JSON line per run: img/s and ms per step from infer_lam's own clock of the evaluation
loop (model build excluded), peak device memory of the run.

`--one_step` runs exactly one B-image step of the batched pipeline after building the model and nothing else (for
`rocprofv3 --kernel-trace --stats -- python tools_dev/lam_optimised_bench.py --one_step`: the per-kernel table of one step)."""
import argparse
import json
import os
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402


def _head(path):
    from excel_amd.model.init_head import init_decoder_state_dict
    torch.save(init_decoder_state_dict(seed=0), path)
    return path


def _run(head, n, bs, S, api_path, tmp):
    """-> seconds of the evaluation loop (infer_lam's own clock: model build and start-up excluded), mIoU, peak device memory."""
    from excel_amd.tools import infer_lam
    out = os.path.join(tmp, "run.json")
    args = infer_lam.get_parser().parse_args(["--ragged", "true", "--synthetic", str(n), "--batch_size", str(bs), "--resize_size", str(S),
                                              "--training_free", "false", "--model_path", head, "--api_path", str(api_path).lower(),
                                              "--gemm_check", "false", "--json_out", out])
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    infer_lam.validate(args)
    rec = json.load(open(out))
    return dict(seconds=rec["seconds_rank0"], miou=rec["miou"], peak_mem_gib=round(torch.cuda.max_memory_allocated() / 2 ** 30, 3))


def one_step(bs, S):
    from excel_amd import ops
    from excel_amd.model import ExCEL_model
    from excel_amd.model.init_head import init_decoder_state_dict
    from excel_amd.pipeline import OptimisedLamPipeline
    from excel_amd.tools import synthetic
    model = ExCEL_model(clip_model="ExCEL_ViT-B/16", num_classes=21, img_size=S, mode="train", state_dict=synthetic.make_vit_state_dict(seed=0),
                        text_features=synthetic.make_text_features(45), decoder_state_dict=init_decoder_state_dict(seed=0))
    ds = synthetic.SyntheticSegDataset(bs, num_classes=21, seed=1234, ragged=True)
    s = [ds[i] for i in range(bs)]
    plan = ops.RaggedPlan([x[1].shape[:2] for x in s], "cuda")
    hwc = torch.from_numpy(np.concatenate([x[1].reshape(-1) for x in s])).cuda()
    gts = torch.from_numpy(np.concatenate([x[2].reshape(-1) for x in s])).cuda()
    cls = torch.from_numpy(np.stack([x[3] for x in s])).cuda()
    pipe = OptimisedLamPipeline(model, num_classes=21, smax=ds.max_k())
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    pipe.run_batch_ragged(hwc, plan, cls, gts, S=S)
    torch.cuda.synchronize()
    print(json.dumps({"one_step": True, "batch_size": bs, "resize_size": S, "peak_mem_gib": round(torch.cuda.max_memory_allocated() / 2 ** 30, 3)}))


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--n", type=int, default=512)
    p.add_argument("--n_api", type=int, default=None, help="images of the per-image run (default: --n)")
    p.add_argument("--batch_size", type=int, default=32)
    p.add_argument("--resize_size", type=int, default=448)
    p.add_argument("--out", default=os.path.join(ROOT, "profiles", "lam_optimised_bench.jsonl"))
    p.add_argument("--one_step", action="store_true")
    a = p.parse_args()
    if a.one_step:
        return one_step(a.batch_size, a.resize_size)
    from excel_amd import build
    from excel_amd.tools import infer_lam
    with tempfile.TemporaryDirectory() as tmp:
        head = _head(os.path.join(tmp, "head.pth"))
        recs = []
        for mode, api, n in (("batched", False, a.n), ("per_image", True, a.n_api or a.n)):
            _run(head, a.batch_size, a.batch_size, a.resize_size, api, tmp)            # warm-up: one step's worth
            r = _run(head, n, a.batch_size, a.resize_size, api, tmp)
            steps = n if api else -(-n // a.batch_size)
            rec = dict(mode=mode, images=n, batch_size=a.batch_size, resize_size=a.resize_size, img_per_s=round(n / r["seconds"], 2),
                       ms_per_step=round(1000.0 * r["seconds"] / steps, 3), step="one image" if api else f"one batch of {a.batch_size}",
                       peak_mem_gib=r["peak_mem_gib"], miou=r["miou"], gemm_mode=infer_lam.validate.last_model.encoder.visual.handle().gemm_mode(),
                       build_id=build.source_id(), device=torch.cuda.get_device_name(0))
            recs.append(rec)
            print(json.dumps(rec), flush=True)
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            for rec in recs:
                f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
