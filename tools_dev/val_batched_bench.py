"""The training programs' validation pass, batched (engine/validatation_engine.build_validation_ragged: ValidationPipeline on ragged
batches, decode threads) against the reference's per-image loop (build_validation over scripts/train_voc._val_batches), in one process
on one box:

    python tools_dev/val_batched_bench.py [--n 1024] [--batch_size 16] [--resize_size 320] [--repeats 2] [--out profiles/val_batched_bench.jsonl]

For 21 classes / T = 45 text rows and 81 classes / T = 103: a seeded ViT-B/16-shaped tower (tools/synthetic.make_vit_state_dict), the
seeded head of model/init_head.init_decoder_state_dict at the crop size, and an on-disk VOC-format tree of N VOC-sized JPEG / PNG pairs
(tools/synthetic.write_voc_tree: 500 x 375 and the other VOC sizes).  Each path runs a 16-image warm-up, then --repeats timed passes over
the N images, the two paths alternating (decode included: the per-image loop decodes on the calling thread, as train() runs it; the
batched pass uses the config's decode threads, the training programs' --num_workers default: 8 for VOC, 4 for COCO).  One JSON line per
pass: img/s, seconds, peak device memory; the last line of a config says whether both paths' confusion matrices are equal."""
import argparse
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402


class _Head:
    """The first k samples of a data set (warm-up)."""

    def __init__(self, ds, k):
        self.ds, self.k = ds, min(k, len(ds))

    def __len__(self):
        return self.k

    def __getitem__(self, i):
        return self.ds[i]

    def max_k(self):
        return self.ds.max_k()


def _model(nc, T, S):
    from excel_amd.model import ExCEL_model
    from excel_amd.model.init_head import init_decoder_state_dict
    from excel_amd.tools import synthetic
    return ExCEL_model(clip_model="ExCEL_ViT-B/16", num_classes=nc, img_size=S, mode="train", state_dict=synthetic.make_vit_state_dict(seed=0),
                       text_features=synthetic.make_text_features(T), embedding_dim=256, in_channels=768,
                       decoder_state_dict=init_decoder_state_dict(num_classes=nc, crop_size=S, seed=0))


def _per_image(model, ds, nc, S):
    from excel_amd.engine import validatation_engine as ve
    from excel_amd.scripts.train_voc import _val_batches
    from excel_amd.utils import evaluate
    from excel_amd.utils.PAR import PAR
    hists = []
    orig = evaluate.scores_from_hist

    def keep(h):
        hists.append(h.clone())
        return orig(h)
    evaluate.scores_from_hist = keep
    try:
        torch.cuda.synchronize()
        t0 = time.time()
        ve.build_validation(model=model, par=PAR(num_iter=20, dilations=[1, 2, 4, 8, 12, 24]), val_loader=_val_batches(ds, "cuda"),
                            device="cuda", num_classes=nc, resize_size=S)
        torch.cuda.synchronize()
        secs = time.time() - t0
    finally:
        evaluate.scores_from_hist = orig
    return secs, hists[0], hists[1]


def _batched(model, ds, nc, S, bs, workers):
    from excel_amd.engine import validatation_engine as ve
    from excel_amd.utils.PAR import PAR
    torch.cuda.synchronize()
    t0 = time.time()
    out = ve.build_validation_ragged(model=model, par=PAR(num_iter=20, dilations=[1, 2, 4, 8, 12, 24]), dataset=ds, device="cuda",
                                     num_classes=nc, resize_size=S, batch_size=bs, num_workers=workers, rank=0, world=1)[3]
    torch.cuda.synchronize()
    return time.time() - t0, out["hist_aff"], out["hist_seg"]


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--n", type=int, default=1024)
    p.add_argument("--batch_size", type=int, default=16)
    p.add_argument("--resize_size", type=int, default=320)
    p.add_argument("--repeats", type=int, default=2)
    p.add_argument("--configs", default="21:45:8,81:103:4,81:103:8", help="num_classes:T:decode threads of the batched pass")
    p.add_argument("--out", default=os.path.join(ROOT, "profiles", "val_batched_bench.jsonl"))
    a = p.parse_args()
    from excel_amd import build
    from excel_amd.datasets import voc
    from excel_amd.tools import synthetic
    S = a.resize_size
    recs = []
    with tempfile.TemporaryDirectory() as tmp:
        for cfg in a.configs.split(","):
            nc, T, workers = (int(v) for v in cfg.split(":"))
            root, lists = os.path.join(tmp, f"voc{nc}"), os.path.join(tmp, f"lists{nc}")
            if not os.path.isdir(root):
                synthetic.write_voc_tree(root, lists, a.n, seed=1234, split="val", num_classes=nc)
            ds = voc.VOC12SegDataset(root_dir=root, name_list_dir=lists, split="val", stage="val")
            model = _model(nc, T, S)
            _per_image(model, _Head(ds, 16), nc, S)                                        # warm-up
            _batched(model, _Head(ds, 16), nc, S, a.batch_size, workers)
            got = {}
            for rep in range(a.repeats):
                for mode in ("per_image", "batched"):
                    torch.cuda.reset_peak_memory_stats()
                    if mode == "per_image":
                        got[mode] = _per_image(model, ds, nc, S)
                    else:
                        got[mode] = _batched(model, ds, nc, S, a.batch_size, workers)
                    secs = got[mode][0]
                    recs.append(dict(mode=mode, rep=rep, num_classes=nc, text_rows=T, images=a.n, resize_size=S,
                                     batch_size=1 if mode == "per_image" else a.batch_size,
                                     decode_threads=0 if mode == "per_image" else workers, seconds=round(secs, 3),
                                     img_per_s=round(a.n / secs, 2), peak_mem_gib=round(torch.cuda.max_memory_allocated() / 2 ** 30, 3),
                                     gemm_mode=model.encoder.visual.handle().gemm_mode(), build_id=build.source_id(),
                                     device=torch.cuda.get_device_name(0)))
                    print(json.dumps(recs[-1]), flush=True)
            same = bool(torch.equal(got["per_image"][1], got["batched"][1]) and torch.equal(got["per_image"][2], got["batched"][2]))
            recs[-1]["hists_equal_per_image"] = same
            recs[-1]["speedup"] = round(got["per_image"][0] / got["batched"][0], 2)
            print(json.dumps({"num_classes": nc, "decode_threads": workers, "hists_equal": same, "speedup": recs[-1]["speedup"]}), flush=True)
            del model
            torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "a") as f:
        for rec in recs:
            f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
