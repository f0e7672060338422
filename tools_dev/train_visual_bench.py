"""Cost of the training-progress panels (--save_visual) at the production shape (ViT-B/16 with seeded synthetic weights, crop 320, spg 4,
21 classes).  One JSON line per measurement.

  (a) ms per plain iteration (DecoderTrainer.train_step: what every iteration, and a log iteration without --save_visual, runs)
  (b) ms per log iteration with --save_visual: train_step(want_visual=True) + ops.train_panels + the one device-to-host copy
  (c) the panel launch alone (HIP events), its output bytes and the HBM floor
  (d) the writer thread's side: Pillow PNG encoding of the six grids (off the training thread)

  python tools_dev/train_visual_bench.py [--reps 10]
  rocprofv3 --kernel-trace --stats -d prof -- python tools_dev/train_visual_bench.py --trace 4 1     # 4 plain + 1 visual iteration:
                                                            # train_panels_kernel must show 1 call, the other kernels 5 iterations' worth
"""
import argparse
import io
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from excel_amd import ops  # noqa: E402
from excel_amd.utils import tbutils  # noqa: E402

HBM_GBS = 8000.0          # MI355X HBM3E peak, GB/s


def timed(fn, reps):
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return round(float(np.median(ts)), 3), round(float(np.min(ts)), 3)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--trace", type=int, nargs=2, default=None, metavar=("PLAIN", "VISUAL"),
                    help="run PLAIN plain iterations, then VISUAL rendering ones, and exit (for a kernel trace)")
    args = ap.parse_args()
    from excel_amd.model import ExCEL_model, init_decoder_state_dict
    from excel_amd.scripts.train_voc import DecoderTrainer
    from excel_amd.tools import synthetic
    from excel_amd.utils.PAR import PAR
    S, B = 320, 4
    rng = np.random.default_rng(0)
    model = ExCEL_model(clip_model="ExCEL_ViT-B/16", num_classes=21, img_size=S, mode="train", state_dict=synthetic.make_vit_state_dict(seed=0),
                        text_features=synthetic.make_text_features(45), in_channels=768,
                        decoder_state_dict=init_decoder_state_dict(21, 768, 256, S, seed=0))
    tr = DecoderTrainer(model, PAR(num_iter=20, dilations=[1, 2, 4, 8, 12, 24]))
    x = ops.normalize_img_u8(torch.from_numpy(rng.integers(0, 256, (B, S, S, 3), dtype=np.uint8)).cuda())
    gt = torch.from_numpy(rng.integers(0, 21, (B, S, S), dtype=np.uint8)).cuda()
    cls = torch.zeros(B, 20, device="cuda")
    cls[:, [0, 14]] = 1

    def plain():
        return tr.train_step(x, cls)

    def visual():
        out = tr.train_step(x, cls, want_visual=True)
        return tbutils.render_panels(x, cls, out, seg_gt=gt).host()

    if args.trace:
        for _ in range(args.trace[0]):
            plain()
        for _ in range(args.trace[1]):
            visual()
        torch.cuda.synchronize()
        return
    p_med, p_min = timed(plain, args.reps)
    v_med, v_min = timed(visual, args.reps)
    print(json.dumps({"what": "iteration", "crop_size": S, "spg": B, "plain_ms_median": p_med, "plain_ms_min": p_min,
                      "save_visual_log_iteration_ms_median": v_med, "save_visual_log_iteration_ms_min": v_min}), flush=True)
    out = tr.train_step(x, cls, want_visual=True)
    render = lambda: tbutils.render_panels(x, cls, out, seg_gt=gt)      # noqa: E731
    panels = render()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ks = []
    for _ in range(max(20, args.reps)):
        e0.record()
        render()
        e1.record()
        e1.synchronize()
        ks.append(e0.elapsed_time(e1))
    nbytes = int(panels.buffer.numel())
    read = x.numel() * 4 * 2 + 3 * B * S * S + B * 400 * 20 * 4
    print(json.dumps({"what": "train_panels", "event_ms_median": round(float(np.median(ks)), 4), "event_ms_min": round(float(np.min(ks)), 4),
                      "out_bytes": nbytes, "hbm_floor_ms": round((nbytes + read) / HBM_GBS / 1e6, 5)}), flush=True)
    c_med, c_min = timed(lambda: panels.buffer.cpu(), args.reps)
    host = panels.host()
    from PIL import Image
    ts = []
    for _ in range(3):
        t0 = time.perf_counter()
        for a in host.values():
            Image.fromarray(a).save(io.BytesIO(), format="PNG")
        ts.append((time.perf_counter() - t0) * 1e3)
    print(json.dumps({"what": "host_side", "d2h_copy_ms_median": c_med, "png_encode_six_panels_ms_writer_thread": round(float(np.median(ts)), 2)}), flush=True)


if __name__ == "__main__":
    main()
