"""Dev: the patch-text CAM kernels alone at the production shape (B=32, N=785, C=512; T=45 is VOC, T=103 COCO, T > 128 the wide kernel),
for a rocprofv3 kernel trace:
   cd /tmp && rocprofv3 --kernel-trace --stats --output-format csv -d out -o cam -- python tools_dev/cam_bench.py
or for comparing two builds (run it from each tree in turn, several times, and compare the medians):
   python tools_dev/cam_bench.py --T 45,103,288 --mode bf16x3,f16x3,f32 --windows 10 --json"""
import argparse, json, sys, os
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np, torch
from excel_amd import ops
ap = argparse.ArgumentParser()
ap.add_argument("--T", default="45", help="text rows, comma separated (foreground classes: 20 at T=45, 80 at T=103, else min(T, 254))")
ap.add_argument("--mode", default="bf16x3", help="bf16x3, f16x3, f32: comma separated")
ap.add_argument("--windows", type=int, default=1, help="timed windows per shape and mode")
ap.add_argument("--calls", type=int, default=50, help="calls per window")
ap.add_argument("--json", action="store_true", help="one JSON line per shape and mode: every window's ms per call and their median")
args = ap.parse_args()
B, N, C = int(os.environ.get("B", 32)), 785, 512
rs = np.random.RandomState(0)
x = torch.from_numpy(rs.standard_normal((B, N, C)).astype(np.float32)).cuda()
for T in [int(v) for v in args.T.split(",")]:
    F = {45: 20, 103: 80}.get(T, min(T, 254))
    t = rs.standard_normal((T, C)).astype(np.float32)
    t = torch.from_numpy(t / np.linalg.norm(t, axis=1, keepdims=True)).cuda()
    for mode in args.mode.split(","):
        for _ in range(5):
            ops.patch_text_cam(x, t, num_fg=F, mode=mode)
        torch.cuda.synchronize()
        ms = []
        for _ in range(args.windows):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(args.calls):
                ops.patch_text_cam(x, t, num_fg=F, mode=mode)
            e1.record()
            torch.cuda.synchronize()
            ms.append(e0.elapsed_time(e1) / args.calls)
        if args.json:
            print(json.dumps({"T": T, "mode": mode, "ms_per_call": [round(v, 5) for v in ms], "median": round(float(np.median(ms)), 5)}), flush=True)
        else:
            print(mode, "T =", T, "ms per call (incl. python + text split + 3 kernels):", float(np.median(ms)))
