#!/usr/bin/env python3
"""Mint tests/golden/conf_labels.npz: the reference's own refine_cams_with_bkg_v2 (utils/affutils.py:101-158) on seeded inputs.

Runs only where the reference checkout exists (never on the GPU box, never from tests).  utils/affutils.py and utils/PAR.py are
imported by file path; affutils imports `cv2` at the top, which is absent here and which v2 never calls: a stand-in module that
holds nothing but a version string sits in sys.modules for this run only.  Only arrays are written - no reference source text.

Two uniform cases, (h, w) = (50, 66) and (33, 47): B = 2, F = 5, present counts [3, 1], an img_box that cuts both axes, smooth random
cams in [0, 1], random images, PAR with num_iter = 10, high_thre 0.7, low_thre 0.25, ignore_index 255.  Per case c:
  img_c, cams_c, cls_c, box_c      the inputs
  lab_c, lab_box_c                 v2's labels without / with img_box (uint8)
  planes_c_b, par_c_b              image b's softmaxed half-size planes and PAR outputs, [2 (high, low), k_b + 1, h // 2, w // 2] float32,
                                   from a replay of v2's own sequence of calls step by step - the script asserts that the replay
                                   reproduces v2's labels exactly
  lab64_c, lab64_box_c             the labels of the same replay in float64

The seed: the project's gate for labels is an agreement of >= 0.999 per image (tests/test_gpu_many_classes.py).  The scan below keeps
the first seed at which the reference's own float32 and float64 labels agree at >= 0.9995 in every image of both cases, with and
without the box, so the reference alone stays inside the gate with room.  The scan of the minting run (smallest agreement over the
images of both cases):
  seed 0  min agreement 1.000000  kept

Usage:  python tests/golden/make_conf_golden.py
"""
import importlib.util
import os
import sys
import types

import numpy as np
import torch
import torch.nn.functional as F

REF = "/root/reference"
HERE = os.path.dirname(os.path.abspath(__file__))

CASES = [(50, 66), (33, 47)]
B, NF, COUNTS = 2, 5, (3, 1)
HIGH, LOW, IGNORE, DS, NUM_ITER = 0.7, 0.25, 255, 2, 10
DILATIONS = [1, 2, 4, 8, 12, 24]
GATE = 0.9995

torch.set_num_threads(8)


def _load_by_path(name, path):
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def load_reference():
    stub = importlib.util.find_spec("cv2") is None
    if stub:
        sys.modules["cv2"] = types.ModuleType("cv2")
        sys.modules["cv2"].__version__ = "4.0.0"              # (affutils reads the major version at import; nothing else is touched)
    try:
        aff = _load_by_path("ref_affutils", os.path.join(REF, "utils", "affutils.py"))
    finally:
        if stub:
            del sys.modules["cv2"]
    par = _load_by_path("ref_PAR", os.path.join(REF, "utils", "PAR.py"))
    return aff, par


def make_inputs(seed, h, w):
    g = torch.Generator().manual_seed(1000 * seed + h)
    img = torch.randn(B, 3, h, w, generator=g)
    low = torch.rand(B, NF, 5, 7, generator=g)
    cams = F.interpolate(low, size=(h, w), mode="bicubic", align_corners=False)
    mn, mx = cams.amin((2, 3), keepdim=True), cams.amax((2, 3), keepdim=True)
    cams = ((cams - mn) / (mx - mn)).clamp(0, 1)
    cls = torch.zeros(B, NF)
    for b, k in enumerate(COUNTS):
        cls[b, torch.randperm(NF, generator=g)[:k]] = 1
    box = torch.tensor([[h // 10, h - h // 8, w // 8, w - w // 10], [0, h - h // 5, w // 6, w]], dtype=torch.int64)
    return img, cams, cls, box


def replay(par, images, cams, cls_labels, box, dtype):
    """v2's own sequence of calls (:112-156) one step at a time in `dtype` -> (labels [B,h,w], per image (planes, par) [2,k+1,hh,wh])"""
    images, cams = images.to(dtype), cams.to(dtype)
    b, _, h, w = images.shape
    hh, wh = h // DS, w // DS
    _images = F.interpolate(images, size=[hh, wh], mode="bilinear", align_corners=False)                         # :113
    cls_all = torch.cat((torch.ones(b, 1), cls_labels), dim=1)                                                    # :120-122
    lab_h = torch.ones(b, h, w, dtype=dtype) * IGNORE
    lab_l = lab_h.clone()
    per_image = []
    both = []
    for thre in (HIGH, LOW):
        with_bkg = torch.cat((torch.ones(b, 1, h, w, dtype=dtype) * thre, cams), dim=1)                          # :115-118, :129, :133
        both.append(F.interpolate(with_bkg, size=[hh, wh], mode="bilinear", align_corners=False))                 # :130-136
    for i in range(b):
        valid_key = torch.nonzero(cls_all[i, ...])[:, 0]                                                          # :139
        planes, outs, labs = [], [], []
        for half in both:
            valid = half[i, valid_key, ...].unsqueeze(0).softmax(dim=1)                                           # :140-141
            refined = par(_images[[i], ...], valid)                                                               # :93
            up = F.interpolate(refined, size=(h, w), mode="bilinear", align_corners=False)                        # :94
            labs.append(valid_key[up.argmax(dim=1)])                                                              # :95-96
            planes.append(valid[0])
            outs.append(refined[0])
        if box is not None:
            c = box[i]
            lab_h[i, c[0]:c[1], c[2]:c[3]] = labs[0][0, c[0]:c[1], c[2]:c[3]].to(dtype)                           # :146-149
            lab_l[i, c[0]:c[1], c[2]:c[3]] = labs[1][0, c[0]:c[1], c[2]:c[3]].to(dtype)
        else:
            lab_h[i], lab_l[i] = labs[0][0].to(dtype), labs[1][0].to(dtype)                                       # :151-152
        per_image.append((torch.stack(planes), torch.stack(outs)))
    out = lab_h.clone()                                                                                           # :154-156
    out[lab_h == 0] = IGNORE
    out[(lab_h + lab_l) == 0] = 0
    return out, per_image


def run_seed(aff, par32, par64, seed):
    out, worst = {}, 1.0
    for c, (h, w) in enumerate(CASES):
        img, cams, cls, box = make_inputs(seed, h, w)
        out.update({f"img_{c}": img.numpy(), f"cams_{c}": cams.numpy(), f"cls_{c}": cls.numpy(), f"box_{c}": box.numpy().astype(np.int32)})
        for tag, bx in (("", None), ("_box", box)):
            with torch.no_grad():
                ref = aff.refine_cams_with_bkg_v2(ref_mod=par32, images=img, cams=cams, cls_labels=cls, high_thre=HIGH, low_thre=LOW,
                                                  ignore_index=IGNORE, img_box=bx, down_scale=DS)
                lab32, per_image = replay(par32, img, cams, cls, bx, torch.float32)
                lab64, _ = replay(par64, img, cams, cls, bx, torch.float64)
            assert torch.equal(ref, lab32), "the step-by-step replay must reproduce refine_cams_with_bkg_v2 exactly"
            out[f"lab{tag}_{c}"] = ref.numpy().astype(np.uint8)
            out[f"lab64{tag}_{c}"] = lab64.numpy().astype(np.uint8)
            for b in range(B):
                worst = min(worst, float((lab32[b] == lab64[b].float()).double().mean()))
            if bx is None:
                for b, (planes, outs) in enumerate(per_image):
                    out[f"planes_{c}_{b}"] = planes.numpy()
                    out[f"par_{c}_{b}"] = outs.numpy()
    return out, worst


def main():
    aff, parmod = load_reference()
    par32 = parmod.PAR(num_iter=NUM_ITER, dilations=DILATIONS)
    par64 = parmod.PAR(num_iter=NUM_ITER, dilations=DILATIONS).double()
    par64.pos = par64.pos.double()
    for seed in range(64):
        out, worst = run_seed(aff, par32, par64, seed)
        ok = worst >= GATE
        print(f"  seed {seed}  min agreement {worst:.6f}  {'kept' if ok else 'rejected'}")
        if ok:
            break
    else:
        raise SystemExit("no seed inside the gate")
    out["meta"] = np.array([HIGH, LOW, IGNORE, DS, NUM_ITER, seed], np.float64)
    path = os.path.join(HERE, "conf_labels.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path}: {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
