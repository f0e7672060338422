#!/usr/bin/env python3
"""Mint tests/golden/workspace_bytes.txt: what every workspace-size query of the library returns, as it stood BEFORE each op's
workspace became one layout description shared by the query and the launch.  Run it at the commit whose totals are the contract.

Each line is `query arg ... : bytes` (tests/_workspace_queries.py explains the arguments).  Per query: a row where every rounded
term is already a multiple of 256 bytes, rows where none is (B = 1, odd H, W, P, C and T not multiples of 4), the shape the
programs run (ViT-B/16 at 448: P = 784, N = 785, C = 512; 21 VOC planes; six PAR dilations), and the rows that walk a query's own
branches: every ndil for PAR, Smax 1 and 18 for the random walk, T on both sides of the narrow / wide CAM kernels, pixel counts on
both sides of a hash-capacity doubling for DenseCRF (cap = the first power of two >= 2 N (D + 1) from 1024: N = 170 | 171 for
D = 2, 85 | 86 for D = 5), mixed class counts for the LAM groups, B in {1, 2} x g in {2, 14, 32} for the three handles.

Usage:  python tests/golden/make_workspace_golden.py          the host queries (no GPU needed); keeps the ViT rows of the file
        python tests/golden/make_workspace_golden.py --gpu    the ViT rows (excel_vit_create needs a device); keeps the others
"""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from _workspace_queries import GOLDEN, VIT_QUERY, query_bytes, read_rows  # noqa: E402

DEC_TINY, DEC_ODD, DEC_VOC = (2, 128, 64, 1, 2, 5), (3, 132, 36, 2, 3, 7), (12, 768, 256, 3, 8, 21)
TEXT_TINY, TEXT_CLIP = (100, 9, 64, 2, 2, 32), (49408, 77, 512, 12, 8, 512)
VIT_TINY = (128, 2, 2, 16, 64)


def host_rows():
    r = []
    add = lambda q, *a: r.append((q, tuple(a)))
    for nd in range(1, 9):
        for cmax in (1, 5, 21):
            add("excel_par_workspace_bytes", 1, cmax, 17, 19, nd)
            add("excel_par_workspace_bytes", 2, cmax, 16, 16, nd)
    for a in ((2, 5, 96, 96, 6), (16, 21, 448, 448, 6), (8, 19, 224, 224, 6)):
        add("excel_par_workspace_bytes", *a)
    for a in ((4096, 4), (12345, 7), (323, 1), (8 * 448 * 448, 21), (16 * 224 * 224, 19)):
        add("excel_par_ragged_workspace_bytes", *a)
    for a in ((1, 64), (1, 49), (3, 196), (8, 784)):
        add("excel_trans_mat_workspace_bytes", *a)
    for a in ((1, 64, 1), (1, 49, 1), (1, 49, 18), (2, 196, 4), (8, 784, 1), (8, 784, 18)):
        add("excel_refine_workspace_bytes", *a)
    for a in ((1, 64, 4), (1, 197, 21), (1, 5, 129), (8, 785, 21), (8, 785, 81)):
        add("excel_cam_workspace_bytes", *a)
    for a in ((1, 64, 256, 128), (1, 197, 64, 21), (1, 197, 64, 129), (1, 5, 32, 1), (2, 785, 512, 512), (8, 785, 512, 21), (8, 785, 512, 81)):
        add("excel_patch_text_cam_workspace_bytes", *a)
    for a in ((1, 4, 16, 16), (1, 21, 17, 19), (1, 2, 1, 1), (8, 21, 448, 448), (4, 81, 448, 448)):
        add("excel_train_losses_workspace_bytes", *a)
    for a in ((1, 4, 64), (1, 5, 49), (3, 7, 197), (8, 256, 784)):
        add("excel_feature_affinity_workspace_bytes", *a)
    for a in ((64, 4, 64, 1), (6, 5, 49, 2), (1, 5, 49, 1), (16, 256, 784, 2), (16, 256, 784, 8), (4, 8, 16, 0)):
        add("excel_feature_affinity_grouped_workspace_bytes", *a)
    for a in ((8, 7), (1, 3), (1, 1), (8, 6), (16, 12)):
        add("excel_attn_select_workspace_bytes", *a)
    for a in ((8, 8, 4), (17, 19, 5), (1, 170, 3), (1, 171, 3), (5, 17, 2), (2, 43, 2), (1, 1, 1), (366, 500, 21), (448, 448, 21), (640, 480, 81)):
        add("excel_dcrf_workspace_bytes", *a)
    for a in ((64, 4), (323, 5), (170, 3), (171, 2), (85, 21), (86, 1), (4 * 366 * 500, 21), (16 * 448 * 448, 2)):
        add("excel_dcrf_ragged_workspace_bytes", *a)
    for imgs in ([(8, 8, 4)], [(17, 19, 3), (8, 8, 1)], [(10, 17, 2)], [(9, 19, 4)], [(5, 17, 2)], [(2, 43, 3)], [(7, 7, 1), (6, 6, 5), (1, 1, 2)],
                 [(366, 500, 4), (375, 500, 2), (333, 500, 7)], [(448, 448, 21)] * 4 + [(448, 448, 2)] * 4):
        add("excel_dcrf_lam_ragged_workspace_bytes", len(imgs), *[v for im in imgs for v in im])
    for B in (1, 2):
        for g in (2, 14, 32):
            for cfg in (DEC_TINY, DEC_ODD, DEC_VOC):
                add("excel_decoder_workspace_bytes", *cfg, B, g)
                add("excel_decoder_train_workspace_bytes", *cfg, B, g)
        for cfg in (TEXT_TINY, TEXT_CLIP):
            add("excel_text_workspace_bytes", *cfg, B)
    for g in (3, 7, 28):                                         # odd token counts (inference only) and the programs' 448 / 16
        add("excel_decoder_workspace_bytes", *DEC_VOC, 1, g)
    add("excel_decoder_workspace_bytes", *DEC_VOC, 8, 28)
    add("excel_decoder_train_workspace_bytes", *DEC_VOC, 8, 28)
    add("excel_text_workspace_bytes", *TEXT_CLIP, 85)
    return r


def gpu_rows():
    return [(VIT_QUERY, VIT_TINY + bs) for bs in ((1, 32), (2, 48), (1, 224))]     # N = 5, 10, 197: both the NP and the KP rounding


def main():
    gpu = "--gpu" in sys.argv
    kept = [row for row in (read_rows() if os.path.exists(GOLDEN) else []) if (row[0] == VIT_QUERY) != gpu]
    new = [(q, a, query_bytes(q, a)) for q, a in (gpu_rows() if gpu else host_rows())]
    rows = (kept + new) if gpu else (new + kept)
    with open(GOLDEN, "w") as f:
        f.write("# query arg ... : bytes   (tests/golden/make_workspace_golden.py; arguments: tests/_workspace_queries.py)\n")
        for q, a, n in rows:
            f.write(f"{q} {' '.join(map(str, a))} : {n}\n")
    print(f"wrote {GOLDEN}: {len(rows)} rows ({len(new)} new)")


if __name__ == "__main__":
    main()
