"""The judge of the boundary-score tests and their shared case table.

judge_counts restates the original Boundary IoU code literally, class by class: mask_to_boundary pads the binary mask with one ring of
zeros, erodes it `d` times with a 3x3 kernel (a pixel survives iff all nine pixels around it are set), cuts the ring off and subtracts
the result from the mask.  It never looks at a (2d+1) window or a run length, so it shares no idea with the kernel or with
utils/image_scores.boundary_counts_numpy.  Counting follows the confusion kernels: a pixel counts iff gt < nc and pred < nc.
"""
import numpy as np


def erode3(mask):
    """One 3x3 erosion of a boolean [h,w] array, border treated as set-less: the output ring is False."""
    out = np.zeros_like(mask)
    if mask.shape[0] < 3 or mask.shape[1] < 3:
        return out
    acc = np.ones((mask.shape[0] - 2, mask.shape[1] - 2), bool)
    for dy in range(3):
        for dx in range(3):
            acc &= mask[dy:dy + acc.shape[0], dx:dx + acc.shape[1]]
    out[1:-1, 1:-1] = acc
    return out


def mask_to_boundary(mask, d):
    """mask - erode(pad(mask, 1, 0), 3x3, iterations=d)[1:-1, 1:-1] for a boolean [H,W] mask."""
    er = np.pad(mask.astype(bool), 1, constant_values=False)
    for _ in range(int(d)):
        if not er.any():
            break
        er = erode3(er)
    return mask.astype(bool) & ~er[1:-1, 1:-1]


def judge_counts(gt, pred, nc, d):
    """int64 [3,nc] of one image: rows as ops.boundary_scores writes them."""
    gt, pred = np.asarray(gt), np.asarray(pred)
    valid = (gt < nc) & (pred < nc)
    out = np.zeros((3, nc), np.int64)
    for c in range(nc):
        mg, mp = gt == c, pred == c
        if not mg.any() and not mp.any():
            continue
        bg, bp = mask_to_boundary(mg, d) & valid, mask_to_boundary(mp, d) & valid
        out[0, c], out[1, c], out[2, c] = bg.sum(), bp.sum(), (bg & bp).sum()
    return out


def judge_band(m, c, d):
    """(band pixels, area) of class c in the raw map m - for the non-vacuity check"""
    mask = np.asarray(m) == c
    return int(mask_to_boundary(mask, d).sum()), int(mask.sum())


def block_maps(h, w, nc, d, seed):
    """A block-structured ground truth and a prediction that is the ground truth shifted and perturbed: blocks of side > 2d+1 where the
    image allows (so bands and interiors both exist), 255 pixels and values in [nc, 255) in the ground truth, a 255 and a wrong block
    in the prediction.  Labels are drawn from min(nc, 5) classes so that every class has area."""
    rs = np.random.RandomState(seed)
    side = max(1, min(2 * d + 3, max(h, w) // 2 if max(h, w) > 1 else 1))
    k = min(nc, 5)
    by, bx = -(-h // side) + 1, -(-w // side) + 1
    blocks = rs.randint(0, k, (by, bx))
    if k > 1:                                              # neighbours differ, so every block edge is a contour
        blocks = (blocks + np.add.outer(np.arange(by), np.arange(bx))) % k
    oy, ox = rs.randint(0, side), rs.randint(0, side)
    big = np.kron(blocks, np.ones((side, side), np.int64))
    gt = big[oy:oy + h, ox:ox + w].astype(np.uint8)
    sy, sx = (1 if h > 2 else 0), (2 if w > 3 else 0)
    pred = np.roll(gt, (sy, sx), (0, 1)).copy()
    n = h * w
    flat_p, flat_g = pred.reshape(-1), gt.copy().reshape(-1)
    if n >= 8:
        idx = rs.choice(n, 6, replace=False)
        flat_p[idx[0]] = 255
        flat_p[idx[1]] = (flat_p[idx[1]] + 1) % k
        flat_g[idx[2]] = 255
        flat_g[idx[3]] = 255
        if nc < 255:
            flat_g[idx[4]] = nc + (int(idx[4]) % (255 - nc))
            flat_p[idx[5]] = nc
    return flat_g.reshape(h, w), flat_p.reshape(h, w)


def sizes(TH, TW):
    return [(1, 1), (1, TW + 1), (TH + 1, 1), (TH - 1, TW - 1), (TH, TW), (TH + 1, TW + 1), (2 * TH + 3, 2 * TW + 5)]


def radii(TH, TW, rmax):
    return sorted({1, 2, TH - 1, TH, TH + 1, TW + 1, rmax})


TILE = (16, 64)                                    # ops.BOUNDARY_TILE; test_gpu_boundary_scores checks that it still is
MAX_RADIUS = 72                                    # ops.boundary_max_radius(), likewise


def case_table(TH=TILE[0], TW=TILE[1], rmax=MAX_RADIUS, ncs=(1, 21, 256)):
    """[(name, h, w, nc, d, seed)]: every size at every radius with nc = 21, and every size at radii 2 and TH+1 with nc = 1 and 256."""
    out = []
    for i, (h, w) in enumerate(sizes(TH, TW)):
        for d in radii(TH, TW, rmax):
            for nc in ncs:
                if nc != 21 and d not in (2, TH + 1):
                    continue
                out.append((f"{h}x{w}-d{d}-nc{nc}", h, w, nc, d, 1000 * i + d))
    return out


_cache = {}


def case(h, w, nc, d, seed):
    """-> (gt, pred, judge counts), computed once per case and shared (read-only) by the tests"""
    key = (h, w, nc, d, seed)
    if key not in _cache:
        g, p = block_maps(h, w, nc, d, seed)
        ref = judge_counts(g, p, nc, d)
        for a in (g, p, ref):
            a.setflags(write=False)
        _cache[key] = (g, p, ref)
    return _cache[key]
