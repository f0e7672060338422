"""The judge of the superpixel snap: both device entries (include/excel_hip.h, "superpixel snap") restated as plain loops over pixels and
centres, straight from the definitions - no numpy arithmetic beyond holding the arrays, nothing imported from excel_amd.  Slow and
obvious on purpose; the case tables of tests/test_host_snap.py and tests/test_gpu_snap.py live here too, and every answer is computed
once per process."""
import functools

import numpy as np

NC = 21


# ------------------------------------------------------------------ the two entries, by the book
def slic(image, S, m, T):
    """[H,W,3] uint8 -> (sp int32 [H,W], centres int32 [gy*gx,5], emptied): emptied = the (iteration, k) pairs at which centre k had
    no pixel in an update and kept its values."""
    H, W = image.shape[:2]
    img = image.astype(np.int64).tolist()
    gx, gy = -(-W // S), -(-H // S)
    cen = []
    for cy in range(gy):
        for cx in range(gx):
            x, y = min(W - 1, cx * S + S // 2), min(H - 1, cy * S + S // 2)
            cen.append([x, y] + img[y][x])

    def assign():
        sp = [[-1] * W for _ in range(H)]
        for y in range(H):
            for x in range(W):
                r, g, b = img[y][x]
                best, bk = None, -1
                for cy in range(y // S - 1, y // S + 2):
                    for cx in range(x // S - 1, x // S + 2):
                        if not (0 <= cy < gy and 0 <= cx < gx):
                            continue
                        k = cy * gx + cx
                        xk, yk, rk, gk, bk_ = cen[k]
                        D = S * S * ((r - rk) ** 2 + (g - gk) ** 2 + (b - bk_) ** 2) + m * m * ((x - xk) ** 2 + (y - yk) ** 2)
                        assert D < 2 ** 31
                        if best is None or D < best or (D == best and k < bk):
                            best, bk = D, k
                sp[y][x] = bk
        return sp

    emptied = []
    for it in range(T):
        sp = assign()
        sums = [[0] * 6 for _ in cen]
        for y in range(H):
            for x in range(W):
                s = sums[sp[y][x]]
                s[0] += x; s[1] += y; s[2] += img[y][x][0]; s[3] += img[y][x][1]; s[4] += img[y][x][2]; s[5] += 1
        for k, s in enumerate(sums):
            if s[5] == 0:
                emptied.append((it, k))
                continue
            cen[k] = [(2 * s[f] + s[5]) // (2 * s[5]) for f in range(5)]
    return np.asarray(assign(), np.int32).reshape(H, W), np.asarray(cen, np.int32).reshape(-1, 5), emptied


def snap(label, sp, nc, pm):
    """[H,W] uint8 labels and int32 sp -> (out uint8, counts int64 [3]) with min_share_pm = pm."""
    H, W = label.shape
    votes = {}
    for y in range(H):
        for x in range(W):
            k, v = int(sp[y, x]), int(label[y, x])
            if k >= 0 and v < nc:
                votes.setdefault(k, {}).setdefault(v, 0)
                votes[k][v] += 1
    win = {}
    for k, h in votes.items():
        tot, top = sum(h.values()), max(h.values())
        if 1000 * top >= pm * tot:
            win[k] = min(v for v, c in h.items() if c == top)
    out = label.copy()
    changed = 0
    for y in range(H):
        for x in range(W):
            k, v = int(sp[y, x]), int(label[y, x])
            if k in win and v < nc:
                out[y, x] = win[k]
                changed += win[k] != v
    return out, np.asarray([len(votes), len(win), changed], np.int64)


# ------------------------------------------------------------------ images
def blocks(h, w, seed=0):
    """A few flat colours in rectangles, +-12 of noise: edges for the superpixels to find."""
    rs = np.random.RandomState(1000 + 7 * h + w + seed)
    y, x = np.mgrid[:h, :w]
    which = ((x * 3 // max(w, 1)) + 2 * (y * 2 // max(h, 1))) % 5
    pal = rs.randint(30, 226, (5, 3))
    return np.clip(pal[which] + rs.randint(-12, 13, (h, w, 3)), 0, 255).astype(np.uint8)


def constant(h, w, seed=0):
    """One colour: every tie is purely spatial."""
    return np.full((h, w, 3), 97, np.uint8)


def checker(h, w, seed=0):
    """A 0 / 255 checkerboard: colour distances are 0 or the maximum, ties everywhere."""
    y, x = np.mgrid[:h, :w]
    return np.repeat((((x + y) & 1) * 255).astype(np.uint8)[:, :, None], 3, axis=2)


PATTERNS = {"blocks": blocks, "constant": constant, "checker": checker}
# ((H, W), step): 1 x 1; both sides below the step (one centre); W = S + 1 (a sliver cell one pixel wide); (2S+1) x (3S-1); the smallest
# step on 5 x 7; the largest step on 70 x 130 (more than one 64 x 16 tile either way)
SHAPES = (((1, 1), 4), ((3, 5), 8), ((6, 5), 4), ((11, 14), 5), ((5, 7), 2), ((70, 130), 64))
PARAMS = ((0, 1), (0, 64), (5, 1), (5, 64))         # (iters, compactness)


@functools.lru_cache(maxsize=None)
def want_slic(pattern, shape, S, T, m):
    img = PATTERNS[pattern](*shape)
    sp, cen, emptied = slic(img, S, m, T)
    for a in (img, sp, cen):
        a.setflags(write=False)
    return img, sp, cen, emptied


def labels_for(sp, ncent, nc=NC, seed=0):
    """A label map with every kind of vote, laid out by the superpixels of sp (pixels in raster order inside each): k % 8 picks
    0 two classes in exact halves (odd sizes: one pixel of 255 first), the larger value first; 1 all 255; 2 values in [nc, 255) around one
    voting pixel; 3 unanimous; 4 a 2 : 1 majority with the minority value smaller; 5 values in [nc, 255) only; 6 three classes with one
    pixel more for the middle one; 7 random classes and ignore.  nc caps the class values."""
    rs = np.random.RandomState(77 + seed)
    lab = np.full(sp.shape, 255, np.uint8)
    c = lambda v: v % nc
    hi = lambda: int(rs.randint(nc, 255)) if nc < 255 else 255
    for k in range(ncent):
        ys, xs = np.nonzero(sp == k)
        n = len(ys)
        kind, vals = k % 8, []
        if kind == 0:
            vals = [255] * (n & 1) + [c(7 + k)] * (n // 2) + [c(3 + k)] * (n // 2)
        elif kind == 1:
            vals = [255] * n
        elif kind == 2:
            vals = [hi() for _ in range(n)]
            if n:
                vals[n // 2] = c(k)
        elif kind == 3:
            vals = [c(5 + k)] * n
        elif kind == 4:
            vals = [c(9 + k) if i % 3 else c(2 + k) for i in range(n)]
        elif kind == 5:
            vals = [hi() for _ in range(n)]
        elif kind == 6:
            vals = [c(k + (i % 3)) for i in range(n)]
        else:
            vals = [255 if rs.rand() < 0.2 else int(rs.randint(0, nc)) for _ in range(n)]
        lab[ys, xs] = np.asarray(vals, np.uint8) if n else []
    return lab


@functools.lru_cache(maxsize=None)
def want_snap(pattern, shape, S, T, m, nc, pm):
    img, sp, cen, _ = want_slic(pattern, shape, S, T, m)
    lab = labels_for(sp, cen.shape[0], nc)
    out, counts = snap(lab, sp, nc, pm)
    for a in (lab, out, counts):
        a.setflags(write=False)
    return lab, out, counts


# ------------------------------------------------------------------ the effect scene and the empty-centre search
def scene(h=187, w=250, seed=5, shift=3, speckle=0.03, noise=12):
    """Three coloured regions with +-noise, the true labels, and the labels displaced by `shift` pixels with `speckle` random classes."""
    rs = np.random.RandomState(seed)
    y, x = np.mgrid[:h, :w]
    truth = np.zeros((h, w), np.uint8)
    truth[(x - 0.35 * w) ** 2 + (y - 0.5 * h) ** 2 < (0.28 * h) ** 2] = 1
    truth[(x > 0.62 * w) & (y > 0.3 * h)] = 2
    pal = np.asarray([[60, 120, 200], [200, 80, 60], [70, 180, 90]])
    img = np.clip(pal[truth] + rs.randint(-noise, noise + 1, (h, w, 3)), 0, 255).astype(np.uint8)
    noisy = np.roll(np.roll(truth, shift, axis=0), shift, axis=1)
    sp = rs.rand(h, w) < speckle
    noisy[sp] = rs.randint(0, 3, int(sp.sum())).astype(np.uint8)
    return img, truth, noisy


def tiny_image(seed, h=6, w=7, colours=2):
    """A seeded tiny image of a few flat colours, no noise: the search space of the empty-centre rule."""
    rs = np.random.RandomState(seed)
    pal = rs.randint(0, 256, (colours, 3))
    return pal[rs.randint(0, colours, (h, w))].astype(np.uint8)


# What the search of tests/test_host_snap.py found first: at step 3, compactness 1, centre 3 of this image loses all its pixels in the
# second update and keeps its values.
EMPTY_CASE = dict(seed=2, colours=3, S=3, m=1, T=5)
