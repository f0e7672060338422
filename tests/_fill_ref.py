"""The judge of the nearest-label fill tests (test infrastructure only) and their case table.

nearest(label, num_classes, mask) is the definition read aloud: for every hole, the squared distances to ALL seeds of the map, and the
first seed, in raster order, that attains their minimum (np.nonzero lists the seeds in raster order and np.argmin returns the first
minimum).  No separable passes, no packed keys: it shares no code with excel_amd/utils/label_fill.py nor with the kernels.  fill() applies
the radius to that answer and restates the contract of include/excel_hip.h ("nearest-label fill") for out, dist2 and counts."""
import numpy as np

T = 256                                            # utils.label_fill.FILL_ROW_THREADS; the tests check that it still is
NC = 21


def nearest(label, num_classes=NC, mask=None):
    """-> (hole bool [H,W], d2 int64 [H,W] (-1 where there is no hole or no seed), value uint8 [H,W] of the nearest seed)"""
    lab = np.asarray(label, np.uint8)
    hole = lab == 255
    if mask is not None:
        hole = hole & (np.asarray(mask) != 255)
    sy, sx = np.nonzero(lab < num_classes)
    d2 = np.full(lab.shape, -1, np.int64)
    value = np.full(lab.shape, 255, np.uint8)
    if len(sy):
        sv = lab[sy, sx]
        for y, x in zip(*np.nonzero(hole)):
            d = (sy - y) ** 2 + (sx - x) ** 2
            k = int(np.argmin(d))
            d2[y, x] = d[k]
            value[y, x] = sv[k]
    return hole, d2, value


def apply_radius(label, near, max_dist2=None, num_classes=NC):
    """-> (out uint8, dist2 int32, counts int64 [3]) from nearest()'s answer: the contract, restated"""
    lab = np.asarray(label, np.uint8)
    hole, d2, value = near
    got = hole & (d2 >= 0)
    if max_dist2 is not None:
        got &= d2 <= max_dist2
    out = lab.copy()
    out[got] = value[got]
    dist2 = np.where(lab < num_classes, 0, -1).astype(np.int32)
    dist2[got] = d2[got]
    return out, dist2, np.asarray([hole.sum(), got.sum(), d2[got].max() if got.any() else 0], np.int64)


def fill(label, num_classes=NC, mask=None, max_dist2=None):
    return apply_radius(label, nearest(label, num_classes, mask), max_dist2, num_classes)


# ------------------------------------------------------------------ sizes (H, W)
# the smallest maps; one row longer than a wave; around the 64 x 16 tile; around the row pass's stride T and beyond two strides, over
# more than two tile rows
SIZES = [(1, 1), (1, 2), (2, 2), (5, 1), (1, 65), (17, 63), (16, 64), (3, T - 1), (2, T), (3, T + 1), (33, 2 * T + 1)]


# ------------------------------------------------------------------ patterns: (H, W) -> uint8 map
def _rs(H, W, salt):
    return np.random.RandomState(H * 1000 + W + salt)


def random21(H, W):
    rs = _rs(H, W, 1)
    m = rs.randint(0, NC, (H, W)).astype(np.uint8)
    m[rs.rand(H, W) < 0.3] = 255
    return m


def sparse_seeds(H, W):
    rs = _rs(H, W, 2)
    m = np.full((H, W), 255, np.uint8)
    s = rs.rand(H, W) < 0.01
    m[s] = rs.randint(0, NC, int(s.sum())).astype(np.uint8)
    return m


def no_seed(H, W):
    return np.full((H, W), 255, np.uint8)


def no_hole(H, W):
    return _rs(H, W, 3).randint(0, NC, (H, W)).astype(np.uint8)


def one_seed_corner(H, W):
    m = np.full((H, W), 255, np.uint8)
    m[H - 1, W - 1] = 5
    return m


def seeds_in_one_column(H, W):
    m = np.full((H, W), 255, np.uint8)
    m[:, W // 2] = _rs(H, W, 4).randint(0, NC, H).astype(np.uint8)
    return m


def seeds_in_one_row(H, W):
    m = np.full((H, W), 255, np.uint8)
    m[H // 2] = _rs(H, W, 5).randint(0, NC, W).astype(np.uint8)
    return m


def passthrough(H, W):
    """Values of 200 between holes and seeds: neither, and they must not block."""
    rs = _rs(H, W, 6)
    m = np.full((H, W), 200, np.uint8)
    r = rs.rand(H, W)
    m[r < 0.35] = 255
    s = r > 0.9
    m[s] = rs.randint(0, NC, int(s.sum())).astype(np.uint8)
    return m


PATTERNS = dict(random21=random21, sparse_seeds=sparse_seeds, no_seed=no_seed, no_hole=no_hole, one_seed_corner=one_seed_corner,
                seeds_in_one_column=seeds_in_one_column, seeds_in_one_row=seeds_in_one_row, passthrough=passthrough)


def mask_of(H, W):
    """About half of the pixels are 255 in the mask: a hole there stays a hole."""
    return np.where(_rs(H, W, 7).rand(H, W) < 0.5, 255, 0).astype(np.uint8)


_JUDGED = {}


def judged(pattern, size, masked=False):
    """(map, mask or None, nearest(map, NC, mask)) of one case, computed once and read-only afterwards."""
    key = (pattern, tuple(size), bool(masked))
    if key not in _JUDGED:
        m = PATTERNS[pattern](*size)
        k = mask_of(*size) if masked else None
        near = nearest(m, NC, k)
        for a in (m, k) + near:
            if a is not None:
                a.setflags(write=False)
        _JUDGED[key] = (m, k, near)
    return _JUDGED[key]


def want(pattern, size, masked=False, max_dist2=None):
    m, k, near = judged(pattern, size, masked)
    return (m, k) + apply_radius(m, near, max_dist2)


# ------------------------------------------------------------------ ties, by hand: (map, hole (y, x), the value it takes, its d2)
def tie_cases():
    out = []
    k = 3
    m = np.full((3, 2 * k + 1), 255, np.uint8)               # one row: seeds k to the left and k to the right -> the left one (smaller x)
    m[1, 0], m[1, 2 * k] = 3, 7
    out.append(("row", m, (1, k), 3, k * k))
    m = np.full((2 * k + 1, 3), 255, np.uint8)               # one column: k above and k below -> the upper one (smaller y)
    m[0, 1], m[2 * k, 1] = 3, 7
    out.append(("column", m, (k, 1), 3, k * k))
    m = np.full((3, 3), 255, np.uint8)                       # (2,0) is in the hole's own row (dx = 2, dy = 0), (0,2) in its own column:
    m[2, 0], m[0, 2] = 3, 7                                  # both at d2 = 4, (0,2) comes first in raster order
    out.append(("row_against_column", m, (2, 2), 7, 4))
    m = np.full((5, 5), 255, np.uint8)
    m[0, 4], m[4, 0] = 7, 3
    out.append(("column_against_row", m, (4, 4), 7, 16))
    return out
