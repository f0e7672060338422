"""The judge of the connected-component tests (test infrastructure only) and their case table.

components(label, connectivity) is the textbook two-pass labelling, pixel by pixel in plain Python: the first pass unites every pixel with
its already visited equal-valued neighbours (left, up; with 8-connectivity up-left and up-right) in a union-find whose smaller index
always becomes the parent, the second pass reads every pixel's root.  The root is then the smallest linear index of the component - its
first pixel in raster order, the canonical label of include/excel_hip.h - and the area is a bincount of the roots.  It shares no code
with excel_amd/utils/components.py (which works on row runs) nor with the kernels (tiles and seams)."""
import numpy as np

TILE = (16, 64)                                    # utils.components.COMPONENTS_TILE; the tests check that it still is
TH, TW = TILE


def components(label, connectivity):
    lab = np.asarray(label)
    H, W = lab.shape
    v = lab.reshape(-1).tolist()
    parent = list(range(H * W))

    def find(x):
        r = x
        while parent[r] != r:
            r = parent[r]
        while parent[x] != r:
            parent[x], x = r, parent[x]
        return r

    def unite(a, b):
        a, b = find(a), find(b)
        if a != b:
            parent[max(a, b)] = min(a, b)
    for y in range(H):
        for x in range(W):
            i = y * W + x
            if x and v[i - 1] == v[i]:
                unite(i, i - 1)
            if y:
                if v[i - W] == v[i]:
                    unite(i, i - W)
                if connectivity == 8:
                    if x and v[i - W - 1] == v[i]:
                        unite(i, i - W - 1)
                    if x + 1 < W and v[i - W + 1] == v[i]:
                        unite(i, i - W + 1)
    comp = np.asarray([find(i) for i in range(H * W)], np.int64)
    area = np.bincount(comp, minlength=H * W)[comp]
    return comp.astype(np.int32).reshape(H, W), area.astype(np.int32).reshape(H, W)


def clean(label, min_area, num_classes, connectivity):
    """-> (cleaned, counts[3]) from the judge's components: the filter's contract restated on them."""
    lab = np.asarray(label, np.uint8)
    comp, area = components(lab, connectivity)
    H, W = lab.shape
    cls = lab < num_classes
    gone = cls & (area < min_area)
    root = comp.reshape(-1) == np.arange(H * W)
    out = lab.copy()
    out[gone] = 255
    return out, np.asarray([(cls.reshape(-1) & root).sum(), (gone.reshape(-1) & root).sum(), gone.sum()], np.int64)


# ------------------------------------------------------------------ sizes
# 1 x 1; one row and one column longer than a tile; every combination of {T-1, T, T+1} per axis; an odd size over more than two tiles
# per axis; exactly 3 x 3 tiles
SIZES = ([(1, 1), (1, TW + 7), (TH + 5, 1)] + [(h, w) for h in (TH - 1, TH, TH + 1) for w in (TW - 1, TW, TW + 1)] +
         [(2 * TH + 3, 2 * TW + 5), (3 * TH, 3 * TW)])


# ------------------------------------------------------------------ patterns: (H, W) -> uint8 map
def constant(H, W):
    return np.full((H, W), 7, np.uint8)


def checkerboard(H, W):
    y, x = np.mgrid[:H, :W]
    return ((y + x) & 1).astype(np.uint8) * 3


def serpentine(H, W):
    """A one-pixel path that runs along every second row and turns at alternating ends: it crosses every vertical seam in every such
    row and every horizontal seam at a turn."""
    m = np.zeros((H, W), np.uint8)
    m[::2] = 1
    for k, y in enumerate(range(1, H, 2)):
        m[y, (W - 1) if k % 2 == 0 else 0] = 1
    return m


def comb(H, W):
    """Teeth in every second column that join only in the last row."""
    m = np.zeros((H, W), np.uint8)
    m[:, ::2] = 5
    m[H - 1] = 5
    return m


def u_shape(H, W):
    """Two arms inside the first tile column that meet only through the tile on the right (or, in a map of one tile column, not at
    all): rows 1 and 3 run from column 2 to the right edge region and are joined by one column there."""
    m = np.zeros((H, W), np.uint8)
    if H < 4 or W < 4:
        return m
    right = min(W - 1, TW + 3)
    m[1, 2:right + 1] = 9
    m[3, 2:right + 1] = 9
    m[1:4, right] = 9
    return m


def corner_diagonals(H, W):
    """Pixels (TH-1, TW-1) and (TH, TW) hold one value, (TH-1, TW) and (TH, TW-1) another: two diagonal pairs through one tile corner,
    joined at 8 and separate at 4 - only the corner rule of the merge sees them.  Smaller maps get the same four pixels at their centre."""
    m = np.zeros((H, W), np.uint8)
    y, x = (TH, TW) if (H > TH and W > TW) else (max(H // 2, 1), max(W // 2, 1))
    if y < H and x < W and y >= 1 and x >= 1:
        m[y - 1, x - 1] = m[y, x] = 11
        m[y - 1, x] = m[y, x - 1] = 12
    return m


def _random(values, with_255=False):
    def make(H, W):
        rs = np.random.RandomState(H * 1000 + W + values)
        m = rs.randint(0, values, (H, W)).astype(np.uint8)
        if with_255:
            m[rs.rand(H, W) < 0.2] = 255
        return m
    return make


def blobs(H, W):
    """A few overlapping discs of different classes on background, plus speckle: what a pseudo-label map looks like."""
    rs = np.random.RandomState(H * 7 + W)
    y, x = np.mgrid[:H, :W]
    m = np.zeros((H, W), np.uint8)
    for k in range(6):
        cy, cx, r = rs.randint(0, H), rs.randint(0, W), rs.randint(2, max(3, min(H, W) // 2 + 2))
        m[(y - cy) ** 2 + (x - cx) ** 2 <= r * r] = 1 + k % 4
    sp = rs.rand(H, W) < 0.03
    m[sp] = rs.randint(0, 6, int(sp.sum())).astype(np.uint8)
    m[rs.rand(H, W) < 0.01] = 255
    return m


PATTERNS = dict(constant=constant, checkerboard=checkerboard, serpentine=serpentine, comb=comb, u_shape=u_shape,
                corner_diagonals=corner_diagonals, random2=_random(2), random21=_random(21), random255=_random(255, with_255=True), blobs=blobs)

_JUDGED = {}


def judged(pattern, size, connectivity):
    """(map, comp, area) of one case, computed once and read-only afterwards."""
    key = (pattern, tuple(size), connectivity)
    if key not in _JUDGED:
        m = PATTERNS[pattern](*size)
        m.setflags(write=False)
        comp, area = components(m, connectivity)
        comp.setflags(write=False)
        area.setflags(write=False)
        _JUDGED[key] = (m, comp, area)
    return _JUDGED[key]
