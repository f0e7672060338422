"""Shared support of tests/test_host_dcrf_filter.py and tests/test_gpu_dcrf_filter.py: one DenseCRF message at a time.

With iters = 1, energies as input and one pairwise weight 1, the other 0, the mean field returns Q = softmax(-U + m), m = the message of
the live kernel on Q0 = softmax(-U), so
    m_k - m_0 = log Q_k - log Q_0 + U_k - U_0
reads the class differences of ONE splat / blur / slice / symmetric normalisation back through the public entry, with no softmax
iterations on top.  The references here:
  filter64 / message64   the value arithmetic of oracle.dcrf.Permutohedral.compute in float64 over the SAME fp32-built lattice (offsets,
                         barycentric weights, neighbours: the rounding decisions of the construction are part of the algorithm)
  exact_message          the dense N x N kernel exp(-|f_i - f_j|^2 / 2) the lattice filter approximates, same normalisation, float64
No torch at module level: the host test imports this too."""
import numpy as np

import oracle.dcrf as odcrf

FLOOR = 2.0 ** -21           # four fp32 roundings at magnitude 1 inside the recovery itself (two log Q, two U)

# (pos_xy_std, bi_xy_std, bi_rgb_std) -> the pairwise weights (pos_w, bi_w) the programs use with them
LAM = (1, 67, 3)             # tools/infer_lam.py and the VOC evaluation
DCRF = (3, 80, 13)           # utils/dcrf.crf_inference
LABEL = (3, 50, 5)           # utils/dcrf.crf_inference_label
LOAD = (1, 67, 1)            # `distinct` only: nearly every vertex its own lattice point
WEIGHTS = {LAM: (3, 4), DCRF: (3, 10), LABEL: (3, 10)}


# ------------------------------------------------------------------ the references
def filter64(lat, values):
    """oracle.dcrf.Permutohedral.compute with float64 values: values [N,C] -> [N,C] float64 (splat, d+1 blur passes, slice)."""
    v = np.asarray(values, np.float64)
    w = lat.bary.astype(np.float64)
    L = np.zeros((lat.M + 1, v.shape[1]), np.float64)            # row 0 = the absent neighbour
    for j in range(lat.d + 1):
        np.add.at(L, lat.offset[:, j] + 1, w[:, j:j + 1] * v)
    for j in range(lat.d + 1):
        new = np.zeros_like(L)
        new[1:] = L[1:] + 0.5 * (L[lat.n1[j] + 1] + L[lat.n2[j] + 1])
        L = new
    alpha = 1.0 / (1.0 + 2.0 ** (-lat.d))
    out = np.zeros_like(v)
    for j in range(lat.d + 1):
        out += w[:, j:j + 1] * L[lat.offset[:, j] + 1] * alpha
    return out


def message64(feature, Q0, lat=None):
    """norm * K(norm * Q0), norm = 1 / sqrt(K 1 + 1e-20), K = filter64 on the lattice of `feature` [N,d] (or on `lat`).  Q0 [N,C]."""
    if lat is None:
        lat = odcrf.Permutohedral(feature)
    norm = 1.0 / np.sqrt(filter64(lat, np.ones((lat.N, 1)))[:, 0] + 1e-20)
    return norm[:, None] * filter64(lat, np.asarray(Q0, np.float64) * norm[:, None])


def exact_message(feature, Q0):
    """The same with the dense kernel K_ij = exp(-|f_i - f_j|^2 / 2), diagonal included."""
    f = np.asarray(feature, np.float64)
    d2 = ((f[:, None, :] - f[None, :, :]) ** 2).sum(-1)
    K = np.exp(-0.5 * d2)
    norm = 1.0 / np.sqrt(K.sum(1) + 1e-20)
    return norm[:, None] * (K @ (np.asarray(Q0, np.float64) * norm[:, None]))


def recover(Q, U):
    """Q, U [C, ...] -> log Q_k - log Q_0 + U_k - U_0 for k >= 1, float64 [C-1, ...]."""
    lq, u = np.log(np.asarray(Q).astype(np.float64)), np.asarray(U).astype(np.float64)
    return lq[1:] - lq[:1] + u[1:] - u[:1]


def softmax64(U):
    """U [C,N] -> softmax(-U) [N,C] in float64."""
    t = -np.asarray(U, np.float64).T
    e = np.exp(t - t.max(1, keepdims=True))
    return e / e.sum(1, keepdims=True)


def differences(m):
    """message [N,C] -> its class differences in the layout of recover: [C-1, N]."""
    return (m[:, 1:] - m[:, :1]).T


def rel(a, b):
    """|a - b| / |b| (Frobenius)."""
    return float(np.linalg.norm(a - b) / np.linalg.norm(b))


# ------------------------------------------------------------------ images, energies, cases
def _noise_half(rs, H, W):
    img = (rs.rand(H, W, 3) * 255).astype(np.uint8)
    img[:, : W // 2] = (img[:, : W // 2] * 0.15 + 140).astype(np.uint8)
    return img


def _smooth(rs, H, W):
    y, x = np.mgrid[0:H, 0:W].astype(np.float64)
    base = np.stack([110 + 60 * np.sin(0.21 * x + 0.13 * y + c) + 25 * np.cos(0.17 * y - 0.05 * x + 2 * c) for c in range(3)], -1)
    base[:, W // 2:] += 50
    return (base + rs.randint(-4, 5, (H, W, 3))).clip(0, 255).astype(np.uint8)


def _uniform(rs, H, W):
    return np.full((H, W, 3), 128, np.uint8)


def _extremes(rs, H, W):
    y, x = np.mgrid[0:H, 0:W]
    return np.repeat((((y // 3 + x // 3) & 1) * 255).astype(np.uint8)[..., None], 3, -1)


def _distinct(rs, H, W):
    """Random colours, no two pixels alike, spread over the whole cube."""
    codes = np.unique(rs.randint(0, 1 << 24, 2 * H * W))           # sorted and distinct; shuffled below
    codes = rs.permutation(codes)[:H * W]
    return np.stack([codes >> 16, (codes >> 8) & 255, codes & 255], -1).astype(np.uint8).reshape(H, W, 3)


IMAGES = dict(noise_half=_noise_half, smooth=_smooth, uniform=_uniform, extremes=_extremes, distinct=_distinct)


def image(kind, H, W, seed):
    return np.ascontiguousarray(IMAGES[kind](np.random.RandomState(seed), H, W))


def energies(C, H, W, seed):
    """U uniform in [0,3], fp32 [C,H,W]."""
    return (np.random.RandomState(seed + 1000).rand(C, H, W) * 3).astype(np.float32)


class Case:
    def __init__(self, kind, H, W, C, params, seed):
        self.kind, self.H, self.W, self.C, self.params, self.seed = kind, H, W, C, tuple(params), seed
        self.id = f"{kind}-{H}x{W}-C{C}-" + "_".join(str(p) for p in params)

    @property
    def N(self):
        return self.H * self.W

    def image(self):
        return image(self.kind, self.H, self.W, self.seed)

    def energies(self):
        return energies(self.C, self.H, self.W, self.seed)


# Every image kind with at least two parameter sets, every degenerate shape with LAM and DCRF; 20 cases, not the full product.
CASES = [
    Case("noise_half", 24, 30, 3, LAM, 1), Case("noise_half", 37, 29, 5, LABEL, 2),
    Case("smooth", 24, 30, 3, DCRF, 3), Case("smooth", 37, 29, 5, DCRF, 4), Case("distinct", 24, 30, 3, LAM, 5),
    Case("uniform", 24, 30, 3, LAM, 6), Case("uniform", 37, 29, 5, LABEL, 7),
    Case("extremes", 24, 30, 3, DCRF, 8), Case("extremes", 37, 29, 5, LAM, 9),
    Case("distinct", 24, 30, 3, LOAD, 10), Case("distinct", 37, 29, 5, LABEL, 11),
    Case("smooth", 80, 72, 21, LAM, 12),                       # 9 N C > 4096 * 256: the grid-stride splat and blur kernels go round twice
    Case("extremes", 2, 2, 2, LAM, 13), Case("distinct", 2, 2, 2, DCRF, 14),
    Case("uniform", 1, 1, 3, LAM, 15), Case("noise_half", 1, 1, 3, DCRF, 16),
    Case("noise_half", 1, 40, 2, LAM, 17), Case("smooth", 1, 40, 2, DCRF, 18),
    Case("smooth", 33, 1, 4, LAM, 19), Case("noise_half", 33, 1, 4, DCRF, 20),
]
SINGLE_CLASS = Case("smooth", 6, 6, 1, LAM, 21)                 # C = 1: no differences to recover, Q must be 1
HASH_STRESS = CASES[9]
BOTH = [CASES[0], CASES[2], CASES[1]]                           # both messages together, production weights (one case per set)
# The exact anchor: the smooth and noise_half images of at most 1200 pixels (one pixel has nothing to approximate: every filter returns
# Q0).  Which parameter set goes with which of these images is chosen for the anchor, see test_host_dcrf_filter.test_exact_anchor.
ANCHOR = [c for c in CASES if c.kind in ("smooth", "noise_half") and 1 < c.N <= 1200]
DEGENERATE = [c for c in CASES if min(c.H, c.W) <= 2] + [SINGLE_CLASS]
KERNELS = ("gauss", "bilateral")


def features(kernel, img, params, scale=1.0):
    """Feature vectors of one kernel at `scale` times the standard deviations."""
    H, W = img.shape[:2]
    sxy, bxy, brgb = params
    if kernel == "gauss":
        return odcrf.features_2d(H, W, sxy * scale)
    return odcrf.features_2d(H, W, bxy * scale, img, brgb * scale)


# ------------------------------------------------------------------ the reference side of one (image, energies, parameter set)
class Reference:
    """Everything the tests need from the CPU for one image: per kernel the float64 differences, the fp32 oracle's Q at iters = 1 and
    its recovery error, and (on demand) the exact kernel's differences.  U [C,H,W] is what the recovery uses: the fp32 energies, or
    -log clip(p) in float64 when the entry is fed probabilities `prob` (the oracle then takes its own fp32 unary_from_softmax)."""

    def __init__(self, img, params, U=None, prob=None):
        self.img, self.params = img, tuple(params)
        H, W = img.shape[:2]
        if prob is not None:
            U = -np.log(np.clip(np.asarray(prob, np.float32).astype(np.float64), 1e-5, 1.0))
            self.U32 = odcrf.unary_from_softmax(prob)
        else:
            self.U32 = np.asarray(U, np.float32).reshape(U.shape[0], -1)
        self.U = np.asarray(U).reshape(U.shape[0], H * W)
        self.C = self.U.shape[0]
        self.Q0 = softmax64(self.U)
        self.kern = {k: odcrf.DenseKernel(features(k, img, params)) for k in KERNELS}
        self.m64 = {k: message64(None, self.Q0, self.kern[k].lat) for k in KERNELS}
        self.d64 = {k: differences(self.m64[k]) for k in KERNELS}
        self._oracle, self._exact = {}, {}

    def oracle_q(self, wg, wb):
        """The body of oracle.dcrf.dense_crf_2d at iters = 1 on the kernels built here -> Q [C,N] fp32."""
        key = (wg, wb)
        if key not in self._oracle:
            Un = self.U32.T
            Q = odcrf._softmax_rows(-Un)
            tmp = -Un + np.float32(wg) * self.kern["gauss"].apply(Q) + np.float32(wb) * self.kern["bilateral"].apply(Q)
            self._oracle[key] = odcrf._softmax_rows(tmp).T
        return self._oracle[key]

    def expected(self, wg, wb):
        return wg * self.d64["gauss"] + wb * self.d64["bilateral"]

    def error(self, Q, wg, wb):
        """max |recover(Q, U) - the float64 differences| of a Q [C, N or H,W]."""
        return float(np.abs(recover(np.asarray(Q).reshape(self.C, -1), self.U) - self.expected(wg, wb)).max())

    def oracle_error(self, wg, wb):
        return self.error(self.oracle_q(wg, wb), wg, wb)

    def bound(self, wg, wb):
        """What the device may differ by: 4 x the fp32 oracle's own error on this case (the device sums in another order: fixed-point
        splat, per-vertex products rounded separately), never below FLOOR."""
        return max(4.0 * self.oracle_error(wg, wb), FLOOR)

    def exact(self, kernel):
        if kernel not in self._exact:
            self._exact[kernel] = differences(exact_message(features(kernel, self.img, self.params), self.Q0))
        return self._exact[kernel]


_REFS = {}


def reference(case):
    """The Reference of a case, computed once and shared."""
    if case.id not in _REFS:
        _REFS[case.id] = Reference(case.image(), case.params, U=case.energies())
    return _REFS[case.id]


ONE_OF = {"gauss": (1.0, 0.0), "bilateral": (0.0, 1.0)}          # (w_g, w_b) that leave one kernel alive
