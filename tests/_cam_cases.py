"""Shared by test_gpu_cam_arms.py (GPU sweep) and test_host_cam_plan.py (selection table, completeness, the reference's and the
comparison's own checks on the CPU): the narrow patch-text CAM's cases, a float64 reference and the comparison functions.  No GPU needed.

Dispatch (cam_plan.hip; excel_patch_text_cam_plan), cdiv(a, b) = ceil(a / b), ct = cdiv(T, 32):

    T > 128                                         -> patch_text_sim_wide_kernel<split>, min / max table of pitch 512
    split modes, T <= 48, C <= 512, C % 256 == 0    -> patch_text_sim_kernel<split, 1 | 2, TLDS>     (ct <= 1 ? 1 : 2)
    split modes otherwise                           -> patch_text_sim_kernel<split, 2 | 4, global>   (ct <= 2 ? 2 : 4)
    f32                                             -> patch_text_sim_kernel<f32, 1 | 2 | 4, global>  (ct <= 1 ? 1 : ct == 2 ? 2 : 4)
    every narrow instance: min / max table of pitch 128

Each split instance is built twice (bf16 and IEEE-half planes: bf16x3 / f16x3).  The wide kernels' cases are CAM_CASES of
test_gpu_wide_vocab.py."""
import numpy as np

MODES = ("f32", "bf16x3", "f16x3")
TOL_FEATURES = 1e-6
TOL_MAPS = {"f32": 2e-5, "bf16x3": 6e-5, "f16x3": 6e-5}           # test_gpu_ops.py::test_patch_text_cam_fused's own bounds
TOL_UNFUSED = 2e-5
TOL_SPLIT = 6e-5                                                  # what a mutant of the reference has to exceed

# (B, N, C, T, F): what each case is the smallest of.  Instances as <class tiles, text source>: split modes | f32
CASES = [
    (2, 37, 256, 20, 20),      # <1,TLDS> | <1>  T <= 32 on a TLDS width; C = 256: one LDS-DMA piece per split row; F = T
    (3, 129, 512, 32, 7),      # <1,TLDS> | <1>  T = 32 fills the class tile; C = 512; N = 129: a second workgroup with three dead waves; B = 3
    (2, 65, 256, 33, 20),      # <2,TLDS> | <2>  first row of the second class tile
    (1, 50, 512, 48, 48),      # <2,TLDS> | <2>  last row that fits the LDS text bank
    (1, 50, 512, 49, 20),      # <2,global> | <2>  first T past the LDS text bank
    (1, 37, 96, 64, 64),       # <2,global> | <2>  three k-blocks (fewer than the prefetch ring); T = 64: two full class tiles
    (1, 33, 768, 45, 20),      # <2,global> | <2>  C above the TLDS width (ViT-L/14 projection width)
    (1, 37, 64, 65, 65),       # <4,global> | <4>  one whole padded class tile; second lane value of the class-prior softmax
    (1, 37, 160, 97, 80),      # <4,global> | <4>  five k-blocks (partial last prefetch group); fourth class tile with one row
    (1, 33, 1024, 128, 128),   # <4,global> | <4>  largest C and largest narrow T
    (1, 513, 64, 9, 4),        # <2,global> | <1>  nine column-norm blocks (second round of the 8-in-flight partial sum); G = 5
    (2, 5, 32, 3, 2),          # <2,global> | <1>  a 2 x 2 grid: one ragged tile, 27 masked token columns
    (1, 17, 32, 1, 1),         # <2,global> | <1>  T = 1: sim is identically 0, every output is NaN (0 / 0), in the reference too
]
DEGENERATE = [c for c in CASES if c[3] == 1]                      # all-NaN cases
TEMP_CASES = [(2, 37, 256, 20, 20), (1, 37, 64, 65, 65)]          # also run at the temperatures below (the default is 2)
TEMPS = (0.5, 20.0)
# Seeds other than N + T + C (test_patch_text_cam_fused's rule).  A kernel that took min / max without the cls token (quirk Q2) can only
# be seen where the cls token holds the min or the max of some class plane.  With seed N + T + C it holds none at these three cases (a
# CPU scan of ref64; every other case has one); each gets the first seed above N + T + C at which it does (test_host_cam_plan.py asserts it).
SEEDS = {(3, 129, 512, 32, 7): 674, (1, 513, 64, 9, 4): 593, (2, 5, 32, 3, 2): 41}
# the cases at which temp = 2.001 instead of 2 moves the maps by more than 1e-4 (measured 1.08e-4 ... 2.9e-4; 4.1e-5 ... 8.6e-5 at the
# others): the only ones where that mutant clears the split-mode bound with room
TEMP_MUTANT_CASES = [(2, 37, 256, 20, 20), (1, 50, 512, 48, 48), (1, 50, 512, 49, 20), (1, 37, 96, 64, 64), (1, 33, 768, 45, 20),
                     (1, 37, 64, 65, 65), (1, 37, 160, 97, 80), (1, 33, 1024, 128, 128), (2, 5, 32, 3, 2)]


def seed_of(case):
    B, N, C, T, F = case
    return SEEDS.get(case, N + T + C)


def build(case):
    """test_patch_text_cam_fused's inputs: columns of x scaled by 1 + 3u (uneven column norms), unit-norm text rows."""
    B, N, C, T, F = case
    rs = np.random.RandomState(seed_of(case))
    x = (rs.standard_normal((B, N, C)) * (1 + rs.rand(1, 1, C) * 3)).astype(np.float32)
    t = rs.standard_normal((T, C)).astype(np.float32)
    t /= np.linalg.norm(t, axis=1, keepdims=True)
    return x, t


def features64(x):
    """clip.py:353: L2 norm over dim=1, the TOKEN axis"""
    x = np.asarray(x, np.float64)
    return x / np.sqrt((x * x).sum(axis=1, keepdims=True))


def _sim64(S, S_cls, temp, red_classes=None):
    """clip.py:295-306 in GEMM form from the similarities S [B,N,T] and the cls token's S_cls [B,1,T] -> un-normalised maps [B,N,T].
    red_classes exists for a mutant below: the redundancy mean summed over the first `red_classes` classes only (still divided by T)."""
    T = S.shape[-1]
    z = temp * S_cls
    e = np.exp(z - z.max(-1, keepdims=True))
    p = e / e.sum(-1, keepdims=True)                                  # :296
    w = p / p.mean(-1, keepdims=True)                                 # :297
    ws = w * S                                                        # :301-302, summed over C
    return ws - ws[..., :red_classes].sum(-1, keepdims=True) / T      # :303-306


def _surgery64(S, S_cls, temp, red_classes=None, first_token=0):
    """... and clip.py:308, min / max over ALL N tokens (quirk Q2; a mutant below takes them from `first_token` on)"""
    sim = _sim64(S, S_cls, temp, red_classes)
    mn, mx = sim[:, first_token:].min(1, keepdims=True), sim[:, first_token:].max(1, keepdims=True)
    with np.errstate(invalid="ignore", divide="ignore"):
        return (sim - mn) / (mx - mn)


def ref64(x, text, temp=2.0):
    """x [B,N,C] un-normalised token features, text [T,C] -> (image_features [B,N,C], attr maps [B,N,T]) in float64: column norms over
    the token axis, S = f @ text.T, w = softmax(temp * S[cls]) / mean, sim = w * S - mean_t(w * S), (sim - min_n) / (max_n - min_n)."""
    f = features64(x)
    S = f @ np.asarray(text, np.float64).T
    return f, _surgery64(S, S[:, :1], temp)


def _round_bf16(a):
    u = np.ascontiguousarray(a, np.float32).view(np.uint32).astype(np.uint64)
    u = (u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFF0000                   # round to nearest even on the upper 16 bits
    return u.astype(np.uint32).view(np.float32).astype(np.float64)


def _round_f16(a):
    return np.asarray(a, np.float32).astype(np.float16).astype(np.float64)


MUTANTS = ("redundancy_drops_last_class", "bf16_lo_plane_lost", "f16_lo_plane_lost", "minmax_without_cls", "temp_2.001")


def mutant64(name, x, text, temp=2.0):
    """ref64's maps with one defect a kernel could have: the comparison has to reject each of them"""
    f = features64(x)
    t = np.asarray(text, np.float64)
    S = f @ t.T
    if name == "redundancy_drops_last_class":
        return _surgery64(S, S[:, :1], temp, red_classes=S.shape[-1] - 1)
    if name in ("bf16_lo_plane_lost", "f16_lo_plane_lost"):           # matrix-core operands as ONE 16-bit value; the class prior keeps its fp32 chain
        rnd = _round_bf16 if name[0] == "b" else _round_f16
        return _surgery64(rnd(f) @ rnd(t).T, S[:, :1], temp)
    if name == "minmax_without_cls":
        return _surgery64(S, S[:, :1], temp, first_token=1)
    if name == "temp_2.001":
        return _surgery64(S, S[:, :1], temp * (2.001 / 2.0))
    raise KeyError(name)


# ---------------------------------------------------------------------------------------------------- the comparison
def max_abs_err(got, ref):
    """max |got - ref| over the positions where the reference is a number (0 when it has none); a NaN of `got` at such a position is inf"""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    m = ~np.isnan(ref)
    if not m.any():
        return 0.0
    d = np.abs(got[m] - ref[m])
    return float("inf") if np.isnan(d).any() else float(d.max())


def same_nan_mask(got, ref):
    return bool(np.array_equal(np.isnan(np.asarray(got)), np.isnan(np.asarray(ref))))


def min_span(x, text, temp=2.0):
    """smallest max_n - min_n of any class plane of the un-normalised similarity (what the final division amplifies errors by)"""
    S = features64(x) @ np.asarray(text, np.float64).T
    sim = _sim64(S, S[:, :1], temp)
    return float((sim.max(1) - sim.min(1)).min())


def cls_is_an_extreme(maps):
    """the cls token holds the min (0) or the max (1) of at least one class plane of at least one image"""
    cls = np.asarray(maps)[:, 0]
    return bool(((cls == 0) | (cls == 1)).any())


_CACHE = {}


def reference(case, temp=2.0):
    """(x, text, features64, maps64) of a case, computed once and read-only"""
    key = (case, float(temp))
    if key not in _CACHE:
        x, t = build(case)
        f, maps = ref64(x, t, temp)
        for a in (x, t, f, maps):
            a.setflags(write=False)
        _CACHE[key] = (x, t, f, maps)
    return _CACHE[key]
