"""Shared by test_gpu_par_shapes.py (GPU sweep) and test_host_par_plan.py (the plan, the table's own consistency, the gates' sensitivity,
on the CPU): the dispatch of the pixel-adaptive refinement as a table, a float64 judge, the two guides and the comparison functions.

Dispatch (par_plan.hip; excel_par_plan), cdiv(a, b) = ceil(a / b), standard set = dilations [1, 2, 4, 8, 12, 24]:
    uniform: recompute = standard set, W % 4 == 0, 16-byte aligned buffers, max(Cmax, 5) * H * W * 4 < 2^31, n_iter > 0, no stream flag
        recompute, W >= 8:  par_stats_tile_kernel + par_iterate_guide_kernel, both on (cdiv(W, 64), cdiv(H, 16), B) x 512 threads
        recompute, W == 4:  par_affinity_kernel<6> writing the 5 statistics on (1, cdiv(H, 4), B) x 256 + par_iterate_guide_kernel
        otherwise:          par_affinity_kernel<ndil> writing 8 * ndil planes + par_iterate_stream_kernel, (cdiv(W, 64), cdiv(H, 4), B) x 256
        n_iter == 0:        the statistics launch of the streamed arm, no step (masks are copied)
    ragged:  the two tile kernels on (tiles of the batch) x 512, or a refusal (n_iter < 1, another dilation set, alignment, 2^31)
Tile kinds of the two tile kernels (64 x 16 pixels at (x0, y0), halo 24):
    x: "single"        W <= 64: the image's only tile column
       "left-full"     x0 = 0, W >= 88: the right halo lies inside the image
       "left-part"     x0 = 0, 64 < W < 88: the right halo is partly inside
       "interior"      x0 - 24 >= 0 and x0 + 88 <= W: staged in 16-byte pieces (every other kind: 4-byte pieces, clamped columns)
       "right-full"    x0 > 0, x0 + 64 <= W < x0 + 88: 64 valid columns, right halo clamped
       "right-partial" x0 > 0, W < x0 + 64
    y: letters  T top halo clamped (y0 < 24),  B bottom halo clamped (y0 + 40 > H),  P partial (H - y0 < 16; implies B),
       "M" = neither halo clamped (y0 >= 24 and y0 + 40 <= H)
"""
import functools

import numpy as np

import oracle

DIL = (1, 2, 4, 8, 12, 24)
TAPS = [(-1, -1), (-1, 0), (-1, 1), (0, -1), (0, 1), (1, -1), (1, 0), (1, 1)]       # PAR.py:39-52
B, CMAX = 3, 4
NCHAN = (4, 1, 3)
VOC_MEAN, VOC_STD = (123.675, 116.28, 103.53), (58.395, 57.12, 57.375)

# (H, W): (x kind of every tile column, y kind of every tile row).  Written out by hand from the rules above, not read back from the library.
TILES = {
    (1, 64): (["single"], ["TBP"]),
    (16, 8): (["single"], ["TB"]),
    (17, 20): (["single"], ["TB", "TBP"]),
    (40, 24): (["single"], ["T", "TB", "BP"]),
    (17, 68): (["left-part", "right-partial"], ["TB", "TBP"]),
    (40, 88): (["left-full", "right-partial"], ["T", "TB", "BP"]),
    (16, 128): (["left-full", "right-full"], ["TB"]),
    (40, 148): (["left-full", "right-full", "right-partial"], ["T", "TB", "BP"]),
    (73, 152): (["left-full", "interior", "right-partial"], ["T", "T", "M", "B", "BP"]),
    (72, 216): (["left-full", "interior", "interior", "right-partial"], ["T", "T", "M", "B", "BP"]),
    (33, 4): (["single"], ["TB", "TB", "BP"]),
    # ragged only
    (40, 151): (["left-full", "right-full", "right-partial"], ["T", "TB", "BP"]),
    (17, 69): (["left-part", "right-partial"], ["TB", "TBP"]),
    (1, 9): (["single"], ["TBP"]),
    (72, 217): (["left-full", "interior", "interior", "right-partial"], ["T", "T", "M", "B", "BP"]),
    (16, 129): (["left-full", "right-full", "right-partial"], ["TB"]),
    (5, 3): (["single"], ["TBP"]),
}
X_KINDS = ("single", "left-full", "left-part", "interior", "right-full", "right-partial")
Y_KINDS = ("T", "TB", "TBP", "BP", "M", "B")

# uniform sweep: (H, W) -> (statistics kernel, step kernel, n_iter values).  1 and 2 everywhere (`out` written directly / through the
# ping-pong buffer), 5 on three shapes, 20 on one
RECOMPUTE = {
    (1, 64): ("tile", (1, 2)), (16, 8): ("tile", (1, 2)), (17, 20): ("tile", (1, 2)), (40, 24): ("tile", (1, 2)),
    (17, 68): ("tile", (1, 2)), (40, 88): ("tile", (1, 2, 5)), (16, 128): ("tile", (1, 2)), (40, 148): ("tile", (1, 2, 20)),
    (73, 152): ("tile", (1, 2, 5)), (72, 216): ("tile", (1, 2, 5)), (33, 4): ("pointwise_compact", (1, 2)),
}
STREAMED = {(17, 67): (1, 2), (40, 150): (1, 2)}          # W % 4 != 0
STREAM_FLAG = {(73, 152): (1, 2)}                         # the flag, on a shape the tile kernels take: bit-equal to them
RAGGED_SIZES = [(73, 152), (40, 151), (17, 69), (1, 9), (72, 217), (16, 129), (5, 3)]
RAGGED_INPUT = (32, 48)                                   # the (non-square) network input every guide of the batch is resized from
RAGGED_NCHAN = (4, 1, 3, 2, 4, 3, 1)
RAGGED_ITERS = (1, 2)
W12 = (0.5, 0.05)                                         # the non-default weights
# dilation sets of the pointwise kernel's other instances, at (17, 67): <2>, <3>, <5>, <7>, and <6> writing planes
OTHER_DILATIONS = {2: (1, 3), 3: (1, 2, 5), 5: (1, 2, 3, 6, 9), 6: (1, 2, 3, 5, 7, 11), 7: (1, 2, 3, 4, 6, 8, 10)}
OTHER_SHAPE = (17, 67)


def x_kind(x0, W):
    if W <= 64:
        return "single"
    if x0 == 0:
        return "left-full" if W >= 88 else "left-part"
    if x0 - 24 >= 0 and x0 + 88 <= W:
        return "interior"
    return "right-full" if x0 + 64 <= W else "right-partial"


def y_kind(y0, H):
    k = ("T" if y0 < 24 else "") + ("B" if y0 + 40 > H else "") + ("P" if H - y0 < 16 else "")
    return k or "M"


def cdiv(a, b):
    return -(-a // b)


def expected_plan(H, W, n_iter, stream=False, dil=DIL, ragged=False, n=B, guide_hw=None):
    """What ops.par_plan must answer for a sweep shape, from the tables above (the arm and the tile kinds) and the grid rules of the
    module docstring."""
    if ragged:
        stats, step = "tile", "recompute"
    elif (H, W) in RECOMPUTE and not stream and tuple(dil) == DIL:
        stats, step = RECOMPUTE[(H, W)][0], "recompute"
    else:
        stats, step = "pointwise_planes", "stream"
    tile_grid = (n * cdiv(W, 64) * cdiv(H, 16), 1, 1) if ragged else (cdiv(W, 64), cdiv(H, 16), n)
    point_grid = (cdiv(W, 64), cdiv(H, 4), n)
    xs, ys = TILES[(H, W)] if step == "recompute" else ([], [])
    return dict(resize=ragged or (guide_hw is not None and tuple(guide_hw) != (H, W)), stats=stats, nd=len(dil), step=step,
                stats_grid=tile_grid if stats == "tile" else point_grid, stats_block=512 if stats == "tile" else 256,
                step_grid=tile_grid if step == "recompute" else point_grid, step_block=512 if step == "recompute" else 256,
                tiles_interior=xs.count("interior") * len(ys), tiles_border=(len(xs) - xs.count("interior")) * len(ys), refused=None)


def tile_id(H, W):
    """the tile kinds of a shape, for test ids"""
    xs, ys = TILES[(H, W)]
    return f"{H}x{W}-x[{','.join(dict.fromkeys(xs))}]-y[{','.join(dict.fromkeys(ys))}]"


# ---------------------------------------------------------------------------------------------------------------- inputs
def noise_guide(n, h, w, seed):
    return np.random.RandomState(seed).standard_normal((n, 3, h, w)).astype(np.float32)


def photo_guide(n, h, w, seed, corner=True):
    """An 8-bit image - smooth gradients, one exactly constant rectangle, one textured region - normalised with the VOC mean and std.
    corner: the rectangle sits in the top left corner, where 30 rows and columns hold every (edge-clamped) tap of the first pixels: all
    48 taps equal, std -> 1e-8.  corner=False (the network input of the ragged batch, which is RESIZED): in the interior and, resized,
    narrower than the 49 pixels the taps span, so no pixel sees it alone.  A resized constant is constant only to fp32 rounding (6e-8),
    which is no smaller than the 1e-8 that stands in for a vanishing std: the weights of such a pixel are rounding noise in ANY fp32
    evaluation - the fp32 oracle itself then sits 0.1 .. 0.23 from the judge (measured on the ragged batch with the corner form) - so
    that regime cannot be judged, by the sweep's own precondition."""
    rs = np.random.RandomState(seed)
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    out = np.empty((n, 3, h, w), np.float32)
    for b in range(n):
        img = np.empty((h, w, 3))
        for c in range(3):
            a, bb, ph = rs.uniform(0.3, 1.5, 3)
            img[:, :, c] = 128 + 70 * np.sin(a * xx / 17 + ph) * np.cos(bb * yy / 13 + c) + 0.6 * (xx - yy) * (c - 1)
        if corner:
            img[:min(30, max(1, (3 * h) // 4)), :min(30, max(1, w // 2))] = rs.randint(40, 216, 3)
        else:
            img[h // 5:max(h // 5 + 1, (3 * h) // 5), w // 6:max(w // 6 + 1, w // 2)] = rs.randint(40, 216, 3)
        ty, tx = h // 2, (2 * w) // 3
        img[ty:, tx:] += rs.randint(-40, 41, (h - ty, w - tx, 3))         # textured
        u8 = np.clip(np.rint(img), 0, 255).astype(np.uint8)
        out[b] = ((u8.astype(np.float64) - VOC_MEAN) / VOC_STD).astype(np.float32).transpose(2, 0, 1)
    return out


GUIDES = {"noise": noise_guide, "photo": photo_guide}


def guide(kind, n, h, w, **kw):
    return GUIDES[kind](n, h, w, 7000 + 13 * h + w, **kw)


def masks(n, c, H, W):
    return np.random.RandomState(9000 + 7 * H + W).rand(n, c, H, W).astype(np.float32)


# ---------------------------------------------------------------------------------------------------------------- the float64 judge
def resize64(x, H, W, swap_hw=False):
    """F.interpolate(mode='bilinear', align_corners=True) (PAR.py:67) in float64.  swap_hw (a wrong variant): the source planes are
    read as [w, h]."""
    x = np.asarray(x, np.float64)
    if swap_hw:
        x = x.reshape(x.shape[:-2] + (x.shape[-1], x.shape[-2]))
    h, w = x.shape[-2:]
    if (h, w) == (H, W):
        return x.copy()

    def idx(n_out, n_in):
        # the sampling positions enter as the fp32 values the reference holds (ATen area_pixel_compute_source_index for float tensors:
        # scale = float(n_in - 1) / float(n_out - 1), src = scale * dst, one fp32 rounding each), like w1, w2 and sqrt(2): they are
        # part of the rule, not of its evaluation.  At float64 positions the fp32 oracle alone sits 1e-5 .. 2.6e-5 from the judge on
        # the resized guides of the ragged batch (a position near 47 carries 4e-6 of fp32 rounding, times the guide's local slope,
        # amplified by 1 / (std w1)^2) and no fp32 implementation could be told from a wrong one at 1e-5.  The blend is float64.
        scale = np.float32(n_in - 1) / np.float32(n_out - 1) if n_out > 1 else np.float32(0)
        src = (scale * np.arange(n_out, dtype=np.float32)).astype(np.float64)
        i0 = np.minimum(np.floor(src).astype(np.int64), n_in - 1)
        return i0, np.minimum(i0 + 1, n_in - 1), src - i0

    y0, y1, ly = idx(H, h)
    x0, x1, lx = idx(W, w)
    ly, lx = ly[:, None], lx[None, :]
    r0, r1 = x[..., y0, :], x[..., y1, :]
    top = (1 - lx) * r0[..., :, x0] + lx * r0[..., :, x1]
    bot = (1 - lx) * r1[..., :, x0] + lx * r1[..., :, x1]
    return (1 - ly) * top + ly * bot


def neighbors64(x, dil, variant=None):
    """x [..., H, W] -> [..., 8 * len(dil), H, W]: edge-clamped dilated taps, dilation-major (PAR.py:39-52).  Wrong variants:
    "swap_taps" exchanges two taps of the first dilation; "clamp_w2" clamps the right-border taps of the last tile column to W - 2."""
    H, W = x.shape[-2:]
    ys, xs = np.arange(H), np.arange(W)
    out = []
    for d in dil:
        for (ty, tx) in TAPS:
            yy = np.clip(ys + ty * d, 0, H - 1)
            xx = np.clip(xs + tx * d, 0, W - 1)
            if variant == "clamp_w2" and W >= 2:
                last = xs >= 64 * ((W - 1) // 64)
                xx = np.where(last, np.clip(xs + tx * d, 0, W - 2), xx)
            out.append(x[..., yy, :][..., :, xx])
    if variant == "swap_taps":
        out[1], out[2] = out[2], out[1]
    return np.stack(out, -3)


def affinity64(g, dil, w1, w2, variant=None):
    """g [B,3,H,W] float64 (already at the masks' size) -> [B, 8 * len(dil), H, W] (PAR.py:70-86).  w1, w2 and sqrt(2) enter as the fp32
    values the reference holds."""
    w1, w2, s2 = float(np.float32(w1)), float(np.float32(w2)), float(np.float32(np.sqrt(2)))
    if variant == "w2_1pct":
        w2 *= 1.01
    nb = neighbors64(g, dil)                                              # [B,3,T,H,W]
    absd = np.abs(nb - g[:, :, None])
    std = nb.std(axis=2, ddof=0 if variant == "biased" else 1, keepdims=True)
    aff = (-((absd / (std + 1e-8) / w1) ** 2)).mean(1)                     # [B,T,H,W]
    ker = np.array([s2, 1, s2, 1, 1, s2, 1, s2])
    pos = np.concatenate([ker * d for d in dil])
    pos_aff = -((pos / (pos.std(ddof=1) + 1e-8) / w1) ** 2)

    def softmax(z, axis):
        e = np.exp(z - z.max(axis, keepdims=True))
        return e / e.sum(axis, keepdims=True)

    aff = softmax(aff, 1)
    if variant != "nopos":
        aff = aff + w2 * softmax(pos_aff, 0).reshape(1, -1, 1, 1)
    return aff


def judge(g, m, dil=DIL, iters=(1,), w1=0.3, w2=0.01, nchan=None, variant=None):
    """PAR.forward (PAR.py:64-92) in float64: g [B,3,h,w] (resized to the masks' size), m [B,C,H,W] -> {n_iter: [B,C,H,W]}.  Channels
    >= nchan[b] are not refined: zero, like a fresh output tensor of the library."""
    m = np.asarray(m, np.float64)
    H, W = m.shape[-2:]
    g = resize64(g, H, W, swap_hw=variant == "swap_hw")
    aff = affinity64(g, dil, w1, w2, variant)
    out, cur = {}, m
    for it in range(1, max(iters) + 1):
        nb = neighbors64(cur, dil, variant if variant in ("swap_taps", "clamp_w2") else None)
        cur = np.einsum("bcthw,bthw->bchw", nb, aff)
        if it in iters:
            o = cur.copy()
            if nchan is not None:
                for b, k in enumerate(nchan):
                    o[b, k:] = 0.0
            out[it] = o
    return out


def oracle32(g, m, dil=DIL, iters=(1,), w1=0.3, w2=0.01, nchan=None):
    """oracle.par (fp32) on the same input -> {n_iter: [B,C,H,W]}"""
    p = oracle.par.PAR(list(dil), max(iters))
    p.w1, p.w2 = np.float32(w1), np.float32(w2)
    m = np.asarray(m, np.float32)
    aff = p.affinity(g, m.shape[-2], m.shape[-1])
    out, cur = {}, m
    for it in range(1, max(iters) + 1):
        cur = (p.neighbors(cur) * aff).sum(2, dtype=np.float32)
        if it in iters:
            o = cur.copy()
            if nchan is not None:
                for b, k in enumerate(nchan):
                    o[b, k:] = 0.0
            out[it] = o
    return out


def maxabs(a, b):
    return float(np.max(np.abs(np.asarray(a, np.float64) - np.asarray(b, np.float64))))


@functools.lru_cache(maxsize=None)
def uniform_case(H, W, kind, iters, dil=DIL, w12=(0.3, 0.01)):
    """(guide, masks, J, o) of one uniform sweep case: J = {n_iter: judge}, o = {n_iter: max |oracle32 - J|}.  Computed once per case;
    the arrays are shared: do not write to them."""
    g, m = guide(kind, B, H, W), masks(B, CMAX, H, W)
    J = judge(g, m, dil, iters, w12[0], w12[1], NCHAN)
    O = oracle32(g, m, dil, iters, w12[0], w12[1], NCHAN)
    return g, m, J, {it: maxabs(O[it], J[it]) for it in iters}


@functools.lru_cache(maxsize=None)
def ragged_case(kind, iters, w12=(0.3, 0.01)):
    """The ragged batch: network input [B,3,32,48], per image masks [Cmax,H_b,W_b], J[b] / o[b] = {n_iter: ...} of image b alone."""
    n = len(RAGGED_SIZES)
    g = guide(kind, n, *RAGGED_INPUT, **(dict(corner=False) if kind == "photo" else {}))
    ms, Js, os_ = [], [], []
    for b, (H, W) in enumerate(RAGGED_SIZES):
        m = masks(1, CMAX, H, W)
        J = judge(g[b:b + 1], m, DIL, iters, w12[0], w12[1], RAGGED_NCHAN[b:b + 1])
        O = oracle32(g[b:b + 1], m, DIL, iters, w12[0], w12[1], RAGGED_NCHAN[b:b + 1])
        ms.append(m[0])
        Js.append({it: J[it][0] for it in iters})
        os_.append({it: maxabs(O[it], J[it]) for it in iters})
    return g, ms, Js, os_


# ---------------------------------------------------------------------------------------------------------------- gates
O_CAP = 5e-6          # precondition: the fp32 oracle stays this close to the judge (a cap, not a measurement)
O_FLOOR = 1e-6
CEILING = 1e-5        # K * max(o, O_FLOOR) must stay below this for every case
OLD_BOUND = 5e-5      # the suite's absolute tolerance for PAR: a ceiling in any event
# Measured on an MI355X over the whole sweep (EXPERIMENTS.md, "PAR tile sweep", 116 figures): the largest err / max(o, 1e-6) is 1.88
# (40 x 148, photo guide, 20 steps: err 3.88e-6, o 2.07e-6); one step stays below 1.01, the ragged batch below 0.85.  K = twice that
# (margin for a compiler that re-associates differently).  The largest o of the sweep is 2.59e-6 (40 x 148, noise, 20 steps):
# K x o = 9.72e-6, inside the ceiling.
MEASURED_RATIO = 1.88
K = 2 * MEASURED_RATIO


def precondition(J, o):
    """On the reference alone -> list of messages (empty = the case may be judged)."""
    bad = []
    if np.isnan(J).any():
        bad.append("NaN in the judge")
    if not o <= O_CAP:
        bad.append(f"oracle32 deviates from the judge by {o:.3e} > {O_CAP:.0e}")
    if not K * max(o, O_FLOOR) < CEILING:
        bad.append(f"K * max(o, 1e-6) = {K * max(o, O_FLOOR):.3e} >= {CEILING:.0e}")
    return bad


def bound(o):
    return min(K * max(o, O_FLOOR), OLD_BOUND)


def numerics_failures(err, o):
    b = bound(o)
    return [] if err <= b else [f"err {err:.3e} > {b:.3e} = K x max(o {o:.3e}, 1e-6)"]


def report(tag, err, o):
    print(f"[par-shapes] {tag}: err {err:.3e} o {o:.3e} err/max(o,1e-6) {err / max(o, O_FLOOR):.2f}")
