"""float64 numpy restatement of the flip / multi-scale LAM fuse (include/excel_hip.h, excel_lam_tta_fuse; utils/camutils.py:8-63) and
the kernel cases the GPU test runs.  Everything, the source coordinates included, is computed in float64."""
import numpy as np

# (B, F, g_out, grids): tests/test_gpu_lam_tta.py's kernel cases
CASES = [(2, 5, 4, (4, 2, 6)), (1, 80, 3, (3, 1, 5)), (3, 20, 28, (28, 14, 21, 42)), (2, 81, 32, (32, 16, 24, 48)), (2, 7, 5, (5,) * 8)]


def case_maps(ci, seed, flip=True):
    """The inputs of case ci: per scale 4 * rand [2B or B, g*g, F] float32 (the un-flipped runs use the first half of the same data)."""
    B, F, g_out, grids = CASES[ci]
    rs = np.random.RandomState(100 * seed + ci)
    maps = [(4 * rs.rand(2 * B, g * g, F)).astype(np.float32) for g in grids]
    return maps if flip else [m[:B].copy() for m in maps]


def _taps(out_size, in_size):
    """F.interpolate(bilinear, align_corners=False): (i0, i1, weight of i1) per output index."""
    src = np.maximum((in_size / out_size) * (np.arange(out_size, dtype=np.float64) + 0.5) - 0.5, 0.0)
    i0 = np.minimum(np.floor(src).astype(np.int64), in_size - 1)
    return i0, np.minimum(i0 + 1, in_size - 1), src - i0


def resize_planes(x, G):
    """x [..., g, g] float64 -> [..., G, G]"""
    g = x.shape[-1]
    y0, y1, ly = _taps(G, g)
    x0, x1, lx = _taps(G, g)
    r0, r1 = x[..., y0, :], x[..., y1, :]
    top = (1 - lx) * r0[..., :, x0] + lx * r0[..., :, x1]
    bot = (1 - lx) * r1[..., :, x0] + lx * r1[..., :, x1]
    return (1 - ly)[:, None] * top + ly[:, None] * bot


def fuse_sums(maps, grids, g_out, flip):
    """maps[s] [2B or B, g_s^2, F] -> the un-normalised sums [B, F, g_out, g_out] (float64)."""
    acc = 0
    for m, g in zip(maps, grids):
        m = np.asarray(m, np.float64)
        nb, P, F = m.shape
        assert P == g * g
        r = resize_planes(m.transpose(0, 2, 1).reshape(nb, F, g, g), g_out)
        acc = acc + (np.maximum(r[:nb // 2], r[nb // 2:][..., ::-1]) if flip else r)
    return acc


def lam_tta_ref(maps, grids, g_out, flip):
    """-> (out [B, g_out^2, F] float64, the smallest range of a plane before the normalisation)"""
    acc = fuse_sums(maps, grids, g_out, flip)
    mn = acc.min(axis=(2, 3), keepdims=True)
    lam = acc - mn
    mx = lam.max(axis=(2, 3), keepdims=True)
    out = lam / (mx + 1e-5)
    B, F = out.shape[:2]
    return out.reshape(B, F, g_out * g_out).transpose(0, 2, 1), float(mx.min())


def oracle_attr_maps(imgs, w, cfg, text_attr, num_fg, f64):
    """[B,3,S,S] -> the model's attribute maps [B,P,num_fg] through the oracle: its own fp32 chain (oracle.cam.attr_maps_raw), or with
    f64 the same formulas in float64 throughout (oracle.vit under precision(float64); clip/clip.py:295-308, :353 restated here)."""
    import oracle
    if not f64:
        return oracle.cam.attr_maps_raw(imgs, w, cfg, text_attr, num_fg)[0]
    with oracle.vit.precision(np.float64):
        x, _, _ = oracle.vit.vit_forward(np.asarray(imgs, np.float64), {k: np.asarray(v, np.float64) for k, v in w.items()}, cfg)
    assert x.dtype == np.float64
    text = np.asarray(text_attr, np.float64).T                                  # [T,C]
    f = x / np.sqrt((x * x).sum(axis=1, keepdims=True))                         # :353, over the token axis
    out = []
    for fi in f:
        z = 2.0 * (fi[:1] @ text.T)                                             # :295-296
        prob = np.exp(z - z.max(-1, keepdims=True))
        prob = prob / prob.sum(-1, keepdims=True)
        wt = prob / prob.mean(-1, keepdims=True)                                # :297
        feats = fi[:, None, :] * text[None, :, :] * wt.reshape(1, -1, 1)        # :301-302
        sim = (feats - feats.mean(1, keepdims=True)).sum(-1)                    # :303-306
        out.append((sim - sim.min(0, keepdims=True)) / (sim.max(0, keepdims=True) - sim.min(0, keepdims=True)))     # :308
    return np.stack(out, 0)[:, 1:, :num_fg]


def oracle_tta_attr(x, w, cfg, text_attr, num_fg, sizes, flip, f64):
    """The whole chain of the step's `attr` for uniform inputs x [B,3,S,S] (float32): per (S_s, g_s) of `sizes` (scale 1.0 first) the
    oracle.interp resize of x, the oracle's maps of [x_s; x_s mirrored], then lam_tta_ref at the grid of sizes[0]."""
    import oracle
    S = x.shape[-1]
    maps = []
    for S_s, _ in sizes:
        xs = x if S_s == S else oracle.interp.bilinear_resize(x, S_s, S_s, align_corners=False)
        maps.append(oracle_attr_maps(np.concatenate([xs, xs[..., ::-1]], 0) if flip else xs, w, cfg, text_attr, num_fg, f64))
    return lam_tta_ref(maps, [g for _, g in sizes], sizes[0][1], flip)[0]
