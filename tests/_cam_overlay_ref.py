"""numpy restatement of tools/infer_lam.py:97-111 (--save_cam) for the CAM overlay tests.

    img = denormalize_img(inputs)[0]                          the round-trip image (imutils.denormalize_roundtrip_table)
    cam_rgb = plt.get_cmap("jet")(cam)[:, :, :3] * 255        float32 cam -> float64 RGB (colormap rules below)
    out = (alpha * cam_rgb + (1 - alpha) * img).astype(np.uint8)
"""
import numpy as np


def jet_rgb(x, lut):
    """Colormap.__call__ for float32 x and N = 256: floor(x*256), x == 1 -> 255, x < 0 -> under (entry 0), x > 1 -> over (entry 255),
    NaN -> bad (RGB 0)."""
    x = np.asarray(x, np.float32)
    xa = x * np.float32(256)
    xa[xa == 256] = 255
    bad = np.isnan(x)
    with np.errstate(invalid="ignore"):
        under, over = xa < 0, xa >= 256
        idx = np.where(under | over | bad, 0, xa).astype(np.int64)
    idx[under] = 0
    idx[over] = 255
    rgb = lut[idx]
    rgb[bad] = 0.0
    return rgb


def overlays(decoded, cams, mode, lut, rt):
    """decoded uint8 [H,W,3], cams f32 [k+1,H,W] (row 0 background) -> the arrays the reference writes: [max overlay] (none when
    k == 0) or one per foreground row."""
    img = np.stack([rt[c][decoded[..., c]] for c in range(3)], -1)              # uint8 [H,W,3]
    fg = np.asarray(cams[1:], np.float32)
    if mode == "max":
        if fg.shape[0] == 0:
            return []
        cam = fg.max(0)                                                          # NaN propagates, like torch.max
        return [(0.5 * (jet_rgb(cam, lut) * 255) + (1 - 0.5) * img).astype(np.uint8)]
    return [(0.6 * (jet_rgb(c, lut) * 255) + (1 - 0.6) * img).astype(np.uint8) for c in fg]
