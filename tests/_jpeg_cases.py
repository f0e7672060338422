"""The images the CAM JPEG tests share: every (shape, content) of the host and the GPU test, built once."""
import io

import numpy as np

SHAPES = [(1, 1), (8, 8), (16, 16), (17, 33), (37, 53), (15, 64), (64, 15), (48, 80)]
CONTENTS = ["zero", "grey", "white", "random", "ramp", "pixel", "checker"]
QUALITIES = [50, 75, 95]


def image(shape, content):
    """uint8 [H,W,3]"""
    H, W = shape
    a = np.zeros((H, W, 3), np.uint8)
    if content == "grey":
        a[:] = 128
    elif content == "white":
        a[:] = 255
    elif content == "random":                       # every category, frequent 0xFF bytes in the stream
        a = np.random.RandomState(1000 * H + W).randint(0, 256, (H, W, 3)).astype(np.uint8)
    elif content == "ramp":                         # long zero runs, EOB
        y, x = np.mgrid[0:H, 0:W]
        a = np.stack([(255 * x) // max(W - 1, 1), (255 * y) // max(H - 1, 1), (255 * (x + y)) // max(H + W - 2, 1)], -1).astype(np.uint8)
    elif content == "pixel":                        # padding: one bright pixel at the last row and column
        a[H - 1, W - 1] = (255, 200, 60)
    elif content == "checker":                      # the largest AC amplitudes, ZRL
        y, x = np.mgrid[0:H, 0:W]
        a[:] = (((x + y) & 1) * 255).astype(np.uint8)[..., None]
    return np.ascontiguousarray(a)


def pillow_bytes(a, quality):
    from PIL import Image
    buf = io.BytesIO()
    Image.fromarray(a).save(buf, format="JPEG", quality=quality)
    return buf.getvalue()


_REF = {}


def ref_bytes(shape, content, quality):
    """the restatement's file, computed once per case"""
    import _jpeg_ref
    key = (shape, content, quality)
    if key not in _REF:
        _REF[key] = _jpeg_ref.encode(image(shape, content), quality)
    return _REF[key]
