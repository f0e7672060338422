"""The library's workspace-size queries as rows of integers: `query arg ... : bytes` (tests/golden/workspace_bytes.txt).

Shared by tests/golden/make_workspace_golden.py, which records the rows, and tests/test_host_workspace_bytes.py, which replays them.
Every query but the ViT's is host arithmetic.  The decoder and text handles only copy their structs at creation, so they are built
from ctypes structs here; excel_text_create checks three weight pointers for null and never reads them, so they hold a dummy value.

Arguments of a row:
  plain queries                                  the C arguments in order
  excel_dcrf_lam_ragged_workspace_bytes          B, then (H, W, nchan) per image
  excel_decoder_[train_]workspace_bytes          vit_layers vit_width embed dec_layers heads num_classes, then B g
  excel_text_workspace_bytes                     vocab_size context_length width layers heads embed_dim, then B
  excel_vit_workspace_bytes                      width layers heads patch out_dim, then B S (needs a device: rows recorded with --gpu)
"""
import ctypes as C
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "workspace_bytes.txt")
VIT_QUERY = "excel_vit_workspace_bytes"


def _decoder_bytes(query, a):
    from excel_amd import _lib
    lib = _lib.lib()
    L, nl = a[0], a[3]
    fuse = (_lib.FuseLayerWeights * max(L, 1))()
    blocks = (_lib.DecoderBlockWeights * max(nl, 1))()
    cfg = _lib.DecoderConfig(*a[:6])
    w = _lib.DecoderWeights(fuse=fuse, blocks=blocks)
    h = C.c_void_p()
    _lib.check(lib.excel_decoder_create(C.byref(cfg), C.byref(w), C.byref(h)), "excel_decoder_create")
    try:
        return int(getattr(lib, query)(h, a[6], a[7]))
    finally:
        lib.excel_decoder_destroy(h)


def _text_bytes(a):
    from excel_amd import _lib
    lib = _lib.lib()
    blocks = (_lib.DecoderBlockWeights * max(a[3], 1))()
    cfg = _lib.TextConfig(*a[:6])
    w = _lib.TextWeights(token_embedding=256, positional_embedding=256, text_projection=256, blocks=blocks)    # checked for null, never read
    h = C.c_void_p()
    _lib.check(lib.excel_text_create(C.byref(cfg), C.byref(w), C.byref(h)), "excel_text_create")
    try:
        return int(lib.excel_text_workspace_bytes(h, a[6]))
    finally:
        lib.excel_text_destroy(h)


def _vit_bytes(a):
    """A ViT with seeded weights on the device (excel_vit_create transposes the projection there)."""
    import torch
    from excel_amd import ops
    from oracle.vit import VitConfig, make_vit_weights
    width, layers, heads, patch, out_dim, B, S = a
    cfg = VitConfig(width=width, layers=layers, heads=heads, patch=patch, out_dim=out_dim, input_resolution=64, n_surgery=1)
    vit = ops.VitHandle(make_vit_weights(cfg, seed=5), width, layers, heads, patch, out_dim, n_surgery=1, device=torch.device("cuda:0"),
                        gemm_mode="f32")
    return int(ops.lib().excel_vit_workspace_bytes(vit._h, B, S))


def query_bytes(query, args):
    from excel_amd import _lib
    lib = _lib.lib()
    a = list(args)
    i32 = C.POINTER(C.c_int32)
    if query in ("excel_decoder_workspace_bytes", "excel_decoder_train_workspace_bytes"):
        return _decoder_bytes(query, a)
    if query == "excel_text_workspace_bytes":
        return _text_bytes(a)
    if query == VIT_QUERY:
        return _vit_bytes(a)
    if query == "excel_dcrf_ragged_workspace_bytes":
        out = C.c_size_t()
        _lib.check(lib.excel_dcrf_ragged_workspace_bytes(a[0], a[1], C.byref(out)), query)
        return int(out.value)
    if query == "excel_dcrf_lam_ragged_workspace_bytes":
        rec = np.array(a[1:], np.int32).reshape(a[0], 3)
        hw, nchan = np.ascontiguousarray(rec[:, :2]), np.ascontiguousarray(rec[:, 2])
        out = C.c_size_t()
        _lib.check(lib.excel_dcrf_lam_ragged_workspace_bytes(hw.ctypes.data_as(i32), nchan.ctypes.data_as(i32), a[0], C.byref(out)), query)
        return int(out.value)
    return int(getattr(lib, query)(*a))


def read_rows(path=GOLDEN):
    rows = []
    for line in open(path):
        if line.startswith("#") or not line.strip():
            continue
        left, right = line.split(":")
        left = left.split()
        rows.append((left[0], tuple(map(int, left[1:])), int(right)))
    return rows
