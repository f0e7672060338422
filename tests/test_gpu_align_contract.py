"""Where a tensor starts in memory does not change a result (the table and the contract: tests/_align_cases.py).

  same bits          every case of the stream contract's table is built twice, on freshly uploaded inputs and on inputs that are views one
                     element into their storage (4 bytes past a 16-byte boundary for fp32 / int32, 1 byte for uint8, 2 for the 16-bit
                     planes, which test_shifted_split_planes hands over), and must return the same bits: the same instructions run on the same values, so there is no tolerance.
  written arguments  every out= / ws= / in-place argument as such a view: the bits of the fresh-tensor call, or a ValueError that names
                     the argument and leaves the view's bytes alone - whichever the table says.
  ABI refusals       every pointer the table holds to more than 4 bytes, handed to its entry 4 bytes (2, 1) further on: EXCEL_ERR_ARG,
                     the argument's name in the error text, every output and workspace still poisoned afterwards.
  PAR                the uniform entry takes misaligned masks / out on its streamed-plane arm, the ragged entry refuses them.
  handles            VitHandle, DecoderHandle and TextHandle built from shifted weight tensors give the bits of plain ones.

No shifted pointer reaches a kernel that was not read to be safe with it: inputs below an op's requirement are copied by ops._realign,
written arguments are refused, and the library's entries check before they launch."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _align_cases as A  # noqa: E402
import _scratch as S  # noqa: E402
import _scratch_cases as SC  # noqa: E402
from _scratch_cases import SIZES, dev  # noqa: E402

POISON = 0xA5


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from excel_amd import ops as _ops
    return _ops


def _bytes(t):
    return t.contiguous().view(-1).view(torch.uint8)


def _same_bytes(a, b, what):
    assert a.shape == b.shape and a.dtype == b.dtype, what
    if not torch.equal(_bytes(a), _bytes(b)):
        d = _bytes(a) != _bytes(b)
        raise AssertionError(f"{what}: {int(d.sum())} of {d.numel()} bytes differ (first at byte {int(d.nonzero()[0])})")


# ------------------------------------------------------------------ same bits
@pytest.mark.parametrize("name", sorted(A.CASES))
def test_shifted_inputs_give_the_same_bits(ops, name):
    with S.poisoned_allocations(0x00):              # (the cases that poison a cached workspace themselves need a block; 0x00 is fresh memory)
        plain = A.CASES[name](ops)
        want = plain.fn()
        torch.cuda.synchronize()
        with A.shifted_uploads():                   # inputs uploaded while the case is built, and those its fn() uploads per call
            case = A.CASES[name](ops)
            got = case.fn()
        torch.cuda.synchronize()
    assert not SC.UPLOADER
    S.assert_same_bits(want, got, plain.defined)


def test_the_shifted_builds_really_are_shifted(ops):
    """the uploader the cases go through hands out views 1 element into their storage, of the dtypes the cases upload (the 16-bit planes
    are outputs of ops there: test_shifted_split_planes hands those over shifted)"""
    seen = []
    real = A.shifted

    def spy(t, device=None):
        v = real(t, device)
        seen.append((v.dtype, v.data_ptr() % 16, v.element_size()))
        return v
    SC.UPLOADER.append(spy)
    try:
        A.CASES["label_ops"](ops)
        A.CASES["gemm_family"](ops)
    finally:
        SC.UPLOADER.pop()
    assert {d for d, _, _ in seen} >= {torch.float32, torch.uint8}
    assert all(off == size for _, off, size in seen) and len(seen) > 10


# ------------------------------------------------------------------ written arguments
def _written_specs(ops):
    """op -> {argument: (initial content of the buffer, run(buffer) -> result tree)}.  Shapes as in the case tables."""
    rs = np.random.RandomState(40)
    H, W = SIZES[0]
    f32, u8, i32, i64 = torch.float32, torch.uint8, torch.int32, torch.int64
    poison = lambda shape, dtype: S_fill(torch.empty(shape, dtype=dtype, device="cuda"))
    zeros = lambda shape, dtype: torch.zeros(shape, dtype=dtype, device="cuda")
    sizes = SIZES + [(9, 6)]
    plan3, plan2 = ops.RaggedPlan(sizes, "cuda"), ops.RaggedPlan(SIZES, "cuda")
    half = ops.conf_half_plan(plan3)
    smax, nc = 3, 21
    onehot = np.zeros((3, 6), np.float32)
    onehot[0, [1, 4]], onehot[1, [2]], onehot[2, [0, 3, 5]] = 1, 1, 1
    idx, ncls, nchan = ops.cls_compact(dev(onehot), smax, want_nchan=True)
    segs = dev(rs.standard_normal((4, nc, 5, 5)).astype(np.float32))
    f30 = dev(rs.standard_normal((4, 30, 25)).astype(np.float32))
    refined = dev(rs.rand(3, smax, 25).astype(np.float32))
    imgs = dev(rs.standard_normal((2, 3, 12, 20)).astype(np.float32))
    m32 = dev(rs.rand(2, 3, 17, 32).astype(np.float32))
    rimgs = dev(rs.standard_normal((2, 3, 16, 16)).astype(np.float32))
    rmasks = dev(SC.pitched(rs, plan2, 3))
    cams4 = dev(SC.pitched(rs, plan3, smax + 1))
    gt = dev(rs.randint(0, 8, plan3.total_label_pix).astype(np.uint8), u8)
    pred = dev(rs.randint(0, 8, plan3.total_label_pix).astype(np.uint8), u8)
    ugt, upred = dev(rs.randint(0, nc, (3, 17, 29)).astype(np.uint8), u8), dev(rs.randint(0, nc, (3, 17, 29)).astype(np.uint8), u8)
    skip = dev(np.array([0, 1, 0], np.int32))
    x = rs.standard_normal((3, 26, 32)).astype(np.float32)
    x[1, 3, 5], x[2, 0, 0] = np.nan, np.inf
    x = dev(x)
    hwc = dev(rs.randint(0, 256, 3 * plan2.total_label_pix).astype(np.uint8), u8)
    planes, _ = ops.conf_planes_ragged(cams4, plan3, half, smax, nchan, 0.7, 0.25)
    labels = dev(rs.randint(0, 4, plan2.total_label_pix).astype(np.uint8), u8)
    items, off, rgb = [], 0, []
    for h, w in SIZES:
        rgb.append(rs.randint(0, 256, 3 * h * w).astype(np.uint8))
        items.append((off, h, w))
        off += 3 * h * w
    rgb = dev(np.concatenate(rgb), u8)
    m5, m3 = dev(rs.rand(6, 25, 4).astype(np.float32)), dev(rs.rand(6, 9, 4).astype(np.float32))
    lam = dev(rs.rand(3, 4, H, W).astype(np.float32))
    par_ws = int(ops.lib().excel_par_workspace_bytes(2, 3, 17, 32, len(ops.PAR_DILATIONS)))
    rag_ws = int(ops.lib().excel_par_ragged_workspace_bytes(plan2.total_pix, 3))
    png_ws = int(ops.lib().excel_png_labels_workspace_bytes(2, 40))

    def jpeg_files(out, table):
        t = table.cpu().numpy()
        end = int(t[-1, 0] + t[-1, 1])
        return dict(bytes=out[:end].clone(), table=table)

    return {
        "seg_scale_accumulate": {"acc": (poison((2, nc, H, W), f32), lambda b: ops.seg_scale_accumulate(segs, b, H, W, True, True))},
        "feature_affinity_grouped": {"out": (poison((4, 25, 25), f32), lambda b: ops.feature_affinity_grouped(f30, "sigmoid", group=1, out=b))},
        "cam_upsample_bkg": {"out": (poison((3, smax + 1, H, W), f32), lambda b: ops.cam_upsample_bkg(refined, ncls, 5, H, W, out=b))},
        "par_forward": {"out": (poison((2, 3, 17, 32), f32), lambda b: ops.par_forward(imgs, m32, num_iter=2, out=b)),
                        "ws": (poison((par_ws,), u8), lambda b: ops.par_forward(imgs, m32, num_iter=2, ws=b))},
        "par_forward_ragged": {"out": (poison((3 * plan2.total_pix,), f32), lambda b: ops.par_forward_ragged(rimgs, rmasks, plan2, 3, num_iter=2, out=b)),
                               "ws": (poison((rag_ws,), u8), lambda b: ops.par_forward_ragged(rimgs, rmasks, plan2, 3, num_iter=2, ws=b))},
        "argmax_label_ragged": {"out": (poison((plan3.total_label_pix,), u8), lambda b: ops.argmax_label_ragged(cams4, plan3, smax + 1, nchan, idx, out=b))},
        "confusion_accumulate": {"hist": (zeros((8, 8), i64), lambda b: ops.confusion_accumulate(gt, pred, 8, hist=b))},
        "confusion_accumulate_masked": {"hist": (zeros((nc, nc), i64), lambda b: ops.confusion_accumulate_masked(ugt, upred, nc, skip, hist=b))},
        "nonfinite_count": {"out": (poison((3,), i32), lambda b: ops.nonfinite_count(x, out=b))},
        "image_scores": {"out": (poison((3, 3, nc), i32), lambda b: ops.image_scores(ugt, upred, nc, skip=skip, out=b))},
        "boundary_scores": {"out": (poison((3, 3, nc), i32), lambda b: ops.boundary_scores(ugt, upred, nc, 2, out=b))},
        "normalize_resize_u8_ragged": {"out": (poison((2, 3, 30, 30), f32), lambda b: ops.normalize_resize_u8_ragged(hwc, plan2, 30, out=b))},
        "normalize_resize_u8_ragged_mirror": {"out": (poison((4, 3, 30, 30), f32), lambda b: ops.normalize_resize_u8_ragged_mirror(hwc, plan2, 30, out=b))},
        "cam_upsample_bkg_ragged": {"out": (poison(((smax + 1) * plan3.total_pix,), f32), lambda b: ops.cam_upsample_bkg_ragged(refined, ncls, 5, plan3, out=b))},
        "conf_planes_ragged": {"out": (poison((2 * (smax + 1) * half.total_pix,), f32),
                                       lambda b: ops.conf_planes_ragged(cams4, plan3, half, smax, nchan, 0.7, 0.25, out=b))},
        "conf_merge_ragged": {"out": (poison((plan3.total_label_pix,), u8), lambda b: ops.conf_merge_ragged(planes, half, plan3, smax, nchan, idx, out=b))},
        "png_encode_labels_ragged": {"out": (poison((ops.png_labels_arena_bytes(SIZES),), u8), lambda b: ops.png_encode_labels_ragged(labels, plan2, out=b)),
                                     "ws": (poison((png_ws,), u8), lambda b: ops.png_encode_labels_ragged(labels, plan2, ws=b))},
        "jpeg_encode_rgb_ragged": {"out": (poison((ops.jpeg_rgb_arena_bytes(SIZES),), u8), lambda b: jpeg_files(*ops.jpeg_encode_rgb_ragged(rgb, items, out=b))),
                                   "ws": (poison((ops.jpeg_rgb_workspace_bytes(SIZES),), u8), lambda b: ops.jpeg_encode_rgb_ragged(rgb, items, ws=b))},
        "lam_scale_accumulate": {"acc": (poison((3, 4, H, W), f32), lambda b: ops.lam_scale_accumulate(m5, b, 5, H, W, init=True))},
        "plane_minmax_normalize_": {"lam": (lam, lambda b: ops.plane_minmax_normalize_(b))},
        "lam_tta_fuse": {"out": (poison((3, 25, 4), f32), lambda b: ops.lam_tta_fuse([m5, m3], (5, 3), 5, True, out=b))},
    }


def S_fill(t):
    t.view(-1).view(torch.uint8).fill_(POISON)
    return t


WRITTEN = sorted((name, arg) for name, row in A.ALIGN.items() for arg in row.written)
_SPECS = {}


@pytest.mark.parametrize("name,arg", WRITTEN)
def test_written_argument_one_element_into_its_storage(ops, name, arg):
    if not _SPECS:
        _SPECS.update(_written_specs(ops))
    assert name in _SPECS and arg in _SPECS[name], f"ALIGN says ops.{name} writes {arg}: no call for it here"
    init, run = _SPECS[name][arg]
    how = A.ALIGN[name].written[arg]
    view = A.shifted(init)
    assert view.data_ptr() % 16 == view.element_size() and view.is_contiguous()
    if how == "refused":
        with pytest.raises(ValueError, match=rf"\b{arg}\b.*aligned"):
            run(view)
        torch.cuda.synchronize()
        _same_bytes(view, init, f"ops.{name} refused {arg}= and yet wrote to it")
        return
    plain = init.clone()
    want = run(plain)
    got = run(view)
    torch.cuda.synchronize()
    _same_bytes(view, plain, f"ops.{name}({arg}= a view one element into its storage)")
    lw, lg = list(S._leaves(want)), list(S._leaves(got))
    assert [p for p, _ in lw] == [p for p, _ in lg] and lw
    for (path, a), (_, b) in zip(lw, lg):
        _same_bytes(a, b, f"ops.{name}({arg}= shifted): {path}")


def test_every_written_argument_has_a_call(ops):
    if not _SPECS:
        _SPECS.update(_written_specs(ops))
    assert sorted((n, a) for n, d in _SPECS.items() for a in d) == WRITTEN


# ------------------------------------------------------------------ the 16-bit split planes are caller-owned tensors too
def test_shifted_split_planes(ops):
    """split_bf16 / pack_f16 return planes that gemm_bf16x3 / gemm_f16x2 take back: each of A_split, W_split, W_half, bias and residual
    as a view one element into its storage (2 bytes past a 16-byte boundary for the planes), alone and all together, gives the bits of
    the fresh-tensor call.  A_split, W_split, bias and residual are copied by ops._realign; W_half goes to the library as it is, which
    leaves a half matrix below 16 bytes unused (gemm_half_ok) and reads the split weights instead."""
    from _stream_cases import GEMM_SHAPES
    rs = np.random.RandomState(44)
    seen = set()

    def sh(t):
        v = A.shifted(t)
        assert v.data_ptr() % 16 == t.element_size() and v.is_contiguous()
        seen.add((v.dtype, v.data_ptr() % 16))
        return v

    for M, N, K in GEMM_SHAPES:
        a = dev(rs.standard_normal((M, K)).astype(np.float32))
        w = dev((rs.standard_normal((N, K)) * 0.05).astype(np.float16).astype(np.float32))         # fp16-valued: gemm_f16x2's precondition
        bias, res = dev(rs.standard_normal(N).astype(np.float32)), dev(rs.standard_normal((M, N)).astype(np.float32))
        for f16 in (False, True):
            As, Ws = ops.split_bf16(a, f16=f16), ops.split_bf16(w, f16=f16)
            assert As.dtype == torch.int16 and As.data_ptr() % 16 == 0
            assert torch.equal(ops.split_bf16(sh(a), f16=f16), As)
            want = ops.gemm_bf16x3(As, Ws, bias=bias, residual=res, act=1, f16=f16)
            want_split = ops.gemm_bf16x3(As, Ws, bias=bias, split_out=True, f16=f16)
            for what, kw in (("A_split", dict(A=sh(As))), ("W_split", dict(W=sh(Ws))), ("bias", dict(bias=sh(bias))), ("residual", dict(res=sh(res))),
                             ("all four", dict(A=sh(As), W=sh(Ws), bias=sh(bias), res=sh(res)))):
                got = ops.gemm_bf16x3(kw.get("A", As), kw.get("W", Ws), bias=kw.get("bias", bias), residual=kw.get("res", res), act=1, f16=f16)
                assert torch.equal(got, want), f"gemm_bf16x3(f16={f16}) {M}x{N}x{K} with a shifted {what}"
                got = ops.gemm_bf16x3(kw.get("A", As), kw.get("W", Ws), bias=kw.get("bias", bias), split_out=True, f16=f16)
                assert torch.equal(got, want_split), f"gemm_bf16x3(f16={f16}, split_out) {M}x{N}x{K} with a shifted {what}"
        Wh, inexact = ops.pack_f16(w)                        # (As, Ws: the IEEE-half planes of the last round)
        assert inexact == 0 and Wh.dtype == torch.int16
        assert torch.equal(ops.pack_f16(sh(w))[0], Wh)
        want = ops.gemm_f16x2(As, Ws, W_half=Wh, bias=bias, residual=res, act=1)
        assert torch.equal(want, ops.gemm_f16x2(As, Ws, bias=bias, residual=res, act=1))           # with and without the half matrix: same bits
        for what, kw in (("A_split", dict(A=sh(As))), ("W_split", dict(W=sh(Ws))), ("W_half", dict(Wh=sh(Wh))), ("bias", dict(bias=sh(bias))),
                         ("residual", dict(res=sh(res))), ("all five", dict(A=sh(As), W=sh(Ws), Wh=sh(Wh), bias=sh(bias), res=sh(res)))):
            got = ops.gemm_f16x2(kw.get("A", As), kw.get("W", Ws), W_half=kw.get("Wh", Wh), bias=kw.get("bias", bias), residual=kw.get("res", res), act=1)
            assert torch.equal(got, want), f"gemm_f16x2 {M}x{N}x{K} with a shifted {what}"
    torch.cuda.synchronize()
    assert seen == {(torch.int16, 2), (torch.float32, 4)}, seen


# ------------------------------------------------------------------ PAR
def test_par_uniform_takes_the_streamed_arm_and_ragged_refuses(ops):
    rs = np.random.RandomState(41)
    imgs = dev(rs.standard_normal((2, 3, 17, 32)).astype(np.float32))              # guide at the masks' size: no resize, imgs itself is staged
    masks = dev(rs.rand(2, 3, 17, 32).astype(np.float32))
    want = ops.par_forward(imgs, masks, num_iter=2)
    assert ops.par_plan(2, 3, 17, 32, num_iter=2, aligned16=True)["step"] == "recompute"
    arm = ops.par_plan(2, 3, 17, 32, num_iter=2, aligned16=False)
    assert arm["step"] == "stream" and arm["stats"] == "pointwise_planes"
    sm, out = A.shifted(masks), A.shifted(S_fill(torch.empty_like(masks)))
    for kw, what in ((dict(masks=sm), "masks"), (dict(masks=masks, out=out), "out"), (dict(masks=sm, out=out), "masks and out")):
        got = ops.par_forward(imgs, kw["masks"], num_iter=2, **({"out": kw["out"]} if "out" in kw else {}))
        assert torch.equal(got, want), f"par_forward with shifted {what}"
        assert got.data_ptr() == (out.data_ptr() if "out" in kw else got.data_ptr())
    assert torch.equal(ops.par_forward(A.shifted(imgs), masks, num_iter=2), want)
    # the ragged entry has the tile kernel alone: reason code 3 of excel_par_plan, EXCEL_ERR_ARG from the entry, a ValueError from ops
    plan = ops.RaggedPlan(SIZES, "cuda")
    assert ops.PAR_PLAN_REFUSALS[3] == "alignment"
    assert ops.par_plan(2, 3, *SIZES[1], num_iter=2, ragged=True, aligned16=False)["refused"] == "alignment"
    rimgs = dev(rs.standard_normal((2, 3, 16, 16)).astype(np.float32))
    rmasks = dev(SC.pitched(rs, plan, 3))
    rwant = ops.par_forward_ragged(rimgs, rmasks, plan, 3, num_iter=2)
    assert torch.equal(ops.par_forward_ragged(rimgs, A.shifted(rmasks), plan, 3, num_iter=2), rwant)      # an input: copied by ops
    rout = A.shifted(S_fill(torch.empty_like(rmasks)))
    with pytest.raises(ValueError, match="out must be 16-byte aligned"):
        ops.par_forward_ragged(rimgs, rmasks, plan, 3, num_iter=2, out=rout)
    torch.cuda.synchronize()
    assert bool((_bytes(rout) == POISON).all())


# ------------------------------------------------------------------ handles
def _shift_weights(w):
    return {k: A.shifted(torch.from_numpy(np.ascontiguousarray(v)), "cuda") for k, v in w.items()}


def test_handles_built_from_shifted_weights(ops):
    from oracle.vit import VitConfig, make_vit_weights
    rs = np.random.RandomState(42)
    cfg = VitConfig(width=128, layers=8, heads=2, patch=16, out_dim=64, input_resolution=64, n_surgery=5)
    w = make_vit_weights(cfg, seed=11)
    imgs = dev(rs.standard_normal((2, 3, 80, 80)).astype(np.float32))
    for mode in ("f32", "bf16x3"):
        outs = []
        for weights in (w, _shift_weights(w)):
            h = ops.VitHandle(weights, cfg.width, cfg.layers, cfg.heads, cfg.patch, cfg.out_dim, n_surgery=cfg.n_surgery, gemm_mode=mode)
            assert all(t.data_ptr() % 16 == 0 for t in h.t.values())
            outs.append(h.forward(imgs, want_w_aff=True, aff_layers=6, n_attn_out=2, want_feats=True, want_raw=True))
        torch.cuda.synchronize()
        S.assert_same_bits(outs[0], outs[1])
    dw = SC.decoder_weights(rs)
    feats = dev(rs.standard_normal((3, 2, 26, 64)).astype(np.float32))
    outs = [SC.decoder_handle(ops, weights).forward(feats) for weights in (dw, _shift_weights(dw))]
    torch.cuda.synchronize()
    S.assert_same_bits(outs[0], outs[1])
    tw = SC.text_weights(rs)
    tok = SC.text_tokens(rs)
    outs = [ops.TextHandle(weights, heads=2).encode(tok) for weights in (tw, _shift_weights(tw))]
    torch.cuda.synchronize()
    S.assert_same_bits(outs[0], outs[1])


# ------------------------------------------------------------------ ABI refusals
class _Mem:
    """Device memory of the refused calls: inputs of zeros (a valid index, a valid float), outputs and workspaces of 0xA5 bytes that must
    still be there at the end.  Every buffer is far larger than the tiny shapes of the calls."""

    def __init__(self, device="cuda"):
        self.outs = []
        self.device = device

    def zin(self, dtype=torch.float32, n=1 << 14):
        return torch.zeros(n, dtype=dtype, device=self.device)

    def out(self, dtype=torch.float32, n=1 << 14):
        t = S_fill(torch.empty(n, dtype=dtype, device=self.device))
        self.outs.append(t)
        return t

    def ws(self, nbytes):
        return self.out(torch.uint8, int(nbytes) + 4096)

    def check(self):
        if self.device == "cuda":
            torch.cuda.synchronize()
        for t in self.outs:
            assert bool((_bytes(t) == POISON).all()), "a refused call wrote to an output or a workspace"


def _handle_calls(ops, m, st, keep):
    """the entries behind a handle: tiny towers (2 ViT layers; the decoder and the text tower of the case tables); the handles are
    appended to `keep` in the order vit, decoder, text"""
    from oracle.vit import VitConfig, make_vit_weights
    L = ops.lib()
    f32, i32 = torch.float32, torch.int32
    calls = {}
    cfg = VitConfig(width=128, layers=2, heads=2, patch=16, out_dim=64, input_resolution=64, n_surgery=1)
    vit = ops.VitHandle(make_vit_weights(cfg, seed=5), cfg.width, cfg.layers, cfg.heads, cfg.patch, cfg.out_dim, n_surgery=1, gemm_mode="f32")
    need = int(L.excel_vit_workspace_bytes(vit._h, 1, 32))
    calls["excel_vit_forward_ex"] = [("h", vit._h), ("img", m.zin()), ("B", 1), ("S", 32), ("workspace", m.ws(need)), ("workspace_bytes", need + 4096),
                                     ("image_features", m.out()), ("x_raw", m.out()), ("w_aff", m.out()), ("aff_layers", 1), ("attn_out", None),
                                     ("n_attn_out", 0), ("feats_out", None), ("ex_attn", None), ("flags", 0), ("stream", st)]
    rs = np.random.RandomState(43)
    dec = SC.decoder_handle(ops, SC.decoder_weights(rs))
    g = 2
    feats = m.zin(f32, 3 * 1 * 5 * 64 + 64)
    need = int(L.excel_decoder_workspace_bytes(dec._h, 1, g))
    calls["excel_decoder_forward"] = [("h", dec._h), ("all_feats", feats), ("B", 1), ("g", g), ("workspace", m.ws(need)), ("workspace_bytes", need + 4096),
                                      ("attn_fts_out", m.out()), ("seg_out", m.out()), ("stream", st)]
    need = int(L.excel_decoder_train_workspace_bytes(dec._h, 1, g))
    tws = m.ws(need)
    calls["excel_decoder_forward_train"] = [("h", dec._h), ("all_feats", feats), ("B", 1), ("g", g), ("workspace", tws), ("workspace_bytes", need + 4096),
                                            ("seg_out", m.out()), ("attn_pred_out", m.out()), ("dropout_p", 0.0), ("dropout_seed", 0), ("stream", st)]
    calls["excel_decoder_train_attn_fts"] = [("h", dec._h), ("B", 1), ("g", g), ("workspace", tws), ("workspace_bytes", need + 4096),
                                             ("attn_fts_out", m.out()), ("stream", st)]
    _, gtable = dec._grad_table()
    calls["excel_decoder_backward"] = [("h", dec._h), ("all_feats", feats), ("B", 1), ("g", g), ("workspace", tws), ("workspace_bytes", need + 4096),
                                       ("d_seg", m.zin()), ("d_attn_pred", None), ("grads", C.byref(gtable)), ("dropout_p", 0.0), ("dropout_seed", 0),
                                       ("stream", st)]
    text = ops.TextHandle(SC.text_weights(rs), heads=2)
    need = int(L.excel_text_workspace_bytes(text._h, 1))
    calls["excel_text_encode"] = [("h", text._h), ("tokens", m.zin(i32)), ("B", 1), ("out", m.out()), ("workspace", m.ws(need)),
                                  ("workspace_bytes", need + 4096), ("stream", st)]
    keep += [vit, dec, text]
    return calls


def _abi_calls(ops, m, handles=True):
    """entry -> [(argument name, value)] in the entry's order: a tensor stands for its pointer, everything else goes as it is.
    handles=False leaves out the entries that need a ViT, decoder or text handle."""
    from excel_amd import _lib
    L = ops.lib()
    f32, u8, i16, i32, i64, f64 = torch.float32, torch.uint8, torch.int16, torch.int32, torch.int64, torch.float64
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream) if m.device == "cuda" else None
    plan = ops.RaggedPlan([SIZES[0], (9, 6)], m.device)        # sizes the case tables run
    par_plan = ops.RaggedPlan(SIZES, m.device)
    info, tab = C.byref(plan.info), plan.table
    keep = [plan, par_plan]
    calls = {}
    calls["excel_gemm_f32"] = [("A", m.zin()), ("Bm", m.zin()), ("C", m.out()), ("bias", m.zin()), ("residual", m.zin()), ("M", 8), ("N", 8), ("K", 8),
                               ("lda", 8), ("ldb", 8), ("ldc", 8), ("ldr", 8), ("b_kmajor", 1), ("act", 0), ("batch", 1), ("sA", 0), ("sB", 0), ("sC", 0),
                               ("sR", 0), ("stream", st)]
    for e in ("excel_split_bf16", "excel_split_f16"):
        calls[e] = [("in", m.zin()), ("out", m.out(i16)), ("rows", 4), ("K", 32), ("stream", st)]
    calls["excel_pack_f16"] = [("in", m.zin()), ("out", m.out(i16)), ("rows", 4), ("K", 32), ("inexact_dev", m.out(i64)), ("stream", st)]
    for e in ("excel_gemm_bf16x3", "excel_gemm_f16x3"):
        calls[e] = [("A_split", m.zin(i16)), ("W_split", m.zin(i16)), ("C", m.out()), ("bias", m.zin()), ("residual", m.zin()), ("M", 8), ("N", 32), ("K", 32),
                    ("act", 0), ("split_out", 0), ("stream", st)]
    calls["excel_gemm_f16x2"] = [("A_split", m.zin(i16)), ("W_split", m.zin(i16)), ("W_half", m.zin(i16)), ("C", m.out()), ("bias", m.zin()),
                                 ("residual", m.zin()), ("M", 8), ("N", 32), ("K", 32), ("act", 0), ("split_out", 0), ("stream", st)]
    calls["excel_layernorm"] = [("x", m.zin()), ("w", m.zin()), ("b", m.zin()), ("y", m.out()), ("rows", 4), ("D", 32), ("eps", 1e-5), ("stream", st)]
    vit = dec = text = None
    if handles:
        calls.update(_handle_calls(ops, m, st, keep))
        vit, dec, text = keep[-3:]
    need = int(L.excel_train_losses_workspace_bytes(1, 3, 4, 4))
    calls["excel_train_losses"] = [("seg", m.zin()), ("attn_pred", m.zin()), ("pseudo", m.zin(u8)), ("aff_labels", None), ("B", 1), ("nc", 3), ("g_h", 2),
                                   ("g_w", 2), ("H", 4), ("W", 4), ("radius", 1), ("ignore_index", 255), ("w_seg", 1.0), ("w_diver", 0.1),
                                   ("losses", m.out()), ("d_seg", m.out()), ("d_attn_pred", m.out()), ("workspace", m.ws(need)), ("stream", st)]
    seg = m.zin()
    segs = (C.c_void_p * 1)(seg.data_ptr())
    keep += [seg, segs]
    calls["excel_seg_msc_fuse_ragged"] = [("segs", segs), ("g", (C.c_int32 * 1)(2)), ("flip_mean", (C.c_int32 * 1)(0)), ("ns", 1), ("nc", 2), ("table", tab),
                                          ("info", info), ("planes", m.out()), ("labels_u8", None), ("stream", st)]
    need = int(L.excel_cam_workspace_bytes(1, 5, 3))
    calls["excel_clip_feature_surgery"] = [("image_features", m.zin()), ("text", m.zin()), ("B", 1), ("N", 5), ("C", 32), ("T", 3), ("F", 3),
                                           ("temperature", 2.0), ("out_full", m.out()), ("out_slice", None), ("workspace", m.ws(need)), ("stream", st)]
    need = int(L.excel_patch_text_cam_workspace_bytes(1, 5, 32, 3))
    calls["excel_patch_text_cam"] = [("x_raw", m.zin()), ("text", m.zin()), ("B", 1), ("N", 5), ("C", 32), ("T", 3), ("F", 3), ("temperature", 2.0),
                                     ("mode", 1), ("out_full", m.out()), ("out_slice", None), ("image_features", m.out()), ("workspace", m.ws(need)),
                                     ("stream", st)]
    calls["excel_attn_select_mean"] = [("attn", m.zin()), ("Lw", 2), ("B", 1), ("N", 5), ("first_layer", 0), ("n_layers", 2), ("seg_attn", m.zin()),
                                       ("w_out", m.out()), ("workspace", m.ws(L.excel_attn_select_workspace_bytes(1, 2))), ("stream", st)]
    calls["excel_feature_affinity"] = [("feats", m.zin()), ("B", 2), ("C", 6), ("P", 4), ("beta", 1.0), ("gamma", 3.0), ("mode", 0), ("out", m.out()),
                                       ("workspace", m.ws(L.excel_feature_affinity_workspace_bytes(2, 6, 4))), ("stream", st)]
    calls["excel_feature_affinity_grouped"] = [("feats", m.zin()), ("B", 2), ("C", 6), ("P", 4), ("group", 1), ("member_stride", 1), ("beta", 1.0),
                                               ("gamma", 3.0), ("mode", 0), ("out", m.out()),
                                               ("workspace", m.ws(L.excel_feature_affinity_grouped_workspace_bytes(2, 6, 4, 1))), ("stream", st)]
    calls["excel_compute_trans_mat"] = [("w_aff", m.zin()), ("B", 1), ("P", 4), ("trans_out", m.out()),
                                        ("workspace", m.ws(L.excel_trans_mat_workspace_bytes(1, 4))), ("stream", st)]
    dil = (C.c_int32 * 6)(*ops.PAR_DILATIONS)
    calls["excel_par_forward_ragged"] = [("imgs", m.zin()), ("h", 4), ("w", 4), ("masks", m.zin()), ("nchan", None), ("table", par_plan.table),
                                         ("info", C.byref(par_plan.info)), ("Cmax", 2), ("dilations", dil), ("ndil", 6), ("n_iter", 1), ("w1", 0.3), ("w2", 0.01), ("out", m.out()),
                                         ("workspace", m.ws(L.excel_par_ragged_workspace_bytes(par_plan.total_pix, 2))), ("stream", st)]
    calls["excel_argmax_label"] = [("cams", m.zin()), ("nchan", None), ("cls_idx", None), ("B", 1), ("Smax", 1), ("Cmax", 2), ("HW", 16),
                                   ("labels_u8", None), ("labels_i64", m.out(i64)), ("stream", st)]
    calls["excel_confusion_accumulate"] = [("gt", m.zin(u8)), ("pred", m.zin(u8)), ("n", 16), ("num_classes", 4), ("hist", m.out(i64)), ("stream", st)]
    calls["excel_confusion_accumulate_masked"] = [("gt", m.zin(u8)), ("pred", m.zin(u8)), ("B", 1), ("per_image", 16), ("table", None), ("info", None),
                                                  ("skip", m.zin(i32)), ("num_classes", 4), ("hist", m.out(i64)), ("stream", st)]
    calls["excel_clip_tags"] = [("x_cls", m.zin()), ("stride", 32), ("text", m.zin()), ("B", 1), ("C", 32), ("T", 3), ("F", 2), ("scale", 100.0),
                                ("rel_thre", 0.2), ("kmax", 1), ("onehot_out", m.out()), ("scores_out", None), ("stream", st)]
    calls["excel_cam_upsample_bkg_ragged"] = [("refined", m.zin()), ("ncls", m.zin(i32)), ("table", tab), ("info", info), ("g", 2), ("Smax", 1),
                                              ("cams", m.out()), ("workspace", m.ws(2 * 1 * 4 * 4)), ("flags", 1), ("stream", st)]       # refined [2,1,4]
    calls["excel_cam_overlay_ragged"] = [("hwc", m.zin(u8)), ("cams", m.zin()), ("Cmax", 2), ("ncls", m.zin(i32)), ("out_off", m.zin(i64)), ("table", tab),
                                         ("info", info), ("mode", 1), ("tables", m.zin(f64)), ("out", m.out(u8)), ("stream", st)]
    calls["excel_cam_overlay"] = [("hwc", m.zin(u8)), ("cams", m.zin()), ("k", 1), ("H", 4), ("W", 4), ("mode", 0), ("tables", m.zin(f64)),
                                  ("out", m.out(u8)), ("stream", st)]
    mean3 = (C.c_float * 3)(0.5, 0.5, 0.5)
    calls["excel_train_panels"] = [("img", m.zin()), ("attr", None), ("cls_label", None), ("pseu_aff", None), ("pseu_mid", None), ("seg_gt", None),
                                   ("seg_pred", None), ("B", 1), ("F", 0), ("P", 0), ("g", 1), ("S", 4), ("nrow", 1), ("panel_mask", 1), ("mean", mean3),
                                   ("std", mean3), ("jet", m.zin(f64)), ("palette", m.zin(u8)), ("out", m.out(u8)), ("out_bytes", 1 << 14), ("stream", st)]
    hw = np.ascontiguousarray(plan.hw, np.int32)
    png_arena = sum(int(L.excel_png_labels_bound_bytes(int(h), int(w))) for h, w in hw)
    png_ws = int(L.excel_png_labels_workspace_bytes(2, int(hw[:, 0].max())))
    hw_p = hw.ctypes.data_as(C.POINTER(C.c_int32))
    keep.append(hw)
    calls["excel_png_encode_labels_ragged"] = [("labels", m.zin(u8)), ("table", tab), ("info", info), ("hw", hw_p), ("palette", m.zin(u8)),
                                               ("arena", m.out(u8, png_arena + 4096)), ("arena_bytes", png_arena), ("out_table", m.out(i64)),
                                               ("workspace", m.ws(png_ws)), ("workspace_bytes", png_ws), ("stream", st)]
    joff = np.array([0, 3 * SIZES[0][0] * SIZES[0][1]], np.int64)
    keep.append(joff)
    jpeg_ws = int(L.excel_jpeg_rgb_workspace_bytes(hw_p, 2))
    calls["excel_jpeg_encode_rgb_ragged"] = [("rgb", m.zin(u8)), ("off", joff.ctypes.data_as(C.POINTER(C.c_int64))), ("hw", hw_p), ("n", 2), ("quality", 75),
                                             ("arena", m.out(u8)), ("arena_bytes", 1 << 14), ("out_table", m.out(i64)),
                                             ("workspace", m.ws(jpeg_ws)), ("workspace_bytes", jpeg_ws), ("stream", st)]
    crf = (1.0, 1.0, 1.0, 1.0, 1.0)
    calls["excel_dcrf_inference"] = [("rgb_hwc", m.zin(u8)), ("prob", m.zin()), ("prob_is_energy", 0), ("H", 4), ("W", 4), ("C", 2), ("iters", 1),
                                     *[(n, v) for n, v in zip(("pos_w", "pos_xy_std", "bi_w", "bi_xy_std", "bi_rgb_std"), crf)], ("q_out", m.out()),
                                     ("workspace", m.ws(L.excel_dcrf_workspace_bytes(4, 4, 2))), ("stream", st)]
    need = C.c_size_t(0)
    assert L.excel_dcrf_ragged_workspace_bytes(plan.total_label_pix, 2, C.byref(need)) == 0
    calls["excel_dcrf_inference_ragged"] = [("hwc", m.zin(u8)), ("unary", m.zin()), ("unary_is_energy", 0), ("table", tab), ("info", info), ("C", 2),
                                            ("iters", 1), *[(n, v) for n, v in zip(("pos_w", "pos_xy_std", "bi_w", "bi_xy_std", "bi_rgb_std"), crf)],
                                            ("labels_u8", m.out(u8)), ("q_out", None), ("workspace", m.ws(need.value)), ("stream", st)]
    nch = np.array([2, 2], np.int32)
    keep.append(nch)
    i32p = C.POINTER(C.c_int32)
    assert L.excel_dcrf_lam_ragged_workspace_bytes(hw_p, nch.ctypes.data_as(i32p), 2, C.byref(need)) == 0
    two = torch.full((1 << 10,), 2, dtype=i32, device=m.device)
    calls["excel_dcrf_lam_ragged"] = [("hwc", m.zin(u8)), ("cams", m.zin()), ("nchan", two), ("nchan_host", nch.ctypes.data_as(i32p)), ("cls_idx", None),
                                      ("table", tab), ("info", info), ("smax", 1), ("Cmax", 2), ("iters", 1),
                                      *[(n, v) for n, v in zip(("pos_w", "pos_xy_std", "bi_w", "bi_xy_std", "bi_rgb_std"), crf)],
                                      ("labels_u8", m.out(u8)), ("q_out", None), ("workspace", m.ws(need.value)), ("stream", st)]
    return calls, keep, (vit, dec, text, _lib)


def _invoke(L, entry, args, shifted_arg=None):
    vals = []
    for name, v in args:
        if isinstance(v, torch.Tensor):
            p = v.data_ptr()
            assert p % 16 == 0
            if name == shifted_arg:
                p += min(4, v.element_size())                    # 4 bytes; 2 for the 16-bit planes, 1 for uint8 workspaces
            v = C.c_void_p(p)
        vals.append(v)
    return getattr(L, entry)(*vals)


def test_abi_refuses_every_pointer_below_its_alignment(ops):
    L = ops.lib()
    m = _Mem()
    calls, keep, (vit, dec, text, _lib) = _abi_calls(ops, m)
    torch.cuda.synchronize()
    refused = []
    for entry, arg, nbytes in A.above_4():
        if arg == "weights":
            continue
        assert entry in calls, f"ALIGN holds {entry}({arg}) to {nbytes} bytes: no call for it here"
        args = calls[entry]
        assert isinstance(dict(args)[arg], torch.Tensor), (entry, arg)
        rc = _invoke(L, entry, args, arg)
        msg = L.excel_last_error().decode()
        assert rc == -1, f"{entry}({arg} {min(4, dict(args)[arg].element_size())} bytes past a 16-byte boundary) returned {rc}: {msg}"
        said = msg.split(": ", 1)[-1]                     # "<who>: <argument> must be N-byte aligned" (or a list of arguments in front of it)
        assert re.search(rf"(^|[ ,]){re.escape(arg)}\b[^:]*-byte aligned", said), f"{entry}({arg}): the error does not name the argument: {msg!r}"
        refused.append((entry, arg))
    # the weight tables of the three *_create entries: a top-level pointer and one inside a block
    top = ("conv1_w", "class_emb", "pos_emb", "ln_pre_w", "ln_pre_b", "ln_post_w", "ln_post_b", "proj")

    def vit_create(field, block=None):
        w = _lib.VitWeights()
        for f in top:
            setattr(w, f, vit.t[f].data_ptr())
        blocks = (_lib.VitBlockWeights * 2)()
        C.memmove(blocks, vit.blocks, C.sizeof(blocks))
        w.blocks = blocks
        tgt = w if block is None else blocks[block]
        setattr(tgt, field, getattr(tgt, field) + 4)
        c = vit.cfg
        pos_grid = int(round((vit.t["pos_emb"].shape[0] - 1) ** 0.5))
        cfg = _lib.VitConfig(c["width"], c["layers"], c["heads"], c["patch"], c["out_dim"], c["n_surgery"], pos_grid)
        h = C.c_void_p()
        return L.excel_vit_create(C.byref(cfg), C.byref(w), C.byref(h)), h

    for field, block in (("ln_pre_w", None), ("proj", None), ("fc1_b", 1), ("in_proj_w", 0)):
        rc, h = vit_create(field, block)
        msg = L.excel_last_error().decode()
        assert rc == -1 and not h.value and field in msg and "16-byte aligned" in msg, (field, rc, msg)

    def dec_create(field, where):
        w = _lib.DecoderWeights()
        fuse = (_lib.FuseLayerWeights * dec.cfg["vit_layers"])()
        C.memmove(fuse, dec.fuse, C.sizeof(fuse))
        blocks = (_lib.DecoderBlockWeights * dec.cfg["dec_layers"])()
        C.memmove(blocks, dec.blocks, C.sizeof(blocks))
        w.fuse, w.blocks = fuse, blocks
        for f in ("fuse_w", "fuse_b", "pred_w", "pred_b"):
            setattr(w, f, dec.t[f].data_ptr())
        tgt = {"top": w, "fuse": fuse[1], "block": blocks[1]}[where]
        setattr(tgt, field, getattr(tgt, field) + 4)
        c = dec.cfg
        cfg = _lib.DecoderConfig(c["vit_layers"], c["vit_width"], c["embed"], c["dec_layers"], c["heads"], c["num_classes"])
        h = C.c_void_p()
        return L.excel_decoder_create(C.byref(cfg), C.byref(w), C.byref(h)), h

    for field, where in (("pred_w", "top"), ("proj2_w", "fuse"), ("ln2_b", "block")):
        rc, h = dec_create(field, where)
        msg = L.excel_last_error().decode()
        assert rc == -1 and not h.value and field in msg and "16-byte aligned" in msg, (field, rc, msg)

    def text_create(field, block=None):
        w = _lib.TextWeights()
        for f in ("token_embedding", "positional_embedding", "ln_final_w", "ln_final_b", "text_projection"):
            setattr(w, f, text.t[f].data_ptr())
        blocks = (_lib.DecoderBlockWeights * text.cfg["layers"])()
        C.memmove(blocks, text.blocks, C.sizeof(blocks))
        w.blocks = blocks
        tgt = w if block is None else blocks[block]
        setattr(tgt, field, getattr(tgt, field) + 4)
        c = text.cfg
        cfg = _lib.TextConfig(c["vocab_size"], c["context_length"], c["width"], c["layers"], c["heads"], c["embed_dim"])
        h = C.c_void_p()
        return L.excel_text_create(C.byref(cfg), C.byref(w), C.byref(h)), h

    for field, block in (("text_projection", None), ("out_proj_w", 0)):
        rc, h = text_create(field, block)
        msg = L.excel_last_error().decode()
        assert rc == -1 and not h.value and field in msg and "16-byte aligned" in msg, (field, rc, msg)
    m.check()
    assert len(refused) >= 70
    # every call is valid but for the one pointer: as it stands the entry takes it (this writes the outputs, so it comes last)
    for entry, args in calls.items():
        rc = _invoke(L, entry, args)
        assert rc == 0, f"{entry}: the call of this table is refused unshifted too (rc {rc}): {L.excel_last_error().decode()}"
    torch.cuda.synchronize()
    del keep
