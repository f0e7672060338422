"""Every F.interpolate(mode='bilinear') site of the library that can be called alone, pinned bit for bit to ops.bilinear_resize: they
all sample through linear_tap + bilinear_blend (csrc/excel_internal.h), so a site that restates the rule in its own spelling - other
fused multiply-adds, other bits - fails here.  Each result is also held to oracle.interp.bilinear_resize within 1e-5 of max |o|, the
gate of test_gpu_seg_eval.py for the same operation.  (The fused kernels seg_msc_fuse_ragged and lam_tta_fuse are pinned to chains of
these ops in test_gpu_seg_eval.py / test_gpu_lam_tta.py, PAR's align_corners=True guide resize in test_gpu_par_shapes.py.)"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

B = 2
# (h, w) -> (H, W): up and non-square, down, identity, both clamps at once; the square-grid ops take g = h
CASES = [((3, 3), (7, 5)), ((5, 4), (3, 2)), ((4, 4), (4, 4)), ((1, 1), (3, 2))]
GRIDS = [3, 5, 4, 1]


@pytest.fixture(scope="module")
def gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from excel_amd import _lib
    _lib.lib()
    return torch.device("cuda")


def _r(x, H, W):
    from excel_amd import ops
    return ops.bilinear_resize(x, H, W, align_corners=False)


def _o(x, H, W):
    from oracle.interp import bilinear_resize
    return bilinear_resize(x.cpu().numpy(), H, W).astype(np.float64)


def _close(got, o):
    err = np.abs(got.cpu().numpy().astype(np.float64) - o).max() / np.abs(o).max()
    print(f"err / max|o| = {err:.3e}")
    assert err <= 1e-5, err


@pytest.mark.parametrize("hw,HW", CASES)
def test_seg_scale_accumulate(gpu, hw, HW):
    from excel_amd import ops
    (h, w), (H, W) = hw, HW
    segs = torch.randn(2 * B, 2, h, w, generator=torch.Generator().manual_seed(h * 10 + w)).to(gpu)
    a, m = segs[:B], segs[B:]
    plain = ops.seg_scale_accumulate(segs, None, H, W, flip_mean=False, init=True, scale=1.0)
    assert torch.equal(plain, _r(a, H, W))
    _close(plain, _o(a, H, W))
    v = (_r(a, H, W) + _r(m, H, W).flip(-1)) / 2
    o = (_o(a, H, W) + _o(m, H, W)[..., ::-1]) / 2
    mean = ops.seg_scale_accumulate(segs, None, H, W, flip_mean=True, init=True, scale=1.0)
    assert torch.equal(mean, v)
    _close(mean, o)
    acc = plain.clone()
    second = ops.seg_scale_accumulate(segs, acc, H, W, flip_mean=True, init=False, scale=0.5)
    assert torch.equal(second, (plain + v) * 0.5)
    _close(second, (_o(a, H, W) + o) * 0.5)


@pytest.mark.parametrize("g,HW", [(g, HW) for g, (_, HW) in zip(GRIDS, CASES)])
def test_lam_scale_accumulate(gpu, g, HW):
    from excel_amd import ops
    H, W = HW
    F = 3
    maps = torch.randn(2 * B, g * g, F, generator=torch.Generator().manual_seed(g)).to(gpu)
    planes = maps.permute(0, 2, 1).reshape(2 * B, F, g, g).contiguous()
    a, m = planes[:B], planes[B:]
    v = torch.maximum(_r(a, H, W), _r(m, H, W).flip(-1))
    o = np.maximum(_o(a, H, W), _o(m, H, W)[..., ::-1])
    first = ops.lam_scale_accumulate(maps, None, g, H, W, init=True)
    assert torch.equal(first, v)
    _close(first, o)
    acc = first.clone()
    second = ops.lam_scale_accumulate(maps, acc, g, H, W, init=False)
    assert torch.equal(second, first + v)
    _close(second, o + o)


@pytest.mark.parametrize("side,g", [(3, 5), (5, 3), (4, 4)])
def test_pos_embed_resize(gpu, side, g):
    from excel_amd import ops
    D = 8
    pos = torch.randn(side * side + 1, D, generator=torch.Generator().manual_seed(side)).to(gpu)
    out = ops.pos_embed_resize(pos, g)
    assert out.shape == (g * g + 1, D)
    assert torch.equal(out[0], pos[0])
    grid = pos[1:].t().reshape(1, D, side, side).contiguous()
    assert torch.equal(out[1:], _r(grid, g, g).reshape(D, g * g).t())
    _close(out[1:], _o(grid, g, g).reshape(D, g * g).T)
