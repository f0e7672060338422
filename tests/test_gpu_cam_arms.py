"""The fused patch-text CAM (excel_patch_text_cam) at every narrow kernel instance it dispatches on, in both split-type builds, against
a float64 reference.

The cases, the reference and the comparison are tests/_cam_cases.py: the smallest shapes that reach each instance of
patch_text_sim_kernel and each edge inside it (LDS text bank rows and DMA pieces, padded class tiles, the x prefetch ring, the column-norm
partial sum, ragged and dead token tiles, T = 1).  tests/test_host_cam_plan.py pins the selection on the CPU, requires these cases to reach
every instance, and shows that the comparison rejects wrong maps.  Bounds: features 1e-6; maps and slice 2e-5 exact fp32 and unfused,
6e-5 split-plane (test_gpu_ops.py::test_patch_text_cam_fused's own: the oracle they were set against is within 2.4e-7 of the reference
here).  Every test prints its figures before asserting them."""
import numpy as np
import pytest

import _cam_cases as K
from test_gpu_ops import dev as _dev, host

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")


def dev(a):
    return _dev(np.array(a))                                          # (the cached reference arrays are read-only: upload a copy)


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from excel_amd import ops as _ops
    return _ops


def _say(what, got, bound):
    print(f"\n[cam-arms] {what}: {got:.3e} (bound {bound:g})")


def _check_fused(ops, case, mode, temp=2.0):
    """one fused call with every output against ref64; -> (full, slice) on the device"""
    B, N, C, T, F = case
    x, t, f, maps = K.reference(case, temp)
    xd, td = dev(x), dev(t)
    full, sl, feats = ops.patch_text_cam(xd, td, num_fg=F, t=temp, want_full=True, want_features=True, mode=mode)
    e_feats, e_full, e_sl = K.max_abs_err(host(feats), f), K.max_abs_err(host(full), maps), K.max_abs_err(host(sl), maps[:, 1:, :F])
    tol = K.TOL_MAPS[mode]
    _say(f"fused {mode} {case} t={temp:g} features", e_feats, K.TOL_FEATURES)
    _say(f"fused {mode} {case} t={temp:g} maps", e_full, tol)
    _say(f"fused {mode} {case} t={temp:g} slice", e_sl, tol)
    assert tuple(full.shape) == (B, N, T) and tuple(sl.shape) == (B, N - 1, F) and tuple(feats.shape) == (B, N, C)
    assert not np.isnan(host(feats)).any() and e_feats < K.TOL_FEATURES
    assert K.same_nan_mask(host(full), maps) and K.same_nan_mask(host(sl), maps[:, 1:, :F])
    assert e_full < tol and e_sl < tol
    assert torch.equal(sl.view(torch.int32), full[:, 1:, :F].contiguous().view(torch.int32))        # bitwise (NaNs included)
    _, sl_only, none = ops.patch_text_cam(xd, td, num_fg=F, t=temp, mode=mode)                      # slice only, no feature write
    assert none is None and torch.equal(sl_only.view(torch.int32), sl.view(torch.int32))
    return xd, td, full, sl


@pytest.mark.parametrize("mode", K.MODES)
@pytest.mark.parametrize("case", K.CASES, ids=str)
def test_patch_text_cam_arm(ops, case, mode):
    B, N, C, T, F = case
    xd, td, full, sl = _check_fused(ops, case, mode)
    if case in K.DEGENERATE:
        assert torch.isnan(full).all() and torch.isnan(sl).all()
    if B > 1:
        # batch invariance, bit for bit: image b alone has the bits of its rows of the batch, and a second batched call repeats the first
        for b in range(B):
            f1, s1, _ = ops.patch_text_cam(xd[b:b + 1].contiguous(), td, num_fg=F, want_full=True, mode=mode)
            assert torch.equal(f1[0].view(torch.int32), full[b].view(torch.int32)), b
            assert torch.equal(s1[0].view(torch.int32), sl[b].view(torch.int32)), b
        full2, sl2, _ = ops.patch_text_cam(xd, td, num_fg=F, want_full=True, mode=mode)
        assert torch.equal(full2.view(torch.int32), full.view(torch.int32)) and torch.equal(sl2.view(torch.int32), sl.view(torch.int32))


@pytest.mark.parametrize("case", K.CASES, ids=str)
def test_clip_feature_surgery_arm(ops, case):
    """The unfused path (similarity GEMM + cam_epilogue_kernel) on the fp32 features: T = 1, 64, 65, 128 and N = 5 (eleven of the
    epilogue kernel's sixteen waves own no token row) are new to it."""
    B, N, C, T, F = case
    _, t, f, maps = K.reference(case)
    full, sl = ops.clip_feature_surgery(dev(f.astype(np.float32)), dev(t), num_fg=F)
    err = K.max_abs_err(host(full), maps)
    _say(f"unfused {case} maps", err, K.TOL_UNFUSED)
    assert tuple(full.shape) == (B, N, T) and tuple(sl.shape) == (B, N - 1, F)
    assert K.same_nan_mask(host(full), maps) and err < K.TOL_UNFUSED
    assert torch.equal(sl.view(torch.int32), full[:, 1:, :F].contiguous().view(torch.int32))
    if case in K.DEGENERATE:
        assert torch.isnan(full).all()


@pytest.mark.parametrize("temp", K.TEMPS)
@pytest.mark.parametrize("mode", K.MODES)
@pytest.mark.parametrize("case", K.TEMP_CASES, ids=str)
def test_patch_text_cam_temperature(ops, case, mode, temp):
    """A temperature other than the default 2 reaches the class-prior softmax (both of its lane values at T = 65), same bounds."""
    _check_fused(ops, case, mode, temp)
