"""The DenseCRF message passing of the device (excel_amd/csrc/crf.hip), one message at a time, against a float64 filter over the same
lattice and against the exact Gaussian kernel (tests/_dcrf_filter_ref.py; tests/test_host_dcrf_filter.py holds the oracle to the same).
iters = 1 with energies and one pairwise weight 1, the other 0, gives Q = softmax(-U + m); log Q_k - log Q_0 + U_k - U_0 reads the class
differences of that one splat / blur / slice / normalisation back, with no mean-field iterations on top to amplify or hide an error.
The per-image entry on every case, the production weights, the exact anchor, the degenerate shapes through the full chain, and the two
group entries (excel_dcrf_inference_ragged, excel_dcrf_lam_ragged) against the reference of every image alone.

Measured on an MI355X (max |recovered - float64| of the fp32 oracle / of the device; then, on the anchor cases, max distance of the
recovered differences to the exact kernel's, oracle / device):
  noise_half-24x30-C3-1_67_3     gauss     3.84e-07 / 2.91e-07   0.052434 / 0.052434
  noise_half-24x30-C3-1_67_3     bilateral 4.78e-07 / 3.34e-07   0.263255 / 0.263255
  noise_half-37x29-C5-3_50_5     gauss     4.11e-07 / 3.42e-07   0.008918 / 0.008918
  noise_half-37x29-C5-3_50_5     bilateral 4.32e-07 / 5.23e-07   0.118318 / 0.118318
  smooth-24x30-C3-3_80_13        gauss     3.91e-07 / 3.30e-07   0.012454 / 0.012454
  smooth-24x30-C3-3_80_13        bilateral 3.55e-07 / 3.40e-07   0.088310 / 0.088310
  smooth-37x29-C5-3_80_13        gauss     3.81e-07 / 3.89e-07   0.007982 / 0.007982
  smooth-37x29-C5-3_80_13        bilateral 4.70e-07 / 3.72e-07   0.051398 / 0.051397
  distinct-24x30-C3-1_67_3       gauss     3.85e-07 / 2.87e-07
  distinct-24x30-C3-1_67_3       bilateral 4.69e-07 / 5.11e-07
  uniform-24x30-C3-1_67_3        gauss     3.85e-07 / 3.33e-07
  uniform-24x30-C3-1_67_3        bilateral 4.85e-07 / 3.33e-07
  uniform-37x29-C5-3_50_5        gauss     4.56e-07 / 3.29e-07
  uniform-37x29-C5-3_50_5        bilateral 4.48e-07 / 3.47e-07
  extremes-24x30-C3-3_80_13      gauss     3.43e-07 / 3.01e-07
  extremes-24x30-C3-3_80_13      bilateral 4.50e-07 / 4.31e-07
  extremes-37x29-C5-1_67_3       gauss     4.44e-07 / 4.22e-07
  extremes-37x29-C5-1_67_3       bilateral 5.46e-07 / 3.63e-07
  distinct-24x30-C3-1_67_1       gauss     3.92e-07 / 3.15e-07
  distinct-24x30-C3-1_67_1       bilateral 3.98e-07 / 3.90e-07
  distinct-37x29-C5-3_50_5       gauss     4.67e-07 / 4.29e-07
  distinct-37x29-C5-3_50_5       bilateral 4.56e-07 / 4.25e-07
  smooth-80x72-C21-1_67_3        gauss     5.12e-07 / 5.12e-07
  smooth-80x72-C21-1_67_3        bilateral 5.57e-07 / 4.79e-07
  extremes-2x2-C2-1_67_3         gauss     6.52e-08 / 6.52e-08
  extremes-2x2-C2-1_67_3         bilateral 1.21e-07 / 1.65e-07
  distinct-2x2-C2-3_80_13        gauss     1.17e-07 / 6.39e-08
  distinct-2x2-C2-3_80_13        bilateral 1.27e-07 / 1.27e-07
  uniform-1x1-C3-1_67_3          gauss     4.16e-08 / 1.04e-07
  uniform-1x1-C3-1_67_3          bilateral 4.16e-08 / 1.04e-07
  noise_half-1x1-C3-3_80_13      gauss     7.67e-08 / 1.76e-08
  noise_half-1x1-C3-3_80_13      bilateral 7.67e-08 / 1.76e-08
  noise_half-1x40-C2-1_67_3      gauss     2.37e-07 / 1.78e-07   0.103117 / 0.103117
  noise_half-1x40-C2-1_67_3      bilateral 3.49e-07 / 3.71e-07   0.064457 / 0.064457
  smooth-1x40-C2-3_80_13         gauss     2.38e-07 / 2.53e-07   0.029749 / 0.029749
  smooth-1x40-C2-3_80_13         bilateral 2.21e-07 / 2.21e-07   0.147690 / 0.147690
  smooth-33x1-C4-1_67_3          gauss     2.95e-07 / 3.13e-07   0.071044 / 0.071044
  smooth-33x1-C4-1_67_3          bilateral 3.39e-07 / 2.85e-07   0.109367 / 0.109367
  noise_half-33x1-C4-3_80_13     gauss     2.68e-07 / 2.15e-07   0.024210 / 0.024210
  noise_half-33x1-C4-3_80_13     bilateral 3.13e-07 / 2.42e-07   0.059856 / 0.059856
  both messages: noise_half 24x30 (3,4) 1.12e-06 / 1.02e-06, smooth 24x30 (3,10) 1.32e-06 / 1.48e-06, noise_half 37x29 (3,10) 2.32e-06 / 2.32e-06
  ragged group (gauss, bilateral per image): 3.42e-07 / 3.26e-07, 4.62e-07 / 4.25e-07; 3.16e-07 / 2.55e-07, 3.02e-07 / 2.13e-07; 2.95e-07 / 2.95e-07, 3.38e-07 / 2.60e-07
  LAM group:                                 4.59e-07 / 6.55e-07, 5.94e-07 / 6.65e-07; 2.24e-07 / 4.38e-07, 3.59e-07 / 3.59e-07; 3.97e-07 / 4.83e-07, 2.99e-07 / 4.91e-07
Before crf_lattice_kernel ran with contraction off (its elevated[j] = sm - j * cf had become an fma) the device stood at 2.16e-06 on
distinct 24x30 (1,67,1) bilateral (bound 1.59e-06), 1.11e-06 on noise_half 24x30 (1,67,3) bilateral and 4.55e-06 with the weights (3,4)
(bound 4.48e-06): the barycentric weights were off the algorithm's by up to 2e-5, which shows wherever pixels couple through few
blur neighbours."""
import numpy as np
import pytest

import _dcrf_filter_ref as R

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")


@pytest.fixture(scope="module")
def gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from excel_amd import _lib
    _lib.lib()
    return torch.device("cuda")


def _ids(cases):
    return [c.id for c in cases]


def _device_q(gpu, img, U, iters, wg, wb, params):
    from excel_amd import ops
    sxy, bxy, brgb = params
    q = ops.dcrf_inference(torch.from_numpy(img).to(gpu), torch.from_numpy(np.ascontiguousarray(U, np.float32)).to(gpu), iters, wg, sxy, wb, bxy,
                           brgb, is_energy=True)
    return q.cpu().numpy()


_Q = {}


def _message_q(gpu, case, wg, wb):
    """Q of the device at iters = 1 on a case, computed once per (case, weights) and shared."""
    key = (case.id, wg, wb)
    if key not in _Q:
        _Q[key] = _device_q(gpu, case.image(), case.energies(), 1, wg, wb, case.params)
    return _Q[key]


def _check(ref, q, wg, wb, what):
    """The recovered differences of q meet the bound of the reference; -> (device error, bound)."""
    assert np.isfinite(q).all(), what
    np.testing.assert_allclose(q.reshape(ref.C, -1).sum(0), 1.0, atol=1e-5)
    err, oracle, bound = ref.error(q, wg, wb), ref.oracle_error(wg, wb), ref.bound(wg, wb)
    print(f"\n{what}: device error = {err:.2e}, oracle error = {oracle:.2e}, bound = {bound:.2e}")
    assert err <= bound, f"{what}: recovered differences off by {err:.3e}, allowed {bound:.3e} (the fp32 oracle: {oracle:.3e})"
    return err, bound


@pytest.mark.parametrize("kernel", R.KERNELS)
@pytest.mark.parametrize("case", R.CASES, ids=_ids(R.CASES))
def test_one_message(gpu, case, kernel):
    """excel_dcrf_inference with one kernel alive: the recovered class differences equal the float64 filter's within 4 x the error of
    the fp32 oracle on the same case (floor 2^-21); Q is a distribution; a second run has the same bits."""
    ref = R.reference(case)
    wg, wb = R.ONE_OF[kernel]
    q = _message_q(gpu, case, wg, wb)
    _check(ref, q, wg, wb, f"{case.id} {kernel}")
    assert np.array_equal(q, _device_q(gpu, case.image(), case.energies(), 1, wg, wb, case.params))


def test_single_class(gpu):
    c = R.SINGLE_CLASS
    for iters in (1, 10):
        q = _device_q(gpu, c.image(), c.energies(), iters, *R.WEIGHTS[c.params], c.params)
        assert np.array_equal(q, np.ones((1, c.H, c.W), np.float32))


@pytest.mark.parametrize("case", R.BOTH, ids=_ids(R.BOTH))
def test_both_messages(gpu, case):
    """The production weights: the mixing t + w_g m_g + w_b m_b, same recovery, same rule for the bound."""
    ref = R.reference(case)
    w = tuple(float(v) for v in R.WEIGHTS[case.params])
    _check(ref, _message_q(gpu, case, *w), *w, f"{case.id} weights {w}")


@pytest.mark.parametrize("kernel", R.KERNELS)
@pytest.mark.parametrize("case", R.ANCHOR, ids=_ids(R.ANCHOR))
def test_exact_anchor(gpu, case, kernel):
    """The device's recovered differences lie as close to those of the exact kernel exp(-|f_i - f_j|^2 / 2) as the oracle's do: within
    the oracle's own distance on the case plus the bound of test_one_message (largest absolute difference, as there)."""
    ref = R.reference(case)
    wg, wb = R.ONE_OF[kernel]
    exact = ref.exact(kernel)
    dev = float(np.abs(R.recover(_message_q(gpu, case, wg, wb).reshape(case.C, -1), ref.U) - exact).max())
    oracle = float(np.abs(R.recover(ref.oracle_q(wg, wb), ref.U) - exact).max())
    print(f"\n{case.id} {kernel}: distance to the exact kernel: device {dev:.6f}, oracle {oracle:.6f} (differences up to {np.abs(exact).max():.3f})")
    assert dev <= oracle + ref.bound(wg, wb)


@pytest.mark.parametrize("case", R.DEGENERATE, ids=_ids(R.DEGENERATE))
def test_degenerate_shapes_through_the_full_chain(gpu, case):
    """One pixel, 2 x 2, one row, one column and one class through ten mean-field steps with the production weights, against
    oracle.dcrf.dense_crf_2d under test_dcrf_vs_oracle's rule."""
    import oracle
    img, U = case.image(), case.energies()
    wg, wb = R.WEIGHTS[case.params]
    sxy, bxy, brgb = case.params
    got = _device_q(gpu, img, U, 10, wg, wb, case.params)
    ref = oracle.dcrf.dense_crf_2d(img, U.reshape(case.C, -1), 10, wg, sxy, wb, bxy, brgb)
    assert got.shape == ref.shape and np.isfinite(got).all()
    np.testing.assert_allclose(got.sum(0), 1.0, atol=1e-5)
    err = float(np.abs(got - ref).max())
    print(f"\n{case.id}: max |Q - oracle| after 10 steps = {err:.3e}")
    assert err < 1e-3 and float(np.abs(got - ref).mean()) < 2e-5
    if case.C == 1:
        assert np.array_equal(got, np.ones_like(got))


# ------------------------------------------------------------------ the group entries
GROUP = [("smooth", 24, 30), ("noise_half", 1, 40), ("extremes", 33, 1)]
GROUP_SIZES = [(H, W) for _, H, W in GROUP]
GROUP_C = 4
LAM_NCHAN, LAM_CMAX = [4, 2, 3], 5
_GROUP = {}


def _group(lam):
    """Images, inputs and per-image references of the group: energies for the uniform entry, probabilities (their own class counts)
    for the LAM entry.  Computed once."""
    if lam not in _GROUP:
        imgs = [R.image(kind, H, W, 40 + b) for b, (kind, H, W) in enumerate(GROUP)]
        if lam:
            ins = [R.softmax64(R.energies(c, H, W, 50 + b).reshape(c, -1)).T.reshape(c, H, W).astype(np.float32)
                   for b, ((_, H, W), c) in enumerate(zip(GROUP, LAM_NCHAN))]
            refs = [R.Reference(i, R.LAM, prob=p) for i, p in zip(imgs, ins)]
        else:
            ins = [R.energies(GROUP_C, H, W, 60 + b) for b, (_, H, W) in enumerate(GROUP)]
            refs = [R.Reference(i, R.LAM, U=u) for i, u in zip(imgs, ins)]
        _GROUP[lam] = (imgs, ins, refs)
    return _GROUP[lam]


@pytest.mark.parametrize("kernel", R.KERNELS)
def test_ragged_group_against_the_reference(gpu, kernel):
    """excel_dcrf_inference_ragged on a group of 24x30, 1x40 and 33x1 (C = 4, energies): every image's recovered differences meet the
    bound of test_one_message against message64 of that image alone."""
    from excel_amd import ops
    imgs, us, refs = _group(False)
    wg, wb = R.ONE_OF[kernel]
    plan = ops.RaggedPlan(GROUP_SIZES, gpu)
    images = torch.from_numpy(np.concatenate([i.reshape(-1) for i in imgs])).to(gpu)
    unary = torch.from_numpy(np.concatenate([u.reshape(-1) for u in us])).to(gpu)
    _, q = ops.dcrf_inference_ragged(images, plan, unary, GROUP_C, 1, wg, R.LAM[0], wb, R.LAM[1], R.LAM[2], is_energy=True, want_labels=False,
                                     want_q=True)
    q = q.cpu().numpy()
    for b, (H, W) in enumerate(GROUP_SIZES):
        lo = GROUP_C * int(plan.loff[b])
        _check(refs[b], q[lo:lo + GROUP_C * H * W].reshape(GROUP_C, H, W), wg, wb, f"ragged image {b} {GROUP[b]} {kernel}")


@pytest.mark.parametrize("kernel", R.KERNELS)
def test_lam_group_against_the_reference(gpu, kernel):
    """excel_dcrf_lam_ragged on the same sizes with 4, 2 and 3 classes, probabilities on pitched planes (NaN in the pad columns and the
    unused planes), iters = 1: the recovery uses U = -log clip(p) computed on the host in float64."""
    from excel_amd import ops
    imgs, ps, refs = _group(True)
    wg, wb = R.ONE_OF[kernel]
    plan = ops.RaggedPlan(GROUP_SIZES, gpu)
    images = torch.from_numpy(np.concatenate([i.reshape(-1) for i in imgs])).to(gpu)
    cams = np.full(LAM_CMAX * plan.total_pix, np.nan, np.float32)
    for b, p in enumerate(ps):
        c, H, W = p.shape
        Wp = (W + 3) // 4 * 4
        o = LAM_CMAX * int(plan.poff[b])
        cams[o:o + LAM_CMAX * H * Wp].reshape(LAM_CMAX, H, Wp)[:c, :, :W] = p
    nc = torch.tensor(LAM_NCHAN, dtype=torch.int32, device=gpu)
    _, q = ops.dcrf_lam_ragged(images, plan, torch.from_numpy(cams).to(gpu), LAM_CMAX, nc, LAM_NCHAN, None, 1, wg, R.LAM[0], wb, R.LAM[1], R.LAM[2],
                               want_labels=False, want_q=True)
    for b, c in enumerate(LAM_NCHAN):
        got = plan.planes(q, b, LAM_CMAX)[:c].cpu().numpy()
        _check(refs[b], got, wg, wb, f"LAM image {b} {GROUP[b]} C={c} {kernel}")
