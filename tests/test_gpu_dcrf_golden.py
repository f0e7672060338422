"""excel_dcrf_inference against recorded bits: tests/golden/dcrf_per_image.npz holds inputs and the marginals the per-image entry gave
on an MI355X BEFORE the kernels learned to run groups of images (they now serve both entries).  The per-image path must still give
exactly those bits, and a group of one must as well.
The marginals were recorded again, on the same inputs, when crf_lattice_kernel stopped contracting elevated[j] = sm - j * cf into an
fma (tests/test_gpu_dcrf_filter.py found the barycentric weights off the algorithm's by up to 2e-5): the lattice weights changed in
their last bits, so every marginal after a message did (figures in DESIGN.md, "One message at a time")."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "dcrf_per_image.npz")


def test_per_image_entry_keeps_its_recorded_bits():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from excel_amd import ops
    g = np.load(GOLDEN)
    n = len([k for k in g.files if k.startswith("q")])
    assert n >= 3
    for i in range(n):
        img, p, q = g[f"img{i}"], g[f"prob{i}"], g[f"q{i}"]
        params = [int(g[f"params{i}"][0])] + [float(v) for v in g[f"params{i}"][1:]]
        dev = lambda a: torch.from_numpy(a).cuda()
        got = ops.dcrf_inference(dev(img), dev(p), *params).cpu().numpy()
        assert np.array_equal(got, q), f"case {i}: max |diff| {np.abs(got - q).max():.3e}"
        C, H, W = p.shape
        plan = ops.RaggedPlan([(H, W)], "cuda")
        _, q1 = ops.dcrf_inference_ragged(dev(img).view(-1), plan, dev(p).view(-1), C, *params, want_labels=False, want_q=True)
        assert np.array_equal(q1.view(C, H, W).cpu().numpy(), q), f"case {i}: group of one"
