"""The pixel-adaptive refinement (excel_par_forward, excel_par_forward_ragged) at every tile kind and kernel arm it dispatches on,
against a float64 judge.

The shapes, the dispatch table, the judge, the two guides and the gates are tests/_par_shapes.py: the smallest shapes at which each kind
of 64 x 16 tile exists (left / interior / right-full / right-partial / single columns; top-clamped / middle / bottom-clamped / partial
rows), on the uniform recompute arm, the streamed arm and a ragged batch with a non-square network input, with non-default w1 / w2 and
with the dilation sets that run the other instances of the pointwise kernel.  Every case first asserts excel_par_plan against the
hand-written table, then the precondition on the reference alone (the fp32 oracle within 5e-6 of the judge), then runs the device and
asserts err <= K x max(o, 1e-6).  tests/test_host_par_plan.py pins the plan on the CPU and shows that the gate rejects wrong variants of
the judge.  Every test prints its figures before asserting them."""
import numpy as np
import pytest

import _par_shapes as P
from test_gpu_ops import dev as _dev, host

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")


def dev(a, dtype=None):
    return _dev(np.array(a), dtype)                                       # (the cached reference arrays are shared: upload a copy)


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from excel_amd import ops as _ops
    return _ops


def _gate(tag, got, J, o, nchan):
    """valid channels against the judge; the others were never written (zero in the library's fresh output tensor)"""
    err = P.maxabs(got, J)
    P.report(tag, err, o)
    assert not np.isnan(got).any(), tag
    for b, k in enumerate(nchan):
        assert not got[b, k:].any(), (tag, "a plane >= nchan was written")
    assert not P.numerics_failures(err, o), (tag, P.numerics_failures(err, o))
    return err


def _run_uniform(ops, H, W, kind, iters, dil=P.DIL, w12=(0.3, 0.01), stream=False):
    g, m, J, o = P.uniform_case(H, W, kind, iters, dil, w12)
    for it in iters:
        assert ops.par_plan(P.B, P.CMAX, H, W, dilations=dil, num_iter=it, stream_affinities=stream) == P.expected_plan(H, W, it, stream=stream, dil=dil)
        assert not P.precondition(J[it], o[it]), (H, W, kind, it, P.precondition(J[it], o[it]))
    gd, md, nch = dev(g), dev(m), dev(np.array(P.NCHAN, np.int32))
    outs = {}
    for it in iters:
        outs[it] = ops.par_forward(gd, md, dil, it, nchan=nch, w1=w12[0], w2=w12[1], stream_affinities=stream)
        _gate(f"{H}x{W} {kind} it={it} nd={len(dil)} w={w12} {'stream' if stream else 'auto'}", host(outs[it]), J[it], o[it], P.NCHAN)
    return gd, md, nch, outs


@pytest.mark.parametrize("kind", list(P.GUIDES))
@pytest.mark.parametrize("shape", list(P.RECOMPUTE), ids=lambda s: f"{P.RECOMPUTE[s][0]}+recompute-{P.tile_id(*s)}")
def test_par_recompute_arm(ops, shape, kind):
    """par_stats_tile_kernel<false> (W = 4: par_affinity_kernel<6,false> writing statistics) + par_iterate_guide_kernel<false>"""
    _run_uniform(ops, *shape, kind, P.RECOMPUTE[shape][1])


@pytest.mark.parametrize("shape", list(P.STREAMED), ids=lambda s: f"planes6+stream-{s[0]}x{s[1]}")
def test_par_streamed_arm(ops, shape):
    """W % 4 != 0: par_affinity_kernel<6,false> writing 48 planes + par_iterate_stream_kernel"""
    _run_uniform(ops, *shape, "noise", P.STREAMED[shape])


@pytest.mark.parametrize("kind", list(P.GUIDES))
@pytest.mark.parametrize("shape", list(P.STREAM_FLAG), ids=lambda s: f"stream-flag-equals-recompute-{P.tile_id(*s)}")
def test_par_stream_flag(ops, shape, kind):
    """EXCEL_PAR_STREAM_AFFINITIES on a shape the tile kernels take: within the gate, and the same bits as the recompute arm."""
    iters = P.STREAM_FLAG[shape]
    gd, md, nch, streamed = _run_uniform(ops, *shape, kind, iters, stream=True)
    for it in iters:
        assert torch.equal(streamed[it], ops.par_forward(gd, md, P.DIL, it, nchan=nch)), it


def _pack_nan(plan, ms, nchan):
    """per-image [Cmax,H,W] masks -> the packed pitched tensor; pad columns and planes >= nchan[b] hold NaN"""
    out = np.full(P.CMAX * plan.total_pix, np.nan, np.float32)
    for b, a in enumerate(ms):
        H, W = a.shape[-2:]
        Wp = (W + 3) // 4 * 4
        v = out[P.CMAX * plan.poff[b]:P.CMAX * plan.poff[b] + P.CMAX * H * Wp].reshape(P.CMAX, H, Wp)
        v[:nchan[b], :, :W] = a[:nchan[b]]
    return out


def _run_ragged(ops, kind, w12=(0.3, 0.01)):
    iters = P.RAGGED_ITERS
    g, ms, Js, os_ = P.ragged_case(kind, iters, w12)
    for b, (H, W) in enumerate(P.RAGGED_SIZES):
        assert ops.par_plan(1, P.CMAX, H, W, num_iter=2, ragged=True, guide_hw=P.RAGGED_INPUT) == P.expected_plan(H, W, 2, ragged=True, n=1)
        for it in iters:
            assert not P.precondition(Js[b][it], os_[b][it]), (b, it, P.precondition(Js[b][it], os_[b][it]))
    plan = ops.RaggedPlan(P.RAGGED_SIZES, "cuda")
    assert plan.total_tiles == sum(len(P.TILES[s][0]) * len(P.TILES[s][1]) for s in P.RAGGED_SIZES)
    gd, md, nch = dev(g), dev(_pack_nan(plan, ms, P.RAGGED_NCHAN)), dev(np.array(P.RAGGED_NCHAN, np.int32))
    for it in iters:
        out = ops.par_forward_ragged(gd, md, plan, P.CMAX, P.DIL, it, nchan=nch, w1=w12[0], w2=w12[1])
        for b, (H, W) in enumerate(P.RAGGED_SIZES):
            k = P.RAGGED_NCHAN[b]
            got = plan.planes(out, b, P.CMAX)[:k]
            tag = f"ragged {H}x{W} {kind} it={it} w={w12}"
            assert not torch.isnan(got).any(), tag                        # no NaN in any valid output element
            err = P.maxabs(host(got), Js[b][it][:k])
            P.report(tag, err, os_[b][it])
            assert not P.numerics_failures(err, os_[b][it]), (tag, P.numerics_failures(err, os_[b][it]))
            if W % 4 == 0:                                                # the uniform call runs the same tile kernels: the same bits
                uni = ops.par_forward(gd[b:b + 1], dev(ms[b][None, :k]), P.DIL, it, w1=w12[0], w2=w12[1])
                assert torch.equal(got, uni[0]), tag


@pytest.mark.parametrize("kind", list(P.GUIDES))
def test_par_ragged_nonsquare_input(ops, kind):
    """par_stats_tile_kernel<true> + par_iterate_guide_kernel<true> on a batch with every tile kind, guides resized from a 32 x 48 network
    input (bilinear_ac_ragged_kernel), NaN in the pad columns and in the planes >= nchan[b]; every image against the judge."""
    _run_ragged(ops, kind)


def test_par_w1_w2_recompute(ops):
    _run_uniform(ops, 40, 148, "noise", (1, 2), w12=P.W12)


def test_par_w1_w2_streamed(ops):
    _run_uniform(ops, *P.OTHER_SHAPE, "noise", (1, 2), w12=P.W12)


def test_par_w1_w2_ragged(ops):
    _run_ragged(ops, "noise", w12=P.W12)


@pytest.mark.parametrize("nd", list(P.OTHER_DILATIONS), ids=lambda nd: f"par_affinity_kernel-ND{nd}-planes")
def test_par_other_dilation_counts(ops, nd):
    """par_affinity_kernel<2>, <3>, <5>, <7> and <6> in plane form (six dilations other than the standard set) + the streamed step"""
    _run_uniform(ops, *P.OTHER_SHAPE, "noise", (1, 2), dil=P.OTHER_DILATIONS[nd])
