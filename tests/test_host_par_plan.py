"""The kernel selection of the pixel-adaptive refinement (excel_par_plan, par_plan.hip) is host arithmetic: it is pinned here, on the
CPU, for every shape of the GPU sweep (tests/test_gpu_par_shapes.py) and at every boundary the launchers dispatch on.  The expected
values are the tables tests/_par_shapes.py writes out by hand from the rules in its docstring, not a recording of the code under test.

The second half checks the sweep's reference and gates on the CPU alone: the fp32 oracle stays within the precondition's cap of the
float64 judge on every sweep input, the gate accepts it, and wrong variants OF THE JUDGE (never of a kernel: nothing wrong runs on a
device) are rejected by the final gate with a factor of at least 4 to spare at one step."""
import ctypes as C

import numpy as np
import pytest

import _par_shapes as P
from excel_amd import ops


def test_tile_table_is_consistent():
    """The hand-written table against the stated rule (no library involved), and: every x kind and every y kind appears in the uniform
    recompute sweep and in the ragged batch."""
    for (H, W), (xs, ys) in P.TILES.items():
        assert len(xs) == P.cdiv(W, 64) and len(ys) == P.cdiv(H, 16), (H, W)
        assert xs == [P.x_kind(64 * i, W) for i in range(len(xs))], (H, W)
        assert ys == [P.y_kind(16 * j, H) for j in range(len(ys))], (H, W)
        for i, k in enumerate(xs):
            assert (k == "interior") == (64 * i - 24 >= 0 and 64 * i + 88 <= W)
    for shapes in ([s for s, (st, _) in P.RECOMPUTE.items() if st == "tile"], P.RAGGED_SIZES):
        assert {k for s in shapes for k in P.TILES[s][0]} == set(P.X_KINDS)
        assert {k for s in shapes for k in P.TILES[s][1]} == set(P.Y_KINDS)
    assert all(s in P.TILES for s in P.RAGGED_SIZES) and all(s in P.TILES for s in P.RECOMPUTE)
    assert all(W % 4 for (_, W) in P.STREAMED) and all(W % 4 == 0 for (_, W) in P.RECOMPUTE)
    # 1 and 2 steps everywhere, 5 on three shapes, 20 on one
    its = [it for (_, it) in P.RECOMPUTE.values()]
    assert all(i[:2] == (1, 2) for i in its) and sum(5 in i for i in its) == 3 and sum(20 in i for i in its) == 1


@pytest.mark.parametrize("shape", list(P.RECOMPUTE) + list(P.STREAMED), ids=lambda s: f"{s[0]}x{s[1]}")
def test_par_plan_of_the_uniform_sweep(shape):
    H, W = shape
    for n_iter in (1, 2, 20):
        for stream in (False, True):
            assert ops.par_plan(P.B, P.CMAX, H, W, num_iter=n_iter, stream_affinities=stream) == P.expected_plan(H, W, n_iter, stream=stream), \
                (shape, n_iter, stream)
    # n_iter = 0: the statistics launch of the streamed arm and no step
    want = dict(P.expected_plan(H, W, 0, stream=True), step="none", step_grid=(0, 0, 0), step_block=0)
    assert ops.par_plan(P.B, P.CMAX, H, W, num_iter=0) == want
    # a resized guide changes nothing but the flag
    assert ops.par_plan(P.B, P.CMAX, H, W, num_iter=2, guide_hw=(32, 48)) == P.expected_plan(H, W, 2, guide_hw=(32, 48))
    # buffers that are not 16-byte aligned: streamed
    assert ops.par_plan(P.B, P.CMAX, H, W, num_iter=2, aligned16=False) == P.expected_plan(H, W, 2, stream=True)


@pytest.mark.parametrize("shape", P.RAGGED_SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_par_plan_of_the_ragged_sweep(shape):
    H, W = shape
    for n in (1, 5):
        assert ops.par_plan(n, P.CMAX, H, W, num_iter=2, ragged=True, guide_hw=P.RAGGED_INPUT) == P.expected_plan(H, W, 2, ragged=True, n=n)
    assert ops.par_plan(1, P.CMAX, H, W, num_iter=2, ragged=True)["resize"] is True          # (H, W) == (h, w) too


def test_par_plan_other_dilation_sets():
    H, W = P.OTHER_SHAPE
    for nd, dil in P.OTHER_DILATIONS.items():
        assert len(dil) == nd
        assert ops.par_plan(P.B, P.CMAX, H, W, dilations=dil, num_iter=2) == P.expected_plan(H, W, 2, dil=dil)
        # ... also at a shape the tile kernels would take with the standard set
        p = ops.par_plan(P.B, P.CMAX, 40, 88, dilations=dil, num_iter=2)
        assert (p["stats"], p["nd"], p["step"], p["tiles_interior"], p["tiles_border"]) == ("pointwise_planes", nd, "stream", 0, 0)
    for nd in (1, 4, 8):
        p = ops.par_plan(1, 2, 40, 88, dilations=tuple(range(1, nd + 1)), num_iter=1)
        assert (p["stats"], p["nd"], p["step"]) == ("pointwise_planes", nd, "stream")
    assert ops.par_plan(1, 2, 40, 88, dilations=(1, 2, 4, 8, 12, 25))["step"] == "stream"      # six, but not the standard set
    assert ops.par_plan(1, 2, 40, 88, dilations=(24, 12, 8, 4, 2, 1))["step"] == "stream"      # ... or not in its order


# W: (statistics, step, interior tiles, border tiles) at H = 16 - by hand: 4 the pointwise statistics; 8 the smallest tile-kernel width;
# 151 / 153 W % 4 != 0; 152 the smallest width with an interior tile (x0 = 64: 40 >= 0, 152 <= 152); 148 / 156 its neighbours
W_BOUNDARIES = {4: ("pointwise_compact", "recompute", 0, 1), 5: ("pointwise_planes", "stream", 0, 0), 8: ("tile", "recompute", 0, 1),
                12: ("tile", "recompute", 0, 1), 148: ("tile", "recompute", 0, 3), 151: ("pointwise_planes", "stream", 0, 0),
                152: ("tile", "recompute", 1, 2), 153: ("pointwise_planes", "stream", 0, 0), 156: ("tile", "recompute", 1, 2),
                216: ("tile", "recompute", 2, 2), 448: ("tile", "recompute", 5, 2)}


def test_par_plan_width_and_height_boundaries():
    for W, (stats, step, ni, nb) in W_BOUNDARIES.items():
        p = ops.par_plan(1, 2, 16, W, num_iter=1)
        assert (p["stats"], p["step"], p["tiles_interior"], p["tiles_border"]) == (stats, step, ni, nb), W
    # ragged: any width, the same interior rule
    for W, ni, nb in ((151, 0, 3), (152, 1, 2), (153, 1, 2), (3, 0, 1), (5, 0, 1)):
        p = ops.par_plan(1, 2, 16, W, num_iter=1, ragged=True)
        assert (p["stats"], p["step"], p["tiles_interior"], p["tiles_border"], p["refused"]) == ("tile", "recompute", ni, nb, None), W
    # H = 71 / 72: five tile rows both; 72 is the smallest height with a row whose halos are both unclamped (the table's "M")
    for H in (71, 72):
        p = ops.par_plan(2, 2, H, 152, num_iter=1)
        assert p["stats_grid"] == p["step_grid"] == (3, 5, 2) and (p["tiles_interior"], p["tiles_border"]) == (5, 10)
    assert "M" not in [P.y_kind(16 * j, 71) for j in range(5)] and [P.y_kind(16 * j, 72) for j in range(5)].count("M") == 1
    assert ops.par_plan(2, 2, 64, 152, num_iter=1)["stats_grid"] == (3, 4, 2) and ops.par_plan(2, 2, 65, 152, num_iter=1)["stats_grid"] == (3, 5, 2)


def test_par_plan_size_limits():
    """32-bit LDS-DMA offsets inside one image: max(Cmax, 5) * H * Wp * 4 < 2^31."""
    H, W = 8192, 13104                                                    # 5 * H * W * 4 = 2^31 - 524288
    assert 5 * H * W * 4 < 2 ** 31 <= 5 * H * (W + 4) * 4
    assert ops.par_plan(1, 5, H, W, num_iter=1)["step"] == "recompute" and ops.par_plan(1, 1, H, W, num_iter=1)["stats"] == "tile"
    assert ops.par_plan(1, 6, H, W, num_iter=1)["step"] == "stream"       # Cmax counts beyond 5 planes
    p = ops.par_plan(1, 5, H, W + 4, num_iter=1)
    assert (p["stats"], p["step"]) == ("pointwise_planes", "stream")
    assert ops.par_plan(1, 5, H, W, num_iter=1, ragged=True)["refused"] is None
    assert ops.par_plan(1, 6, H, W, num_iter=1, ragged=True)["refused"] == "size"
    assert ops.par_plan(1, 5, H, W + 1, num_iter=1, ragged=True)["refused"] == "size"      # the pitch counts: Wp = W + 4


def test_par_plan_ragged_refusals():
    """What excel_par_forward_ragged refuses, in its order: n_iter < 1, another dilation set, alignment, size."""
    zero = dict(resize=False, stats="tile", nd=0, step="none", stats_grid=(0, 0, 0), stats_block=0, step_grid=(0, 0, 0), step_block=0,
                tiles_interior=0, tiles_border=0)
    assert ops.par_plan(2, 3, 40, 151, num_iter=0, ragged=True) == dict(zero, refused="n_iter")
    assert ops.par_plan(2, 3, 40, 151, num_iter=0, ragged=True, dilations=(1, 2))["refused"] == "n_iter"
    assert ops.par_plan(2, 3, 40, 151, num_iter=1, ragged=True, dilations=(1, 2)) == dict(zero, refused="dilations")
    assert ops.par_plan(2, 3, 40, 151, num_iter=1, ragged=True, dilations=(1, 2), aligned16=False)["refused"] == "dilations"
    assert ops.par_plan(2, 3, 40, 151, num_iter=1, ragged=True, aligned16=False) == dict(zero, refused="alignment")
    assert ops.par_plan(2, 3, 40, 151, num_iter=1, ragged=True)["refused"] is None


def test_par_plan_rejects_bad_arguments():
    for bad in ((0, 2, 16, 16), (1, 0, 16, 16), (1, 2, 0, 16), (1, 2, 16, 0), (1, 2, 16, -4), (70000, 2, 16, 16)):
        with pytest.raises(RuntimeError, match="par_plan"):
            ops.par_plan(*bad)
    for kw in (dict(dilations=(1,) * 9), dict(dilations=(1, 0)), dict(num_iter=-1), dict(guide_hw=(0, 8))):
        with pytest.raises(RuntimeError, match="par_plan"):
            ops.par_plan(1, 2, 16, 16, **kw)
    from excel_amd._lib import lib
    plan, dil = (C.c_int32 * 15)(), (C.c_int32 * 6)(*P.DIL)
    L = lib().excel_par_plan
    assert L(1, 2, 16, 16, 16, 16, dil, 6, 1, 0, 0, 1, plan) == 0
    assert L(1, 2, 16, 16, 16, 16, dil, 6, 1, 2, 0, 1, plan) != 0          # no such flag
    assert L(1, 2, 16, 16, 16, 16, dil, 6, 1, 0, 2, 1, plan) != 0          # ragged, aligned16 are 0 / 1
    assert L(1, 2, 16, 16, 16, 16, dil, 6, 1, 0, 0, -1, plan) != 0
    assert L(1, 2, 16, 16, 16, 16, dil, 0, 1, 0, 0, 1, plan) != 0
    assert L(1, 2, 16, 16, 16, 16, None, 6, 1, 0, 0, 1, plan) != 0
    assert L(1, 2, 16, 16, 16, 16, dil, 6, 1, 0, 0, 1, None) != 0


# ---------------------------------------------------------------------------------------------------- the sweep's judge and gates, on the CPU
def _accept(J, o, tag):
    assert not P.precondition(J, o), (tag, P.precondition(J, o))
    assert not P.numerics_failures(o, o), tag                           # the fp32 oracle itself passes the gate (its err is o)


@pytest.mark.parametrize("kind", list(P.GUIDES))
def test_oracle_meets_the_precondition_uniform(kind):
    worst = 0.0
    for (H, W), (_, iters) in P.RECOMPUTE.items():
        g, m, J, o = P.uniform_case(H, W, kind, iters)
        for it in iters:
            _accept(J[it], o[it], (H, W, kind, it))
            worst = max(worst, o[it])
    print(f"[par-shapes] oracle32 vs float64, uniform recompute shapes, {kind}: worst {worst:.2e}")


def test_oracle_meets_the_precondition_elsewhere():
    for (H, W), iters in P.STREAMED.items():
        for w12 in ((0.3, 0.01),) + ((P.W12,) if (H, W) == P.OTHER_SHAPE else ()):
            g, m, J, o = P.uniform_case(H, W, "noise", iters, P.DIL, w12)
            for it in iters:
                _accept(J[it], o[it], (H, W, it, w12))
    for nd, dil in P.OTHER_DILATIONS.items():
        g, m, J, o = P.uniform_case(*P.OTHER_SHAPE, "noise", (1, 2), dil)
        for it in (1, 2):
            _accept(J[it], o[it], (nd, it))
    g, m, J, o = P.uniform_case(40, 148, "noise", (1, 2), P.DIL, P.W12)
    for it in (1, 2):
        _accept(J[it], o[it], ("w12", it))
    for kind, w12 in (("noise", (0.3, 0.01)), ("photo", (0.3, 0.01)), ("noise", P.W12)):
        g, ms, Js, os_ = P.ragged_case(kind, P.RAGGED_ITERS, w12)
        for b in range(len(P.RAGGED_SIZES)):
            for it in P.RAGGED_ITERS:
                _accept(Js[b][it], os_[b][it], (kind, w12, b, it))


def test_photo_guide_is_what_it_says():
    g = P.guide("photo", P.B, 40, 148)
    u8 = np.rint(g.transpose(0, 2, 3, 1).astype(np.float64) * P.VOC_STD + P.VOC_MEAN)
    assert np.abs(u8 - (g.transpose(0, 2, 3, 1).astype(np.float64) * P.VOC_STD + P.VOC_MEAN)).max() < 1e-4 and u8.min() >= 0 and u8.max() <= 255
    nb = P.neighbors64(g.astype(np.float64), P.DIL)
    assert (nb.std(axis=2, ddof=1) == 0).all(1).any(), "no pixel whose 48 taps are exactly constant in all three channels"


VARIANTS = ("biased", "nopos", "w2_1pct", "swap_taps", "clamp_w2", "swap_hw")


@pytest.mark.parametrize("variant", VARIANTS)
def test_gate_rejects_a_wrong_judge(variant):
    """Each wrong variant of the judge, at one step, lies at least 4 gate widths from the judge: biased instead of unbiased std, the
    position term dropped, w2 off by 1 %, two taps of d = 1 exchanged, the right-border taps of the last tile column clamped to W - 2,
    the guide resized with h and w exchanged (on the ragged batch's non-square input)."""
    if variant == "swap_hw":
        H, W = P.RAGGED_SIZES[1]
        g, m = P.guide("noise", 1, *P.RAGGED_INPUT), P.masks(1, P.CMAX, H, W)
        J = P.judge(g, m)[1]
        o = P.maxabs(P.oracle32(g, m)[1], J)
    else:
        H, W = 40, 152
        g, m = P.guide("noise", P.B, H, W), P.masks(P.B, P.CMAX, H, W)
        J = P.judge(g, m, nchan=P.NCHAN)[1]
        o = P.maxabs(P.oracle32(g, m, nchan=P.NCHAN)[1], J)
    assert not P.precondition(J, o)
    bad = P.judge(g, m, nchan=None if variant == "swap_hw" else P.NCHAN, variant=variant)[1]
    err = P.maxabs(bad, J)
    print(f"[par-shapes] wrong judge {variant}: moves the result by {err:.3e}; gate {P.bound(o):.3e} (o {o:.3e})")
    assert P.numerics_failures(err, o)
    assert err >= 4 * P.bound(o)


def test_gate_constants():
    assert P.K == 2 * P.MEASURED_RATIO and P.CEILING < P.OLD_BOUND
    assert P.bound(0.0) == P.K * P.O_FLOOR < P.CEILING and P.bound(1.0) == P.OLD_BOUND
