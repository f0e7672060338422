"""The split-plane GEMM's kernel selection (excel_gemm_plan, gemm_plan.hip) is host arithmetic: it is pinned here, on the CPU, for every
GEMM shape the ViT forward and the GPU tests run, in every mode and output form they use, on 256 and on 304 compute units.
The expected plans (tests/golden/gemm_plans.txt) were recorded by running the pre-planner launcher's selection code in a host-only harness
that logged each kernel launch (instance, grid, block, mixed-height / two-instance split) in place of launching it."""
import os

import pytest

from excel_amd import ops

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "gemm_plans.txt")
MODES = {1: "bf16x3", 2: "f16x3", 3: "f16x2"}
OUTS = {0: "plain", 1: "qkv", 2: "split"}


def _rows():
    rows = []
    for line in open(GOLDEN):
        if line.startswith("#"):
            continue
        problem, plan = line.split(":")
        rows.append((tuple(map(int, problem.split())), tuple(map(int, plan.split()))))
    return rows


def test_gemm_plan_matches_the_recorded_selection():
    rows = _rows()
    assert len(rows) > 1000 and {r[0][8] for r in rows} == {256, 304}
    bad = []
    for (M, N, K, batch, out, res, mode, half, n_cu), want in rows:
        p = ops.gemm_plan(M, N, K, n_cu, mode=MODES[mode], batch=batch, out=OUTS[out], residual=bool(res), half=bool(half))
        got = (ops.GEMM_PLAN_KERNELS.index(p["kernel"]), p["tile"], p["nt_m"], p["x2"], p["tall"], p["shrt"], p["second"],
               p["grid_x"], p["grid_y"], p["block"])
        if got != want:
            bad.append(((M, N, K, batch, out, res, mode, half, n_cu), want, got))
    assert not bad, f"{len(bad)} plans differ, first: {bad[:3]}"
    # every kind of plan is in the table
    assert {r[1][0] for r in rows} == {0, 1, 2, 3} and {r[1][3] for r in rows} == {0, 1, 2}


def test_gemm_plan_rejects_bad_arguments():
    with pytest.raises(RuntimeError, match="gemm_plan"):
        ops.gemm_plan(0, 768, 768, 256)
    with pytest.raises(RuntimeError, match="gemm_plan"):
        ops.gemm_plan(25120, 768, 768, 0)
