"""The fused patch-text CAM's kernel selection (excel_patch_text_cam_plan, cam_plan.hip) is host arithmetic: it is pinned here, on the
CPU, for every T in 1..512, every C in 32, 64, ..., 1024 and every mode.  The expected values are the tables below, written out by hand
from the rules in tests/_cam_cases.py, not a recording of the code under test.  The completeness test then requires that the cases of the
GPU sweeps (tests/_cam_cases.py x three modes, and CAM_CASES of test_gpu_wide_vocab.py) reach every instance the selection can name.

The second half checks the GPU sweep's own yardstick (tests/_cam_cases.py) on the CPU: the float64 reference against the fp32 oracle at
every case, and that the comparison rejects four defects a kernel could have at every case where they can show."""
import ctypes as C

import numpy as np
import pytest

import _cam_cases as K
import oracle
from excel_amd import ops
from excel_amd._lib import lib

ALL_MODES = ("f32", "bf16x3", "f16x3", "f16x2")
BUILD = {"f32": None, "bf16x3": "bf16", "f16x3": "f16", "f16x2": "f16"}      # which split-type build of cam.hip a mode runs (f16x2 runs as f16x3)
WIDTHS = tuple(range(32, 1025, 32))
TLDS_WIDTHS = (256, 512)                                                     # C <= 512 and C % 256 == 0
OTHER_WIDTHS = tuple(c for c in WIDTHS if c not in TLDS_WIDTHS)
# (first T, last T, widths) -> (kernel, class tiles, text bank in LDS, pitch of the min / max table)
SPLIT_TABLE = [
    (1, 32, TLDS_WIDTHS, ("narrow", 1, True, 128)),
    (33, 48, TLDS_WIDTHS, ("narrow", 2, True, 128)),
    (1, 48, OTHER_WIDTHS, ("narrow", 2, False, 128)),
    (49, 64, WIDTHS, ("narrow", 2, False, 128)),
    (65, 128, WIDTHS, ("narrow", 4, False, 128)),
    (129, 512, WIDTHS, ("wide", 0, False, 512)),
]
F32_TABLE = [
    (1, 32, WIDTHS, ("narrow", 1, False, 128)),
    (33, 64, WIDTHS, ("narrow", 2, False, 128)),
    (65, 128, WIDTHS, ("narrow", 4, False, 128)),
    (129, 512, WIDTHS, ("wide", 0, False, 512)),
]
# the instance column of the case table: case -> ((class tiles, LDS text bank) in the split modes, class tiles in f32)
CASE_INSTANCES = {
    (2, 37, 256, 20, 20): ((1, True), 1), (3, 129, 512, 32, 7): ((1, True), 1), (2, 65, 256, 33, 20): ((2, True), 2),
    (1, 50, 512, 48, 48): ((2, True), 2), (1, 50, 512, 49, 20): ((2, False), 2), (1, 37, 96, 64, 64): ((2, False), 2),
    (1, 33, 768, 45, 20): ((2, False), 2), (1, 37, 64, 65, 65): ((4, False), 4), (1, 37, 160, 97, 80): ((4, False), 4),
    (1, 33, 1024, 128, 128): ((4, False), 4), (1, 513, 64, 9, 4): ((2, False), 1), (2, 5, 32, 3, 2): ((2, False), 1),
    (1, 17, 32, 1, 1): ((2, False), 1),
}
# N -> workgroups per image, by hand: 4 tiles of 32 tokens per workgroup, so 128 tokens each
GROUPS = {1: 1, 5: 1, 32: 1, 33: 1, 128: 1, 129: 2, 256: 2, 257: 3, 513: 5, 785: 7, 1025: 9}


def cdiv(a, b):
    return -(-a // b)


def _expand(table):
    out = {}
    for lo, hi, widths, inst in table:
        for T in range(lo, hi + 1):
            for c in widths:
                assert (T, c) not in out, (T, c)
                out[(T, c)] = inst
    return out


def _instance(p, mode):
    return (p["kernel"], p["split"], p["ct"], p["tlds"], p["finish_pitch"], BUILD[mode])


def test_selection_tables_cover_the_domain_once():
    """The hand-written tables against their own defining property (no library involved): every (T, C) exactly once."""
    for table in (SPLIT_TABLE, F32_TABLE):
        assert sorted(_expand(table)) == [(T, c) for T in range(1, 513) for c in WIDTHS]


@pytest.mark.parametrize("mode", ALL_MODES)
def test_cam_plan_every_T_and_C(mode):
    want = _expand(F32_TABLE if mode == "f32" else SPLIT_TABLE)
    B, N = 3, 197
    for (T, c), (kernel, ct, tlds, pitch) in want.items():
        p = ops.cam_plan(B, N, c, T, mode=mode)
        assert p == dict(kernel=kernel, split=mode != "f32", ct=ct, tlds=tlds, groups=2, prep_grid=(4, B, cdiv(c, 256) + 1), sim_grid=(2, B),
                         block=256, finish_grid=(4, B), finish_pitch=pitch), (T, c)


@pytest.mark.parametrize("mode", ALL_MODES)
def test_cam_plan_grids(mode):
    for N, G in GROUPS.items():
        for B in (1, 2, 5):
            for c, T in ((32, 3), (512, 45), (768, 103), (1024, 300)):
                p = ops.cam_plan(B, N, c, T, mode=mode)
                assert p["groups"] == G == cdiv(cdiv(N, 32), 4) and p["sim_grid"] == (G, B) and p["block"] == 256, (N, B, c, T)
                assert p["prep_grid"] == (cdiv(N, 64), B, cdiv(c, 256) + 1) and p["finish_grid"] == (cdiv(N, 64), B), (N, B, c, T)
                assert p["finish_pitch"] == (128 if T <= 128 else 512)


def test_cam_plan_of_the_cases():
    assert sorted(CASE_INSTANCES) == sorted(K.CASES) and len(set(K.CASES)) == len(K.CASES)
    for case, ((ct_s, tlds), ct_f) in CASE_INSTANCES.items():
        B, N, c, T, F = case
        assert 1 <= F <= T and N <= 513
        for mode in ALL_MODES:
            p = ops.cam_plan(B, N, c, T, mode=mode)
            want = (ct_f, False) if mode == "f32" else (ct_s, tlds)
            assert (p["kernel"], p["ct"], p["tlds"]) == ("narrow",) + want, (case, mode)


def test_cam_plan_rejects_bad_arguments():
    for bad in ((0, 37, 64, 9), (1, 0, 64, 9), (1, 37, 64, 0), (1, 37, 64, 513), (1, 37, 0, 9), (1, 37, 16, 9), (1, 37, 48, 9),
                (1, 37, 1056, 9), (70000, 37, 64, 9), (1, (1 << 20) + 1, 64, 9), (1, 37, 64, -3)):
        with pytest.raises(RuntimeError, match="patch_text_cam_plan"):
            ops.cam_plan(*bad)
    plan = (C.c_int32 * 14)()
    assert lib().excel_patch_text_cam_plan(1, 37, 64, 9, 4, plan) != 0      # no such gemm_mode
    assert lib().excel_patch_text_cam_plan(1, 37, 64, 9, -1, plan) != 0
    assert lib().excel_patch_text_cam_plan(1, 37, 64, 9, 1, None) != 0
    assert lib().excel_patch_text_cam_plan(1, 37, 64, 9, 1, plan) == 0
    assert lib().excel_abi_version() >= 5


def test_cases_reach_every_instance():
    """Every (kernel, split, class tiles, LDS text bank, table pitch, split-type build) the selection names anywhere in its domain is
    launched by a case of the GPU sweeps.  An instance added to the dispatch without a case fails here; so does a case taken away."""
    from test_gpu_wide_vocab import CAM_CASES as WIDE_CASES
    # the rows that share an instance differ in what they are the smallest of (tests/_cam_cases.py): none may go
    assert sorted(K.CASES) == sorted(CASE_INSTANCES), sorted(set(CASE_INSTANCES) ^ set(K.CASES))
    domain = {_instance(ops.cam_plan(1, 37, c, T, mode=mode), mode) for mode in ALL_MODES for T in range(1, 513) for c in WIDTHS}
    reached = {_instance(ops.cam_plan(B, N, c, T, mode=mode), mode) for (B, N, c, T, F) in list(K.CASES) + list(WIDE_CASES) for mode in K.MODES}
    assert len(domain) == 14                                        # 5 split instances x 2 builds + 4 exact-fp32 ones
    assert reached == domain, sorted(domain - reached, key=str)
    # each narrow instance has to be reached by the narrow cases alone
    narrow = {i for i in domain if i[0] == "narrow"}
    assert {_instance(ops.cam_plan(B, N, c, T, mode=mode), mode) for (B, N, c, T, F) in K.CASES for mode in K.MODES} == narrow


# ---------------------------------------------------------------------------------------------------- the sweep's yardstick, on the CPU
def _oracle(x, t, temp=2.0):
    """the fp32 numpy oracle test_patch_text_cam_fused compares against: clip.py:353, then clip_feature_surgery"""
    f = (x / np.sqrt((x * x).sum(axis=1, keepdims=True, dtype=np.float32))).astype(np.float32)
    with np.errstate(all="ignore"):
        return f, oracle.cam.clip_feature_surgery(f, t, t=temp)


@pytest.mark.parametrize("case", K.CASES, ids=str)
def test_ref64_agrees_with_the_oracle(case):
    """The GPU bounds (2e-5 / 6e-5) were set against the fp32 oracle; they carry over to ref64 because the two agree 40x closer than
    the tightest of them at these shapes (measured: maps <= 2.4e-7, features <= 9.5e-8), and no class plane has a small span (>= 0.198)
    that would amplify an error of the similarities."""
    x, t, f, maps = K.reference(case)
    of, om = _oracle(x, t)
    print(f"\n[cam-cases] {case} oracle vs ref64: maps {K.max_abs_err(om, maps):.3e} (5e-7), features {K.max_abs_err(of, f):.3e} (2e-7), "
          f"smallest span {K.min_span(x, t):.3f}")
    assert K.same_nan_mask(om, maps) and not np.isnan(f).any()
    assert K.max_abs_err(om, maps) < 5e-7 and K.max_abs_err(of, f) < 2e-7
    if case in K.DEGENERATE:
        assert np.isnan(maps).all() and np.isnan(om).all()           # T = 1: 0 / 0 everywhere
    else:
        assert not np.isnan(maps).any() and K.min_span(x, t) >= 0.1
        assert maps.min() == 0.0 and maps.max() == 1.0


@pytest.mark.parametrize("temp", K.TEMPS)
@pytest.mark.parametrize("case", K.TEMP_CASES, ids=str)
def test_ref64_agrees_with_the_oracle_at_other_temperatures(case, temp):
    x, t, f, maps = K.reference(case, temp)
    _, om = _oracle(x, t, temp)
    print(f"\n[cam-cases] {case} t = {temp:g} oracle vs ref64: maps {K.max_abs_err(om, maps):.3e} (5e-7), smallest span {K.min_span(x, t, temp):.3f}")
    assert K.same_nan_mask(om, maps) and K.max_abs_err(om, maps) < 5e-7 and K.min_span(x, t, temp) >= 0.1
    assert K.max_abs_err(K.reference(case)[3], maps) > 1e-2         # and the temperature matters


@pytest.mark.parametrize("case", [c for c in K.CASES if c not in K.DEGENERATE], ids=str)
def test_comparison_rejects_wrong_maps(case):
    """Four defects of a kernel, applied to ref64: each has to exceed the loosest bound of the GPU sweep (6e-5) at every case."""
    x, t, _, maps = K.reference(case)
    assert K.cls_is_an_extreme(maps), "the cls token holds no min / max here: the min / max-without-cls mutant cannot show (change the seed)"
    names = [m for m in K.MUTANTS if m != "temp_2.001" or case in K.TEMP_MUTANT_CASES]
    assert len(names) >= 4
    for name in names:
        err = K.max_abs_err(K.mutant64(name, x, t), maps)
        print(f"\n[cam-cases] {case} mutant {name}: {err:.3e}")
        assert err > K.TOL_SPLIT, name
    assert K.TOL_SPLIT == max(K.TOL_MAPS.values()) >= K.TOL_UNFUSED


def test_comparison_functions():
    ref = np.array([[0.0, np.nan], [1.0, 0.5]])
    assert K.max_abs_err(ref, ref) == 0.0 and K.same_nan_mask(ref, ref)
    got = ref.copy()
    got[1, 1] = 0.75
    assert K.max_abs_err(got, ref) == 0.25 and K.same_nan_mask(got, ref)
    got[0, 1] = 3.0                                                 # a number where the reference has none: only the mask test sees it
    assert K.max_abs_err(got, ref) == 0.25 and not K.same_nan_mask(got, ref)
    got = ref.copy()
    got[0, 0] = np.nan                                              # no number where the reference has one: both see it
    assert K.max_abs_err(got, ref) == float("inf") and not K.same_nan_mask(got, ref)
    allnan = np.full((2, 2), np.nan)
    assert K.max_abs_err(allnan, allnan) == 0.0 and K.same_nan_mask(allnan, allnan) and not K.same_nan_mask(ref, allnan)
