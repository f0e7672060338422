"""Host side of the batched DenseCRF (excel_dcrf_inference_ragged): the C ABI declares and exports the new entries, the group workspace
(a host function of the group's pixel count) equals the per-image workspace for a group of one, grows with every image added and
refuses a group whose lattice vertices overflow the 32-bit indices, and ops.dcrf_groups cuts a batch into consecutive runs within a
memory budget.  No device is touched."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["excel_dcrf_ragged_workspace_bytes", "excel_dcrf_inference_ragged", "excel_seg_softmax_resize_ragged"]
SHAPES = [(1, 1), (3, 7), (37, 53), (375, 500), (480, 640), (500, 333)]


def _ws(hw, C):
    from excel_amd import ops
    return ops.dcrf_ragged_workspace_bytes(hw, C)


def test_new_entries_declared_exported_and_bound():
    from excel_amd import _lib
    src = open(os.path.join(ROOT, "include", "excel_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    handle = ctypes.CDLL(_lib.LIB_PATH)
    for n in NEW:
        assert re.search(r"\b%s\s*\(" % n, src), f"{n} is not declared in include/excel_hip.h"
        assert hasattr(handle, n), f"{n} is not exported"
        assert n in _lib.SIGNATURES
    _lib.lib()


@pytest.mark.parametrize("C", [1, 5, 21, 81])
def test_group_of_one_costs_what_the_image_costs(C):
    from excel_amd import _lib
    for H, W in SHAPES:
        assert _ws([(H, W)], C) == _lib.lib().excel_dcrf_workspace_bytes(H, W, C), (H, W, C)


@pytest.mark.parametrize("C", [5, 21, 81])
def test_workspace_grows_with_every_image(C):
    sizes = [(37, 53), (1, 1), (375, 500), (2, 3), (480, 640), (500, 333)]
    got = [_ws(sizes[:k], C) for k in range(1, len(sizes) + 1)]
    assert all(a < b for a, b in zip(got, got[1:])), got
    # a function of the pixel count alone: the order of the images does not matter
    assert _ws(sizes[::-1], C) == got[-1]


def test_vertex_overflow_is_refused():
    from excel_amd import _lib
    lib = _lib.lib()
    out = ctypes.c_size_t(123)
    for total in ((1 << 31) // 6 + 1, 1 << 31, 1 << 40):         # total * 6 no longer fits an int32 vertex index
        assert lib.excel_dcrf_ragged_workspace_bytes(total, 21, ctypes.byref(out)) != 0, total
        assert b"32-bit" in lib.excel_last_error()
        assert out.value == 123
    assert lib.excel_dcrf_ragged_workspace_bytes(0, 21, ctypes.byref(out)) != 0
    assert lib.excel_dcrf_ragged_workspace_bytes(100, 0, ctypes.byref(out)) != 0
    assert lib.excel_dcrf_ragged_workspace_bytes(100, 21, None) != 0
    assert lib.excel_dcrf_ragged_workspace_bytes(100, 21, ctypes.byref(out)) == 0 and out.value > 0
    with pytest.raises(RuntimeError, match="32-bit"):
        _ws([(40000, 40000)], 21)


def _check_runs(runs, sizes, C, budget):
    assert [s for s, _ in runs] == [0] + [e for _, e in runs[:-1]] and runs[-1][1] == len(sizes)     # every image once, in order
    assert all(e > s for s, e in runs)
    for k, (s, e) in enumerate(runs):
        if e - s > 1:
            assert _ws(sizes[s:e], C) <= budget
        else:
            # a single image: over the budget by itself, or the next image would not have fitted with it
            alone = _ws(sizes[s:e], C) > budget
            assert alone or e == len(sizes) or _ws(sizes[s:e + 1], C) > budget
        if e < len(sizes) and _ws(sizes[s:e], C) <= budget:
            assert _ws(sizes[s:e + 1], C) > budget, "the run stopped although the next image fits"


@pytest.mark.parametrize("C", [21, 81])
def test_dcrf_groups(C):
    from excel_amd import ops
    sizes = [(375, 500), (500, 333), (37, 53), (480, 640), (1, 1), (16, 3), (480, 640), (333, 500), (12, 12)]
    one = [_ws([s], C) for s in sizes]
    whole = _ws(sizes, C)
    assert ops.dcrf_groups(sizes, C, whole) == [(0, len(sizes))]
    assert ops.dcrf_groups(sizes, C, 1) == [(b, b + 1) for b in range(len(sizes))]           # every image is over the budget: all alone
    for budget in (max(one), 2 * max(one), max(one) + min(one), whole // 2, whole - 1):
        runs = ops.dcrf_groups(sizes, C, budget)
        _check_runs(runs, sizes, C, budget)
        assert runs == ops.dcrf_groups(list(sizes), C, budget)                              # deterministic
        assert len(runs) > 1
    # the over-budget image is isolated; its neighbours still group
    budget = _ws([(375, 500), (500, 333), (37, 53)], C)
    runs = ops.dcrf_groups(sizes, C, budget)
    _check_runs(runs, sizes, C, budget)
    assert runs[0] == (0, 3)
    small = _ws([(480, 640)], C) - 1
    runs = ops.dcrf_groups(sizes, C, small)
    _check_runs(runs, sizes, C, small)
    assert (3, 4) in runs and (6, 7) in runs
    assert ops.dcrf_groups([(5, 5)], C, 1) == [(0, 1)]
    assert ops.dcrf_groups([], C, 1) == []


def test_gpu_tests_use_the_trees_parameter_sets(monkeypatch):
    """The two parameter sets tests/test_gpu_dcrf_ragged.py runs are the ones the tree uses: CRF_PARAMS of infer_seg_voc and the
    constants utils/dcrf.crf_inference hands to the library (captured from the call, not copied)."""
    import test_gpu_dcrf_ragged as G
    from excel_amd.tools.infer_seg_voc import CRF_PARAMS as P
    from excel_amd.utils import dcrf
    assert G.VOC_SET == (P["iter_max"], P["pos_w"], P["pos_xy_std"], P["bi_w"], P["bi_xy_std"], P["bi_rgb_std"])
    seen = []
    monkeypatch.setattr(dcrf, "_run", lambda image, prob, *params, **kw: seen.append(params))
    dcrf.crf_inference(None, None)
    assert seen == [G.DCRF_SET]
