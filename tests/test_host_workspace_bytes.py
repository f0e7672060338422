"""Every workspace-size query returns what it returned before each op's workspace became one layout description shared by the query
and the launch (common.h `Workspace`): tests/golden/workspace_bytes.txt, recorded by tests/golden/make_workspace_golden.py at the
commit before that change.  ops.dcrf_groups / ops.dcrf_lam_groups budget their groups from these totals, and callers size their
buffers from them, so a total that moves is a change of behaviour.  All host arithmetic but the ViT query, whose handle needs a device."""
import pytest

from excel_amd import _lib

from _workspace_queries import VIT_QUERY, query_bytes, read_rows

# queries without rows in the golden file, each with its reason
EXEMPT = {
    "excel_train_augment_workspace_bytes": "returns a field of the plan excel_train_aug_plan filled",
    "excel_png_labels_workspace_bytes": "png.hip sizes and carves from one plan, which the layout change did not touch",
    "excel_jpeg_rgb_workspace_bytes": "jpeg.hip sizes and carves from one plan (jpeg_plan), which the layout change did not touch",
}


def _check(rows):
    bad = [(q, a, want, got) for q, a, want in rows for got in [query_bytes(q, a)] if got != want]
    assert not bad, f"{len(bad)} totals differ (query, args, recorded, now), first: {bad[:3]}"


def test_host_queries_return_the_recorded_totals():
    rows = [r for r in read_rows() if r[0] != VIT_QUERY]
    assert len(rows) > 150
    _check(rows)


def test_every_workspace_query_is_pinned_or_exempt():
    queries = {n for n in _lib.SIGNATURES if n.endswith("_workspace_bytes")}
    pinned = {r[0] for r in read_rows()}
    assert pinned <= queries and not (pinned & set(EXEMPT)) and set(EXEMPT) <= queries
    assert queries - pinned - set(EXEMPT) == set()
    assert VIT_QUERY in pinned            # recorded on the GPU, replayed by the gpu test below


@pytest.mark.gpu
def test_vit_query_returns_the_recorded_totals():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    rows = [r for r in read_rows() if r[0] == VIT_QUERY]
    assert {r[1][-2:] for r in rows} == {(1, 32), (2, 48), (1, 224)}
    _check(rows)
