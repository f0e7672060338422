"""No op reads its scratch or output memory before writing it.

Every entry point of excel_amd/ops.py that allocates a workspace (and every op's torch.empty outputs) runs twice on seeded inputs:
with all of that memory starting as 0x00 bytes, then as 0xFF bytes (NaN in every float lane, -1 in every int32).  The two results
must be bit-identical and finite, every workspace's 64 KiB guard tail must be intact, and a region an op documents as not written must
still hold the byte it started with.  A difference means a kernel read a pad column, a table slot or an output element it had not
written: in the programs that memory is recycled by the caching allocator and holds what the previous op left there.

The cases, their shapes and the reading of every workspace carve-up are in tests/_scratch_cases.py; the helpers in tests/_scratch.py
(their negative control runs without a GPU in tests/test_host_scratch.py)."""
import os
import sys

import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _scratch as S  # noqa: E402
import _scratch_cases as T  # noqa: E402


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from excel_amd import ops as _ops
    return _ops


def _record_calls(ops, monkeypatch, names):
    """wrap the named functions / methods of ops so that a call leaves its name in the returned set"""
    called = set()
    for name in names:
        *path, attr = name.split(".")
        owner = ops
        for p in path:
            owner = getattr(owner, p)
        real = getattr(owner, attr)

        def wrap(*args, _real=real, _name=name, **kwargs):
            called.add(_name)
            return _real(*args, **kwargs)
        monkeypatch.setattr(owner, attr, wrap)
    return called


@pytest.mark.parametrize("name", sorted(T.CASES))
def test_scratch_contract(ops, name, monkeypatch):
    stands_for = [op for op, cases in T.COVERS.items() if name in cases]
    called = _record_calls(ops, monkeypatch, stands_for)
    case = T.CASES[name](ops)
    ws = S.guarded_ws(ops, monkeypatch)
    a, b = S.run_twice(case.fn, ws)
    assert called == set(stands_for), f"the case stands for {stands_for} but ran only {sorted(called)}"
    S.assert_same_bits(a, b, case.defined)
    if case.holes is not None:
        for byte, r in zip(S.BYTES, (a, b)):
            holes = case.holes(r)
            assert holes and all(h.numel() for h in holes), "the case names a hole that is empty"
            for h in holes:
                S.assert_holds(h, byte)
    ws.check_tails()
    if case.n_ws:
        assert ws.bufs, "the case stands for a workspace user, but nothing was allocated through ops._ws"
