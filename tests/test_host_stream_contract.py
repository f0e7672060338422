"""The case table of tests/test_gpu_stream_contract.py names every function and method of excel_amd/ops.py that passes _stream() to the
library (no GPU needed).  There is no "covered elsewhere" list: an op that launches has a case in tests/_stream_cases.py, or this
fails.  That a case really calls the ops it stands for is asserted where it runs."""
import ast
import inspect
import os
import sys

import pytest

pytest.importorskip("torch")
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _stream_cases as T  # noqa: E402


def stream_users(src):
    """qualified names of the module-level functions and the methods of `src` whose body calls _stream()"""
    users = []

    def visit(fn, prefix):
        if fn.name == "_stream":
            return
        if any(isinstance(c, ast.Call) and isinstance(c.func, ast.Name) and c.func.id == "_stream" for stmt in fn.body for c in ast.walk(stmt)):
            users.append(prefix + fn.name)

    for node in ast.parse(src).body:
        if isinstance(node, ast.FunctionDef):
            visit(node, "")
        elif isinstance(node, ast.ClassDef):
            for sub in node.body:
                if isinstance(sub, ast.FunctionDef):
                    visit(sub, node.name + ".")
    return users


def _ops_source():
    from excel_amd import ops
    return inspect.getsource(ops)


def test_the_collector_sees_functions_and_methods():
    src = ("def _stream():\n    return 0\n\ndef launches(x):\n    return lib().k(x, _stream())\n\ndef host_only(x):\n    return x\n\n"
           "class H:\n    def run(self):\n        check(lib().k(self.h, _stream()), 'k')\n    def cfg(self):\n        return 1\n")
    assert stream_users(src) == ["launches", "H.run"]


def test_every_stream_user_has_a_case():
    users = stream_users(_ops_source())
    # the collector has not gone blind
    assert len(users) >= 60 and len(set(users)) == len(users), users
    for name in ("par_forward", "DecoderHandle.backward", "image_scores", "VitHandle.forward", "gemm", "lam_tta_fuse"):
        assert name in users, name
    missing = [u for u in users if u not in T.STREAM_COVERS]
    assert not missing, f"ops.py passes _stream() to the library in {missing}, which have no case in tests/_stream_cases.py"
    stale = [n for n in T.STREAM_COVERS if n not in users]
    assert not stale, f"named in STREAM_COVERS but no _stream() caller of ops.py (renamed?): {stale}"
    for name, cases in T.STREAM_COVERS.items():
        assert cases and all(c in T.CASES for c in cases), f"{name}: names a case that does not exist"


def test_a_new_stream_user_without_a_case_is_reported():
    """the completeness check fails for a launcher added to ops.py without a case (here: appended to a copy of the source)"""
    src = _ops_source() + "\n\ndef brand_new_op(x):\n    check(lib().excel_brand_new(_p(x), _stream()), 'excel_brand_new')\n    return x\n"
    users = stream_users(src)
    assert [u for u in users if u not in T.STREAM_COVERS] == ["brand_new_op"]


def test_the_scratch_cases_are_reused_not_copied():
    import _scratch_cases as SC
    assert all(T.CASES[name] is build for name, build in SC.CASES.items())
    assert len(T.CASES) > len(SC.CASES)
