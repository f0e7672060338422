"""The alignment table of tests/_align_cases.py is complete and agrees with include/excel_hip.h (no GPU needed).

Every op of the stream contract's table, and every function or method of excel_amd/ops.py that hands a pointer to the library (_p),
has a row; every entry a row names is declared in the header; every requirement is a power of two up to 16; and the comment of every
entry that holds a pointer to more than 4 bytes says so, in the words the C ABI's callers read."""
import ast
import inspect
import os
import re
import sys

import pytest

torch = pytest.importorskip("torch")
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _align_cases as A  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def pointer_users(src):
    """qualified names of the module-level functions and the methods of `src` whose body calls _p()"""
    users = []

    def visit(fn, prefix):
        if fn.name == "_p":
            return
        if any(isinstance(c, ast.Call) and isinstance(c.func, ast.Name) and c.func.id == "_p" for stmt in fn.body for c in ast.walk(stmt)):
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


def _header():
    with open(os.path.join(ROOT, "include", "excel_hip.h")) as f:
        return f.read()


def entry_paragraph(header, entry):
    """The paragraph of the header (lines between two empty lines) that declares `entry`: its comment and the declarations that share it"""
    m = re.search(r"^(?:int|size_t)\s+" + re.escape(entry) + r"\s*\(", header, flags=re.M)
    assert m, f"{entry} is not declared in include/excel_hip.h"
    start = header.rfind("\n\n", 0, m.start())
    end = header.find("\n\n", m.end())
    return header[start + 2:end if end >= 0 else len(header)]


def missing_rows(users, align):
    return [u for u in users if u not in align]


def test_the_collector_sees_functions_and_methods():
    src = ("def _p(t):\n    return t\n\ndef hands_over(x):\n    return lib().k(_p(x))\n\ndef host_only(x):\n    return x\n\n"
           "class H:\n    def run(self, x):\n        check(lib().k(self.h, _p(x)), 'k')\n    def cfg(self):\n        return 1\n")
    assert pointer_users(src) == ["hands_over", "H.run"]


def test_every_op_has_a_row():
    users = pointer_users(_ops_source())
    assert len(users) >= 60 and len(set(users)) == len(users), users            # the collector has not gone blind
    for name in ("par_forward", "DecoderHandle.backward", "image_scores", "VitHandle.forward", "gemm", "lam_tta_fuse", "_label_pair"):
        assert name in users, name
    missing = missing_rows(list(A.STREAM_COVERS) + users, A.ALIGN)
    assert not missing, f"no row in tests/_align_cases.py ALIGN for {sorted(set(missing))}"
    stale = [n for n in A.ALIGN if n not in users and n not in A.STREAM_COVERS]
    assert not stale, f"rows of ALIGN that name no op of ops.py (renamed?): {stale}"


@pytest.mark.parametrize("name", sorted(A.ALIGN))
def test_removing_a_row_is_reported(name):
    """the completeness check fails for every single row taken out of the table"""
    users = list(A.STREAM_COVERS) + pointer_users(_ops_source())
    less = {k: v for k, v in A.ALIGN.items() if k != name}
    assert set(missing_rows(users, less)) == {name}


def test_a_new_op_without_a_row_is_reported():
    src = _ops_source() + "\n\ndef brand_new_op(x):\n    check(lib().excel_brand_new(_p(x), _stream()), 'excel_brand_new')\n    return x\n"
    assert missing_rows(pointer_users(src), A.ALIGN) == ["brand_new_op"]


def test_rows_are_well_formed():
    header = _header()
    from excel_amd import ops
    for name, row in A.ALIGN.items():
        assert row.args, f"{name}: no entry"
        for entry, args in row.args.items():
            entry_paragraph(header, entry)                                      # declared
            assert args, f"{name}: {entry} lists no pointer"
            for arg, (nbytes, why) in args.items():
                assert nbytes in (1, 2, 4, 8, 16), f"{name}: {entry}({arg}) needs {nbytes} bytes?"
                assert isinstance(why, str) and len(why) >= 6, f"{name}: {entry}({arg}) gives no reason"
        # what the op writes is an argument of the op
        *path, attr = name.split(".")
        owner = ops
        for p in path:
            owner = getattr(owner, p)
        params = inspect.signature(getattr(owner, attr)).parameters
        for arg, how in row.written.items():
            assert how in ("same_bits", "refused"), f"{name}: written argument {arg}: {how!r}"
            assert arg in params, f"{name}: written argument {arg} is no parameter of ops.{name}"
        assert row.parent in ("safe", "checked", "unguarded"), name


def test_every_out_ws_and_in_place_argument_is_in_the_table():
    """an op with an out= / ws= / hist= / acc parameter, or whose name ends in an underscore, states what happens to a shifted one"""
    from excel_amd import ops
    for name, row in A.ALIGN.items():
        *path, attr = name.split(".")
        owner = ops
        for p in path:
            owner = getattr(owner, p)
        params = inspect.signature(getattr(owner, attr)).parameters
        for arg in ("out", "ws", "hist", "acc"):
            if arg in params:
                assert arg in row.written, f"{name}: {arg}= is written by the op and has no entry in the row's `written`"
        if attr.endswith("_") and not attr.startswith("_"):
            assert row.written, f"{name} works in place and states nothing about its argument"


def test_the_header_states_every_requirement_above_4_bytes():
    header = _header()
    for entry, arg, nbytes in A.above_4():
        text = entry_paragraph(header, entry)
        assert "16-byte aligned" in text or "8-byte aligned" in text, \
            f"ALIGN holds {entry}({arg}) to {nbytes} bytes; its comment in include/excel_hip.h says neither '16-byte aligned' nor '8-byte aligned'"
        assert f"{nbytes}-byte aligned" in text, f"{entry}({arg}): the table says {nbytes} bytes, the header's comment does not"


def test_shifted_uploads_on_cpu_tensors():
    rs = torch.Generator().manual_seed(0)
    cases = [torch.randn((3, 5, 7), generator=rs), torch.randint(0, 255, (4, 9), generator=rs).to(torch.uint8),
             torch.randint(-5, 5, (6,), generator=rs).to(torch.int32), torch.randint(-5, 5, (2, 3), generator=rs).to(torch.int16),
             torch.randint(0, 9, (5,), generator=rs), torch.randn((2, 2), generator=rs).double(), torch.rand((4, 4), generator=rs) < 0.5,
             torch.tensor([float("nan"), float("inf"), -0.0, 1.5])]
    for t in cases:
        v = A.shifted(t)
        assert v.is_contiguous() and v.shape == t.shape and v.dtype == t.dtype and v.device == t.device
        assert v.data_ptr() % 16 == t.element_size(), (t.dtype, v.data_ptr() % 16)
        assert v.untyped_storage().nbytes() == (t.numel() + 1) * t.element_size()
        assert bytes(v.contiguous().view(-1).view(torch.uint8).tolist()) == bytes(t.contiguous().view(-1).view(torch.uint8).tolist())
    # a view of a strided tensor comes back contiguous, with the values of the view
    s = torch.arange(24.).reshape(4, 6)[:, ::2]
    assert torch.equal(A.shifted(s), s) and A.shifted(s).is_contiguous()


def test_the_uploader_is_swapped_only_inside_the_block():
    import _scratch_cases as SC
    import _stream_cases as T
    assert T.dev is SC.dev and not SC.UPLOADER
    with A.shifted_uploads():
        assert SC.UPLOADER == [A.shifted]
        with pytest.raises(RuntimeError):
            raise RuntimeError("the block is left on an exception too")
    assert not SC.UPLOADER


def test_realign_and_written_on_cpu_tensors():
    """ops._realign returns the tensor itself when it meets the requirement (the aligned path: one integer test) and a fresh copy when not;
    ops._written names the argument"""
    from excel_amd import ops
    t = torch.arange(32, dtype=torch.float32)
    assert t.data_ptr() % 16 == 0
    assert ops._realign(t) is t and ops._realign(None) is None and ops.f32c(t, 16) is t and ops.f32c(t) is t
    v = t[1:17]
    r = ops._realign(v)
    assert r is not v and r.data_ptr() % 16 == 0 and torch.equal(r, v) and r.is_contiguous()
    assert ops._realign(v, 4) is v and ops.f32c(v) is v and ops.f32c(v, 16).data_ptr() % 16 == 0
    assert ops._written(t, "op", "out") is t and ops._written(None, "op", "out") is None and ops._written(v, "op", "out", 4) is v
    with pytest.raises(ValueError, match=r"some_op: out must be 16-byte aligned"):
        ops._written(v, "some_op", "out")
