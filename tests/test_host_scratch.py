"""The scratch-contract checker itself, without a GPU: poisoned_allocations does what it says, run_twice + assert_same_bits reject a
fake op that reads a pad column it never wrote (and accept the same op once it zeroes the pad first), and the case table of
tests/test_gpu_scratch_contract.py names every workspace user of excel_amd/ops.py."""
import ast
import inspect
import os
import sys

import pytest

torch = pytest.importorskip("torch")
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _scratch as S  # noqa: E402
import _scratch_cases as T  # noqa: E402


@pytest.mark.parametrize("dtype", [torch.float32, torch.int32, torch.uint8, torch.int16, torch.int64, torch.float64])
@pytest.mark.parametrize("byte", S.BYTES)
def test_poisoned_allocations_fill_every_byte(dtype, byte):
    real, real_like = torch.empty, torch.empty_like
    like = torch.zeros((4, 6), dtype=dtype)
    with S.poisoned_allocations(byte):
        assert torch.empty is not real and torch.empty_like is not real_like and S.current_byte() == byte
        strided = torch.empty_like(like.t())                      # preserve_format: a non-contiguous allocation
        assert strided.stride() == like.t().stride() and bool((strided.contiguous().view(-1).view(torch.uint8) == byte).all())
        for t in (torch.empty((3, 5), dtype=dtype), torch.empty(7, dtype=dtype, device="cpu"), torch.empty((0,), dtype=dtype),
                  torch.empty_like(like), torch.empty_like(like, dtype=torch.uint8).to(dtype)[:0], torch.empty_like(like[:0])):
            assert t.dtype == dtype
            assert bool((t.view(-1).view(torch.uint8) == byte).all())
        if byte == 0xFF and dtype.is_floating_point:
            assert bool(torch.isnan(torch.empty(4, dtype=dtype)).all())
        if byte == 0xFF and dtype in (torch.int32, torch.int16, torch.int64):
            assert bool((torch.empty(4, dtype=dtype) == -1).all())
    assert torch.empty is real and torch.empty_like is real_like
    assert not like.any()


def test_poisoned_allocations_restore_and_leave_the_rest_alone():
    real_empty, real_like, real_zeros, real_full = torch.empty, torch.empty_like, torch.zeros, torch.full
    with pytest.raises(KeyError):
        with S.poisoned_allocations(0xFF):
            assert torch.zeros is real_zeros and torch.full is real_full
            assert not torch.zeros(5).any() and bool((torch.full((5,), 3.0) == 3).all()) and not torch.zeros_like(torch.ones(3)).any()
            raise KeyError("inside the block")
    assert torch.empty is real_empty and torch.empty_like is real_like and torch.zeros is real_zeros and torch.full is real_full
    with pytest.raises(RuntimeError):
        S.current_byte()
    for bad in (0xA5, 0x7F, 1):                        # only 0x00 and 0xFF: no random or large-positive patterns
        with pytest.raises(ValueError):
            with S.poisoned_allocations(bad):
                pass
    assert torch.empty is real_empty and torch.empty_like is real_like


# ------------------------------------------------------------------ negative control: a fake op with a pad column in its scratch
class _FakeOps:
    """x [R, W] -> row sums, through a workspace with rows padded to Wp = W rounded up to 4 (the ops' idiom)."""

    def __init__(self, zero_pad):
        self.zero_pad = zero_pad

    @staticmethod
    def _ws(nbytes, device):
        return torch.empty(max(int(nbytes), 256), dtype=torch.uint8, device=device)

    def row_sums(self, x):
        R, W = x.shape
        Wp = (W + 3) // 4 * 4
        scratch = self._ws(R * Wp * 4, x.device)[:R * Wp * 4].view(torch.float32).view(R, Wp)
        scratch[:, :W] = x
        if self.zero_pad:
            scratch[:, W:] = 0                         # the producer zeroes its own padding
        out = torch.empty((R,), dtype=torch.float32, device=x.device)
        out[:] = scratch.sum(1)                        # ... because the consumer adds up the whole pitched row
        return out


def test_checker_rejects_a_read_of_unwritten_scratch(monkeypatch):
    x = torch.arange(15, dtype=torch.float32).reshape(3, 5)
    bad = _FakeOps(zero_pad=False)
    ws = S.guarded_ws(bad, monkeypatch)
    a, b = S.run_twice(lambda: bad.row_sums(x), ws)
    assert torch.equal(a, x.sum(1))                    # on zero-filled memory the bug is invisible: what the suite saw so far
    with pytest.raises(AssertionError):
        S.assert_same_bits(a, b)
    ws.check_tails()
    assert len(ws.bufs) == 2


def test_checker_accepts_the_op_that_zeroes_its_pad(monkeypatch):
    x = torch.arange(15, dtype=torch.float32).reshape(3, 5)
    good = _FakeOps(zero_pad=True)
    ws = S.guarded_ws(good, monkeypatch)
    a, b = S.run_twice(lambda: good.row_sums(x), ws)
    S.assert_same_bits(a, b)
    assert torch.equal(b, x.sum(1))
    ws.check_tails()


def test_checker_sees_integer_outputs_masks_and_tails(monkeypatch):
    def partly_written():
        lab = torch.empty((2, 6), dtype=torch.int32)
        lab[:, :4] = 7                                  # columns 4, 5 are a documented hole
        return dict(lab=lab)
    a, b = S.run_twice(partly_written)
    with pytest.raises(AssertionError):
        S.assert_same_bits(a, b)                        # an unwritten int32 differs (0 vs -1) although nothing is NaN
    S.assert_same_bits(a, b, defined=lambda path, t: t[:, :4])
    for byte, r in zip(S.BYTES, (a, b)):
        S.assert_holds(r["lab"][:, 4:], byte)
        with pytest.raises(AssertionError):
            S.assert_holds(r["lab"][:, 3:], byte)       # a mask that hides a write is caught
    fake = _FakeOps(True)
    ws = S.guarded_ws(fake, monkeypatch)
    buf = fake._ws(100, "cpu")
    assert buf.numel() == 256 and bool((buf == 0xFF).all())
    ws.check_tails()
    ws.bufs[0][0][256 + 3] = 0                          # one byte behind the workspace
    with pytest.raises(AssertionError):
        ws.check_tails()


# ------------------------------------------------------------------ completeness: no workspace user of ops.py is left out
# the only workspace users that may be left to another test: the ViT split-mode workspace (test_gpu_attn_shapes.py) and the training
# ops (test_gpu_train_grad.py).  Kept here, apart from the table it limits.
ALLOWED_ALREADY_COVERED = {"VitHandle.workspace", "DecoderHandle.forward_train", "DecoderHandle.backward", "DecoderHandle.train_attn_fts",
                           "train_losses"}


def _workspace_users():
    """qualified names of the functions / methods of excel_amd/ops.py that call _ws( or self.workspace(, or take a ws= parameter"""
    from excel_amd import ops
    src = inspect.getsource(ops)
    users = []

    def visit(fn, prefix):
        if fn.name == "_ws":
            return
        calls = [c.func for stmt in fn.body for c in ast.walk(stmt) if isinstance(c, ast.Call)]
        allocates = any((isinstance(f, ast.Name) and f.id == "_ws") or
                        (isinstance(f, ast.Attribute) and f.attr == "workspace" and isinstance(f.value, ast.Name) and f.value.id == "self")
                        for f in calls)
        names = [a.arg for a in fn.args.args + fn.args.kwonlyargs]
        if allocates or "ws" in names or (prefix and fn.name == "workspace"):
            users.append(prefix + fn.name)

    for node in ast.parse(src).body:
        if isinstance(node, ast.FunctionDef):
            visit(node, "")
        elif isinstance(node, ast.ClassDef):
            for sub in node.body:
                if isinstance(sub, ast.FunctionDef):
                    visit(sub, node.name + ".")
    return users


def test_every_workspace_user_has_a_case():
    users = _workspace_users()
    assert len(users) >= 20 and "DecoderHandle.forward" in users and "par_forward" in users and "dcrf_lam_ragged" in users, users
    # the ctx of forward_train carries its workspace into these two, which therefore neither allocate nor take one
    users += ["DecoderHandle.backward", "DecoderHandle.train_attn_fts"]
    assert set(T.ALREADY_COVERED) <= ALLOWED_ALREADY_COVERED, "only the ViT split-mode workspace and the training ops are covered elsewhere"
    missing = [u for u in users if u not in T.COVERS and u not in T.ALREADY_COVERED]
    assert not missing, f"workspace users of ops.py without a case in tests/_scratch_cases.py: {missing}"
    for name, cases in T.COVERS.items():                 # (that a case really calls the op it stands for is asserted where it runs)
        assert cases and all(c in T.CASES for c in cases), f"{name}: names a case that does not exist"
    stale = [n for n in list(T.COVERS) + list(T.ALREADY_COVERED) if n not in users]
    assert not stale, f"named in the case table but no workspace user of ops.py (renamed?): {stale}"
    # the named tests exist
    here = os.path.dirname(os.path.abspath(__file__))
    for name, where in T.ALREADY_COVERED.items():
        fname, test = where.split(" ")[0].split("::")
        assert f"def {test}(" in open(os.path.join(here, fname)).read(), (name, where)
