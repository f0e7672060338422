"""Scratch-memory contract helpers (device-agnostic; test infrastructure only).

The ops allocate their workspaces and outputs with torch.empty and torch.empty_like.  In a test process that memory is usually fresh and reads as zero; in
the programs it is recycled by the caching allocator and holds what the previous op left there.  These helpers make an op run on
memory of a chosen byte pattern, twice, and compare the results bit for bit: a kernel that reads a pad column, a table slot or an output
element before writing it gives different bits (or NaN) in the two runs.

Only the bytes 0x00 and 0xFF are used.  0xFF is NaN in every fp32 / f16 / bf16 lane and -1 in every int32: an uninitialised integer read
as -1 lands next to its buffer (the guard tail of guarded_ws), it does not go wild.  The point is a wrong bit, not a wild access.
"""
import contextlib

import torch

BYTES = (0x00, 0xFF)
SENTINEL = 0xA5
TAIL = 64 << 10
_ACTIVE = []


def fill_bytes(t, byte):
    """Every byte of the contiguous tensor t := byte (in place, any dtype, any device).  -> t"""
    if byte not in BYTES:
        raise ValueError(f"only the bytes 0x00 and 0xFF are used, got {byte:#x}")
    if t.numel():
        if not t.is_contiguous():
            raise ValueError("fill_bytes needs a contiguous tensor")
        t.view(-1).view(torch.uint8).fill_(byte)
    return t


@contextlib.contextmanager
def poisoned_allocations(byte):
    """torch.empty and torch.empty_like (the two allocators of uninitialised memory ops uses) return their allocation with every byte
    set to `byte`, for the duration of the block only (restored on exit, also on an exception).  ops looks them up at call time, so
    this covers its _ws workspaces and its outputs alike; torch.zeros, torch.full and the rest are untouched."""
    if byte not in BYTES:
        raise ValueError(f"only the bytes 0x00 and 0xFF are used, got {byte:#x}")
    real, real_like = torch.empty, torch.empty_like

    def empty(*args, **kwargs):
        return fill_bytes(real(*args, **kwargs), byte)

    def empty_like(*args, **kwargs):
        t = real_like(*args, **kwargs)
        return fill_bytes(t, byte) if t.is_contiguous() else _fill_strided(t, byte)     # (preserve_format of a strided input)

    torch.empty, torch.empty_like = empty, empty_like
    _ACTIVE.append(byte)
    try:
        yield
    finally:
        _ACTIVE.pop()
        torch.empty, torch.empty_like = real, real_like


def _fill_strided(t, byte):
    """fill_bytes for a non-contiguous allocation: every element's bytes := byte, through a contiguous twin"""
    twin = fill_bytes(torch.zeros(t.shape, dtype=t.dtype, device=t.device), byte)
    t.copy_(twin)
    return t


def current_byte():
    """The byte of the innermost active poisoned_allocations block (for closures that poison a buffer an op caches across calls)."""
    if not _ACTIVE:
        raise RuntimeError("no poisoned_allocations block is active")
    return _ACTIVE[-1]


class GuardedWs:
    """Replacement of ops._ws: the requested bytes filled with `byte` (settable between runs), followed by a 64 KiB tail of 0xA5.  Hands
    out the front view and records (buffer, n); check_tails() asserts that every tail is intact."""

    def __init__(self, byte):
        self.byte = byte
        self.bufs = []

    def __call__(self, nbytes, device):
        n = max(int(nbytes), 256)
        buf = torch.full((n + TAIL,), SENTINEL, dtype=torch.uint8, device=device)
        buf[:n] = self.byte
        self.bufs.append((buf, n))
        return buf[:n]

    def check_tails(self):
        for buf, n in self.bufs:
            assert bool((buf[n:] == SENTINEL).all()), f"a kernel wrote past its {n}-byte workspace"


def guarded_ws(ops, monkeypatch, byte=0xFF):
    """Install a GuardedWs as ops._ws (undone by monkeypatch) and return it."""
    g = GuardedWs(byte)
    monkeypatch.setattr(ops, "_ws", g)
    return g


def run_twice(fn, ws=None):
    """fn() under byte 0x00, then under 0xFF -> (result tree, result tree).  A closure that passes caller-owned out= / ws= buffers
    allocates them with torch.empty inside fn: they then start as the run's byte.  ws: a GuardedWs whose fill byte follows the run."""
    out = []
    for byte in BYTES:
        if ws is not None:
            ws.byte = byte
        with poisoned_allocations(byte):
            r = fn()
        if torch.cuda.is_available():
            torch.cuda.synchronize()
        out.append(r)
    return tuple(out)


def _leaves(tree, path="out"):
    if tree is None:
        return
    if isinstance(tree, torch.Tensor):
        yield path, tree
    elif isinstance(tree, dict):
        for k in tree:
            yield from _leaves(tree[k], f"{path}[{k!r}]")
    elif isinstance(tree, (list, tuple)):
        for i, v in enumerate(tree):
            yield from _leaves(v, f"{path}[{i}]")
    else:
        yield path, torch.as_tensor(tree)


def assert_same_bits(a, b, defined=None):
    """The two result trees of run_twice (a under 0x00, b under 0xFF) hold the same tensors bit for bit, and every float of b is
    finite.  defined(path, tensor) -> tensor cuts an output down to the region the op documents as written (identity when None)."""
    la, lb = list(_leaves(a)), list(_leaves(b))
    assert [p for p, _ in la] == [p for p, _ in lb], "the two runs returned different result trees"
    assert la, "nothing to compare"
    for (path, x), (_, y) in zip(la, lb):
        assert x.shape == y.shape and x.dtype == y.dtype, path
        if defined is not None:
            x, y = defined(path, x), defined(path, y)
        if y.is_floating_point():
            assert bool(torch.isfinite(y).all()), f"{path}: non-finite values when scratch and outputs start as 0xFF bytes"
        if not torch.equal(x, y):
            d = (x != y)
            raise AssertionError(f"{path}: {int(d.sum())} of {d.numel()} elements depend on the bytes the op's scratch / output memory "
                                 f"held before the call (first at flat index {int(d.reshape(-1).nonzero()[0])})")


def assert_holds(t, byte):
    """Every byte of t still is `byte`: a documented-unwritten region really was left alone (the mask hides no write of garbage)."""
    v = t.contiguous().view(-1).view(torch.uint8)
    assert bool((v == byte).all()), f"{int((v != byte).sum())} bytes of a region documented as not written were written"
