"""No op leaves its stream.

Every function and method of excel_amd/ops.py that launches (tests/test_host_stream_contract.py keeps the table complete) runs on a
side stream in the two arrangements of tests/_streams.py, on scratch and output memory of 0xFF bytes, and must give the bits of its
run on the idle default stream:

  behind   the op is queued behind a chain of matmuls on its own stream while stream 0 is idle: a stage that went to stream 0 runs
           ahead of its predecessors;
  beside   the chain runs on stream 0 and only the side stream is synchronised: (a) the result, snapshot at that moment, is the
           reference's (a stage on stream 0 is still stuck behind the chain), (b) so are the tensors after the device has drained (a
           straggler on stream 0 would overwrite them late), (c) stream 0 is still busy at that moment (the op neither waited for
           stream 0 nor synchronised the device).

The controls at the end run the same two arrangements on plain torch "fake ops" with one stream slip each, and prove that the
arrangements can fail on this runtime - in particular that the side streams they run on (tests/_streams.py: concurrent_stream drops
the streams that share the default stream's hardware queue) are not implicitly ordered against stream 0."""
import os
import sys

import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _scratch as S  # noqa: E402
import _stream_cases as T  # noqa: E402
import _streams as St  # noqa: E402

ARRANGEMENTS = ("behind", "beside")
_PREPARED = {}


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from excel_amd import ops as _ops
    return _ops


@pytest.fixture(scope="module")
def t_link(ops):
    """seconds per chain link, measured once"""
    t = St.time_link()
    print(f"\n[stream-contract] one chain link ({St.CHAIN_N} x {St.CHAIN_N} matmul + scale): {t * 1e6:.0f} us")
    assert t > 0
    return t


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


def _prepared(ops, name):
    """(case, reference) of a case: built, warmed up and run once on the idle default stream, shared by its two arrangements"""
    if name not in _PREPARED:
        case = T.CASES[name](ops)
        _PREPARED[name] = (case, St.reference(case.fn))
    return _PREPARED[name]


def _run(arrangement, fn, ref, t_link, ws=None):
    """fn in the arrangement, behind / beside a chain sized for the case -> the Run (its figures printed)"""
    links = St.links_for(ref.t_case, t_link)
    run = (St.run_behind if arrangement == "behind" else St.run_beside)(fn, links, ws)
    print(f"\n[stream-contract] {arrangement}: t_case {ref.t_case * 1e3:.2f} ms, {run.links} links, side-stream run {run.host_s * 1e3:.2f} ms on stream "
          f"{run.stream:#x}, default stream busy afterwards: {run.busy}")
    return run


def _check(arrangement, fn, ref, defined, t_link, ws=None):
    """run fn in the arrangement and assert (a), (b) and (c) -> the Run"""
    run = _run(arrangement, fn, ref, t_link, ws)
    if arrangement == "behind":
        St.assert_matches(ref.tree, run.final, defined, "queued behind a busy chain on its own stream")
        return run
    St.assert_matches(ref.tree, run.early, defined, "(a) beside a busy default stream, read when the side stream was done")
    St.assert_matches(ref.tree, run.final, defined, "(b) beside a busy default stream, read after the device had drained")
    assert run.busy, "(c) " + St.busy_message(run, ref.t_case, t_link)
    return run


@pytest.mark.parametrize("arrangement", ARRANGEMENTS)
@pytest.mark.parametrize("name", sorted(T.CASES))
def test_stream_contract(ops, name, arrangement, t_link, monkeypatch):
    case, ref = _prepared(ops, name)
    stands_for = [op for op, cases in T.STREAM_COVERS.items() if name in cases]
    assert stands_for, "a case that stands for no op"
    called = _record_calls(ops, monkeypatch, stands_for)
    ws = S.guarded_ws(ops, monkeypatch)
    _check(arrangement, case.fn, ref, case.defined, t_link, ws)
    assert called == set(stands_for), f"the case stands for {stands_for} but ran only {sorted(called)}"
    ws.check_tails()


# ------------------------------------------------------------------ controls: plain torch fake ops with one stream slip each
def _fake_op(slip):
    """x -> 2 x + 1 in two stages through a torch.empty intermediate, then summed into a zero-filled accumulator; `slip` misplaces one
    step: "first" / "second" issue that stage on the default stream, "zero_fill" the accumulator's zero-fill, "sync" synchronises the
    device between the stages; None is the clean op."""
    x = torch.arange(1 << 16, dtype=torch.float32, device="cuda").reshape(256, 256) / 256
    zero = torch.cuda.default_stream()

    def on(name):
        return torch.cuda.stream(zero if slip == name else torch.cuda.current_stream())

    def fn():
        tmp, out, acc = torch.empty_like(x), torch.empty_like(x), torch.empty((256,), dtype=torch.float32, device="cuda")
        with on("zero_fill"):
            acc.zero_()
        with on("first"):
            torch.mul(x, 2, out=tmp)
        if slip == "sync":
            torch.cuda.synchronize()
        with on("second"):
            torch.add(tmp, 1, out=out)
        acc += out.sum(1)
        return dict(out=out, acc=acc)
    return fn


def _control(slip, arrangement, t_link):
    fn = _fake_op(slip)
    ref = St.reference(fn)
    assert torch.equal(ref.tree["out"], _fake_op(None)()["out"])          # on the idle default stream every slip is invisible
    return _check(arrangement, fn, ref, None, t_link)


@pytest.mark.parametrize("arrangement", ARRANGEMENTS)
def test_control_clean_op_passes(ops, arrangement, t_link):
    _control(None, arrangement, t_link)
    dropped = [f"{s:#x}: {dt * 1e3:.2f} of {c * 1e3:.2f} ms, busy {b}" for s, ok, b, dt, c in St.PROBED["log"] if not ok]
    print(f"\n[stream-contract] side streams so far: {St.PROBED['taken']} taken, {St.PROBED['dropped']} dropped (ordered against stream 0) {dropped}")


def test_control_second_stage_on_stream_0_is_flagged_by_beside_a(ops, t_link):
    with pytest.raises(AssertionError, match=r"^\(a\) "):
        _control("second", "beside", t_link)


def test_control_zero_fill_on_stream_0_is_flagged_by_beside(ops, t_link):
    """the accumulate reads 0xFF bytes (a), and the late zero-fill then wipes the sums (b)"""
    with pytest.raises(AssertionError, match=r"^\(a\) .*acc"):
        _control("zero_fill", "beside", t_link)
    fn = _fake_op("zero_fill")
    ref = St.reference(fn)
    run = _run("beside", fn, ref, t_link)
    with pytest.raises(AssertionError):
        St.assert_matches(ref.tree, run.final, None, "(b)")
    assert run.busy


def test_control_device_synchronize_is_flagged_by_c(ops, t_link):
    """a device-wide wait between the stages: the bits are right, the default stream has drained"""
    fn = _fake_op("sync")
    ref = St.reference(fn)
    run = _run("beside", fn, ref, t_link)
    St.assert_matches(ref.tree, run.early, None, "(a)")
    St.assert_matches(ref.tree, run.final, None, "(b)")
    assert not run.busy
    assert run.host_s >= 0.5 * St.MIN_CHAIN_S, St.busy_message(run, ref.t_case, t_link)      # the host waited for the chain
    with pytest.raises(AssertionError, match=r"^\(c\) "):
        _control("sync", "beside", t_link)


def test_control_first_stage_on_stream_0_is_flagged_by_both(ops, t_link):
    """A first stage on stream 0 is flagged by BOTH arrangements.  behind: it runs at once, the 0xFF fill of its torch.empty output
    (queued on the side stream behind the chain) lands on top of it, and the second stage reads the fill.  beside: it is stuck behind
    the chain, and the second stage reads the fill."""
    with pytest.raises(AssertionError, match="queued behind"):
        _control("first", "behind", t_link)
    with pytest.raises(AssertionError, match=r"^\(a\) "):
        _control("first", "beside", t_link)
