"""Stream-contract helpers (test infrastructure only): run an op on a side stream that is busy itself ("behind") or beside a busy
default stream ("beside"), on poisoned scratch and output memory, and compare with a reference run on the idle default stream.

The programs run ops on side streams (run_batch_split, run_batch_overlapped, the loader's copy stream) and assume that an op does ALL
of its device work on torch.cuda.current_stream() and waits for no other stream.  On an idle stream 0 with a device-wide synchronise
around the call, a launch that forgot its stream, a memset on stream 0 or a stray hipDeviceSynchronize all give the right answer;
here they do not:

  behind   the default stream is idle, the side stream first gets a chain of matmuls, then the op.  A stage that went to stream 0
           runs at once, ahead of the stages (and of the 0xFF fills of the op's torch.empty memory) that wait behind the chain.
  beside   the DEFAULT stream gets the chain, the op runs on the idle side stream and only the side stream is synchronised.  A
           stage that went to stream 0 is still stuck behind the chain when the result is snapshot (its consumers read 0xFF
           bytes), and the default stream must still be busy then: the op neither waited for it nor synchronised the device.

Every delay is a bounded chain of ordinary matmuls (a = a @ a * 1e-3): nothing spins, nothing can hang.  The chain is sized from
measurements: one link is timed with events once, and a case gets links for max(50 ms, 10 x its own run time).

The side stream is a fresh torch.cuda.Stream() that concurrent_stream() has seen run beside a busy default stream.  The HIP runtime
multiplexes its streams over a few hardware queues (GPU_MAX_HW_QUEUES, 4 by default), and a stream that lands on the default
stream's queue executes in submission order with it: measured on an MI355X, every fourth stream torch hands out finished a single
tiny kernel only when a 50 ms chain on stream 0 had drained.  On such a stream no slip can show (everything runs in the order the
host issued it) and no op, not even a plain torch one, can meet (c); it is not a stream the programs gain anything from either.
The probe takes the next stream instead."""
import math
import time
from collections import namedtuple

import torch

import _scratch as S

CHAIN_N = 2048                 # side of the chain's square matrix
MIN_CHAIN_S = 0.050            # the chain lasts at least this long ...
CASE_FACTOR = 10               # ... and this many times the case's own run time (host launch jitter between the two runs)
MAX_CHAIN_S = 2.0              # a case that would need more is too big: shrink the case

PROBE_LINKS = 160              # the probe chain of concurrent_stream(): ~20 ms
PROBE_TRIES = 12
PROBED = dict(taken=0, dropped=0, log=[])      # streams concurrent_stream() returned / dropped so far, and every verdict (reported by the tests)

Reference = namedtuple("Reference", "tree t_case")
Run = namedtuple("Run", "early final busy host_s links stream")


def chain_seed():
    """The matrix a chain starts from (allocated on the current stream; synchronise before another stream uses it)"""
    return torch.randn(CHAIN_N, CHAIN_N, device="cuda")


def enqueue_chain(a, links):
    """`links` dependent matmuls on the current stream -> the last product (keep it alive until the stream is synchronised)"""
    for _ in range(links):
        a = a @ a * 1e-3
    return a


def time_link(links=50):
    """Seconds one chain link takes on the idle device, from events around `links` of them (after a warm-up of as many)."""
    a = chain_seed()
    enqueue_chain(a, links)
    torch.cuda.synchronize()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    enqueue_chain(a, links)
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) * 1e-3 / links


def concurrent_stream():
    """A fresh torch.cuda.Stream() that runs beside the default stream: one small kernel on it completes, on the host's clock, in
    less than a quarter of the time a short chain keeps the default stream busy (and the default stream is still busy then).  A
    stream that shares the default stream's hardware queue (see the module text) needs the whole chain's time and is dropped; so is
    one whose first use happened to be slow, which only costs another try."""
    seed = chain_seed()
    for _ in range(PROBE_TRIES):
        side = torch.cuda.Stream()
        torch.cuda.synchronize()
        tail = enqueue_chain(seed, PROBE_LINKS)
        t0 = time.perf_counter()
        with torch.cuda.stream(side):
            probe = seed[0] + 1
        side.synchronize()
        dt = time.perf_counter() - t0
        busy = not torch.cuda.default_stream().query()
        torch.cuda.synchronize()
        chain_s = time.perf_counter() - t0
        del tail, probe
        beside = busy and dt < 0.25 * chain_s
        PROBED["taken" if beside else "dropped"] += 1
        PROBED["log"].append((side.cuda_stream, beside, busy, dt, chain_s))
        if beside:
            return side
    raise AssertionError(f"none of {PROBE_TRIES} fresh streams ran beside a busy default stream: this runtime orders every side stream "
                         "against stream 0, and the stream contract cannot be observed on it")


def links_for(t_case, t_link):
    """Number of links of a chain that lasts max(50 ms, 10 x t_case)."""
    need = max(MIN_CHAIN_S, CASE_FACTOR * t_case)
    assert need <= MAX_CHAIN_S, (f"the case runs for {t_case * 1e3:.1f} ms: its chain would last {need:.2f} s, more than {MAX_CHAIN_S} s - "
                                 "shrink the case")
    return max(1, math.ceil(need / t_link))


def clone_tree(tree):
    """The result tree with every tensor cloned on the current stream"""
    if isinstance(tree, torch.Tensor):
        return tree.clone()
    if isinstance(tree, dict):
        return {k: clone_tree(v) for k, v in tree.items()}
    if isinstance(tree, (list, tuple)):
        return type(tree)(clone_tree(v) for v in tree)
    return tree


def reference(fn):
    """fn() twice on the idle default stream: a warm-up (one-time set-up: cached tables, allocator growth), then the reference, timed
    on the host around fn() + synchronize().  Both under poisoned_allocations(0x00): closures that poison a cached buffer themselves
    need a block to be active, and zero bytes are what fresh memory holds anyway."""
    torch.cuda.synchronize()
    with S.poisoned_allocations(0x00):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    with S.poisoned_allocations(0x00):
        tree = fn()
    torch.cuda.synchronize()
    return Reference(tree, time.perf_counter() - t0)


def _poisoned_on(side, fn, ws):
    if ws is not None:
        ws.byte = 0xFF
    with torch.cuda.stream(side), S.poisoned_allocations(0xFF):
        return fn()


def run_behind(fn, links, ws=None):
    """The default stream idle; a fresh side stream gets `links` chain links, then fn() on memory of 0xFF bytes -> Run (early = final =
    the result after side.synchronize(); busy is None)."""
    side = concurrent_stream()
    seed = chain_seed()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    with torch.cuda.stream(side):
        tail = enqueue_chain(seed, links)
    tree = _poisoned_on(side, fn, ws)
    side.synchronize()
    host = time.perf_counter() - t0
    torch.cuda.synchronize()
    del tail
    return Run(tree, tree, None, host, links, side.cuda_stream)


def run_beside(fn, links, ws=None):
    """`links` chain links on the DEFAULT stream; fn() on a fresh, idle side stream on memory of 0xFF bytes; side.synchronize() only.
    -> Run: early = clones of the result made on the side stream at that moment, busy = the default stream was still working then,
    final = the result tensors after the device-wide synchronise, host_s = host seconds from the call of fn() to the return of
    side.synchronize()."""
    side = concurrent_stream()
    seed = chain_seed()
    torch.cuda.synchronize()
    tail = enqueue_chain(seed, links)
    t0 = time.perf_counter()
    tree = _poisoned_on(side, fn, ws)
    side.synchronize()
    host = time.perf_counter() - t0
    busy = not torch.cuda.default_stream().query()
    with torch.cuda.stream(side):
        early = clone_tree(tree)
    side.synchronize()
    torch.cuda.synchronize()
    del tail
    return Run(early, tree, busy, host, links, side.cuda_stream)


def assert_matches(ref, got, defined, what):
    """_scratch.assert_same_bits (bit equality in the region `defined` cuts out, every float finite) with the arrangement named"""
    try:
        S.assert_same_bits(ref, got, defined)
    except AssertionError as e:
        raise AssertionError(f"{what}: differs from the run on the idle default stream - {e}") from None


def busy_message(run, t_case, t_link):
    """What a reader needs to tell "the op synchronised" (host time ~ chain time) from "the chain was too short" """
    return (f"the default stream had drained when the side stream was done: the op waited for stream 0 or synchronised the device "
            f"(t_case {t_case * 1e3:.2f} ms, link {t_link * 1e6:.0f} us, {run.links} links = {run.links * t_link * 1e3:.0f} ms of chain, "
            f"side-stream run took {run.host_s * 1e3:.2f} ms on the host)")
