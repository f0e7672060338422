"""Host-side tests of tools/infer_lam --overflow_guard: the policy resolution and the two-pass control flow of the batched loop, driven
by a stub pipeline on CPU tensors that hands out scripted tickets and records what it is asked to do (no GPU)."""
import contextlib
import os
import socket

import numpy as np
import pytest

import oracle

torch = pytest.importorskip("torch")


# ------------------------------------------------------------------ the policy
def test_resolve_overflow_guard_every_mode_and_policy():
    from excel_amd.tools.infer_lam import resolve_overflow_guard as r
    modes = ["f32", "bf16x3", "f16x3", "f16x2", None]
    for mode in modes:
        for on_gpu in (False, True):
            for batched in (False, True):
                want = "rerun" if (mode in ("f16x3", "f16x2") and on_gpu and batched) else "off"
                assert r("auto", mode, on_gpu, batched) == want, (mode, on_gpu, batched)
                assert r("off", mode, on_gpu, batched) == "off"
                for policy in ("raise", "rerun"):
                    if batched:
                        assert r(policy, mode, on_gpu, batched) == policy
                    else:
                        with pytest.raises(ValueError, match="per-image"):
                            r(policy, mode, on_gpu, batched)
    with pytest.raises(ValueError):
        r("maybe", "f16x3", True, True)


def test_flag_is_parsed_and_defaults_to_auto():
    from excel_amd.tools import infer_lam
    p = infer_lam.get_parser()
    assert p.parse_args([]).overflow_guard == "auto"
    for v in ("auto", "off", "raise", "rerun"):
        assert p.parse_args(["--overflow_guard", v]).overflow_guard == v
    with pytest.raises(SystemExit):
        p.parse_args(["--overflow_guard", "sometimes"])


# ------------------------------------------------------------------ the control flow, through a stub
class _IndexedSet:
    """(name, image u8 [h,w,3], label u8 [h,w], cls f32 [20]); byte 0 of an image is its data set index, so the stub knows who is who."""

    def __init__(self, n):
        self.n = n

    def __len__(self):
        return self.n

    def max_k(self):
        return 2

    def __getitem__(self, i):
        i = int(i)
        rs = np.random.RandomState(900 + i)
        h, w = 5 + i % 7, 4 + (3 * i) % 5
        img = rs.randint(0, 256, (h, w, 3)).astype(np.uint8)
        img[0, 0, 0] = i
        gt = rs.randint(0, 21, (h, w)).astype(np.uint8)
        gt[rs.rand(h, w) < 0.1] = 255
        cls = np.zeros(20, np.float32)
        cls[i % 20] = 1
        return f"s{i:03d}", img, gt, cls


def _sample_hist(ds, i):
    _, img, gt, _ = ds[i]
    return oracle.evaluate.fast_hist(gt.flatten(), img.reshape(-1, 3)[:, 0].astype(np.int64) % 21, 21)


class _Ticket:
    def __init__(self, flags, log, not_ready_polls):
        self._flags, self._log, self._wait = np.asarray(flags, np.int32), log, not_ready_polls

    def ready(self):
        self._log.append(("poll",))
        if self._wait > 0:
            self._wait -= 1
            return False
        return True

    def flags(self):
        self._log.append(("read", tuple(int(f) for f in self._flags)))
        return self._flags


class _GuardStub:
    """Stands in for a guarded pipeline: labels = a function of the image bytes; an image whose index is in bad[mode] (mode "fast" or
    "exact") gets a non-zero flag, and with guard "skip" stays out of `hist`.  Every ticket says "not ready" on its first poll."""
    device, smax = "cpu", 2

    def __init__(self, guard, bad_fast=(), bad_exact=(), log=None):
        self.guard, self.bad, self.mode = guard, {"fast": set(bad_fast), "exact": set(bad_exact)}, "fast"
        self.hist, self.log = None, ([] if log is None else log)
        self.ticket_looks = 0
        self._ticket = None

    @property
    def last_guard(self):
        self.ticket_looks += 1
        return self._ticket

    @contextlib.contextmanager
    def exact_mode(self):
        self.log.append(("enter_exact",))
        self.mode = "exact"
        try:
            yield self
        finally:
            self.mode = "fast"
            self.log.append(("exit_exact",))

    def run_batch_ragged(self, images, plan, cls, gts, S=448, return_intermediates=False):
        px = images.view(-1, 3).numpy()
        pred = (px[:, 0].astype(np.int64) % 21)
        idx = [int(px[int(plan.loff[b]), 0]) for b in range(plan.B)]
        flags = [3 if i in self.bad[self.mode] else 0 for i in idx]
        g = gts.numpy()
        for b in range(plan.B):
            if self.guard == "skip" and flags[b]:
                continue
            lo, hi = int(plan.loff[b]), int(plan.loff[b + 1])
            self.hist += torch.from_numpy(oracle.evaluate.fast_hist(g[lo:hi], pred[lo:hi], 21))
        self.log.append(("step", self.mode, self.guard, tuple(idx)))
        self._ticket = _Ticket(flags, self.log, not_ready_polls=1) if self.guard is not None else None
        return torch.from_numpy(pred.astype(np.uint8))


class _FakeLabelSaver:
    """Replaces infer_lam._LabelSaver (the real one encodes on the device): records the writes and the barrier."""
    log = None

    def __init__(self, args, directory=None):
        pass

    def ragged(self, names, plan, labels_flat):
        self.log.append(("write", tuple(str(n) for n in names)))

    def barrier(self):
        self.log.append(("barrier",))

    def close(self):
        self.log.append(("close",))


def _args(*extra):
    from excel_amd.tools import infer_lam
    return infer_lam.get_parser().parse_args(["--batch_size", "3", "--num_workers", "0", "--backend", "gloo"] + list(extra))


def _steps(log):
    return [e for e in log if e[0] == "step"]


def test_rerun_runs_flagged_images_once_ascending_in_exact_mode_after_the_writes(monkeypatch):
    from excel_amd.tools import infer_lam
    n = 8
    ds = _IndexedSet(n)
    log = []
    _FakeLabelSaver.log = log
    monkeypatch.setattr(infer_lam, "_LabelSaver", _FakeLabelSaver)
    pipe = _GuardStub("skip", bad_fast={6, 1, 4}, bad_exact={4}, log=log)
    score, total = infer_lam.validate(_args("--overflow_guard", "rerun", "--save_label", "true"), dataset=ds, pipe=pipe)
    steps = _steps(log)
    assert steps[:3] == [("step", "fast", "skip", (0, 1, 2)), ("step", "fast", "skip", (3, 4, 5)), ("step", "fast", "skip", (6, 7))]
    assert steps[3:] == [("step", "exact", "observe", (1, 4, 6))]                    # once, ascending, one batch of --batch_size
    assert pipe.guard == "skip" and pipe.mode == "fast"                              # both restored
    pos = {k: [i for i, e in enumerate(log) if e[0] == k] for k in ("write", "barrier", "enter_exact", "exit_exact", "step", "close")}
    assert len(pos["write"]) == 4 and len(pos["barrier"]) == 1
    second_step = pos["step"][3]
    assert max(pos["write"][:3]) < pos["barrier"][0] < pos["enter_exact"][0] < second_step < pos["write"][3] < pos["exit_exact"][0] < pos["close"][0]
    assert log[pos["write"][3]] == ("write", ("s001", "s004", "s006"))               # the same consumers, files overwritten by name
    # no wait inside the loop: a ticket that is not ready is left alone - each step's ticket is read only after a later poll
    first_read = next(i for i, e in enumerate(log) if e[0] == "read")
    assert first_read > pos["step"][1]
    rep = infer_lam.validate.last_guard
    assert rep == {"policy": "rerun", "mode": None, "checked": n, "flagged": ["s001", "s004", "s006"], "rerun": 3, "nonfinite_in_f32": ["s004"]}
    # every image is in the histogram exactly once (image 4, flagged again in fp32, is accepted as fp32 computed it)
    assert np.array_equal(total.numpy(), np.sum([_sample_hist(ds, i) for i in range(n)], 0))
    assert sum(len(e[3]) for e in steps) == n + 3


def test_nimg_counts_every_image_once():
    from excel_amd.tools import infer_lam
    args = _args("--overflow_guard", "rerun")
    args.ragged_batches = True                        # what validate sets for an injected data set
    pipe = _GuardStub("skip", bad_fast={0, 5})
    hist, nimg, _ = infer_lam.build_validation(None, None, _IndexedSet(7), np.arange(7), "cpu", args, pipe=pipe)
    assert nimg == 7 and infer_lam.build_validation.last_guard["rerun"] == 2 and infer_lam.build_validation.last_guard["checked"] == 7


def test_raise_names_the_images_and_closes_the_writers(monkeypatch):
    from excel_amd.tools import infer_lam
    log = []
    _FakeLabelSaver.log = log
    monkeypatch.setattr(infer_lam, "_LabelSaver", _FakeLabelSaver)
    pipe = _GuardStub("skip", bad_fast={4}, log=log)
    with pytest.raises(RuntimeError) as e:
        infer_lam.validate(_args("--overflow_guard", "raise", "--save_label", "true"), dataset=_IndexedSet(8), pipe=pipe)
    assert "s004" in str(e.value) and "s003" not in str(e.value)
    assert ("close",) in log and not any(x[0] == "enter_exact" for x in log)


def test_off_never_reads_a_ticket_and_per_image_loop_refuses():
    from excel_amd.tools import infer_lam
    ds = _IndexedSet(7)
    pipe = _GuardStub("skip", bad_fast={2})
    infer_lam.validate(_args("--overflow_guard", "off"), dataset=ds, pipe=pipe)
    assert pipe.ticket_looks == 0 and not any(e[0] in ("poll", "read", "enter_exact") for e in pipe.log)
    assert infer_lam.validate.last_guard["policy"] == "off"
    pipe = _GuardStub("skip", bad_fast={2})
    infer_lam.validate(_args(), dataset=ds, pipe=pipe)                               # auto on a CPU run: off
    assert pipe.ticket_looks == 0 and infer_lam.validate.last_guard["policy"] == "off"
    plain = _GuardStub(None)                                                         # a pipeline built without a guard keeps it that way
    _, total = infer_lam.validate(_args("--overflow_guard", "rerun"), dataset=ds, pipe=plain)
    assert infer_lam.validate.last_guard["policy"] == "off" and plain.ticket_looks == 0
    assert np.array_equal(total.numpy(), np.sum([_sample_hist(ds, i) for i in range(7)], 0))
    for policy in ("raise", "rerun"):
        with pytest.raises(ValueError, match="per-image"):
            infer_lam.validate(_args("--overflow_guard", policy, "--api_path", "true"), dataset=ds, pipe=_GuardStub("skip"))


# ------------------------------------------------------------------ two ranks: the second pass is rank-local
def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _guard_worker(rank, world, port, n, q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(rank))
    import torch.distributed as dist
    from excel_amd.tools import infer_lam
    pipe = _GuardStub("skip", bad_fast={4})                                           # index 4 belongs to rank 0 (0, 2, 4, 6)
    _, total = infer_lam.validate(_args("--overflow_guard", "rerun"), dataset=_IndexedSet(n), pipe=pipe)
    q.put((rank, _steps(pipe.log), dict(infer_lam.validate.last_guard), total.numpy()))
    dist.barrier()
    dist.destroy_process_group()


def test_world2_only_the_rank_with_a_flagged_image_runs_a_second_pass():
    import torch.multiprocessing as mp
    n, world = 7, 2
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_guard_worker, args=(r, world, port, n, q)) for r in range(world)]
    for p in procs:
        p.start()
    res = {r[0]: r for r in [q.get(timeout=180) for _ in range(world)]}
    for p in procs:
        p.join(60)
        assert p.exitcode == 0
    ds = _IndexedSet(n)
    ref = np.sum([_sample_hist(ds, i) for i in range(n)], 0)
    _, steps0, rep0, total0 = res[0]
    _, steps1, rep1, total1 = res[1]
    assert [s[1:] for s in steps0] == [("fast", "skip", (0, 2, 4)), ("fast", "skip", (6,)), ("exact", "observe", (4,))]
    assert [s[1:] for s in steps1] == [("fast", "skip", (1, 3, 5))]
    assert rep0["flagged"] == ["s004"] and rep0["rerun"] == 1 and rep0["checked"] == 4
    assert rep1["flagged"] == [] and rep1["rerun"] == 0 and rep1["checked"] == 3
    assert np.array_equal(total0, ref) and np.array_equal(total1, ref)                # the one gather still matches
