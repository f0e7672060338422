"""Resumable decoder training, host side: the loader's start position, the state files (round trip, atomic write, newest, pruning,
compatibility, loss-log truncation), the flags on both parsers, and train()'s stop / continue logic over a stub loop (no GPU)."""
import os
import types
import zlib

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from excel_amd.datasets import loader  # noqa: E402
from excel_amd.scripts import train_coco, train_voc  # noqa: E402
from excel_amd.utils import train_state as ts  # noqa: E402


class _CountingSet:
    """sample(idx, epoch) of a training dataset; records every call"""

    def __init__(self, n=11):
        self.n, self.calls = n, []

    def __len__(self):
        return self.n

    def sample(self, idx, epoch):
        name = f"e{epoch}_i{idx}"
        self.calls.append(name)
        return name, np.full((2, 2, 3), idx, np.uint8), np.zeros((2, 2), np.uint8), np.ones(3, np.float32), np.int32(idx)


def _take(it, k):
    out = [list(next(it).names) for _ in range(k)]
    it.close()
    return out


# ---------------------------------------------------------------------------------------------------------------- 1. positions
@pytest.mark.parametrize("world,rank", [(1, 0), (2, 0), (2, 1)])
def test_train_batches_start_position(world, rank):
    n, bs = 11, 2
    nb = ((n - n % world) // world) // bs
    assert nb == (5 if world == 1 else 2)
    half = max(1, nb // 2)
    for step in (half, nb, 2 * nb + half):                    # mid-epoch, an epoch boundary, the middle of a later epoch
        straight = _take(loader.train_batches(_CountingSet(n), bs, rank=rank, world=world, seed=7, num_threads=2), step + 5)
        e, b = loader.resume_position(step, n, world, bs)
        assert (e, b) == (step // nb, step % nb)
        ds = _CountingSet(n)
        resumed = _take(loader.train_batches(ds, bs, rank=rank, world=world, seed=7, start_epoch=e, num_threads=2, ahead=1, start_batch=b), 5)
        assert resumed == straight[step:step + 5]
        # with one batch in flight, exactly the samples of the five batches served were decoded: none of the `step` skipped ones
        assert sorted(ds.calls) == sorted(x for batch in resumed for x in batch)
        assert len(ds.calls) == 5 * bs < (step + 5) * bs
        assert not set(ds.calls) & {x for batch in straight[:step] for x in batch}
    # ranks of one step see disjoint samples of one epoch
    if world == 2:
        other = _take(loader.train_batches(_CountingSet(n), bs, rank=1 - rank, world=2, seed=7, num_threads=2, start_batch=1), 1)
        mine = _take(loader.train_batches(_CountingSet(n), bs, rank=rank, world=2, seed=7, num_threads=2, start_batch=1), 1)
        assert not set(other[0]) & set(mine[0])


def test_train_batches_start_batch_refused():
    with pytest.raises(ValueError, match="start_batch"):
        next(loader.train_batches(_CountingSet(11), 2, num_threads=1, start_batch=5))          # 5 batches per epoch: 0..4
    with pytest.raises(ValueError, match="start_batch"):
        next(loader.train_batches(_CountingSet(11), 2, num_threads=1, start_batch=-1))
    assert _take(loader.train_batches(_CountingSet(11), 2, num_threads=1, start_batch=4), 1)
    with pytest.raises(ValueError, match="no full batch"):
        next(loader.train_batches(_CountingSet(1), 2, num_threads=1))
    with pytest.raises(ValueError, match="no full batch"):
        loader.resume_position(3, 1, 1, 2)
    with pytest.raises(ValueError, match="no full batch"):
        loader.resume_position(3, 3, 2, 2)                                                     # 3 samples, 2 ranks: one each


# ---------------------------------------------------------------------------------------------------------------- 2., 3. the file
RUN = dict(seed=5, world=1, spg=2, n_train=8, crop_size=96, max_iters=7, warmup_iters=50, lr=1e-4, warmup_lr=1e-6, power=1.0,
           wt_decay=1e-2, w_diver=0.1, radius=2, num_classes=5, train_set="train", name="voc", caa_thre=0.79, lvc_iter=2, seg_aff_iter=None)


def _fake_state(seed):
    g = torch.Generator().manual_seed(seed)
    shapes = {"fuse0.proj_w": (4, 3), "fuse0.proj_b": (4,), "pred_w": (5, 4), "pred_b": (5,)}
    model = {"decoder_fts_fuse.linear_fuse.weight": torch.randn(4, 3, 1, 1, generator=g), "decoder.linear_pred.bias": torch.randn(5, generator=g)}
    model["decoder.linear_pred.bias"][0] = float("-0.0")
    model["decoder.linear_pred.bias"][1] = 1e-42                                               # a denormal survives too
    opt = {part: {k: torch.randn(*s, generator=g) for k, s in shapes.items()} for part in ("exp_avg", "exp_avg_sq")}
    return model, opt


def _bits(t):
    return t.contiguous().view(torch.int32)


def _same_tensors(a, b):
    assert list(a) == list(b)
    for k in a:
        assert a[k].dtype == b[k].dtype and a[k].shape == b[k].shape and torch.equal(_bits(a[k]), _bits(b[k])), k


def test_state_file_round_trip(tmp_path):
    model, opt = _fake_state(0)
    path = ts.state_path(str(tmp_path), 12)
    assert os.path.basename(path) == "train_state_iter_12.pth"
    assert ts.save_train_state(path, 12, model, opt, 3.5e-4, RUN) == path
    raw = torch.load(path, map_location="cpu", weights_only=True)                              # tensors, numbers, strings, None, dicts only
    assert set(raw) == {"step", "model_state_dict", "optimizer_state_dict", "lr", "format_version", "run"}
    st = ts.load_train_state(path)
    assert st["step"] == 12 and st["lr"] == 3.5e-4 and st["format_version"] == 1 and st["run"] == RUN
    assert st["run"]["seg_aff_iter"] is None and type(st["run"]["lvc_iter"]) is int
    _same_tensors(st["model_state_dict"], model)
    assert set(st["optimizer_state_dict"]) == {"exp_avg", "exp_avg_sq"}
    for part in opt:
        _same_tensors(st["optimizer_state_dict"][part], opt[part])
    assert os.listdir(tmp_path) == ["train_state_iter_12.pth"]
    with pytest.raises(FileNotFoundError):
        ts.load_train_state(str(tmp_path / "train_state_iter_13.pth"))
    torch.save({"step": 1, "model_state_dict": {}, "optimizer_state_dict": {"state": {}, "param_groups": []}, "lr": 0.1},
               str(tmp_path / "ref.pth"))                                                       # what the reference's save_train writes
    with pytest.raises(ValueError, match="format_version"):
        ts.load_train_state(str(tmp_path / "ref.pth"))


def test_state_file_write_is_atomic(tmp_path, monkeypatch):
    real_save = torch.save

    def broken_save(obj, f, *a, **k):
        f.write(b"half a file")
        f.flush()
        raise RuntimeError("disk full")

    model, opt = _fake_state(1)
    path = ts.state_path(str(tmp_path), 4)
    monkeypatch.setattr(torch, "save", broken_save)
    with pytest.raises(RuntimeError, match="disk full"):
        ts.save_train_state(path, 4, model, opt, 1e-3, RUN)
    assert not os.path.exists(path) and os.listdir(tmp_path) == []                             # no final file, no temporary file
    monkeypatch.setattr(torch, "save", real_save)
    ts.save_train_state(path, 4, model, opt, 1e-3, RUN)
    before = open(path, "rb").read()
    monkeypatch.setattr(torch, "save", broken_save)
    model2, opt2 = _fake_state(2)
    with pytest.raises(RuntimeError, match="disk full"):
        ts.save_train_state(path, 4, model2, opt2, 2e-3, RUN)
    assert open(path, "rb").read() == before and os.listdir(tmp_path) == ["train_state_iter_4.pth"]
    monkeypatch.setattr(torch, "save", real_save)
    _same_tensors(ts.load_train_state(path)["model_state_dict"], model)


# ---------------------------------------------------------------------------------------------------------------- 4., 5. the directory
def _touch(d, *names):
    for nm in names:
        (d / nm).write_bytes(b"x")


def test_find_latest_state(tmp_path):
    assert ts.find_latest_state(str(tmp_path)) is None
    assert ts.find_latest_state(str(tmp_path / "missing")) is None
    _touch(tmp_path, "model_iter_50.pth", "train_state_iter_x.pth", ".train_state_iter_99.pth.tmp123", "train_state_iter_77.pth.tmp",
           "train_state_iter_.pth", "xtrain_state_iter_88.pth")
    assert ts.find_latest_state(str(tmp_path)) is None
    _touch(tmp_path, "train_state_iter_9.pth")
    assert ts.find_latest_state(str(tmp_path)) == str(tmp_path / "train_state_iter_9.pth")
    _touch(tmp_path, "train_state_iter_10.pth")
    assert ts.find_latest_state(str(tmp_path)) == str(tmp_path / "train_state_iter_10.pth")      # by number, not by name


def test_prune_states_keeps_newest_and_model_files(tmp_path):
    _touch(tmp_path, *[f"train_state_iter_{n}.pth" for n in (2, 4, 9, 10)], "model_iter_2.pth", "model_iter_4.pth", "model_iter_10.pth",
           "train_state_iter_x.pth", ".train_state_iter_3.pth.tmp7")
    gone = ts.prune_states(str(tmp_path), 2)
    assert sorted(os.path.basename(p) for p in gone) == ["train_state_iter_2.pth", "train_state_iter_4.pth"]
    assert sorted(os.listdir(tmp_path)) == sorted(["train_state_iter_9.pth", "train_state_iter_10.pth", "model_iter_2.pth", "model_iter_4.pth",
                                                   "model_iter_10.pth", "train_state_iter_x.pth", ".train_state_iter_3.pth.tmp7"])
    assert ts.prune_states(str(tmp_path), 2) == []
    assert ts.prune_states(str(tmp_path / "missing"), 2) == []


# ---------------------------------------------------------------------------------------------------------------- 6. compatibility
@pytest.mark.parametrize("key,other", [("seed", 6), ("world", 2), ("spg", 1), ("max_iters", 8), ("n_train", 9), ("lvc_iter", 3),
                                       ("seg_aff_iter", 4), ("caa_thre", 0.88), ("train_set", "train_aug"), ("name", "coco")])
def test_check_resume_compat_names_the_key(key, other):
    ts.check_resume_compat(dict(RUN), dict(RUN))
    cur = dict(RUN)
    cur[key] = other
    with pytest.raises(ValueError) as e:
        ts.check_resume_compat(dict(RUN), cur)
    msg = str(e.value)
    assert key in msg and repr(RUN[key]) in msg and repr(other) in msg
    # the FIRST differing key in the documented order
    cur["radius"] = 99
    first = key if ts.RUN_KEYS.index(key) < ts.RUN_KEYS.index("radius") else "radius"
    with pytest.raises(ValueError, match=f"cannot resume: {first} "):
        ts.check_resume_compat(dict(RUN), cur)


def test_check_resume_compat_missing_key_and_run_config():
    cur = dict(RUN)
    del cur["spg"]
    with pytest.raises(ValueError, match="spg"):
        ts.check_resume_compat(dict(RUN), cur)
    a = train_voc.get_parser().parse_args(["--seed", "5", "--spg", "2", "--crop_size", "96"])
    run = ts.run_config(a, train_voc.VOC, 1, 8)
    assert set(run) == set(ts.RUN_KEYS) == set(RUN)
    assert (run["seed"], run["world"], run["spg"], run["n_train"], run["crop_size"], run["name"], run["lvc_iter"], run["seg_aff_iter"]) == \
        (5, 1, 2, 8, 96, "voc", 14000, 24000)
    assert ts.run_config(train_coco.get_parser().parse_args([]), train_coco.COCO, 8, 100)["seg_aff_iter"] is None
    # what only reports or paces is not in it
    b = train_voc.get_parser().parse_args(["--seed", "5", "--spg", "2", "--crop_size", "96", "--eval_iters", "7", "--log_iters", "3",
                                           "--num_workers", "1", "--val_batch_size", "2", "--save_visual", "true", "--work_dir", "elsewhere"])
    ts.check_resume_compat(run, ts.run_config(b, train_voc.VOC, 1, 8))


# ---------------------------------------------------------------------------------------------------------------- 7. the loss log
def test_truncate_loss_log(tmp_path):
    p = str(tmp_path / "losses.txt")
    assert ts.truncate_loss_log(p, 3) == 0 and open(p, "rb").read() == b""                    # created
    lines = [b"%d %.9g %.9g %.9g\n" % (i, 1.0 / i, 0.123456789 * i, 1e-4 * i) for i in range(1, 11)]
    open(p, "wb").write(b"".join(lines))
    assert ts.truncate_loss_log(p, 10) == 10 and open(p, "rb").read() == b"".join(lines)
    assert ts.truncate_loss_log(p, 9) == 9 and open(p, "rb").read() == b"".join(lines[:9])    # 10 > 9 goes, "1 ..." stays: by number
    open(p, "ab").write(b"10 0.5 0.")                                                          # a process killed in the middle of a line
    assert ts.truncate_loss_log(p, 12) == 9 and open(p, "rb").read() == b"".join(lines[:9])
    assert ts.truncate_loss_log(p, 4) == 4 and open(p, "rb").read() == b"".join(lines[:4])
    assert ts.truncate_loss_log(p, 0) == 0 and open(p, "rb").read() == b""
    assert os.listdir(tmp_path) == ["losses.txt"]


# ---------------------------------------------------------------------------------------------------------------- 8. the flags
@pytest.mark.parametrize("prog", [train_voc, train_coco])
def test_resume_flags_and_defaults(prog):
    a = prog.get_parser().parse_args([])
    assert (a.save_state_iters, a.keep_states, a.iters_per_run, a.resume) == (0, 2, 0, None)
    b = prog.get_parser().parse_args(["--save_state_iters", "2000", "--keep_states", "3", "--iters_per_run", "10000", "--resume", "auto"])
    assert (b.save_state_iters, b.keep_states, b.iters_per_run, b.resume) == (2000, 3, 10000, "auto")
    assert prog.get_parser().parse_args(["--resume", "a/b.pth"]).resume == "a/b.pth"
    assert hasattr(a, "save_ckpt_from") == (prog is train_coco)


# ---------------------------------------------------------------------------------------------------------------- train() over stubs
def _stub_train(monkeypatch, tmp_path, work, extra, n_train=8):
    """train() with the device-side pieces stubbed: the REAL loader positions and state files, a trainer whose 'weights' and 'moments'
    are running sums of a hash of the batch's names, so a wrong position, step or state shows in every later loss."""
    from excel_amd.engine import validatation_engine as ve
    val_calls = []

    class _Trainer:
        def __init__(self, model, par, seed=0, **k):
            self.model, self.global_step, self.seed = model, 0, seed
            self.w, self.m = torch.zeros(3, dtype=torch.float64), None

        def train_step(self, names, cls, n_iter):
            assert n_iter == self.global_step
            h = zlib.crc32(" ".join(names).encode()) % 1000 + self.seed * 1000003 + self.global_step
            self.m = (torch.zeros(3, dtype=torch.float64) if self.m is None else self.m) * 0.9 + h
            self.w = self.w + self.m * 1e-3
            self.model.w = self.w                             # what the 'model' checkpoints and validates
            self.global_step += 1
            return dict(seg_loss=float(self.w.sum()), diver_loss=float(self.m[0]), lr=1.0 / self.global_step)

        def state_dict(self):
            return dict(global_step=self.global_step, model={"decoder.w": self.w.clone()},
                        optimizer=None if self.m is None else {"exp_avg": {"w": self.m.clone()}, "exp_avg_sq": {"w": self.m.clone() * 2}})

        def load_state_dict(self, st):
            self.global_step, self.w, self.m = st["global_step"], st["model"]["decoder.w"].clone(), st["optimizer"]["exp_avg"]["w"].clone()
            assert torch.equal(st["optimizer"]["exp_avg_sq"]["w"], self.m * 2)
            self.model.w = self.w

    class _Feeder:
        def __init__(self, batches, device, **k):
            self.batches = batches

        def __iter__(self):
            for rb in self.batches:
                yield list(rb.names), None, list(rb.names), None, None

        def close(self):
            self.batches.close()

    class _Variant(train_voc.TrainVariant):
        lvc_iter, seg_aff_iter = 2, 4

        @staticmethod
        def datasets(args):
            class _Val:
                def __len__(self):
                    return 2
            return _CountingSet(n_train), _Val()

        @staticmethod
        def augment(images, plan, labels, args):
            return images                                     # the stub feeder hands the names over in `images`' place

    def fake_ragged(**kw):
        val_calls.append(kw)
        return "TABLE w=%r" % kw["model"].w.tolist(), {}, {}, {}

    monkeypatch.setattr(ve, "build_validation_ragged", fake_ragged)
    monkeypatch.setattr(train_voc, "DecoderTrainer", _Trainer)
    monkeypatch.setattr(loader, "DeviceFeeder", _Feeder)
    monkeypatch.setattr(torch.cuda, "set_device", lambda *a, **k: None)
    monkeypatch.setattr(torch.cuda, "synchronize", lambda *a, **k: None)
    args = train_voc.get_parser().parse_args(["--max_iters", "7", "--eval_iters", "3", "--log_iters", "2", "--spg", "2", "--seed", "5",
                                              "--work_dir", str(tmp_path / work), "--num_classes", "5", "--num_workers", "1"] + list(extra))
    model = types.SimpleNamespace(w=None)
    model.state_dict = lambda: {"decoder.w": torch.zeros(3) if model.w is None else model.w}
    return train_voc.train(args, model=model, variant=_Variant()), val_calls


@pytest.mark.parametrize("K", [2, 3])
def test_train_split_run_equals_straight_run_over_stubs(monkeypatch, tmp_path, K):
    res_a, val_a = _stub_train(monkeypatch, tmp_path, "a", [])
    assert set(res_a) == {"history", "tables", "ckpts", "val_seconds"}                         # no new flag: the keys of before
    assert len(res_a["history"]) == 7 and len(res_a["tables"]) == 2
    assert not [f for f in os.listdir(tmp_path / "a" / "checkpoints") if f.startswith("train_state")]
    runs = []
    while not runs or runs[-1]["history"][-1]["iter"] < 7:
        runs.append(_stub_train(monkeypatch, tmp_path, "b", ["--iters_per_run", str(K), "--resume", "auto"])[0])
        assert len(runs) <= 4
    stops = [r["history"][-1]["iter"] for r in runs]
    assert stops == ([2, 4, 6, 7] if K == 2 else [3, 6, 7])
    assert open(tmp_path / "b" / "losses.txt", "rb").read() == open(tmp_path / "a" / "losses.txt", "rb").read()
    assert len(open(tmp_path / "b" / "losses.txt").read().splitlines()) == 7
    assert [h for r in runs for h in r["history"]] == res_a["history"]
    assert [t for r in runs for t in r["tables"]] == res_a["tables"]                            # no validation ran twice
    ck = str(tmp_path / "b" / "checkpoints")
    assert runs[0]["resumed_from"] is None
    assert [r["resumed_from"] for r in runs[1:]] == [ts.state_path(ck, n) for n in stops[:-1]]
    assert [r["states"] for r in runs] == [[ts.state_path(ck, n)] for n in stops[:-1]] + [[]]
    for n in (3, 6):
        a = torch.load(str(tmp_path / "a" / "checkpoints" / f"model_iter_{n}.pth"))
        b = torch.load(os.path.join(ck, f"model_iter_{n}.pth"))
        assert torch.equal(a["decoder.w"], b["decoder.w"])
    # a finished run: nothing to do, nothing touched
    st = ts.load_train_state(ts.state_path(ck, stops[-2]))
    ts.save_train_state(ts.state_path(ck, 7), 7, st["model_state_dict"], st["optimizer_state_dict"], 0.1, st["run"])
    log = open(tmp_path / "b" / "losses.txt", "rb").read()
    done = _stub_train(monkeypatch, tmp_path, "b", ["--iters_per_run", str(K), "--resume", "auto"])[0]
    assert done["history"] == [] and done["tables"] == [] and done["resumed_from"] == ts.state_path(ck, 7)
    assert open(tmp_path / "b" / "losses.txt", "rb").read() == log


def test_train_resume_refusals_and_pruning_over_stubs(monkeypatch, tmp_path):
    res, _ = _stub_train(monkeypatch, tmp_path, "c", ["--save_state_iters", "2", "--keep_states", "2"])
    ck = str(tmp_path / "c" / "checkpoints")
    assert res["states"] == [ts.state_path(ck, n) for n in (2, 4, 6)] and res["resumed_from"] is None
    assert sorted(f for f in os.listdir(ck) if f.startswith("train_state")) == ["train_state_iter_4.pth", "train_state_iter_6.pth"]
    assert sorted(f for f in os.listdir(ck) if f.startswith("model_iter")) == ["model_iter_3.pth", "model_iter_6.pth"]
    log = open(tmp_path / "c" / "losses.txt", "rb").read()
    for flag, val, key in (("--seed", "6", "seed"), ("--spg", "1", "spg"), ("--max_iters", "8", "max_iters")):
        with pytest.raises(ValueError, match=f"cannot resume: {key} "):
            _stub_train(monkeypatch, tmp_path, "c", ["--resume", "auto", flag, val])
        assert open(tmp_path / "c" / "losses.txt", "rb").read() == log
    with pytest.raises(ValueError, match="cannot resume: n_train "):
        _stub_train(monkeypatch, tmp_path, "c", ["--resume", "auto"], n_train=9)
    with pytest.raises(FileNotFoundError):
        _stub_train(monkeypatch, tmp_path, "c", ["--resume", str(tmp_path / "c" / "checkpoints" / "train_state_iter_5.pth")])
    assert open(tmp_path / "c" / "losses.txt", "rb").read() == log
    # a process that got further than its last state: resuming from iteration 4 rewrites lines 5..7 to the same bytes
    again, _ = _stub_train(monkeypatch, tmp_path, "c", ["--resume", ts.state_path(ck, 4), "--eval_iters", "100"])
    assert [h["iter"] for h in again["history"]] == [5, 6, 7] and again["tables"] == []
    assert open(tmp_path / "c" / "losses.txt", "rb").read() == log
