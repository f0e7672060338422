"""Resumable decoder training on the device: a run cut into pieces (--iters_per_run / --resume auto, every piece on a freshly built
model) equals the uninterrupted run bit for bit - loss log, checkpoints, head, AdamW moments, validation tables - across both schedule
switches (lvc_iter, seg_aff_iter), at mid-epoch stops, an epoch boundary and validation iterations; refusals; pruning; in-place loads.
No tolerance anywhere: every comparison is equality."""
import logging
import os

import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

from _train_tiny import tiny_model, train_args, voc_tree  # noqa: E402


def _variant():
    from excel_amd.scripts.train_voc import TrainVariant

    class _Early(TrainVariant):          # VOC with both switches inside a 7-iteration run, so a resumed piece crosses them
        lvc_iter = 2
        seg_aff_iter = 4
    return _Early()


def _states_in(work):
    return sorted(f for f in os.listdir(os.path.join(work, "checkpoints")) if f.startswith("train_state"))


def _same(a, b):
    assert list(a) == list(b)
    for k in a:
        assert a[k].dtype == b[k].dtype and torch.equal(a[k].cpu(), b[k].cpu()), k


@pytest.fixture(scope="module")
def run_a(tmp_path_factory):
    """The uninterrupted run: 7 iterations (4 batches per epoch), validation and checkpoint at 3 and 6.  Computed once, read only."""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from excel_amd.scripts.train_voc import train
    base = tmp_path_factory.mktemp("resume")
    root, lists = voc_tree(base)
    model = tiny_model()
    work = str(base / "a")
    res = train(train_args(root, lists, work), model=model, variant=_variant())
    assert len(res["history"]) == 7
    return dict(root=root, lists=lists, work=work, res=res, log=open(os.path.join(work, "losses.txt"), "rb").read(),
                head={k: v.cpu() for k, v in model.state_dict().items()}, opt=model._dec.optimizer_state())


@pytest.mark.timeout(600)
@pytest.mark.parametrize("K", [2, 3])
def test_split_run_equals_straight_run(run_a, tmp_path, caplog, K):
    """K = 2 stops at 2 and 6 (mid-epoch) and 4 (an epoch boundary), none a validation iteration; K = 3 stops at 3 and 6, mid-epoch and
    both validation iterations.  Every piece starts from a model at its INITIAL weights: what it continues with comes from the file."""
    from excel_amd.scripts.train_voc import train
    caplog.set_level(logging.INFO)
    work = str(tmp_path / "b")
    pieces = []
    while not pieces or pieces[-1]["history"][-1]["iter"] < 7:
        assert len(pieces) < 4
        model = tiny_model()
        pieces.append(train(train_args(run_a["root"], run_a["lists"], work, extra=["--iters_per_run", str(K), "--resume", "auto"]),
                            model=model, variant=_variant()))
    stops = [p["history"][-1]["iter"] for p in pieces]
    assert stops == ([2, 4, 6, 7] if K == 2 else [3, 6, 7])
    log_b = open(os.path.join(work, "losses.txt"), "rb").read()
    assert log_b == run_a["log"] and len(log_b.splitlines()) == 7
    assert [h for p in pieces for h in p["history"]] == run_a["res"]["history"]
    for n in (3, 6):
        _same(torch.load(os.path.join(run_a["work"], "checkpoints", f"model_iter_{n}.pth")),
              torch.load(os.path.join(work, "checkpoints", f"model_iter_{n}.pth")))
    assert [os.path.basename(c) for p in pieces for c in p["ckpts"]] == ["model_iter_3.pth", "model_iter_6.pth"]
    _same(run_a["head"], model.state_dict())
    opt_b = model._dec.optimizer_state()
    assert set(opt_b) == set(run_a["opt"]) == {"exp_avg", "exp_avg_sq"}
    for part in opt_b:
        _same(run_a["opt"][part], opt_b[part])
    tables_b = [t for p in pieces for t in p["tables"]]
    assert len(run_a["res"]["tables"]) == 2 and tables_b == run_a["res"]["tables"]              # no validation ran twice
    ck = os.path.join(work, "checkpoints")
    assert pieces[0]["resumed_from"] is None
    assert [p["resumed_from"] for p in pieces[1:]] == [os.path.join(ck, f"train_state_iter_{n}.pth") for n in stops[:-1]]
    assert pieces[-1]["resumed_from"] == os.path.join(ck, "train_state_iter_6.pth")
    assert [p["states"] for p in pieces] == [[os.path.join(ck, f"train_state_iter_{n}.pth")] for n in stops[:-1]] + [[]]
    assert "train_state_iter_6.pth: continuing after iteration 6 of 7" in caplog.text
    # the file itself: the reference's keys, plain data, the head's keys of model_iter_N.pth
    st = torch.load(os.path.join(ck, "train_state_iter_6.pth"), map_location="cpu", weights_only=True)
    assert set(st) == {"step", "model_state_dict", "optimizer_state_dict", "lr", "format_version", "run"} and st["step"] == 6
    assert list(st["model_state_dict"]) == list(torch.load(os.path.join(ck, "model_iter_6.pth")))
    assert st["lr"] == run_a["res"]["history"][5]["lr"] and st["run"]["lvc_iter"] == 2 and st["run"]["n_train"] == 8


@pytest.mark.timeout(600)
def test_refusals_come_before_any_work(run_a, tmp_path):
    from excel_amd.scripts.train_voc import train
    work = str(tmp_path / "b")
    args = lambda extra=(), **over: train_args(run_a["root"], run_a["lists"], work, extra=list(extra), **over)
    first = train(args(["--iters_per_run", "2", "--resume", "auto"]), model=tiny_model(), variant=_variant())
    assert _states_in(work) == ["train_state_iter_2.pth"] and first["history"][-1]["iter"] == 2
    log = open(os.path.join(work, "losses.txt"), "rb").read()
    assert log == b"".join(run_a["log"].splitlines(keepends=True)[:2])
    model = tiny_model()
    before = {k: v.clone() for k, v in model.state_dict().items()}
    for over, key in ((dict(seed=6), "seed"), (dict(spg=1), "spg"), (dict(max_iters=8), "max_iters")):
        with pytest.raises(ValueError, match=f"cannot resume: {key} "):
            train(args(["--resume", "auto"], **over), model=model, variant=_variant())
        assert open(os.path.join(work, "losses.txt"), "rb").read() == log
    from excel_amd.scripts.train_voc import VOC
    with pytest.raises(ValueError, match="cannot resume: lvc_iter "):                           # the variant's switches are part of the run
        train(args(["--resume", "auto"]), model=model, variant=VOC)
    with pytest.raises(FileNotFoundError):
        train(args(["--resume", os.path.join(work, "checkpoints", "train_state_iter_3.pth")]), model=model, variant=_variant())
    assert open(os.path.join(work, "losses.txt"), "rb").read() == log and _states_in(work) == ["train_state_iter_2.pth"]
    _same(before, model.state_dict())
    assert model._dec.optimizer_state() is None
    # `--resume auto` with nothing to resume: the run from scratch
    empty = str(tmp_path / "c")
    res = train(train_args(run_a["root"], run_a["lists"], empty, extra=["--resume", "auto"]), model=model, variant=_variant())
    assert res["resumed_from"] is None and res["states"] == [] and _states_in(empty) == []
    assert open(os.path.join(empty, "losses.txt"), "rb").read() == run_a["log"]
    assert res["tables"] == run_a["res"]["tables"]
    _same(run_a["head"], model.state_dict())


@pytest.mark.timeout(600)
def test_off_by_default_and_pruning(run_a, tmp_path):
    from excel_amd.scripts.train_voc import train
    assert _states_in(run_a["work"]) == []                                                      # run A had none of the flags
    assert set(run_a["res"]) == {"history", "tables", "ckpts", "val_seconds"}
    work = str(tmp_path / "s")
    res = train(train_args(run_a["root"], run_a["lists"], work, extra=["--save_state_iters", "2", "--keep_states", "2"]),
                model=tiny_model(), variant=_variant())
    ck = os.path.join(work, "checkpoints")
    assert res["states"] == [os.path.join(ck, f"train_state_iter_{n}.pth") for n in (2, 4, 6)] and res["resumed_from"] is None
    assert _states_in(work) == ["train_state_iter_4.pth", "train_state_iter_6.pth"]
    assert sorted(f for f in os.listdir(ck) if f.startswith("model_iter")) == ["model_iter_3.pth", "model_iter_6.pth"]
    assert open(os.path.join(work, "losses.txt"), "rb").read() == run_a["log"]                  # writing states changes nothing


@pytest.mark.timeout(600)
def test_in_place_load(run_a):
    from excel_amd.scripts.train_voc import DecoderTrainer
    model = tiny_model()
    dec = model._dec
    ptrs = {k: t.data_ptr() for k, t in dec.t.items()}
    assert dec.optimizer_state() is None
    assert model.load_decoder_state_dict(run_a["head"]) is model
    dec.load_optimizer_state(run_a["opt"])
    adam_ptrs = {k: (m.data_ptr(), v.data_ptr()) for k, (m, v) in dec._adam.items()}
    dec.load_optimizer_state(run_a["opt"])
    model.load_decoder_state_dict(run_a["head"])
    assert {k: t.data_ptr() for k, t in dec.t.items()} == ptrs
    assert {k: (m.data_ptr(), v.data_ptr()) for k, (m, v) in dec._adam.items()} == adam_ptrs
    _same(run_a["head"], model.state_dict())
    for part in run_a["opt"]:
        _same(run_a["opt"][part], dec.optimizer_state()[part])
    assert list(model.decoder_fts_fuse.state_dict()) == [k[len("decoder_fts_fuse."):] for k in run_a["head"] if k.startswith("decoder_fts_fuse.")]
    assert torch.equal(model.decoder.state_dict()["linear_pred.bias"], run_a["head"]["decoder.linear_pred.bias"])
    x = torch.randn(2, 3, 96, 96, generator=torch.Generator().manual_seed(0)).cuda()
    assert torch.equal(model(x)[0], tiny_model(dec=run_a["head"])(x)[0])                         # the C handle reads the loaded weights

    # refusals name the key and leave everything as it was
    keep_w = {k: t.clone() for k, t in dec.t.items()}
    keep_m = dec.optimizer_state()
    gone = "decoder.transformer.resblocks.1.mlp.c_fc.weight"
    with pytest.raises(ValueError, match=gone.replace(".", r"\.")):
        model.load_decoder_state_dict({k: v * 2 for k, v in run_a["head"].items() if k != gone})
    bad = {k: v * 2 for k, v in run_a["head"].items()}
    bad["decoder_fts_fuse.linear_fuse.weight"] = bad["decoder_fts_fuse.linear_fuse.weight"][:, :-1]
    with pytest.raises(ValueError, match=r"decoder_fts_fuse\.linear_fuse\.weight"):
        model.load_decoder_state_dict(bad)
    double = lambda: {part: {k: v * 2 for k, v in d.items()} for part, d in run_a["opt"].items()}
    o = double()
    del o["exp_avg_sq"]["blk0.fc1_w"]
    with pytest.raises(ValueError, match=r"missing key exp_avg_sq\.blk0\.fc1_w"):
        dec.load_optimizer_state(o)
    o = double()
    o["exp_avg"]["nobody"] = torch.zeros(1)
    with pytest.raises(ValueError, match=r"extra key exp_avg\.nobody"):
        dec.load_optimizer_state(o)
    o = double()
    o["exp_avg_sq"]["pred_b"] = o["exp_avg_sq"]["pred_b"][:-1]
    with pytest.raises(ValueError, match=r"exp_avg_sq\.pred_b has shape"):
        dec.load_optimizer_state(o)
    o = double()
    o["exp_avg"]["pred_w"] = o["exp_avg"]["pred_w"].double()
    with pytest.raises(ValueError, match=r"exp_avg\.pred_w is torch\.float64"):
        dec.load_optimizer_state(o)
    with pytest.raises(ValueError, match="exp_avg_sq"):
        dec.load_optimizer_state({"exp_avg": o["exp_avg"]})
    _same(keep_w, dec.t)
    for part in keep_m:
        _same(keep_m[part], dec.optimizer_state()[part])
    assert {k: t.data_ptr() for k, t in dec.t.items()} == ptrs

    # DecoderTrainer carries the three together
    from excel_amd.utils.PAR import PAR
    tr = DecoderTrainer(model, PAR(num_iter=20, dilations=[1, 2, 4, 8, 12, 24]))
    tr.global_step = 7
    sd = tr.state_dict()
    assert set(sd) == {"global_step", "model", "optimizer"} and sd["global_step"] == 7 and all(not v.is_cuda for v in sd["model"].values())
    other = tiny_model()
    tr2 = DecoderTrainer(other, tr.par)
    assert tr2.state_dict()["optimizer"] is None and tr2.global_step == 0
    tr2.load_state_dict(sd)
    assert tr2.global_step == 7
    _same(sd["model"], tr2.state_dict()["model"])
    for part in sd["optimizer"]:
        _same(sd["optimizer"][part], tr2.state_dict()["optimizer"][part])
