"""CPU tests of the training data path: the host tables of ops.train_augment reproduce Pillow bit for bit, the augmentation draws are
deterministic, rank shards partition an epoch, the initial head has the model's key set, and checkpoints load through infer_lam."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import _train_aug_ref as R  # noqa: E402

REC = 40


def _apply_tables(table, b, img, lab):
    """Pillow's two 8-bit passes and the NEAREST lookup, driven by the tables excel_train_aug_plan built (full rescaled image)."""
    r = table[REC * b:REC * b + REC]
    h, w, h2, w2, kx, ky = r[0], r[1], r[2], r[3], r[7], r[9]
    mid = img.astype(np.int64)
    if kx:
        t = table[r[6]:r[6] + w2 * (2 + kx)].reshape(w2, 2 + kx)
        out = np.empty((h, w2, 3), np.int64)
        for x in range(w2):
            acc = (1 << 21) + (mid[:, t[x, 0]:t[x, 0] + t[x, 1], :] * t[x, 2:2 + t[x, 1]][None, :, None]).sum(1)
            out[:, x] = np.clip(acc >> 22, 0, 255)
        mid = out
    if ky:
        t = table[r[8]:r[8] + h2 * (2 + ky)].reshape(h2, 2 + ky)
        out = np.empty((h2, w2, 3), np.int64)
        for y in range(h2):
            acc = (1 << 21) + (mid[t[y, 0]:t[y, 0] + t[y, 1]] * t[y, 2:2 + t[y, 1]][:, None, None]).sum(0)
            out[y] = np.clip(acc >> 22, 0, 255)
        mid = out
    nx, ny = table[r[10]:r[10] + w2], table[r[11]:r[11] + h2]
    return mid.astype(np.uint8), lab[ny][:, nx]


def test_aug_tables_reproduce_pillow_bit_for_bit():
    from excel_amd import ops
    rng = np.random.default_rng(0)
    sizes = [(375, 500), (500, 333)] + [tuple(rng.integers(8, 160, 2)) for _ in range(30)]
    for i, (h, w) in enumerate(sizes):
        img = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
        lab = rng.integers(0, 21, (h, w), dtype=np.uint8)
        p = R.make_params(1)
        p[0]["ratio"] = {0: 0.5, 1: 2.0, 2: 1.0 + 0.5 / w, 3: 1.0}.get(i, rng.uniform(0.5, 2.0))
        plan = ops.TrainAugPlan([(h, w)], p, 8, None)
        got_img, got_lab = _apply_tables(plan.table_host, 0, img, lab)
        ref_img, ref_lab = R.rescale(img, lab, float(p[0]["ratio"]))
        assert got_img.shape == ref_img.shape and np.array_equal(got_img, ref_img), (h, w, float(p[0]["ratio"]))
        assert np.array_equal(got_lab, ref_lab), (h, w, float(p[0]["ratio"]))
    # the width-unchanged case really skips the horizontal pass (Pillow does)
    p = R.make_params(1)
    p[0]["ratio"] = 1.0 + 0.5 / 500
    assert ops.TrainAugPlan([(375, 500)], p, 8, None).table_host[7] == 0


def test_aug_plan_refuses_out_of_range_params():
    from excel_amd import ops
    p = R.make_params(1)
    p[0]["ratio"] = 1.0
    ops.TrainAugPlan([(40, 50)], p, 32, None)
    for field, value, msg in (("ratio", 9.0, "ratio"), ("flip", 2, "flip"), ("h_pad", 1, "placement"), ("w_pad", -1, "placement")):
        q = p.copy()
        q[0][field] = value
        with pytest.raises(RuntimeError, match=msg):
            ops.TrainAugPlan([(40, 50)], q, 32, None)
    q = p.copy()
    q[0]["cand_w"][3] = 50 - 32 + 1
    with pytest.raises(RuntimeError, match="candidate 3"):
        ops.TrainAugPlan([(40, 50)], q, 32, None)
    with pytest.raises(RuntimeError, match="S"):
        ops.TrainAugPlan([(40, 50)], p, 0, None)


def _tiny_voc(tmp_path, n=6, seed=0):
    from PIL import Image
    rng = np.random.default_rng(seed)
    root = tmp_path / "VOC"
    (root / "JPEGImages").mkdir(parents=True)
    (root / "SegmentationClassAug").mkdir()
    names, onehot = [], {}
    for i in range(n):
        name = f"2007_{i:06d}"
        h, w = int(rng.integers(40, 90)), int(rng.integers(40, 90))
        Image.fromarray(rng.integers(0, 256, (h, w, 3), dtype=np.uint8)).save(root / "JPEGImages" / f"{name}.jpg")
        lab = rng.integers(0, 3, (h, w)).astype(np.uint8)
        im = Image.fromarray(lab, mode="P")
        im.putpalette([0, 0, 0, 128, 0, 0, 0, 128, 0] + [0] * (253 * 3))
        im.save(root / "SegmentationClassAug" / f"{name}.png")
        names.append(name)
        onehot[name] = np.eye(20, dtype=np.float32)[[1]].sum(0)
    (tmp_path / "train.txt").write_text("\n".join(names) + "\n")
    np.save(tmp_path / "cls_labels_onehot.npy", onehot)
    return str(root), str(tmp_path)


def test_param_draws_are_deterministic(tmp_path):
    from excel_amd.datasets import voc
    root, lists = _tiny_voc(tmp_path)
    a = voc.VOC12ClsDataset(root, lists, "train", crop_size=48, seed=3)
    b = voc.VOC12ClsDataset(root, lists, "train", crop_size=48, seed=3)
    s1 = [a.sample(i, epoch=2)[4] for i in range(len(a))]
    s2 = [b.sample(i, epoch=2)[4] for i in reversed(range(len(b)))][::-1]          # order / worker independent
    assert all(x.tobytes() == y.tobytes() for x, y in zip(s1, s2))
    assert a.sample(0, epoch=3)[4].tobytes() != s1[0].tobytes()
    c = voc.VOC12ClsDataset(root, lists, "train", crop_size=48, seed=4)
    assert c.sample(0, epoch=2)[4].tobytes() != s1[0].tobytes()
    name, img, lab, cls, p = a.sample(1, epoch=0)
    h, w = img.shape[:2]
    h2, w2 = int(float(p["ratio"]) * h), int(float(p["ratio"]) * w)
    H, W = max(48, h2), max(48, w2)
    assert 0.5 <= float(p["ratio"]) <= 2.0 and 0 <= p["h_pad"] <= H - h2 and 0 <= p["w_pad"] <= W - w2
    assert np.all((0 <= p["cand_h"]) & (p["cand_h"] <= H - 48)) and np.all((0 <= p["cand_w"]) & (p["cand_w"] <= W - 48))
    assert lab.shape == (h, w) and lab.dtype == np.uint8 and cls.shape == (20,)
    from excel_amd import ops
    ops.TrainAugPlan([(h, w)], p[None], 48, None)                                     # in range for the plan's checks


@pytest.mark.parametrize("n", [96, 101])
def test_rank_shards_are_disjoint_and_cover_the_epoch(n):
    from excel_amd.datasets.loader import epoch_shard
    for world in (1, 2, 4):
        for epoch in (0, 1):
            shards = [epoch_shard(n, epoch, r, world, seed=7) for r in range(world)]
            allidx = np.concatenate(shards)
            assert len(set(allidx.tolist())) == len(allidx) == n - n % world
            assert all(len(s) == n // world for s in shards)
        assert not np.array_equal(epoch_shard(n, 0, 0, world, 7), epoch_shard(n, 1, 0, world, 7))


def test_train_batches_shape_and_drop_last(tmp_path):
    from excel_amd.datasets import loader, voc
    root, lists = _tiny_voc(tmp_path, n=5)
    ds = voc.VOC12ClsDataset(root, lists, "train", crop_size=48, seed=1)
    it = loader.train_batches(ds, 2, num_threads=2)
    seen = [next(it) for _ in range(4)]                     # 5 samples, batch 2: two batches per epoch, the fifth sample dropped
    for rb in seen:
        assert len(rb) == 2 and rb.params.shape == (2,) and rb.images.numel() == 3 * int((rb.hw[:, 0] * rb.hw[:, 1]).sum())
    first = {n for rb in seen[:2] for n in rb.names}
    assert len(first) == 4
    it.close()


def test_init_decoder_state_dict_keys_and_shapes():
    from excel_amd.model import init_decoder_state_dict
    from excel_amd.model.decoder.TransDecoder import DecoderTransformer
    from excel_amd.model.segformer_head import SegFormerHead
    sd = init_decoder_state_dict(num_classes=21, in_channels=768, embedding_dim=256, crop_size=320, seed=0)
    fuse = {k[len("decoder_fts_fuse."):]: v for k, v in sd.items() if k.startswith("decoder_fts_fuse.")}
    dec = {k[len("decoder."):]: v for k, v in sd.items() if k.startswith("decoder.")}
    assert len(fuse) + len(dec) == len(sd)
    head, tr = SegFormerHead(in_channels=768, embedding_dim=256, num_classes=21, index=12), DecoderTransformer(256, 3, 8, 21)
    need_fuse = {f"linears_modulelist.{l}.{k}" for l in range(12) for k in ("proj.weight", "proj.bias", "proj_2.weight", "proj_2.bias")}
    need_fuse |= {"linear_fuse.weight", "linear_fuse.bias"}
    assert set(fuse) == need_fuse
    head.load_state_dict(fuse)
    tr.load_state_dict(dec)
    blk = {"ln_1.weight", "ln_1.bias", "attn.in_proj_weight", "attn.in_proj_bias", "attn.out_proj.weight", "attn.out_proj.bias",
           "ln_2.weight", "ln_2.bias", "mlp.c_fc.weight", "mlp.c_fc.bias", "mlp.c_proj.weight", "mlp.c_proj.bias"}
    assert set(dec) == {f"transformer.resblocks.{l}.{k}" for l in range(3) for k in blk} | {"linear_pred.weight", "linear_pred.bias"}
    assert tuple(fuse["linears_modulelist.0.proj.weight"].shape) == (256, 768)
    assert tuple(fuse["linear_fuse.weight"].shape) == (256, 256 * 12, 1, 1)
    assert tuple(dec["transformer.resblocks.0.attn.in_proj_weight"].shape) == (768, 256)
    assert tuple(dec["linear_pred.weight"].shape) == (21, 256, 1, 1)
    # the modules' own initialisation: zero attention biases, unit LayerNorm, xavier-uniform in_proj, kaiming-uniform Linear bound
    assert float(dec["transformer.resblocks.1.attn.in_proj_bias"].abs().max()) == 0.0
    assert float(dec["transformer.resblocks.1.attn.out_proj.bias"].abs().max()) == 0.0
    assert float((dec["transformer.resblocks.2.ln_1.weight"] - 1).abs().max()) == 0.0
    assert float(dec["transformer.resblocks.0.attn.in_proj_weight"].abs().max()) <= (6 / (256 + 768)) ** 0.5
    assert float(fuse["linears_modulelist.3.proj.weight"].abs().max()) <= 1 / 768 ** 0.5
    again = init_decoder_state_dict(num_classes=21, in_channels=768, embedding_dim=256, crop_size=320, seed=0)
    assert all(bool((again[k] == v).all()) for k, v in sd.items())
    other = init_decoder_state_dict(num_classes=21, in_channels=768, embedding_dim=256, crop_size=320, seed=1)
    assert not bool((other["decoder.linear_pred.weight"] == sd["decoder.linear_pred.weight"]).all())


def test_checkpoint_keys_round_trip_through_infer_lam_loader(tmp_path):
    import torch
    from excel_amd.model import init_decoder_state_dict
    from excel_amd.tools import infer_lam
    sd = init_decoder_state_dict(num_classes=5, in_channels=128, embedding_dim=32, crop_size=96, seed=0, index=8)
    path = str(tmp_path / "model_iter_3.pth")
    torch.save(sd, path)
    ddp = str(tmp_path / "ddp.pth")                                        # the reference's DDP checkpoints carry "module."
    torch.save({"module." + k: v for k, v in sd.items()}, ddp)
    args = infer_lam.get_parser().parse_args(["--training_free", "false", "--synthetic", "4"])
    for p in (path, ddp):
        args.model_path = p
        kw = infer_lam.resolve_model_inputs(args)
        got = kw["decoder_state_dict"]
        assert set(got) == set(sd)
        assert all(bool((got[k] == sd[k]).all()) for k in sd)
