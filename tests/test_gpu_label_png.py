"""--save_label on the GPU: excel_png_encode_labels_ragged (png.hip) read back by Pillow AND walked chunk by chunk here with zlib.crc32 /
zlib.decompress (the encoder is never its own judge), batch / stream invariance, the size condition, and infer_lam + eval_labels end to end.

Sizes measured on the MI355X (printed by test_blob_maps_are_at_most_an_eighth_of_raw, not asserted): the 24 blob maps are 4 163 480 B raw,
333 553 B as device files (raw / 12.5) and 165 995 B from Pillow (device / Pillow = 2.01); EXPERIMENTS.md, "Label PNG files"."""
import io
import os
import struct
import zlib

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

SIG = b"\x89PNG\r\n\x1a\n"
CANARY = 0xA5


@pytest.fixture(scope="module")
def gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import excel_amd.ops  # noqa: F401
    return True


def _encode(maps, palette=None, canary=True):
    """Label maps [H_b, W_b] uint8 -> (files [bytes], table [B,2], arena bytes).  The arena is pre-filled with a canary: the encoder clears
    the slots it was given; whatever lies behind the bound of the batch must stay untouched."""
    from excel_amd import ops
    hw = [m.shape for m in maps]
    plan = ops.RaggedPlan(hw, "cuda")
    flat = torch.from_numpy(np.concatenate([m.reshape(-1) for m in maps])).cuda()
    need = ops.png_labels_arena_bytes(hw)
    arena = torch.full((need + 4096,), CANARY, dtype=torch.uint8, device="cuda")
    data, table = ops.png_encode_labels_ragged(flat, plan, palette=palette, out=arena)
    torch.cuda.synchronize()
    assert data.numel() == need
    host, tab = arena.cpu().numpy(), table.cpu().numpy()
    assert (host[need:] == CANARY).all(), "bytes behind the arena bound were written"
    off = 0
    files = []
    for b, (h, w) in enumerate(hw):
        bound = ops.png_labels_bound_bytes(h, w)
        assert int(tab[b, 0]) == off and 0 < int(tab[b, 1]) <= bound, (b, tab[b], bound)
        assert not host[off + int(tab[b, 1]):off + bound].any(), f"image {b}: bytes behind the file inside its slot are not zero"
        files.append(host[off:off + int(tab[b, 1])].tobytes())
        off += bound
    return files, tab, need


def _chunks(f):
    assert f[:8] == SIG
    out, p = [], 8
    while p < len(f):
        n, typ = struct.unpack(">I4s", f[p:p + 8])
        body = f[p + 8:p + 8 + n]
        crc, = struct.unpack(">I", f[p + 8 + n:p + 12 + n])
        assert crc == zlib.crc32(typ + body), (typ, hex(crc), hex(zlib.crc32(typ + body)))
        out.append((typ, body))
        p += 12 + n
    assert p == len(f), "bytes behind IEND"
    return out


def _check_file(f, m, palette):
    """Pillow's reading and the chunk walk both give the label map back, exactly."""
    from PIL import Image
    h, w = m.shape
    im = Image.open(io.BytesIO(f))
    assert im.mode == "P" and im.size == (w, h)
    assert np.array_equal(np.asarray(im), m)
    assert list(im.getpalette()) == [int(v) for v in np.asarray(palette).reshape(-1)]
    ch = _chunks(f)
    assert [c[0] for c in ch] == [b"IHDR", b"PLTE", b"IDAT", b"IEND"]
    assert ch[0][1] == struct.pack(">IIBBBBB", w, h, 8, 3, 0, 0, 0)
    assert ch[1][1] == np.asarray(palette, np.uint8).tobytes() and ch[3][1] == b""
    idat = ch[2][1]
    assert idat[:2] == b"\x78\x01" and (idat[2] & 7) == 3, "zlib header / one final fixed-Huffman block"
    raw = zlib.decompress(idat)                                     # verifies the Adler-32
    assert raw == b"".join(b"\x00" + m[y].tobytes() for y in range(h))


def _palette():
    from excel_amd.utils import imutils
    return imutils.colormap()


def _staircase():
    """Run lengths 1, 2, 3, ... 600 back to back in rows of 601 pixels, values cycling over both literal lengths: every length code and
    every extra-bits class, runs that cross rows and (in wide rows) several maximal matches."""
    vals = [0, 143, 144, 255, 7, 200]
    flat = np.concatenate([np.full(L, vals[L % len(vals)], np.uint8) for L in range(1, 601)])
    W = 601
    H = -(-flat.size // W)
    out = np.full(H * W, 9, np.uint8)
    out[:flat.size] = flat
    return out.reshape(H, W)


def _blob_map(rs, h, w):
    """Smooth-noise blobs, 1-3 foreground classes over background: what a pseudo label looks like."""
    k = int(rs.randint(1, 4))
    classes = rs.choice(np.arange(1, 21), size=k, replace=False)
    gh, gw = h // 32 + 2, w // 32 + 2
    ys, xs = np.linspace(0, gh - 1.001, h), np.linspace(0, gw - 1.001, w)
    y0, x0 = ys.astype(int), xs.astype(int)
    fy, fx = (ys - y0)[:, None], (xs - x0)[None, :]
    planes = [np.full((h, w), 0.55)]
    for _ in range(k):
        g = rs.rand(gh, gw)
        a, b_, c, d = g[y0][:, x0], g[y0][:, x0 + 1], g[y0 + 1][:, x0], g[y0 + 1][:, x0 + 1]
        planes.append((a * (1 - fx) + b_ * fx) * (1 - fy) + (c * (1 - fx) + d * fx) * fy)
    idx = np.argmax(np.stack(planes), 0)
    return np.concatenate([[0], classes]).astype(np.uint8)[idx]


def _blob_maps():
    rs = np.random.RandomState(2024)
    return [_blob_map(rs, int(rs.randint(300, 501)), int(rs.randint(300, 501))) for _ in range(24)]


def _voc_like_batch(n=32, seed=11, nc=21):
    from excel_amd.tools import synthetic
    rs = np.random.RandomState(seed)
    maps = []
    for i in range(n):
        h, w = synthetic.draw_voc_like_size(rs)
        m = _blob_map(rs, h, w) if i % 2 else rs.randint(0, nc, (h // 16 + 1, w // 16 + 1)).astype(np.uint8).repeat(16, 0).repeat(16, 1)[:h, :w]
        m = m.copy()
        m[rs.rand(h, w) < 0.002] = 255
        maps.append(np.ascontiguousarray(m))
    return maps


# ------------------------------------------------------------------ round trips
def test_small_and_boundary_shapes_round_trip(gpu):
    rs = np.random.RandomState(1)
    shapes = [(1, 1), (1, 37), (29, 1)] + [(3, w) for w in (2, 3, 4)] + [(2, w) for w in range(257, 263)] + [(2, w) for w in range(515, 521)]
    maps = []
    for h, w in shapes:
        maps.append(np.full((h, w), 5, np.uint8))                                    # one run per row: maximal matches + leftovers 0, 1, 2
        maps.append(rs.randint(0, 3, (h, w)).astype(np.uint8))                       # short runs
    files, _, _ = _encode(maps)
    for f, m in zip(files, maps):
        _check_file(f, m, _palette())


def test_staircase_hits_every_length_code(gpu):
    m = _staircase()
    files, _, _ = _encode([m, np.ascontiguousarray(m.T)])
    _check_file(files[0], m, _palette())
    _check_file(files[1], np.ascontiguousarray(m.T), _palette())


@pytest.mark.parametrize("value", [0, 143, 144, 255])
def test_one_value_only(gpu, value):
    maps = [np.full((40, 300), value, np.uint8), np.full((5, 1000), value, np.uint8)]
    files, _, _ = _encode(maps)
    for f, m in zip(files, maps):
        _check_file(f, m, _palette())


def test_checkerboard_never_reaches_a_match(gpu):
    y, x = np.mgrid[:67, :131]
    for m in (((y + x) & 1).astype(np.uint8) * 200, ((y + x // 2) & 1).astype(np.uint8) + 143):
        files, _, _ = _encode([m])
        _check_file(files[0], m, _palette())


def test_random_bytes_stay_inside_the_bound(gpu):
    from excel_amd import ops
    m = np.random.RandomState(4).randint(0, 256, (375, 500)).astype(np.uint8)
    files, tab, _ = _encode([m])
    _check_file(files[0], m, _palette())
    bound = ops.png_labels_bound_bytes(375, 500)
    assert bound == (9 * 501 * 375 + 7) // 8 + 880 + (-((9 * 501 * 375 + 7) // 8 + 880)) % 16
    assert len(files[0]) <= bound and len(files[0]) > 375 * 500            # 8- and 9-bit literals, almost no runs


def test_coco_sized_map_and_a_custom_palette(gpu):
    rs = np.random.RandomState(6)
    m = rs.randint(0, 81, (40, 40)).astype(np.uint8).repeat(16, 0).repeat(16, 1)
    m[rs.rand(640, 640) < 0.01] = 255
    pal = rs.randint(0, 256, (256, 3)).astype(np.uint8)
    files, _, _ = _encode([m], palette=pal)
    _check_file(files[0], m, pal)


def test_uniform_tensor_goes_through_the_same_entry(gpu):
    from excel_amd import ops
    rs = np.random.RandomState(8)
    lab = rs.randint(0, 4, (3, 50, 70)).astype(np.uint8).repeat(2, 1)
    data, table = ops.png_encode_labels_ragged(torch.from_numpy(lab).cuda(), None)
    host, tab = data.cpu().numpy(), table.cpu().numpy()
    files, _, _ = _encode([lab[b] for b in range(3)])
    for b in range(3):
        f = host[int(tab[b, 0]):int(tab[b, 0]) + int(tab[b, 1])].tobytes()
        assert f == files[b]
        _check_file(f, lab[b], _palette())


# ------------------------------------------------------------------ invariance
def test_ragged_batch_of_32_and_batch_invariance(gpu):
    maps = _voc_like_batch()
    files, _, _ = _encode(maps)
    for f, m in zip(files, maps):
        _check_file(f, m, _palette())
    again, _, _ = _encode(maps)
    assert again == files, "two runs differ"
    for b in (0, 7, 31):
        alone, _, _ = _encode([maps[b]])
        assert alone[0] == files[b], f"image {b} alone differs from image {b} in the batch"


def test_busy_side_stream_gives_the_same_bytes(gpu):
    from excel_amd import ops
    maps = _voc_like_batch(8, seed=5)
    hw = [m.shape for m in maps]
    plan = ops.RaggedPlan(hw, "cuda")
    flat = torch.from_numpy(np.concatenate([m.reshape(-1) for m in maps])).cuda()
    ref, ref_tab = ops.png_encode_labels_ragged(flat, plan)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    a = torch.randn(2048, 2048, device="cuda")
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(20):                       # keep the side stream busy ahead of the encoder
            a = a @ a * 1e-3
        out, tab = ops.png_encode_labels_ragged(flat, plan)
    b = torch.randn(2048, 2048, device="cuda")
    b = b @ b                                     # ... and the default stream busy beside it
    torch.cuda.current_stream().wait_stream(side)
    assert torch.equal(out, ref) and torch.equal(tab, ref_tab)


# ------------------------------------------------------------------ size
def test_blob_maps_are_at_most_an_eighth_of_raw(gpu):
    """A stored-block or literals-only encoder cannot pass: 24 blob maps, total file bytes <= raw bytes / 8.
    Measured (MI355X): raw / 12.5, 2.01x Pillow's bytes - the ratio to Pillow's own encoder is printed, not asserted."""
    from PIL import Image
    maps = _blob_maps()
    files, _, _ = _encode(maps)
    for f, m in zip(files[:4], maps[:4]):
        _check_file(f, m, _palette())
    raw = sum(m.size for m in maps)
    total = sum(len(f) for f in files)
    pil = 0
    for m in maps:
        im = Image.fromarray(m)
        im.putpalette(_palette().reshape(-1).tolist())
        buf = io.BytesIO()
        im.save(buf, format="PNG")
        pil += buf.tell()
    print(f"\n[label_png] 24 blob maps: raw {raw} B, device files {total} B (raw / {raw / total:.1f}), Pillow {pil} B (device / Pillow = {total / pil:.2f})")
    assert total <= raw / 8, (total, raw)


# ------------------------------------------------------------------ bad arguments
def test_bad_arguments_are_refused_before_any_launch(gpu):
    import ctypes as C
    from excel_amd import ops
    from excel_amd._lib import lib
    m = np.zeros((20, 30), np.uint8)
    plan = ops.RaggedPlan([m.shape], "cuda")
    flat = torch.from_numpy(m.reshape(-1)).cuda()
    with pytest.raises(RuntimeError, match="arena of"):
        ops.png_encode_labels_ragged(flat, plan, out=torch.empty(ops.png_labels_bound_bytes(20, 30) - 16, dtype=torch.uint8, device="cuda"))
    with pytest.raises(RuntimeError, match="workspace of"):
        ops.png_encode_labels_ragged(flat, plan, ws=torch.empty(8, dtype=torch.uint8, device="cuda"))
    hw = np.array([[20, 30]], np.int32)
    rc = lib().excel_png_encode_labels_ragged(None, None, C.byref(plan.info), hw.ctypes.data_as(C.POINTER(C.c_int32)), None, None, 0, None, None, 0, None)
    assert rc < 0 and b"null argument" in lib().excel_last_error()
    with pytest.raises(ValueError, match="uint8 values"):
        ops.png_encode_labels_ragged(flat[:-1], plan)
    assert lib().excel_png_labels_bound_bytes(0, 5) == 0


# ------------------------------------------------------------------ the writer
def test_writer_writes_every_file_and_surfaces_errors(gpu, tmp_path):
    from excel_amd import ops
    from excel_amd.utils import imutils
    maps = _voc_like_batch(6, seed=9)
    files, _, _ = _encode(maps)
    plan = ops.RaggedPlan([m.shape for m in maps], "cuda")
    flat = torch.from_numpy(np.concatenate([m.reshape(-1) for m in maps])).cuda()
    wr = imutils.LabelPngWriter(threads=2, slots=2)
    arena = torch.empty(ops.png_labels_arena_bytes(plan.hw), dtype=torch.uint8, device="cuda")
    for rnd in range(5):                                         # more rounds than slots, ONE device arena: the ring must hold the bytes
        data, table = ops.png_encode_labels_ragged(flat, plan, out=arena)
        wr.submit(data, table, [tmp_path / f"r{rnd}_{b}.png" for b in range(6)])
    assert wr.close() == 30
    for rnd in range(5):
        for b in range(6):
            assert (tmp_path / f"r{rnd}_{b}.png").read_bytes() == files[b]
    bad = imutils.LabelPngWriter(threads=1)
    data, table = ops.png_encode_labels_ragged(flat, plan)
    bad.submit(data, table, [tmp_path / "no_such_dir" / f"{b}.png" for b in range(6)])
    with pytest.raises(FileNotFoundError):
        bad.close()


# ------------------------------------------------------------------ infer_lam + eval_labels end to end
def _eval(pred_dir, root, lists, split="val"):
    from excel_amd.tools import eval_labels
    return eval_labels.validate(eval_labels.get_parser().parse_args(["--pred_dir", str(pred_dir), "--data_folder", str(root), "--list_folder", str(lists),
                                                                     "--infer_set", split, "--num_workers", "2"]))


def _check_dir(label_dir, ids, root, lists, total):
    from PIL import Image
    assert sorted(os.listdir(label_dir)) == sorted(n + ".png" for n in ids)
    out = _eval(label_dir, root, lists)
    assert np.array_equal(out["hist"].numpy(), total.cpu().numpy()), "the files do not hold the labels the run scored"
    for n in ids[:3]:
        f = open(os.path.join(label_dir, n + ".png"), "rb").read()
        _check_file(f, np.asarray(Image.open(io.BytesIO(f))), _palette())
        assert Image.open(io.BytesIO(f)).size == Image.open(os.path.join(root, "SegmentationClassAug", n + ".png")).size


def test_infer_lam_save_label_on_disk_voc(gpu, tmp_path, monkeypatch):
    """Ragged batches, --api_path true and the optimised regime: exactly one file per listed name, eval_labels over the directory gives
    the run's own confusion matrix; the default flags create no directory and score the same."""
    from _clip_files import write_tiny_clip
    from excel_amd.model.init_head import init_decoder_state_dict
    from excel_amd.tools import infer_lam, synthetic
    root, lists = tmp_path / "VOC2012", tmp_path / "lists"
    ids, _ = synthetic.write_voc_tree(str(root), str(lists), 9, seed=4, split="val")
    ckpt, bpe_path, _ = write_tiny_clip(tmp_path)
    common = ["--data_folder", str(root), "--list_folder", str(lists), "--infer_set", "val", "--resize_size", "128", "--model", ckpt,
              "--bpe_path", bpe_path, "--batch_size", "4", "--num_workers", "2"]
    parse = infer_lam.get_parser().parse_args
    monkeypatch.chdir(tmp_path)
    _, plain = infer_lam.validate(parse(common))
    assert not os.path.exists(tmp_path / infer_lam.DEFAULT_CAM_ROOT), "off means off: no directory"
    d1 = tmp_path / "labels"
    _, t1 = infer_lam.validate(parse(common + ["--save_label", "true", "--label_dir", str(d1)]))
    assert torch.equal(plain.cpu(), t1.cpu())
    _check_dir(d1, ids, root, lists, t1)
    # the default directory, next to the CAM directories
    _, t1b = infer_lam.validate(parse(common + ["--save_label", "true"]))
    _check_dir(tmp_path / infer_lam.label_output_dir(None, "val"), ids, root, lists, t1b)
    # the per-image path writes the same labels it scores
    d2 = tmp_path / "labels_api"
    _, t2 = infer_lam.validate(parse(common + ["--save_label", "true", "--label_dir", str(d2), "--api_path", "true"]))
    _check_dir(d2, ids, root, lists, t2)
    # the optimised regime with a tiny head
    head = str(tmp_path / "head.pth")
    torch.save({"module." + k: v for k, v in init_decoder_state_dict(num_classes=21, in_channels=128, embedding_dim=32, index=8, layers=2, seed=3).items()}, head)
    d3 = tmp_path / "labels_opt"
    opt = common + ["--training_free", "false", "--model_path", head, "--in_channels", "128", "--embedding_dim", "32"]
    _, t3 = infer_lam.validate(parse(opt + ["--save_label", "true", "--label_dir", str(d3)]))
    _, t3_plain = infer_lam.validate(parse(opt))
    assert torch.equal(t3.cpu(), t3_plain.cpu())
    _check_dir(d3, ids, root, lists, t3)


def test_infer_lam_save_label_uniform_batches(gpu, tmp_path):
    """The uniform batched path (--synthetic without --ragged): the ground truth of the synthetic samples is written out so eval_labels
    can score the exported directory."""
    from PIL import Image
    from _clip_files import write_tiny_clip
    from excel_amd.tools import infer_lam, synthetic
    ckpt, bpe_path, _ = write_tiny_clip(tmp_path)
    common = ["--synthetic", "6", "--resize_size", "128", "--model", ckpt, "--bpe_path", bpe_path, "--batch_size", "4"]
    parse = infer_lam.get_parser().parse_args
    d = tmp_path / "labels"
    _, plain = infer_lam.validate(parse(common))
    _, t = infer_lam.validate(parse(common + ["--save_label", "true", "--label_dir", str(d)]))
    assert torch.equal(plain.cpu(), t.cpu())
    ds = synthetic.SyntheticSegDataset(6, (128, 128), num_classes=21, seed=1234)
    root, lists = tmp_path / "gt", tmp_path / "lists"
    os.makedirs(root / "SegmentationClassAug")
    os.makedirs(lists)
    ids = []
    for i in range(6):
        name, _, gt, _ = ds[i]
        Image.fromarray(gt).save(root / "SegmentationClassAug" / (name + ".png"))
        ids.append(name)
    (lists / "val.txt").write_text("\n".join(ids) + "\n")
    _check_dir(d, ids, root, lists, t)
