"""The device JPEG encoder of --save_cam --cam_device_jpeg (jpeg.hip): bit identity with the numpy restatement (tests/_jpeg_ref.py, which
test_host_cam_jpeg.py holds against Pillow), ragged batches, a busy neighbour stream, the overflow flag, the refused arguments, and
infer_lam writing the same files with the flag on and off."""
import ctypes as C
import io
import os

import numpy as np
import pytest
import torch

import _jpeg_cases as cases

pytestmark = pytest.mark.gpu
SENTINEL = 0xA5


@pytest.fixture(scope="module")
def gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import excel_amd.ops  # noqa: F401
    return True


def _encode(images, quality=75, lead=0, arena=None):
    """images at odd offsets behind `lead` bytes -> (arena bytes as numpy, table as numpy, items)"""
    from excel_amd import ops
    flat, items, at = [np.full(lead, 7, np.uint8)], [], lead
    for a in images:
        items.append((at, a.shape[0], a.shape[1]))
        flat.append(a.reshape(-1))
        at += a.size
    hw = [(h, w) for _, h, w in items]
    # room for any file: every 8 x 8 block at its worst case of 208 bytes, each of them stuffed (the raw-size bound of
    # ops.jpeg_rgb_arena_bytes is for photographs: the file of a 1 x 1 image has 631 bytes, its bound 628)
    n = sum(625 + 2 * 208 * 6 * (-(-h // 16)) * (-(-w // 16)) for h, w in hw) if arena is None else arena
    out = torch.full((n + 64,), SENTINEL, dtype=torch.uint8, device="cuda")
    data, table = ops.jpeg_encode_rgb_ragged(torch.from_numpy(np.concatenate(flat)).cuda(), items, quality, out=out[:n])
    return out.cpu().numpy(), table.cpu().numpy(), items


def _files(buf, table):
    return [bytes(buf[o:o + s]) if s >= 0 else None for o, s in table.tolist()]


@pytest.mark.parametrize("shape", cases.SHAPES, ids=lambda s: "%dx%d" % s)
def test_one_image_equals_the_restatement(gpu, shape):
    from PIL import Image
    for content in cases.CONTENTS:
        a = cases.image(shape, content)
        for q in cases.QUALITIES:
            buf, table, _ = _encode([a], q, lead=3)
            want = cases.ref_bytes(shape, content, q)
            assert table.tolist() == [[0, len(want)]], (content, q)
            assert bytes(buf[:len(want)]) == want, (content, q)
            assert (buf[len(want):] == SENTINEL).all(), (content, q)
            im = Image.open(io.BytesIO(want))
            im.load()
            assert im.size == (shape[1], shape[0])


MIXED = [((37, 53), "random"), ((1, 1), "white"), ((17, 33), "checker"), ((64, 15), "ramp"), ((8, 8), "pixel"), ((48, 80), "random"), ((15, 64), "grey")]


@pytest.mark.parametrize("quality", cases.QUALITIES)
def test_ragged_batch_of_mixed_sizes(gpu, quality):
    """the per-class layout of cam_overlay_ragged: tight images one behind the other, so most start at an odd byte"""
    buf, table, items = _encode([cases.image(s, c) for s, c in MIXED], quality, lead=1)
    assert any(off & 1 for off, _, _ in items) and any(not off & 1 for off, _, _ in items)
    want = [cases.ref_bytes(s, c, quality) for s, c in MIXED]
    assert _files(buf, table) == want
    assert table[:, 0].tolist() == np.concatenate([[0], np.cumsum([len(f) for f in want])])[:-1].tolist()      # back to back
    assert (buf[sum(len(f) for f in want):] == SENTINEL).all()                                               # nothing behind the last file


def test_batch_of_32_equals_the_single_images(gpu):
    rs = np.random.RandomState(5)
    imgs = [rs.randint(0, 256, (37, 53, 3)).astype(np.uint8) for _ in range(32)]
    buf, table, _ = _encode(imgs)
    files = _files(buf, table)
    import _jpeg_ref
    for b in (0, 13, 31):
        assert files[b] == _jpeg_ref.encode(imgs[b], 75)
    for b, a in enumerate(imgs):
        one, t1, _ = _encode([a])
        assert files[b] == bytes(one[:t1[0, 1]]), b


def test_busy_side_stream_gives_the_same_bytes(gpu):
    imgs = [cases.image(s, c) for s, c in MIXED]
    ref, rt, _ = _encode(imgs, lead=1)
    side = torch.cuda.Stream()
    a = torch.randn(2048, 2048, device="cuda")
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(20):                       # keep the side stream busy ahead of the encoder
            a = a @ a * 1e-3
        out, ot, _ = _encode(imgs, lead=1)
    torch.cuda.current_stream().wait_stream(side)
    assert np.array_equal(rt, ot) and np.array_equal(ref, out)


def test_a_file_above_the_raw_size_bound_is_flagged(gpu):
    """the bound of the arena is the raw size plus the header: the one file of a 1 x 1 image is 3 bytes longer"""
    from excel_amd import ops
    a = cases.image((1, 1), "zero")
    want = cases.ref_bytes((1, 1), "zero", 75)
    bound = ops.jpeg_rgb_arena_bytes([(1, 1)])
    assert bound == 628 and len(want) == 631
    buf, table, _ = _encode([a], arena=bound)
    assert table.tolist() == [[0, -1]] and (buf == SENTINEL).all()


def test_a_file_that_does_not_fit_is_flagged_and_not_written(gpu):
    want = [cases.ref_bytes(s, c, 75) for s, c in MIXED]
    total = sum(len(f) for f in want)
    buf, table, _ = _encode([cases.image(s, c) for s, c in MIXED], arena=total - 1)
    assert table[:-1, 1].tolist() == [len(f) for f in want[:-1]] and table[-1, 1] == -1
    assert _files(buf, table)[:-1] == want[:-1]
    assert (buf[total - len(want[-1]):] == SENTINEL).all()          # its part of the arena and everything behind it are untouched
    buf, table, _ = _encode([cases.image(s, c) for s, c in MIXED], arena=total)
    assert _files(buf, table) == want


def test_refused_arguments(gpu):
    from excel_amd import ops
    from excel_amd._lib import lib
    rgb = torch.zeros(3 * 16 * 16, dtype=torch.uint8, device="cuda")
    arena = torch.zeros(4096, dtype=torch.uint8, device="cuda")
    table = torch.zeros((2, 2), dtype=torch.int64, device="cuda")
    ws = torch.zeros(1 << 20, dtype=torch.uint8, device="cuda")

    def call(hw, n=1, quality=75, ws_bytes=ws.numel()):
        hw = np.ascontiguousarray(hw, np.int32)
        off = np.zeros(max(n, 1), np.int64)
        return lib().excel_jpeg_encode_rgb_ragged(rgb.data_ptr(), off.ctypes.data_as(C.POINTER(C.c_int64)), hw.ctypes.data_as(C.POINTER(C.c_int32)),
                                                  n, quality, arena.data_ptr(), arena.numel(), table.data_ptr(), ws.data_ptr(), ws_bytes, None)
    assert call([[16, 16]]) == 0
    for kw in (dict(hw=[[16, 16]], n=0), dict(hw=[[16, 16]], n=-3), dict(hw=[[0, 16]]), dict(hw=[[16, 0]]), dict(hw=[[65536, 1]]),
               dict(hw=[[1, 65536]]), dict(hw=[[30000, 30000]]), dict(hw=[[16, 16]], quality=0), dict(hw=[[16, 16]], quality=101),
               dict(hw=[[16, 16]], ws_bytes=ops.jpeg_rgb_workspace_bytes([(16, 16)]) - 1)):
        assert call(**kw) == -1, kw
        assert b"jpeg_encode_rgb_ragged" in lib().excel_last_error()
    assert ops.jpeg_rgb_arena_bytes([(16, 16), (3, 5)]) == 2 * 625 + 3 * (256 + 15)
    assert ops.jpeg_rgb_arena_bytes([(0, 5)]) == 0 and ops.jpeg_rgb_workspace_bytes([(70000, 5)]) == 0
    with pytest.raises(ValueError):
        ops.jpeg_encode_rgb_ragged(rgb, [(1, 16, 16)])              # reaches behind the buffer
    torch.cuda.synchronize()


def _dir(d):
    return {f: open(os.path.join(d, f), "rb").read() for f in sorted(os.listdir(d))}


def test_infer_lam_writes_the_same_files_with_the_flag_on_and_off(gpu, tmp_path):
    from _clip_files import write_tiny_clip
    from excel_amd.tools import infer_lam, synthetic
    root, lists = tmp_path / "VOC2012", tmp_path / "lists"
    synthetic.write_voc_tree(str(root), str(lists), 9, seed=4, split="val")
    ckpt, bpe_path, _ = write_tiny_clip(tmp_path)
    common = ["--data_folder", str(root), "--list_folder", str(lists), "--infer_set", "val", "--resize_size", "128", "--model", ckpt,
              "--bpe_path", bpe_path, "--batch_size", "4", "--num_workers", "2", "--save_cam", "true"]
    parse = infer_lam.get_parser().parse_args
    for mode, flag in (("per_class", "--cs_cam_dir"), ("max", "--cam_dir")):
        extra = [] if mode == "per_class" else ["--save_cls_specific_cam", "false"]
        _, t_off = infer_lam.validate(parse(common + extra + [flag, str(tmp_path / (mode + "_off"))]))
        _, t_on = infer_lam.validate(parse(common + extra + [flag, str(tmp_path / (mode + "_on")), "--cam_device_jpeg", "true"]))
        assert torch.equal(t_off.cpu(), t_on.cpu())
        off, on = _dir(tmp_path / (mode + "_off")), _dir(tmp_path / (mode + "_on"))
        assert len(off) >= 1 and sorted(off) == sorted(on)
        assert off == on, mode
