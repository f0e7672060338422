"""--save_cam --cam_device_jpeg, host side (no GPU): the numpy restatement of the device encoder (tests/_jpeg_ref.py) against Pillow, the
assumption about Pillow's file layout, the C ABI's declarations and bindings, the flag, and CamJpegWriter's host fallback."""
import os
import re

import numpy as np
import pytest

import _jpeg_cases as cases
import _jpeg_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
JPEG_SYMBOLS = ("excel_jpeg_rgb_arena_bytes", "excel_jpeg_rgb_workspace_bytes", "excel_jpeg_encode_rgb_ragged")


@pytest.mark.parametrize("content", cases.CONTENTS)
@pytest.mark.parametrize("shape", cases.SHAPES, ids=lambda s: "%dx%d" % s)
def test_restatement_writes_pillows_bytes(shape, content):
    a = cases.image(shape, content)
    for q in cases.QUALITIES:
        assert cases.ref_bytes(shape, content, q) == cases.pillow_bytes(a, q), (shape, content, q)


def test_pillow_writes_the_markers_the_encoder_assumes():
    d = cases.pillow_bytes(cases.image((16, 16), "random"), 75)
    assert d[:2] == b"\xff\xd8" and d[-2:] == b"\xff\xd9"
    at, seen = 2, []
    while True:
        assert d[at] == 0xFF
        seen.append(d[at + 1])
        if d[at + 1] == 0xDA:
            break
        at += 2 + d[at + 2] * 256 + d[at + 3]
    assert seen == [0xE0, 0xDB, 0xDB, 0xC0, 0xC4, 0xC4, 0xC4, 0xC4, 0xDA]
    assert at + 2 + 12 == _jpeg_ref.HEADER_BYTES


def test_quality_scaling_and_huffman_tables():
    assert _jpeg_ref.quant_tables(50).tolist() == _jpeg_ref.QUANT_BASE.tolist()
    assert _jpeg_ref.quant_tables(75)[0][:4].tolist() == [8, 6, 5, 8] and _jpeg_ref.quant_tables(100).max() == 1
    assert _jpeg_ref.quant_tables(1).max() == 255
    for bits, vals in zip(_jpeg_ref.AC_BITS, _jpeg_ref.AC_VALS):
        assert sum(bits) == len(vals) == len(set(vals)) == 162
    ac = _jpeg_ref.huffman_codes(_jpeg_ref.AC_BITS[0], _jpeg_ref.AC_VALS[0])
    assert ac[0x00] == (0b1010, 4) and ac[0xF0] == (0b11111111001, 11) and max(n for _, n in ac.values()) == 16


def test_header_declares_the_entries_and_they_are_bound():
    from excel_amd import _lib
    header = open(os.path.join(ROOT, "include", "excel_hip.h")).read()
    for name in JPEG_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert name in _lib.SIGNATURES, name
    assert "tools/infer_lam.py:104,111" in header
    res, args = _lib.SIGNATURES["excel_jpeg_encode_rgb_ragged"]
    assert res is _lib.c_i and len(args) == 11
    assert _lib.SIGNATURES["excel_jpeg_rgb_arena_bytes"][0] is _lib.c_sz and _lib.SIGNATURES["excel_jpeg_rgb_workspace_bytes"][0] is _lib.c_sz
    from excel_amd import build
    assert "jpeg.hip" in build.SOURCES and build.NO_SCRATCH_EXPECTED["jpeg"] in build.NO_SCRATCH


def test_parser_knows_the_flag_and_it_defaults_to_off():
    from excel_amd.tools import infer_lam
    assert infer_lam.get_parser().parse_args([]).cam_device_jpeg is False
    assert infer_lam.get_parser().parse_args(["--save_cam", "true", "--cam_device_jpeg", "true"]).cam_device_jpeg is True


def test_writer_falls_back_to_the_host_encoder_for_a_file_that_did_not_fit(tmp_path):
    """A hand-made batch as it lies in a pinned slot once its copy has landed: file 0 encoded, file 1 flagged -1.  CPU tensors stand in
    for the slot and for the device buffer of raw overlays."""
    import torch
    from excel_amd.utils import imutils
    a, b = cases.image((17, 33), "random"), cases.image((37, 53), "ramp")
    rgb = torch.from_numpy(np.concatenate([np.zeros(5, np.uint8), a.reshape(-1), b.reshape(-1)]))
    items = [(5, 17, 33), (5 + a.size, 37, 53)]
    f0 = cases.ref_bytes((17, 33), "random", 75)
    slot = dict(bytes=torch.from_numpy(np.frombuffer(f0 + b"\xa5" * 9, np.uint8).copy()),
                table=torch.tensor([[0, len(f0)], [len(f0), -1]], dtype=torch.int64), futures=[])
    paths = [str(tmp_path / "a.jpg"), str(tmp_path / "b.jpg")]
    w = imutils.CamJpegWriter(threads=2)
    w._slots[0] = slot
    w._hand_over(slot, paths, items, rgb)
    assert w.close() == 2 and w.fallbacks == 1 and w.ratio is None
    assert open(paths[0], "rb").read() == f0
    imutils.save_jpeg(str(tmp_path / "want.jpg"), b)
    assert open(paths[1], "rb").read() == open(tmp_path / "want.jpg", "rb").read() == cases.ref_bytes((37, 53), "ramp", 75)


def test_writer_reports_a_failed_write(tmp_path):
    import torch
    from excel_amd.utils import imutils
    f0 = cases.ref_bytes((8, 8), "grey", 75)
    slot = dict(bytes=torch.from_numpy(np.frombuffer(f0, np.uint8).copy()), table=torch.tensor([[0, len(f0)]], dtype=torch.int64), futures=[])
    w = imutils.CamJpegWriter(threads=1)
    w._slots[0] = slot
    w._hand_over(slot, [str(tmp_path / "missing" / "a.jpg")], [(0, 8, 8)], torch.zeros(192, dtype=torch.uint8))
    with pytest.raises(FileNotFoundError):
        w.close()
    assert w.ratio == len(f0) / 192
