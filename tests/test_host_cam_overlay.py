"""--save_cam (tools/infer_lam.py:97-111) on the host: flags, output paths, the jet table, the round-trip table and the colormap rules
of the numpy restatement the GPU tests hold the kernel to."""
import os

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from _cam_overlay_ref import jet_rgb, overlays  # noqa: E402
from excel_amd.tools import infer_lam  # noqa: E402
from excel_amd.utils import imutils  # noqa: E402


def test_parser_defaults_match_the_reference():
    a = infer_lam.get_parser().parse_args([])
    assert a.save_cam is False and a.save_cls_specific_cam is True and a.refine_with_aff is True
    b = infer_lam.get_parser().parse_args(["--save_cam", "true", "--save_cls_specific_cam", "false", "--refine_with_aff", "false"])
    assert b.save_cam is True and b.save_cls_specific_cam is False and b.refine_with_aff is False


@pytest.mark.parametrize("training_free", [True, False])
@pytest.mark.parametrize("refine_with_aff", [True, False])
def test_output_dirs_follow_the_reference(training_free, refine_with_aff):
    model_path, infer_set = "./00_sota/voc/checkpoints/model_iter_30000.pth", "train"
    # :242-267, restated
    base_dir = model_path.split("checkpoints/")[0] + f"/{infer_set}/"
    cpt_name = model_path.split("checkpoints/")[-1].replace(".pth", "")
    if training_free:
        tag = "lam_training_free/aff_lam" if refine_with_aff else "lam_training_free/seeds_lam"
    else:
        tag = "lam_optimized/aff_lam" if refine_with_aff else "lam_optimized/seeds_lam"
    cs_cam_dir = os.path.join(base_dir, f"{infer_set}_{cpt_name}_{tag}_class_specific_img")
    cam_dir = os.path.join(base_dir, f"{infer_set}_{cpt_name}_{tag}_img")
    d = infer_lam.cam_output_dirs(model_path, infer_set, training_free, refine_with_aff)
    assert d["tag"] == tag
    assert d["cam_dir"] == os.path.normpath(cam_dir) and d["cs_cam_dir"] == os.path.normpath(cs_cam_dir)
    # no "checkpoints/": the checkpoint's own directory; no model path: the documented default under the working directory
    d2 = infer_lam.cam_output_dirs("/w/run/model.pth", "val")
    assert d2["cam_dir"] == "/w/run/val/val_model_lam_training_free/aff_lam_img"
    d3 = infer_lam.cam_output_dirs(None, "val")
    assert d3["cs_cam_dir"] == os.path.join("lam_cams", "val", "val_none_lam_training_free/aff_lam_class_specific_img")


def test_jet_lut_anchors_and_sum():
    lut = imutils.jet_lut()
    assert lut.shape == (256, 3) and lut.dtype == np.float64
    anchors = {0: (0, 0, 0.5), 64: (0, 0.503921568627, 1), 89: (0, 0.896078431373, 0.970904490829), 128: (0.490196078431, 1, 0.477545857052),
               192: (1, 0.581699346405, 0), 255: (0.5, 0, 0)}
    for i, rgb in anchors.items():
        np.testing.assert_allclose(lut[i], rgb, rtol=0, atol=5e-12)
    assert lut.sum() == 372.79707128208076


def test_jet_lut_equals_matplotlib_when_present():
    mpl = pytest.importorskip("matplotlib")
    cm = mpl.colormaps["jet"]
    cm._init()
    assert np.array_equal(imutils.jet_lut(), cm._lut[:256, :3])


def _reference_roundtrip(decoded, mean=(123.675, 116.28, 103.53), std=(58.395, 57.12, 57.375)):
    """datasets/transforms.py:7-14 then utils/imutils.py:11-18 on a decoded [H,W,3] image."""
    imgarr = np.asarray(decoded)
    proc_img = np.empty_like(imgarr, np.float32)
    for c in range(3):
        proc_img[..., c] = (imgarr[..., c] - mean[c]) / std[c]
    imgs = torch.from_numpy(proc_img).permute(2, 0, 1).unsqueeze(0)
    _imgs = torch.zeros_like(imgs)
    for c in range(3):
        _imgs[:, c, :, :] = imgs[:, c, :, :] * std[c] + mean[c]
    return _imgs.type(torch.uint8)[0].permute(1, 2, 0).numpy()


def test_roundtrip_table_equals_the_reference_lines():
    v = np.arange(256, dtype=np.uint8)
    decoded = np.stack([v, v, v], -1)[None]
    ref = _reference_roundtrip(decoded)[0].T                      # [3,256]
    rt = imutils.denormalize_roundtrip_table()
    assert rt.dtype == np.uint8 and rt.shape == (3, 256) and np.array_equal(rt, ref)
    assert [int((rt[c] != v).sum()) for c in range(3)] == [1, 5, 14]
    assert rt[0, 1] == 0
    tabs = imutils.cam_overlay_tables(0.6)
    assert tabs.shape == (2, 768) and tabs.dtype == np.float64
    assert np.array_equal(tabs[0], (0.6 * (imutils.jet_lut() * 255)).reshape(-1))
    assert np.array_equal(tabs[1], ((1 - 0.6) * rt.astype(np.float64)).reshape(-1))


def test_colormap_edge_cases_of_the_restatement():
    lut = imutils.jet_lut()
    below1 = np.nextafter(np.float32(1), np.float32(0))
    x = np.array([0, 1, below1, -1e-7, -3, 1 + 1e-6, 1e30, np.inf, -np.inf, np.nan, 0.5, 1 / 256, 255 / 256], np.float32)
    got = jet_rgb(x, lut)
    want_idx = [0, 255, 255, 0, 0, 255, 255, 255, 0, None, 128, 1, 255]
    for g, i in zip(got, want_idx):
        assert np.array_equal(g, np.zeros(3) if i is None else lut[i])
    mpl = None
    try:
        import matplotlib as mpl
    except ImportError:
        pass
    if mpl is not None:
        assert np.array_equal(got, mpl.colormaps["jet"](x)[:, :3])
    # the blend and its truncation, both modes, on a 1 x 13 image
    rs = np.random.RandomState(0)
    decoded = rs.randint(0, 256, (1, x.size, 3)).astype(np.uint8)
    rt = imutils.denormalize_roundtrip_table()
    cams = np.stack([np.zeros_like(x), x, x[::-1].copy()])[:, None, :]
    img = _reference_roundtrip(decoded).astype(np.float64)
    (mx,) = overlays(decoded, cams, "max", lut, rt)
    cam = np.max(cams[1:], 0)[0]
    assert np.array_equal(mx[0], (0.5 * (jet_rgb(cam, lut) * 255) + 0.5 * img[0]).astype(np.uint8))
    assert np.isnan(cam).sum() == 2 and np.array_equal(mx[0][np.isnan(cam)], (0.5 * img[0][np.isnan(cam)]).astype(np.uint8))
    pcs = overlays(decoded, cams, "per_class", lut, rt)
    assert len(pcs) == 2 and np.array_equal(pcs[0][0], (0.6 * (jet_rgb(x, lut) * 255) + (1 - 0.6) * img[0]).astype(np.uint8))
    assert overlays(decoded, cams[:1], "max", lut, rt) == [] and overlays(decoded, cams[:1], "per_class", lut, rt) == []


def test_save_cam_refuses_the_uniform_batched_path():
    args = infer_lam.get_parser().parse_args(["--save_cam", "true"])
    args.ragged_batches = False
    with pytest.raises(ValueError, match="--save_cam needs"):
        infer_lam.build_validation(None, None, None, np.arange(2), "cpu", args, pipe=object())


def test_writer_pool_is_sized_from_the_cpu_budget(monkeypatch):
    monkeypatch.setattr(infer_lam, "host_cpu_budget", lambda: 16)
    assert infer_lam.default_cam_writers(1) == 4 and infer_lam.default_cam_writers(8) == 1
