"""Host side of the flip / multi-scale LAM fuse (infer_lam --cam_scales / --cam_flip): the network sizes of a scale list, what is
refused, the parser defaults, and the float64 reference of the GPU tests pinned to oracle.interp."""
import os
import sys

import numpy as np
import pytest

import oracle

torch = pytest.importorskip("torch")
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _lam_tta_ref as R  # noqa: E402

DEFAULT4 = (1.0, 0.5, 0.75, 1.5)


def test_tta_sizes_written_out():
    from excel_amd.tools import infer_lam
    assert infer_lam.tta_sizes(448, DEFAULT4) == [(448, 28), (224, 14), (336, 21), (672, 42)]
    assert infer_lam.tta_sizes(320, DEFAULT4) == [(320, 20), (160, 10), (240, 15), (480, 30)]
    assert infer_lam.tta_sizes(512, DEFAULT4) == [(512, 32), (256, 16), (384, 24), (768, 48)]
    assert infer_lam.tta_sizes(448, (1.0,)) == [(448, 28)]
    # 1.0 goes first wherever it was listed; the others keep their order; rounding is int(s * S) // 16 * 16
    assert infer_lam.tta_sizes(448, (1.5, 0.5, 1.0, 0.75)) == [(448, 28), (672, 42), (224, 14), (336, 21)]
    assert infer_lam.tta_sizes(100, (1.0, 0.5)) == [(100, 6), (48, 3)]


@pytest.mark.parametrize("S,scales,names", [
    (448, (0.5, 1.5), "1.0"),                                          # no scale 1.0
    (448, (1.0, 0.5, 0.6, 0.7, 0.8, 0.9, 1.1, 1.2, 1.3), "9 scales"),     # more than 8
    (64, (1.0, 0.2), "0.2"),                                           # int(12.8) // 16 * 16 = 0 < 16
    (512, (1.0, 2.0), "2.0"),                                          # grid 64 > 48
    (64, (1.0, 0.5, 0.6), "0.6"),                                      # 38 -> 32, the size of 0.5
    (448, (1.0, 0.5, 1.0), "1.0"),                                     # 1.0 twice
])
def test_tta_sizes_rejections(S, scales, names):
    from excel_amd.tools import infer_lam
    with pytest.raises(ValueError) as e:
        infer_lam.tta_sizes(S, scales)
    assert names in str(e.value), str(e.value)


def test_parser_defaults_and_resolve():
    from excel_amd.tools import infer_lam
    from excel_amd.tools.infer_seg_voc import parse_scales
    p = infer_lam.get_parser()
    a = p.parse_args([])
    assert a.cam_scales == "1.0" and a.cam_flip is False
    assert infer_lam.resolve_tta(a) == (None, False)                       # the plain step
    a = p.parse_args(["--cam_scales", "1.0,0.5,0.75,1.5", "--cam_flip", "true"])
    assert parse_scales(a.cam_scales) == DEFAULT4 and a.cam_flip is True
    assert infer_lam.resolve_tta(a) == (DEFAULT4, True)
    assert infer_lam.resolve_tta(p.parse_args(["--cam_flip", "true"])) == ((1.0,), True)
    assert infer_lam.resolve_tta(p.parse_args(["--cam_scales", "0.5,1.0"])) == ((0.5, 1.0), False)
    with pytest.raises(ValueError, match="2.0"):                           # checked against --resize_size before a model is built
        infer_lam.resolve_tta(p.parse_args(["--cam_scales", "1.0,2.0", "--resize_size", "512"]))


@pytest.mark.parametrize("flags", [["--cam_flip", "true"], ["--cam_scales", "1.0,0.5"]])
def test_training_free_false_conflict(flags):
    from excel_amd.tools import infer_lam
    p = infer_lam.get_parser()
    a = p.parse_args(["--training_free", "false"] + flags)
    with pytest.raises(ValueError, match="training_free"):
        infer_lam.resolve_tta(a)
    with pytest.raises(ValueError, match="training_free"):
        infer_lam.validate(a)                                              # stops before a device or a model is touched
    assert infer_lam.resolve_tta(p.parse_args(["--training_free", "false"])) == (None, False)


def test_pipeline_options_host_side():
    """The options are validated where the pipeline is built; the regimes out of scope name the option they refuse."""
    from excel_amd import pipeline
    pipe = pipeline.TrainingFreePipeline(None)
    assert pipe.tta is False and pipe.tta_scales == (1.0,) and pipe.tta_flip is False
    assert pipeline.TrainingFreePipeline(None, tta_scales=(1.0,), tta_flip=False).tta is False
    on = pipeline.TrainingFreePipeline(None, tta_scales=DEFAULT4, tta_flip=True)
    assert on.tta and on.tta_scales == DEFAULT4
    with pytest.raises(ValueError, match="1.0"):
        pipeline.TrainingFreePipeline(None, tta_scales=(0.5, 1.5))
    x = torch.zeros(2, 3, 32, 32)
    for call in (lambda: on.run_batch_split(x, None), lambda: on.run_batch_overlapped(x, None)):
        with pytest.raises(ValueError, match="tta_scales"):
            call()
    for cls in (pipeline.OptimisedLamPipeline, pipeline.ValidationPipeline):
        with pytest.raises(ValueError, match="tta_flip"):
            cls(None, tta_flip=True)
        with pytest.raises(ValueError, match="tta_scales"):
            cls(None, tta_scales=(1.0, 0.5))


def test_reference_pinned_to_oracle_interp():
    """_lam_tta_ref against oracle.interp.bilinear_resize (float32 coefficients, ATen's rule) + plain numpy on one small case."""
    B, F, G, grids = 2, 3, 5, (5, 2, 7)
    rs = np.random.RandomState(3)
    maps = [(4 * rs.rand(2 * B, g * g, F)).astype(np.float32) for g in grids]
    for flip in (True, False):
        ms = maps if flip else [m[:B] for m in maps]
        acc = 0
        for m, g in zip(ms, grids):
            r = oracle.interp.bilinear_resize(m.transpose(0, 2, 1).reshape(-1, F, g, g), G, G, align_corners=False).astype(np.float64)
            acc = acc + (np.maximum(r[:B], r[B:][..., ::-1]) if flip else r)
        lam = acc - acc.min(axis=(2, 3), keepdims=True)
        want = (lam / (lam.max(axis=(2, 3), keepdims=True) + 1e-5)).reshape(B, F, G * G).transpose(0, 2, 1)
        got, rng = R.lam_tta_ref(ms, grids, G, flip)
        assert got.shape == (B, G * G, F) and got.dtype == np.float64
        assert rng >= 1.0
        assert float(np.abs(got - want).max()) < 2e-6                      # float32 coefficients against float64 ones
        assert got.min() == 0.0 and 0.999 < got.max() < 1.0
    # the mirrored half alone: one hot value at column 0 of the flipped plane lands at column G - 1
    one = np.zeros((2, G * G, 1), np.float32)
    one[1, 2 * G + 0, 0] = 1.0
    out, _ = R.lam_tta_ref([one], (G,), G, True)
    assert out[0, 2 * G + G - 1, 0] > 0.99 and np.count_nonzero(out) == 1
    assert [c[2] for c in R.CASES] == [4, 3, 28, 32, 5] and len(R.CASES[4][3]) == 8
