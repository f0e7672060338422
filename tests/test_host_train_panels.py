"""Training-progress panels on the host: excel_train_panels_plan (trainviz.hip, host arithmetic) against the numpy restatement of
torchvision.utils.make_grid's layout (tests/_train_panels_ref.py), its argument errors, the tbutils call surface, the new flags and the
order in which a TensorBoard-like writer receives the reference's tags (scripts/train_voc.py:240-246)."""
import ctypes as C

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import _train_panels_ref as R  # noqa: E402
from excel_amd import _lib, ops  # noqa: E402


@pytest.mark.parametrize("S,g", [(48, 3), (320, 20)])
@pytest.mark.parametrize("B", [1, 2, 3, 4, 5])
def test_plan_matches_make_grid_layout(B, S, g):
    plan, total = ops.train_panels_plan(B, S, g, nrow=2)
    ref, ref_total = R.plan(B, S, g)
    assert list(plan) == list(R.PANELS) and plan == ref and total == ref_total
    # the layout itself: where make_grid puts the images, on a batch of constant images
    for h in (S, g):
        imgs = np.stack([np.full((h, h, 3), k + 1, np.uint8) for k in range(B)])
        grid = R.make_grid(imgs)
        Hg, Wg = plan["pseu_mid" if h == g else "img1"][:2]
        assert grid.shape == (Hg, Wg, 3)
        assert int((grid != 0).sum()) == 3 * B * h * h
    # a subset: tight, in panel order
    sub, sub_total = ops.train_panels_plan(B, S, g, panels=("seg_pred", "cam1"))
    assert list(sub) == ["cam1", "seg_pred"] and (sub, sub_total) == R.plan(B, S, g, panels=("cam1", "seg_pred"))


def test_plan_argument_errors():
    out = (C.c_int64 * 19)()
    lib = _lib.lib()
    good = (4, 2, 320, 20, 63)
    assert lib.excel_train_panels_plan(*good, out) == 0 and out[18] == R.plan(4, 320, 20)[1]
    for bad in [(0, 2, 320, 20, 63), (4, 0, 320, 20, 63), (4, 2, 0, 20, 63), (4, 2, 320, 0, 63), (4, 2, 320, 20, 0), (4, 2, 320, 20, 64),
                (4, 2, 320, 20, -1), (4, 2, 20000, 20, 1), (4, 2, 320, 30000, 8)]:
        assert lib.excel_train_panels_plan(*bad, out) != 0, bad
        assert lib.excel_last_error()
    assert lib.excel_train_panels_plan(*good, None) != 0
    with pytest.raises(ValueError):
        ops.train_panels_plan(4, 320, 20, panels=("img1", "nope"))


def test_launch_argument_errors_need_no_device():
    """the launch entry refuses a panel requested without its input, and P != g*g, before it touches the device"""
    lib = _lib.lib()
    m, s = (C.c_float * 3)(*R.MEAN), (C.c_float * 3)(*R.STD)
    x = C.c_void_p(256)                      # never dereferenced: every call below fails its argument checks

    def call(img=x, attr=x, cls=x, aff=x, mid=x, gt=x, pred=x, B=2, F_=4, P=9, g=3, S=48, mask=63, jet=x, pal=x, out=x, nbytes=1 << 30):
        return lib.excel_train_panels(img, attr, cls, aff, mid, gt, pred, B, F_, P, g, S, 2, mask, m, s, jet, pal, out, nbytes, None)

    for kw in (dict(img=None), dict(attr=None), dict(cls=None), dict(aff=None), dict(mid=None), dict(gt=None), dict(pred=None), dict(out=None),
               dict(jet=None), dict(pal=None), dict(P=8), dict(F_=0), dict(nbytes=16), dict(mask=0), dict(B=0), dict(S=30000),
               dict(img=None, mask=1), dict(img=None, mask=2), dict(gt=None, mask=16)):
        assert call(**kw) != 0, kw
        assert b"launch" not in lib.excel_last_error(), kw            # refused by the argument checks, not by a failed launch


def test_tbutils_surface_and_flags():
    from excel_amd.scripts import train_coco, train_voc
    from excel_amd.utils import tbutils
    assert callable(tbutils.make_grid_image) and callable(tbutils.make_grid_label)
    assert tbutils.TAGS == ("visual/img1", "visual/cam1", "visual/pseu_aff", "visual/pseu_mid", "visual/seg_gt", "visual/seg_pred")
    for mod in (train_voc, train_coco):
        a = mod.get_parser().parse_args([])
        assert a.save_visual is False and a.visual_dir is None and (a.bkg_thre, a.high_thre, a.low_thre) == (0.5, 0.7, 0.25)
        b = mod.get_parser().parse_args(["--save_visual", "true", "--visual_dir", "/tmp/v"])
        assert b.save_visual is True and b.visual_dir == "/tmp/v"
    # the palette the kernel reads is the reference's COLORMAP
    from excel_amd.utils import imutils
    assert np.array_equal(imutils.colormap(), R.colormap()) and tuple(R.colormap()[255]) == (224, 224, 192)


class _Writer:
    def __init__(self):
        self.calls = []

    def add_image(self, tag, img, global_step=None):
        self.calls.append((tag, tuple(img.shape), img.dtype, global_step))


@pytest.mark.parametrize("with_gt", [True, False])
def test_writer_receives_the_reference_tags_in_order(with_gt):
    """log_panels on a CPU stand-in for ops.train_panels' result: VOC six tags, COCO five (no seg_gt), each a CHW uint8 grid"""
    from excel_amd.utils import tbutils
    B, S, g = 3, 48, 3
    names = [n for n in R.PANELS if with_gt or n != "seg_gt"]
    plan, total = ops.train_panels_plan(B, S, g, panels=names)
    buf = torch.zeros(total, dtype=torch.uint8)
    panels = {n: buf[off:off + 3 * Hg * Wg].view(Hg, Wg, 3) for n, (Hg, Wg, off) in reversed(list(plan.items()))}    # insertion order must not matter
    w = _Writer()
    tbutils.log_panels(w, panels, 200)
    assert [c[0] for c in w.calls] == ["visual/" + n for n in names]
    for (tag, shape, dtype, step), n in zip(w.calls, names):
        assert shape == (3,) + plan[n][:2] and dtype == torch.uint8 and step == 200


def test_panel_writer_writes_and_reraises(tmp_path):
    from PIL import Image
    from excel_amd.utils import tbutils
    rgb = np.random.default_rng(0).integers(0, 256, (7, 9, 3), dtype=np.uint8)
    w = tbutils.PanelWriter()
    w.submit(str(tmp_path / "iter_2"), dict(img1=rgb))
    assert w.close() == [str(tmp_path / "iter_2")]
    im = Image.open(tmp_path / "iter_2" / "img1.png")
    assert im.mode == "RGB" and np.array_equal(np.asarray(im), rgb)
    blocker = tmp_path / "file"
    blocker.write_text("x")
    w = tbutils.PanelWriter()
    w.submit(str(blocker / "iter_2"), dict(img1=rgb))          # a directory below a regular file: the write fails in the thread
    with pytest.raises(OSError):
        w.close()
