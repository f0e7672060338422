"""ops.train_panels (trainviz.hip) against the torch-CPU restatement of the reference's progress panels (tests/_train_panels_ref.py):
img1 and the label panels bit for bit, cam1 bit for bit outside the jet-bin margins, and the tbutils call surface over the op.

Shapes (B, F, g, S): (3, 4, 3, 48) - an odd batch with an empty cell, S no multiple of the 64-column tile; (1, 4, 3, 48) - the bare
single image; (4, 4, 6, 96) - a full 2 x 2 grid, more than one tile per row.

cam1's gate: float32 bilinear sums taken in another order than F.interpolate's may land in the neighbouring jet bin where the oracle's
own cam_max * 256 lies within 1e-3 of an integer in 1..255.  Those pixels (the reference alone puts 0.13-0.34 % of these inputs there)
must carry the oracle's bytes for that bin or an adjacent one, and stay below 1 % of the panel; every other pixel is bit-identical."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

import _train_panels_ref as R  # noqa: E402

SHAPES = [(3, 4, 3, 48), (1, 4, 3, 48), (4, 4, 6, 96)]
_CASES = {}


def _case(shape):
    """inputs and the oracle's panels of one shape, built once and shared (never modified)"""
    if shape in _CASES:
        return _CASES[shape]
    from excel_amd.utils import imutils
    B, F_, g, S = shape
    rng = np.random.default_rng(sum(shape))
    u8 = torch.from_numpy(rng.integers(0, 256, (B, 3, S, S), dtype=np.uint8))
    x = u8.to(torch.float32) / 255
    for c in range(3):
        x[:, c] = (x[:, c] - R.MEAN[c]) / R.STD[c]                    # normalised in float32
    attr = torch.from_numpy(rng.uniform(-0.1, 1.1, (B, g * g, F_)).astype(np.float32))
    cls = torch.zeros((B, F_), dtype=torch.float32)
    for b in range(B):
        cls[b, b % F_] = 1
        cls[b, (b + 2) % F_] = 1                                        # two present, two absent classes per image
    f0 = 0                                                              # present in image 0
    attr[0, 0, :] = 0.5
    attr[0, 0, f0] = 1.0                                                # top-left corner patch: an exact 1.0 is the maximum there
    attr[0, g - 1, :] = -0.05
    attr[0, g - 1, f0] = 0.0                                            # top-right corner patch: an exact 0.0 is the maximum there
    attr[0, g * (g - 1), 1] = float("nan")                              # bottom-left corner patch, an ABSENT class: NaN * 0 propagates
    labs = {n: torch.from_numpy(rng.integers(0, 21, (B, S, S), dtype=np.uint8)) for n in ("pseu_aff", "seg_gt", "seg_pred")}
    labs["pseu_mid"] = torch.from_numpy(rng.integers(0, 21, (B, g, g), dtype=np.uint8))
    for t in labs.values():
        t[:, 0, :] = 255
        t[:, -1, -1] = 255
    lut = imutils.jet_lut()
    img = R.img1(x)
    cmax = R.cam_max(attr, cls, S)
    ref = dict(img1=R.make_grid(img), cam1=R.make_grid(R.jet_blend(cmax, img, lut)))
    for n, t in labs.items():
        ref[n] = R.make_grid(R.label_rgb(t.numpy()))
    _CASES[shape] = dict(x=x, attr=attr, cls=cls, labs=labs, img=img, cmax=cmax, lut=lut, ref=ref)
    return _CASES[shape]


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from excel_amd import ops
    return ops


def _render(ops, c, **kw):
    return ops.train_panels(inputs=c["x"].cuda(), attr_maps_raw=c["attr"].cuda(), cls_label=c["cls"].cuda(),
                            **{n: t.cuda() for n, t in c["labs"].items()}, **kw)


@pytest.mark.parametrize("shape", SHAPES)
def test_panels_match_the_reference(ops, shape):
    B, F_, g, S = shape
    c = _case(shape)
    assert np.isnan(c["cmax"]).any() and (c["cmax"] == 1.0).any() and (c["cmax"] == 0.0).any()        # the planted values reach the maximum
    p = _render(ops, c)
    plan, total = R.plan(B, S, g)
    assert list(p) == list(R.PANELS) and p.plan == plan and p.buffer.numel() == total
    got = p.host()
    for n in R.PANELS:
        assert got[n].shape == c["ref"][n].shape, n
        assert np.array_equal(p[n].cpu().numpy(), got[n]), n                                       # the views and the one-copy path agree
        if n != "cam1":
            assert np.array_equal(got[n], c["ref"][n]), n
    # cam1: the margin pixels of the oracle, in grid coordinates
    xa = c["cmax"].astype(np.float64) * 256
    with np.errstate(invalid="ignore"):
        near = np.rint(xa)
        margin = (np.abs(xa - near) < 1e-3) & (near >= 1) & (near <= 255)
    share = margin.mean()
    print(f"shape {shape}: margin share {100 * share:.3f} % of {margin.size} pixels")
    assert share < 0.01
    mgrid = R.make_grid(np.repeat(margin[..., None], 3, -1).astype(np.uint8)).astype(bool)
    diff = got["cam1"] != c["ref"]["cam1"]
    print(f"shape {shape}: {int(diff.any(-1).sum())} differing pixels, {int((diff & ~mgrid).any(-1).sum())} outside the margin")
    assert not (diff & ~mgrid).any()
    # inside the margin: the oracle's bytes for its own bin or an adjacent one
    with np.errstate(invalid="ignore"):
        idx0 = np.clip(np.where(np.isnan(xa), 0, np.floor(xa)), 0, 255).astype(np.int64)
    ok = np.zeros(mgrid.shape[:2], bool)
    for d in (-1, 0, 1):
        alt = R.make_grid(R.jet_blend(np.clip(idx0 + d, 0, 255), c["img"], c["lut"], by_index=True))
        ok |= (got["cam1"] == alt).all(-1)
    assert ok[mgrid.all(-1)].all()


def test_subset_and_nrow(ops):
    """a subset of the panels is tight and equal to the full render's; nrow 3 puts the odd batch on one row"""
    shape = SHAPES[0]
    B, F_, g, S = shape
    c = _case(shape)
    full = _render(ops, c).host()
    sub = ops.train_panels(inputs=c["x"].cuda(), seg_pred=c["labs"]["seg_pred"].cuda(), pseu_mid=c["labs"]["pseu_mid"].cuda())
    assert list(sub) == ["img1", "pseu_mid", "seg_pred"] and sub.plan == R.plan(B, S, g, panels=list(sub))[0]
    for n, a in sub.host().items():
        assert np.array_equal(a, full[n]), n
    wide = ops.train_panels(inputs=c["x"].cuda(), nrow=3)["img1"].cpu().numpy()
    assert wide.shape == (S + 4, 3 * (S + 2) + 2, 3) and np.array_equal(wide, R.make_grid(c["img"], nrow=3))
    with pytest.raises(ValueError):
        ops.train_panels(inputs=c["x"].cuda(), seg_pred=c["labs"]["pseu_mid"].cuda())              # a [B,g,g] map where [B,S,S] belongs


@pytest.mark.parametrize("shape", SHAPES[:2])
def test_tbutils_equals_the_op(ops, shape):
    from excel_amd.utils import tbutils
    c = _case(shape)
    p = _render(ops, c)
    grid_img, grid_cam = tbutils.make_grid_image(c["x"].cuda(), c["attr"].cuda(), cls_label=c["cls"].cuda())
    assert grid_img.dtype == torch.uint8 and grid_img.shape[0] == 3
    assert torch.equal(grid_img, p["img1"].permute(2, 0, 1)) and torch.equal(grid_cam, p["cam1"].permute(2, 0, 1))
    for n in ("pseu_aff", "pseu_mid"):
        lab = c["labs"][n].cuda()
        assert torch.equal(tbutils.make_grid_label(lab), p[n].permute(2, 0, 1)), n
        assert torch.equal(tbutils.make_grid_label(lab.long()), p[n].permute(2, 0, 1)), n          # the reference's labels are int64
