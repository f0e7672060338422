"""The training iteration (train.hip) at the production head shapes against the float64 autograd oracle (oracle/train.py, itself
pinned to the reference's goldens by tests/test_oracle_train.py): the train-mode forward, both losses and their gradients, the
gradient of every parameter, Dropout2d, the aff_labels_u8 regime, AdamW, reproducibility and the workspace bounds.

tests/test_gpu_train.py checks one tiny shape (head dim 4, 36 tokens, radius 2 < g); the cases here are the train_voc defaults and
the corners a tiny shape cannot reach: P = 784, ncp != nc, a head wider than 4*embed (D > 4E), one decoder layer (4*nl < L), B = 1,
nc = 2, radius < g."""
import numpy as np
import pytest

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(1200)]
torch = pytest.importorskip("torch")
from oracle import train as otrain  # noqa: E402

CASES = {
    "prod320": dict(B=4, g=20, L=12, D=768, E=256, heads=8, nl=3, nc=21, radius=8),
    "prod448": dict(B=2, g=28, L=12, D=768, E=256, heads=8, nl=3, nc=21, radius=8),
    "coco": dict(B=2, g=20, L=12, D=768, E=256, heads=8, nl=3, nc=81, radius=8),
    "narrow": dict(B=3, g=10, L=12, D=768, E=128, heads=8, nl=3, nc=21, radius=8),
    "shallow": dict(B=1, g=14, L=12, D=768, E=256, heads=4, nl=1, nc=2, radius=3),
}
W_SEG, W_DIVER = 1.0, 0.1
# bounds on relmax = max abs error / the oracle tensor's own max abs.  Worst measured on an MI355X over every case here:
# seg / attn_pred 1.5e-6, losses 1.0e-7 (relative), d_seg 1.9e-7, d_attn_pred 4.6e-8, parameter gradients 2.5e-6.
TOL = dict(fwd=1e-5, loss=1e-6, d_seg=2e-6, d_ap=1e-6, grad=1e-5)


def dev(a):
    return torch.as_tensor(np.ascontiguousarray(a)).cuda()


def host(t):
    return t.detach().cpu().numpy()


def relmax(a, b):
    return float(np.max(np.abs(np.asarray(a, np.float64) - np.asarray(b, np.float64)))) / max(float(np.max(np.abs(b))), 1e-30)


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from excel_amd import ops as _ops
    return _ops


# ---------------------------------------------------------------------------------------------------------------- inputs
def make_weights(c, seed):
    """init_decoder_state_dict with every parameter perturbed (non-zero biases, LN gamma = 1 +- 0.1, non-zero LN beta), so no term
    of the backward multiplies a zero -> {"fuse.*" / "dec.*": fp32}."""
    from excel_amd.model import init_decoder_state_dict
    sd = init_decoder_state_dict(num_classes=c["nc"], in_channels=c["D"], embedding_dim=c["E"], seed=seed, index=c["L"], layers=c["nl"],
                                 heads=c["heads"])
    rs = np.random.RandomState(seed + 100)
    w = {}
    for k, v in sd.items():
        v = v.numpy().astype(np.float32)
        if ".ln_" in k:
            v = (1 + rs.uniform(-0.1, 0.1, v.shape) if k.endswith("weight") else rs.normal(0, 0.05, v.shape)).astype(np.float32)
        elif k.endswith("bias"):
            v = (v + rs.normal(0, 0.02, v.shape)).astype(np.float32)
        w[("fuse." + k[len("decoder_fts_fuse."):]) if k.startswith("decoder_fts_fuse.") else ("dec." + k[len("decoder."):])] = v
    return w


def make_feats(c, seed):
    """all_feats [L,B,1+P,D] with ViT-like magnitudes: the residual stream grows with depth and a few channels are outliers."""
    rs = np.random.RandomState(seed + 200)
    L, B, D, N = c["L"], c["B"], c["D"], c["g"] ** 2 + 1
    f = rs.standard_normal((L, B, N, D)).astype(np.float32)
    f *= np.linspace(0.5, 2.5, L, dtype=np.float32)[:, None, None, None]
    f[..., rs.choice(D, 3, replace=False)] *= 8
    return f


def make_labels(B, g, nc, seed, kind="blobs"):
    """Pseudo labels [B,16g,16g] u8 built from structure: class blobs on the token grid (background + up to 3 foreground classes),
    nearest-up-sampled, boundaries moved by a few pixels (pixels whose bilinear stencil mixes classes), a band of 255 that covers
    a row of sampled tokens, and scattered 255 pixels.  kind: "blobs", "no_fg" (background only), "no_bg" (foreground only),
    "one_ignored" (blobs, image 0 entirely 255)."""
    rs = np.random.RandomState(seed + 300)
    H = 16 * g
    r, cc = np.mgrid[0:g, 0:g]
    out = np.empty((B, H, H), np.uint8)
    for b in range(B):
        k = 4
        cy, cx = rs.uniform(0, g, k), rs.uniform(0, g, k)
        cls = np.concatenate([[0], rs.randint(1, nc, k - 1)]) if nc > 1 else np.zeros(k, int)
        if kind == "no_fg":
            cls[:] = 0
        elif kind == "no_bg":
            cls = rs.randint(1, nc, k) if nc > 2 else np.ones(k, int)
        lab_g = cls[np.argmin((r[None] - cy[:, None, None]) ** 2 + (cc[None] - cx[:, None, None]) ** 2, 0)]
        pix = np.repeat(np.repeat(lab_g, 16, 0), 16, 1).astype(np.uint8)
        sh = np.roll(pix, 3, axis=1)
        edge = (sh != pix) & (rs.rand(H, H) < 0.5)
        pix[edge] = sh[edge]
        t = rs.randint(1, g - 1)
        pix[16 * t - 4:16 * t + 12, : H // 2] = 255
        pix[rs.rand(H, H) < 0.03] = 255
        out[b] = pix
    if kind == "one_ignored":
        out[0] = 255
    return out


_CACHE = {}


def case_inputs(name, seed=0):
    if (name, seed) not in _CACHE:
        c = CASES[name]
        _CACHE[(name, seed)] = (make_weights(c, seed), make_feats(c, seed), make_labels(c["B"], c["g"], c["nc"], seed))
    return _CACHE[(name, seed)]


def handle(ops, w, heads):
    """DecoderHandle over the weights + {handle key: oracle key}."""
    h = ops.DecoderHandle({k[5:]: v for k, v in w.items() if k.startswith("fuse.")}, {k[4:]: v for k, v in w.items() if k.startswith("dec.")},
                          heads=heads)
    names = {"fuse_w": "fuse.linear_fuse.weight", "fuse_b": "fuse.linear_fuse.bias", "pred_w": "dec.linear_pred.weight",
             "pred_b": "dec.linear_pred.bias"}
    for l in range(h.cfg["vit_layers"]):
        for f, k in (("proj_w", "proj.weight"), ("proj_b", "proj.bias"), ("proj2_w", "proj_2.weight"), ("proj2_b", "proj_2.bias")):
            names[f"fuse{l}.{f}"] = f"fuse.linears_modulelist.{l}.{k}"
    for l in range(h.cfg["dec_layers"]):
        for f, k in ops._BLOCK_KEYS.items():
            names[f"blk{l}.{f}"] = f"dec.transformer.resblocks.{l}.{k}"
    return h, names


def group(key):
    if key in ("fuse_w", "fuse_b"):
        return "linear_fuse"
    if key.startswith("fuse"):
        return "fuse_mlp"
    if key.startswith("blk"):
        f = key.split(".")[1]
        return "ln" if f.startswith("ln") else ("mha" if "proj" in f else "mlp")
    return "linear_pred"


def tr_hash(a, b, c):
    """train.hip tr_hash restated in numpy uint32 arithmetic (wrapping multiplies)."""
    u = lambda x: np.asarray(x, np.uint32)
    x = (u(a) * u(0x9E3779B1)) ^ ((u(b) + u(0x7F4A7C15)) * u(0x85EBCA6B)) ^ ((u(c) + u(0x165667B1)) * u(0xC2B2AE35))
    x ^= x >> u(16)
    x *= u(0x7FEB352D)
    x ^= x >> u(15)
    x *= u(0x846CA68B)
    x ^= x >> u(16)
    return x


def keep_mask(seed, B, E, p):
    """Dropout2d keep mask [B,E] of tr_dropout2d_kernel: u = (hash >> 8) * 2^-24 (fp32), dropped where u < p."""
    b, c = np.meshgrid(np.arange(B, dtype=np.uint32), np.arange(E, dtype=np.uint32), indexing="ij")
    h = tr_hash(np.full((B, E), seed, np.uint32), b, c)
    u = (h >> np.uint32(8)).astype(np.float32) * np.float32(1.0 / 16777216.0)
    return (~(u < np.float32(p))).astype(np.float64)


# ---------------------------------------------------------------------------------------------------------------- one iteration
def device_iteration(ops, h, feats, labels, radius, dropout_p=0.0, dropout_seed=0, aff_labels=None):
    seg, ap, ctx = h.forward_train(dev(feats), dropout_p=dropout_p, dropout_seed=dropout_seed)
    losses, d_seg, d_ap = ops.train_losses(seg, ap, dev(labels), radius=radius, w_seg=W_SEG, w_diver=W_DIVER,
                                           aff_labels_u8=dev(aff_labels) if aff_labels is not None else None)
    h._grad_table()
    h.grad_flat.fill_(float("nan"))                     # an element the backward never writes stays NaN and fails the comparison
    grads = h.backward(ctx, d_seg, d_ap)
    torch.cuda.synchronize()
    return dict(seg=host(seg), attn_pred=host(ap), losses=host(losses), d_seg=host(d_seg), d_attn_pred=host(d_ap),
                grads={k: host(v) for k, v in grads.items()}, ctx=ctx)


def errors(d, o, h, names):
    """relmax of every compared tensor, keyed by name, plus the worst per gradient group."""
    assert set(d["grads"]) == set(h.t) == set(names)
    e = dict(seg=relmax(d["seg"], o["seg"]), attn_pred=relmax(d["attn_pred"], o["attn_pred"]),
             seg_loss=abs(float(d["losses"][0]) - o["seg_loss"]) / abs(o["seg_loss"]),
             diver_loss=abs(float(d["losses"][1]) - o["diver_loss"]) / abs(o["diver_loss"]),
             d_seg=relmax(d["d_seg"], o["d_seg"]), d_attn_pred=relmax(d["d_attn_pred"], o["d_attn_pred"]))
    grads = {}
    for k, ok in names.items():
        g = d["grads"][k]
        grads[k] = float("inf") if not np.all(np.isfinite(g)) else relmax(g, o["grads"][ok].reshape(g.shape))
    return e, grads


def check(name, d, o, h, names):
    e, grads = errors(d, o, h, names)
    worst = max(grads, key=grads.get)
    per_group = {}
    for k, v in grads.items():
        per_group[group(k)] = max(per_group.get(group(k), 0.0), v)
    print(f"\n[{name}] " + " ".join(f"{k}={v:.2e}" for k, v in e.items()) + " | grads " +
          " ".join(f"{k}={v:.2e}" for k, v in sorted(per_group.items())) + f" | worst {worst} {grads[worst]:.2e}")
    assert e["seg"] < TOL["fwd"] and e["attn_pred"] < TOL["fwd"], e
    assert e["seg_loss"] < TOL["loss"] and e["diver_loss"] < TOL["loss"], e
    assert e["d_seg"] < TOL["d_seg"], e
    # d attn_pred: zero exactly where the affinity label is "ignore", and the two values -w/(2 pos_count), w/(2 neg_count)
    assert np.array_equal(d["d_attn_pred"] == 0, o["aff_mask"] == 255)
    for t, v in ((1, -0.5 * W_DIVER / o["pos_count"]), (0, 0.5 * W_DIVER / o["neg_count"])):
        sel = o["aff_mask"] == t
        if sel.any():
            assert np.all(np.abs(d["d_attn_pred"][sel] - v) <= TOL["d_ap"] * abs(v)), (t, v)
    assert grads[worst] < TOL["grad"], (worst, grads[worst])
    return e, grads


def run_case(ops, name, dropout_p=0.0, dropout_seed=0, aff_labels=None, seed=0):
    c = CASES[name]
    w, feats, labels = case_inputs(name, seed)
    h, names = handle(ops, w, c["heads"])
    d = device_iteration(ops, h, feats, labels, c["radius"], dropout_p, dropout_seed, aff_labels)
    keep = None
    if dropout_p > 0:
        keep = keep_mask(dropout_seed, c["B"], c["E"], dropout_p)
        fts = host(h.train_attn_fts(d["ctx"]))
        dead = np.all(fts == 0, axis=(2, 3))
        assert np.array_equal(dead, keep == 0), "the restated tr_hash mask differs from the device's dropped planes"
        assert 0 < dead.sum() < dead.size
    o = otrain.train_iteration(feats, w, labels, c["heads"], c["radius"], W_SEG, W_DIVER, aff_labels=aff_labels, keep=keep,
                               dropout_p=dropout_p)
    return h, names, d, o, keep


# ---------------------------------------------------------------------------------------------------------------- tests
@pytest.mark.parametrize("name", list(CASES))
def test_iteration_matches_float64_autograd(ops, name):
    h, names, d, o, _ = run_case(ops, name)
    assert 0 < o["pos_count"] - 1 and 0 < o["neg_count"] - 1             # both kinds of affinity pair occur inside the radius
    check(name, d, o, h, names)


@pytest.mark.parametrize("p", [0.1, 0.5])
def test_dropout_matches_float64_autograd(ops, p):
    h, names, d, o, _ = run_case(ops, "prod320", dropout_p=p, dropout_seed=1234)
    check(f"prod320 dropout {p}", d, o, h, names)


def test_affinity_labels_from_another_map(ops):
    """The seg_aff_iter regime (scripts/train_voc.py:210): the affinity target comes from a map other than the pseudo labels."""
    c = CASES["prod320"]
    other = make_labels(c["B"], c["g"], c["nc"], seed=9)
    h, names, d, o, _ = run_case(ops, "prod320", aff_labels=other)
    o_same = otrain.affinity_label(case_inputs("prod320")[2], c["g"], c["radius"]).numpy()
    assert not np.array_equal(o["aff_mask"], o_same)
    check("prod320 aff_labels", d, o, h, names)


@pytest.mark.parametrize("g", [20, 28])
@pytest.mark.parametrize("radius", [0, 8, 40])
@pytest.mark.parametrize("kind", ["blobs", "no_fg", "no_bg", "one_ignored"])
def test_losses_sweep(ops, g, radius, kind):
    """ops.train_losses alone on random seg / attn_pred, H = W = 16 g, radius 0, 8 and >= g, label maps with no foreground, no
    background or an entirely ignored image: losses and both gradients, with the +1e-6 and +1 terms of the reference."""
    rs = np.random.RandomState(g * 100 + radius)
    B, nc, P = 2, 21, g * g
    seg = (rs.standard_normal((B, nc, g, g)) * 3).astype(np.float32)
    ap = rs.uniform(0.0, 1.0, (B, P, P)).astype(np.float32)
    labels = make_labels(B, g, nc, seed=g + radius, kind=kind)
    losses, d_seg, d_ap = ops.train_losses(dev(seg), dev(ap), dev(labels), radius=radius, w_seg=W_SEG, w_diver=W_DIVER)
    o = otrain.losses_and_grads(seg, ap, labels, radius, w_seg=W_SEG, w_diver=W_DIVER)
    l = host(losses)
    e_seg = abs(float(l[0]) - o["seg_loss"]) / max(abs(o["seg_loss"]), 1e-30)
    e_div = abs(float(l[1]) - o["diver_loss"]) / max(abs(o["diver_loss"]), 1e-30)
    e_ds = relmax(host(d_seg), o["d_seg"])
    print(f"\n[losses g={g} r={radius} {kind}] seg_loss={e_seg:.2e} diver_loss={e_div:.2e} d_seg={e_ds:.2e} "
          f"pos={o['pos_count']} neg={o['neg_count']}")
    assert e_seg < TOL["loss"] and e_div < TOL["loss"]
    assert e_ds < TOL["d_seg"]
    d = host(d_ap)
    assert np.array_equal(d == 0, o["aff_mask"] == 255)
    assert relmax(d, o["d_attn_pred"]) < TOL["d_ap"]
    if kind == "no_fg":
        assert o["pos_count"] > 1
    if radius == 0:
        assert o["neg_count"] == 1                                           # only self pairs: the +1 alone
    if kind == "one_ignored":
        assert np.all(d[0] == 0)


def test_adamw_three_steps_across_warmup(ops):
    """Three PolyWarmupAdamW steps at prod320 with warmup_iters = 2 (the third step is past warm-up): the device's own gradients
    fed to torch.optim.AdamW in float64 give the device's parameters."""
    from excel_amd.scripts.train_voc import poly_warmup_lr
    c = CASES["prod320"]
    w, feats, labels = case_inputs("prod320")
    h, names = handle(ops, w, c["heads"])
    ref = {k: torch.tensor(host(v), dtype=torch.float64, requires_grad=True) for k, v in h.t.items()}
    opt = torch.optim.AdamW(list(ref.values()), lr=1.0, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2)
    lrs = []
    for it in range(3):
        d = device_iteration(ops, h, feats, labels, c["radius"])
        lr = poly_warmup_lr(1e-3, it, 2, 100, 1e-6, 1)
        lrs.append(lr)
        for k, p in ref.items():
            p.grad = torch.from_numpy(d["grads"][k].astype(np.float64))
        for gr in opt.param_groups:
            gr["lr"] = lr
        opt.step()
        h.adamw_step(lr, it + 1, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2)
        torch.cuda.synchronize()
        for k, p in ref.items():
            r = p.detach().numpy()
            err = np.abs(host(h.t[k]).astype(np.float64) - r)
            assert np.all(err <= 2e-6 * np.maximum(1.0, np.abs(r))), (it, k, float(err.max()))
    assert lrs[0] < lrs[1] < 1e-3 and lrs[2] == 1e-3 * (1 - 2 / 100)                   # warm-up, warm-up, poly decay


def test_backward_is_bitwise_reproducible(ops):
    c = CASES["prod320"]
    w, feats, labels = case_inputs("prod320")
    h, _ = handle(ops, w, c["heads"])
    first = device_iteration(ops, h, feats, labels, c["radius"], dropout_p=0.1, dropout_seed=5)
    again = device_iteration(ops, h, feats, labels, c["radius"], dropout_p=0.1, dropout_seed=5)
    for k in ("seg", "attn_pred", "losses", "d_seg", "d_attn_pred"):
        assert np.array_equal(first[k], again[k]), k
    for k, v in first["grads"].items():
        assert np.array_equal(v, again["grads"][k]), k


@pytest.mark.parametrize("name", ["prod320", "narrow", "shallow"])
def test_workspaces_stay_in_bounds(ops, name, monkeypatch):
    """Every workspace gets a 1 MiB sentinel tail; forward_train, train_attn_fts, backward and train_losses leave it untouched.  The
    workspace itself starts as NaN bytes, so a read of anything the kernels did not write first shows up as a non-finite result."""
    SENT, TAIL = 0xA5, 1 << 20
    bufs = []

    def guarded_ws(nbytes, device):
        n = max(int(nbytes), 256)
        buf = torch.full((n + TAIL,), SENT, dtype=torch.uint8, device=device)
        buf[:n] = 0xFF
        bufs.append((buf, n))
        return buf[:n]

    monkeypatch.setattr(ops, "_ws", guarded_ws)
    c = CASES[name]
    w, feats, labels = case_inputs(name)
    h, _ = handle(ops, w, c["heads"])
    d = device_iteration(ops, h, feats, labels, c["radius"], dropout_p=0.1, dropout_seed=3)
    h.train_attn_fts(d["ctx"])
    torch.cuda.synchronize()
    assert len(bufs) >= 2
    for buf, n in bufs:
        assert bool((buf[n:] == SENT).all()), f"a kernel wrote past its {n}-byte workspace"
    for k in ("seg", "attn_pred", "losses", "d_seg", "d_attn_pred"):
        assert np.all(np.isfinite(d[k])), k
    assert all(np.all(np.isfinite(v)) for v in d["grads"].values())


def test_negative_controls(ops):
    """The comparisons at prod320 catch a real mistake: the oracle with one deliberate error at a time (per-image instead of global
    mean in attn_pred; radius - 1; the dropout mask shifted by one channel) is more than 10x the tolerance away from the kernels."""
    c = CASES["prod320"]
    w, feats, labels = case_inputs("prod320")

    def ratio(d, o, h, names):
        e, grads = errors(d, o, h, names)
        tol = dict(seg=TOL["fwd"], attn_pred=TOL["fwd"], seg_loss=TOL["loss"], diver_loss=TOL["loss"], d_seg=TOL["d_seg"], d_attn_pred=TOL["d_ap"])
        r = {k: e[k] / tol[k] for k in e}
        r["grads"] = max(grads.values()) / TOL["grad"]
        return r

    h, names, d, o, _ = run_case(ops, "prod320")
    bad = otrain.train_iteration(feats, w, labels, c["heads"], c["radius"], W_SEG, W_DIVER, attn_mean="per_image")
    r1 = ratio(d, bad, h, names)
    bad = otrain.train_iteration(feats, w, labels, c["heads"], c["radius"] - 1, W_SEG, W_DIVER)
    r2 = ratio(d, bad, h, names)
    h, names, d, o, keep = run_case(ops, "prod320", dropout_p=0.1, dropout_seed=1234)
    bad = otrain.train_iteration(feats, w, labels, c["heads"], c["radius"], W_SEG, W_DIVER, keep=np.roll(keep, 1, axis=1), dropout_p=0.1)
    r3 = ratio(d, bad, h, names)
    for what, r in (("per-image mean", r1), ("radius - 1", r2), ("shifted dropout mask", r3)):
        print(f"\n[negative control: {what}] " + " ".join(f"{k}={v:.1f}x" for k, v in r.items()))
    assert r1["attn_pred"] > 10 and r1["grads"] > 10
    assert r2["diver_loss"] > 10 and r2["d_attn_pred"] > 10 and r2["grads"] > 10
    assert r3["seg"] > 10 and r3["attn_pred"] > 10 and r3["grads"] > 10


def test_token_count_not_multiple_of_4_is_refused(ops):
    """g = 21 (P = 441): refused with an error before any launch, not run on a misaligned layout (support is out of scope)."""
    c = dict(CASES["shallow"], g=21)
    w = make_weights(c, 0)
    h, _ = handle(ops, w, c["heads"])
    feats = dev(np.zeros((c["L"], 1, 21 * 21 + 1, c["D"]), np.float32))
    with pytest.raises(RuntimeError, match="multiple of 4"):
        h.forward_train(feats)
    torch.cuda.synchronize()


def test_train_step_with_a_head_wider_than_4x_embed(ops, golden):
    """DecoderTrainer.train_step with D > 4E (the tiny tower's width 128, a 16-wide 4-head head) and one decoder layer: these head
    shapes used to be refused at the first backward."""
    from oracle.vit import VitConfig, make_vit_weights
    from excel_amd.model import ExCEL_model, init_decoder_state_dict
    from excel_amd.scripts.train_voc import DecoderTrainer
    from excel_amd.utils.PAR import PAR
    TINY = VitConfig(width=128, layers=8, heads=2, patch=16, out_dim=64, input_resolution=64, n_surgery=5)
    kw = dict(width=128, layers=8, heads=2, patch=16, output_dim=64, input_resolution=64)
    rs = np.random.RandomState(3)
    text = rs.standard_normal((9, 64)).astype(np.float32)
    text /= np.linalg.norm(text, axis=1, keepdims=True)
    x = dev(np.random.RandomState(5).standard_normal((2, 3, 96, 96)).astype(np.float32))
    cls = dev(np.array([[1, 0, 1, 0], [0, 1, 0, 0]], np.float32))
    for layers in (3, 1):
        sd = init_decoder_state_dict(num_classes=5, in_channels=128, embedding_dim=16, seed=1, index=8, layers=layers, heads=4)
        model = ExCEL_model(clip_model="tiny", num_classes=5, img_size=96, mode="train", state_dict=make_vit_weights(TINY, seed=11), vit_cfg=kw,
                            text_attr=text.T.copy(), gemm_mode="f32", embedding_dim=16, in_channels=128, decoder_state_dict=sd, decoder_heads=4)
        tr = DecoderTrainer(model, PAR(num_iter=10, dilations=[1, 2, 4, 8, 12, 24]), lr=1e-3, warmup_iters=2, max_iters=100, radius=2,
                            lvc_iter=10 ** 9, dropout_p=0.0)
        hist = [tr.train_step(x, cls) for _ in range(6)]
        assert all(np.isfinite(hh["seg_loss"]) and np.isfinite(hh["diver_loss"]) for hh in hist), layers
        assert hist[-1]["seg_loss"] < hist[0]["seg_loss"], layers
