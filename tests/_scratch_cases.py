"""Case table of tests/test_gpu_scratch_contract.py (importable without a GPU: the host completeness test reads COVERS from it).

One entry per op (or small family of ops): build(ops) -> Case(fn, defined, holes, n_ws; n_ws > 0: the ops allocate through ops._ws).  fn() calls the op(s) on seeded inputs and returns
the outputs as a tree; it is run twice, on scratch / output memory of 0x00 and of 0xFF bytes, and the two trees must be bit-identical.
Shapes are the smallest that still have padding in every buffer that can have it (P = 25 -> Pp = 28, nc = 21 -> ncp = 24, C = 30 ->
Cp = 32, W % 4 != 0 in every pitched plane).  The *_many cases run the class-count dependent ops again at the COCO counts (Smax = 18, Cmax = 19,
images of 18, 9 and 1 present classes): the Smax- / Cmax-sized regions of their workspaces at the size production gives them.

What each workspace holds, and the invariant that keeps an unwritten byte from reaching a result:
  DecoderHandle.forward      dec_ws_layout: nine float regions, no integer table.  Score rows have pitch Pp; dec_row_softmax_kernel zeroes
                             columns [P, Pp), the K tail of P.V (Kld = Pp); the NN GEMM guards V's rows by K = P.  segt pad columns
                             [nc, ncp) are never read (dec_transpose_kernel stops at Cc = nc).
  TextHandle.encode          text_ws_layout: seven float regions, no integer table; the same preln_blocks as the decoder (causal).
  feature_affinity(+grouped) inv | fn [B,P,Cp] | double partials | mean: floats only.  lvc_transpose_scale_kernel writes fn's columns
                             [C, Cp) as zeros; partials / means are written for exactly the indices the next kernel reads.
  attn_select_mean           double partials [B,L,64] | float mask [B,L+1]: every slot written by lvc_layer_diff / lvc_layer_mask first.
  compute_trans_mat, refine  T | Tsym | column sums | v | u: floats only; bbox_mask / matvec touch rows < ncls[b] only, on both sides.
  cam_upsample_bkg(_ragged)  one float region (min-max normalised maps), rows < ncls[b] written and read.
  clip_feature_surgery       S [B*N, ldT]: the epilogue reads columns < T only.
  patch_text_cam             sim | split text | per-workgroup min/max | column partials: floats / bf16; every slot a later kernel
                             reads is written by the kernel in front of it (part: tid < CT*32 written, tid < T <= CT*32 read).
  par_forward(_ragged)       affinities or 5 statistics planes | ping-pong | resized guide: floats only.  Pad columns of the pitched
                             planes are read only into the pad lane of a pixel pair (stat_load) and staged with the column clamped
                             to W - 1, so they reach no pixel; include/excel_hip.h documents out's pad columns as undefined.
  dcrf_inference(+ragged, lam) two lattices: keys, bary (all vertices written by crf_lattice_kernel); hash table (memset 0xFF = -1) and
                             counter (memset 0) before crf_hash_insert_kernel; rep [all], latidx [representatives] written there and
                             read only through rep / the hash table; offset [all]; nbr [j <= D, i < counter] written and read for the
                             same range; the CSR lists reuse dead tables after a memset of cnt / fill / cursor; accumulators memset;
                             lat0 / lat1 written by blur pass j before pass j + 1 reads them; LAM class counts for i < counter.
  train_augment(_image)      histograms (memset) | chosen window (aug_choose_kernel) | horizontal-pass rows (written for the rows and
                             columns the vertical pass reads); all coefficient / index tables come from the host plan.
  png_encode_labels_ragged   uint2 row records [B, Hmax]: rows r < H_b written by the measuring pass, the same rows read; arena memset.
  jpeg_encode_rgb_ragged     records (jpeg_table_kernel) | sizes (layout / count) | block lengths (measuring pass, every block) |
                             coefficients (every live MCU) | stream words (memset, OR-ed into).
  VitHandle.forward f32      vit_ws_layout: floats only; a_sum [B,N,NP] is written for columns < NP (zero in [N, NP)), the K tail of
                             A_sum.V (Kld = NP).
"""
from collections import namedtuple

import numpy as np

Case = namedtuple("Case", "fn defined holes n_ws", defaults=(None, None, 0))

# ops.py function / method -> the cases that run it (the host completeness test requires every workspace user here or in ALREADY_COVERED)
COVERS = {
    "DecoderHandle.forward": ["decoder"],
    "TextHandle.encode": ["text"],
    "feature_affinity": ["feature_affinity"],
    "feature_affinity_grouped": ["feature_affinity_grouped"],
    "attn_select_mean": ["attn_means"],
    "compute_trans_mat": ["trans_mat"],
    "refine_cams_with_aff_batched": ["refine", "refine_many"],
    "cam_upsample_bkg": ["cam_upsample", "cam_upsample_many"],
    "cam_upsample_bkg_ragged": ["cam_upsample_ragged", "cam_upsample_ragged_many"],
    "clip_feature_surgery": ["clip_feature_surgery"],
    "patch_text_cam": ["patch_text_cam"],
    "par_forward": ["par_forward", "par_forward_many"],
    "par_forward_ragged": ["par_forward_ragged", "par_forward_ragged_many"],
    "dcrf_inference": ["dcrf"],
    "dcrf_inference_ragged": ["dcrf_ragged"],
    "dcrf_lam_ragged": ["dcrf_lam"],
    "train_augment": ["train_augment"],
    "train_augment_image": ["train_augment"],
    "png_encode_labels_ragged": ["png"],
    "jpeg_encode_rgb_ragged": ["jpeg"],
    "VitHandle.forward": ["vit_f32"],
}
# workspace users another test already runs on poisoned memory: name -> that test
ALREADY_COVERED = {
    "VitHandle.workspace": "test_gpu_attn_shapes.py::test_workspace_padding_is_never_read_as_data (bf16x3 / f16x3; the f32 mode is case vit_f32)",
    "DecoderHandle.forward_train": "test_gpu_train_grad.py::test_workspaces_stay_in_bounds",
    "DecoderHandle.backward": "test_gpu_train_grad.py::test_workspaces_stay_in_bounds",
    "DecoderHandle.train_attn_fts": "test_gpu_train_grad.py::test_workspaces_stay_in_bounds",
    "train_losses": "test_gpu_train_grad.py::test_workspaces_stay_in_bounds",
}

SIZES = [(17, 29), (40, 33)]           # two images, widths no multiple of 4 (Wp = 32, 36)
CRF_PARAMS = (2, 3, 1, 4, 67, 3)       # test_dcrf_vs_oracle's parameter set, 2 iterations


def _torch():
    import torch
    return torch


UPLOADER = []       # tests/_align_cases.py: while this holds a function, dev() uploads through it (a view one element into its storage)


def dev(a, dtype=None):
    torch = _torch()
    t = torch.as_tensor(np.ascontiguousarray(a))
    if dtype is not None:
        t = t.to(dtype)
    return UPLOADER[-1](t, "cuda") if UPLOADER else t.cuda()


# ------------------------------------------------------------------ shared input builders (also used by test_gpu_padded_shapes.py)
def decoder_weights(rs, L=3, D=64, E=32, nc=21, layers=2):
    """state_dict-keyed weights of a small head ("fuse." / "dec." prefixes, oracle.decoder's convention)"""
    f = lambda *s, k=1.0: (rs.standard_normal(s) * k).astype(np.float32)
    w = {}
    for l in range(L):
        w[f"fuse.linears_modulelist.{l}.proj.weight"] = f(E, D, k=D ** -0.5)
        w[f"fuse.linears_modulelist.{l}.proj.bias"] = f(E, k=0.1)
        w[f"fuse.linears_modulelist.{l}.proj_2.weight"] = f(E, E, k=E ** -0.5)
        w[f"fuse.linears_modulelist.{l}.proj_2.bias"] = f(E, k=0.1)
    w["fuse.linear_fuse.weight"] = f(E, L * E, 1, 1, k=(L * E) ** -0.5)
    w["fuse.linear_fuse.bias"] = f(E, k=0.1)
    for l in range(layers):
        w.update(block_weights(rs, f"dec.transformer.resblocks.{l}.", E))
    w["dec.linear_pred.weight"] = f(nc, E, 1, 1, k=E ** -0.5)
    w["dec.linear_pred.bias"] = f(nc, k=0.1)
    return w


def block_weights(rs, p, E):
    f = lambda *s, k=1.0: (rs.standard_normal(s) * k).astype(np.float32)
    return {p + "ln_1.weight": 1 + f(E, k=0.1), p + "ln_1.bias": f(E, k=0.1), p + "ln_2.weight": 1 + f(E, k=0.1), p + "ln_2.bias": f(E, k=0.1),
            p + "attn.in_proj_weight": f(3 * E, E, k=E ** -0.5), p + "attn.in_proj_bias": f(3 * E, k=0.1),
            p + "attn.out_proj.weight": f(E, E, k=E ** -0.5), p + "attn.out_proj.bias": f(E, k=0.1),
            p + "mlp.c_fc.weight": f(4 * E, E, k=E ** -0.5), p + "mlp.c_fc.bias": f(4 * E, k=0.1),
            p + "mlp.c_proj.weight": f(E, 4 * E, k=(4 * E) ** -0.5), p + "mlp.c_proj.bias": f(E, k=0.1)}


def decoder_handle(ops, w, heads=8):
    return ops.DecoderHandle({k[5:]: v for k, v in w.items() if k.startswith("fuse.")}, {k[4:]: v for k, v in w.items() if k.startswith("dec.")},
                             heads=heads)


def text_weights(rs, ctx=9, E=32, V=50, C=16, layers=2):
    f = lambda *s, k=1.0: (rs.standard_normal(s) * k).astype(np.float32)
    w = {"token_embedding.weight": f(V, E, k=0.5), "positional_embedding": f(ctx, E, k=0.1), "ln_final.weight": 1 + f(E, k=0.1),
         "ln_final.bias": f(E, k=0.1), "text_projection": f(E, C, k=E ** -0.5)}
    for l in range(layers):
        w.update(block_weights(rs, f"transformer.resblocks.{l}.", E))
    return w


def text_tokens(rs, B=3, ctx=9, V=50, eot=(2, 5, 8)):
    """B prompts whose EOT token (the largest id) sits at a different position each, the last one in the last slot"""
    tok = np.zeros((B, ctx), np.int64)
    for b, n in enumerate(eot):
        tok[b, :n] = rs.randint(1, V - 2, n)
        tok[b, n] = V - 1
    return tok


def pitched(rs, plan, K, lo=0.0, hi=1.0):
    """K pitched planes per image of plan, uniform values (pad columns included: inputs are not what is under test)"""
    return (rs.rand(K * plan.total_pix) * (hi - lo) + lo).astype(np.float32)


def pitched_mask(plan, K, nch=None):
    """bool [K * total_pix]: True at (plane c < nch[b], column x < W_b) of every image - the written part of a pitched output"""
    m = np.zeros(K * plan.total_pix, bool)
    for b in range(plan.B):
        H, W = int(plan.hw[b, 0]), int(plan.hw[b, 1])
        Wp = (W + 3) // 4 * 4
        v = m[K * plan.poff[b]:K * plan.poff[b] + K * H * Wp].reshape(K, H, Wp)
        v[:K if nch is None else int(nch[b]), :, :W] = True
    return m


def aug_params(ops, hw, S, ratios, flips, rs):
    p = np.zeros(len(hw), ops.aug_params_dtype())
    for b, (h, w) in enumerate(hw):
        r = ratios[b]
        h2, w2 = int(r * h), int(r * w)
        H, W = max(S, h2), max(S, w2)
        p[b]["ratio"], p[b]["flip"] = r, flips[b]
        p[b]["h_pad"], p[b]["w_pad"] = rs.randint(H - h2 + 1), rs.randint(W - w2 + 1)
        p[b]["cand_h"], p[b]["cand_w"] = rs.randint(0, H - S + 1, 10), rs.randint(0, W - S + 1, 10)
    return p


# ------------------------------------------------------------------ the cases
def _decoder(ops):
    rs = np.random.RandomState(1)
    w = decoder_weights(rs)
    h = decoder_handle(ops, w)
    feats = dev(rs.standard_normal((3, 2, 26, 64)).astype(np.float32))          # g = 5: P = 25, Pp = 28; nc = 21, ncp = 24

    def fn():
        fts, seg = h.forward(feats)
        fts_only, none = h.forward(feats, want_seg=False)
        assert none is None
        return dict(fts=fts, seg=seg, fts_only=fts_only)
    return Case(fn, n_ws=2)


def _text(ops):
    rs = np.random.RandomState(2)
    h = ops.TextHandle(text_weights(rs), heads=2)                                  # context 9: Pp = 12
    tok = text_tokens(rs)
    return Case(lambda: h.encode(tok), n_ws=1)


def _feature_affinity(ops):
    rs = np.random.RandomState(3)
    f30 = dev(rs.standard_normal((4, 30, 5, 5)).astype(np.float32))              # Cp = 32
    f6 = dev(rs.standard_normal((4, 6, 25)).astype(np.float32))                  # Cp = 8
    return Case(lambda: {(c, m): ops.feature_affinity(f, m) for c, f in ((30, f30), (6, f6)) for m in ("sigmoid", "mask_softmax")}, n_ws=4)


def _feature_affinity_grouped(ops):
    torch = _torch()
    rs = np.random.RandomState(4)
    f30 = dev(rs.standard_normal((4, 30, 5, 5)).astype(np.float32))
    f6 = dev(rs.standard_normal((4, 6, 25)).astype(np.float32))

    def fn():
        r = {}
        for c, f in ((30, f30), (6, f6)):
            for m in ("sigmoid", "mask_softmax"):
                r[c, m, 1] = ops.feature_affinity_grouped(f, m, group=2, member_stride=1)
                r[c, m, 2] = ops.feature_affinity_grouped(f, m, group=2, member_stride=2)      # B / group: the (x, flip x) pairing
        own = torch.empty((4, 25, 25), dtype=torch.float32, device="cuda")                      # a caller's out=, starting as the run's byte
        r["out="] = ops.feature_affinity_grouped(f30, "sigmoid", group=1, out=own)
        assert r["out="] is own
        return r
    return Case(fn, n_ws=9)


def _attn_means(ops):
    rs = np.random.RandomState(5)
    attn = dev(rs.rand(8, 2, 26, 26).astype(np.float32))
    seg = dev(rs.rand(2, 25, 25).astype(np.float32))
    return Case(lambda: dict(select=ops.attn_select_mean(attn, seg, 6), mean=ops.attn_layer_mean(attn, 6)), n_ws=1)


def _trans_mat(ops):
    """excel_compute_trans_mat refuses P % 4 != 0 (its P x P GEMM has K = P), so g = 5 is not a shape of this op: g = 6 (P = 36, more
    than one 32-wide tile of the symmetrise kernel), and the refusal itself is part of the case."""
    import pytest
    rs = np.random.RandomState(6)
    w36 = dev(rs.rand(2, 36, 36).astype(np.float32) ** 6 + 1e-4)
    w25 = dev(rs.rand(2, 25, 25).astype(np.float32) + 1e-4)

    def fn():
        with pytest.raises(RuntimeError):
            ops.compute_trans_mat(w25)
        return dict(batch=ops.compute_trans_mat(w36), single=ops.compute_trans_mat(w36[0]))
    return Case(fn, n_ws=3)


def _cam_inputs(ops, seed, many=False):
    """-> (rs, cls_idx, ncls, nchan, host counts, F, smax).  many: the COCO class counts (datasets/coco.py: max_k() == 18) - F = 80,
    smax = 18, images of 9, 1 and 18 present classes (the first and the last class among them): the Smax- / Cmax-dependent regions
    of the workspaces at the size production runs them with, next to an image that uses one row of them."""
    rs = np.random.RandomState(seed)
    F, smax = (80, 18) if many else (6, 3)
    onehot = np.zeros((3, F), np.float32)
    if many:
        onehot[0, rs.choice(F, 9, replace=False)] = 1
        onehot[1, [41]] = 1
        onehot[2, np.concatenate([[0, F - 1], 1 + rs.choice(F - 2, 16, replace=False)])] = 1
    else:
        onehot[0, [1, 4]] = 1
        onehot[1, [2]] = 1                                                      # one class
        onehot[2, [0, 3, 5]] = 1
    idx, ncls, nchan = ops.cls_compact(dev(onehot), smax, want_nchan=True)
    return rs, idx, ncls, nchan, onehot.sum(1).astype(np.int64), F, smax


def _refine(ops, many=False):
    rs, idx, ncls, _, _, F, _ = _cam_inputs(ops, 7, many)
    attr = dev(rs.rand(3, 25, F).astype(np.float32))
    w_aff = dev(rs.rand(3, 25, 25).astype(np.float32) ** 6 + 1e-4)
    return Case(lambda: ops.refine_cams_with_aff_batched(attr, w_aff, idx, ncls, 5), n_ws=1)


def _cam_upsample(ops, many=False):
    """zero_unused=False: "channels > ncls[b] are zero unless zero_unused=False: nothing on the path reads them" (ops.cam_upsample_bkg):
    those channels are the documented hole."""
    torch = _torch()
    rs, _, ncls, _, n, _, smax = _cam_inputs(ops, 8, many)
    refined = dev(rs.rand(3, smax, 25).astype(np.float32))
    H, W = 17, 29

    def fn():
        own = torch.empty((3, smax + 1, H, W), dtype=torch.float32, device="cuda")
        return dict(zeroed=ops.cam_upsample_bkg(refined, ncls, 5, H, W), own=ops.cam_upsample_bkg(refined, ncls, 5, H, W, out=own),
                    unused=ops.cam_upsample_bkg(refined, ncls, 5, H, W, zero_unused=False))

    def defined(path, t):
        return torch.cat([t[b, :n[b] + 1].reshape(-1) for b in range(3)]) if "unused" in path else t
    return Case(fn, defined, lambda r: [r["unused"][b, n[b] + 1:] for b in range(3) if n[b] < smax], n_ws=3)


def _cam_upsample_ragged(ops, many=False):
    """Pitched planes: "the pad columns (x >= W_b) of the pitched rows are not written" (ops.cam_upsample_bkg_ragged), and with
    zero_unused=False neither are the planes > ncls[b]."""
    torch = _torch()
    rs, _, ncls, _, n, _, smax = _cam_inputs(ops, 9, many)
    sizes = SIZES + [(9, 6)]
    plan = ops.RaggedPlan(sizes, "cuda")
    refined = dev(rs.rand(3, smax, 25).astype(np.float32))
    C = smax + 1
    m_all, m_used = dev(pitched_mask(plan, C)), dev(pitched_mask(plan, C, n + 1))

    def fn():
        own = torch.empty((C * plan.total_pix,), dtype=torch.float32, device="cuda")
        return dict(zeroed=ops.cam_upsample_bkg_ragged(refined, ncls, 5, plan, out=own),
                    unused=ops.cam_upsample_bkg_ragged(refined, ncls, 5, plan, zero_unused=False))
    return Case(fn, lambda path, t: t[m_used if "unused" in path else m_all], lambda r: [r["zeroed"][~m_all], r["unused"][~m_used]], n_ws=2)


def _clip_feature_surgery(ops):
    rs = np.random.RandomState(10)
    f = rs.standard_normal((2, 26, 32)).astype(np.float32)
    f /= np.linalg.norm(f, axis=1, keepdims=True)
    t = rs.standard_normal((9, 32)).astype(np.float32)                             # T = 9: ldT = 12
    t /= np.linalg.norm(t, axis=1, keepdims=True)
    f, t = dev(f), dev(t)
    return Case(lambda: dict(both=ops.clip_feature_surgery(f, t, num_fg=4), slice=ops.clip_feature_surgery(f, t, num_fg=4, want_full=False),
                             full=ops.clip_feature_surgery(f, t)), n_ws=3)


def _patch_text_cam(ops):
    rs = np.random.RandomState(11)
    x = dev(rs.standard_normal((2, 26, 32)).astype(np.float32))
    t = rs.standard_normal((9, 32)).astype(np.float32)
    t = dev(t / np.linalg.norm(t, axis=1, keepdims=True))

    def fn():
        r = {}
        for mode in ("f32", "bf16x3"):
            r[mode, "all"] = ops.patch_text_cam(x, t, num_fg=4, want_full=True, want_features=True, mode=mode)
            r[mode, "slice"] = ops.patch_text_cam(x, t, num_fg=4, mode=mode)
            r[mode, "full"] = ops.patch_text_cam(x, t, want_full=True, mode=mode)
        return r
    return Case(fn, n_ws=6)


def _par_forward(ops, many=False):
    """"Channels >= nchan[b] of `out` are not written" (ops.par_forward): the hole of a caller's out=.  Recomputing kernel at W % 4 == 0
    (with a guide that is resized, so the guide region of the workspace is in use), streamed planes on request and at W % 4 != 0.
    many: Cmax = 19 (18 classes + background), an image of 2 channels (one class) next to one of 19."""
    torch = _torch()
    rs = np.random.RandomState(12)
    C, lo = (19, 2) if many else (3, 1)
    imgs = dev(rs.standard_normal((2, 3, 12, 20)).astype(np.float32))
    m32 = dev(rs.rand(2, C, 17, 32).astype(np.float32))
    m29 = dev(rs.rand(2, C, 17, 29).astype(np.float32))
    nchan = dev(np.array([lo, C], np.int32))

    def fn():
        r = dict(recompute=ops.par_forward(imgs, m32, num_iter=2), streamed=ops.par_forward(imgs, m32, num_iter=2, stream_affinities=True),
                 odd=ops.par_forward(imgs, m29, num_iter=2), nchan=ops.par_forward(imgs, m32, num_iter=2, nchan=nchan),
                 nchan_streamed=ops.par_forward(imgs, m29, num_iter=2, nchan=nchan))
        assert torch.equal(r["recompute"], r["streamed"])
        need = ops.lib().excel_par_workspace_bytes(2, C, 17, 32, len(ops.PAR_DILATIONS))
        own, ws = torch.empty(m32.shape, dtype=torch.float32, device="cuda"), torch.empty(need, dtype=torch.uint8, device="cuda")
        r["own"] = ops.par_forward(imgs, m32, num_iter=2, nchan=nchan, out=own, ws=ws)
        return r

    def defined(path, t):
        return torch.cat([t[0, :lo].reshape(-1), t[1].reshape(-1)]) if "own" in path else t
    return Case(fn, defined, lambda r: [r["own"][0, lo:]], n_ws=5)


def _par_forward_ragged(ops, many=False):
    """"The pad columns (W_b <= x < Wp_b) of `out` and its planes c >= nchan[b] are UNDEFINED on return" (include/excel_hip.h,
    excel_par_forward_ragged): undefined, not unwritten (the pixel-pair store of an odd W writes its pad lane), so they are masked
    and not required to keep the poison."""
    torch = _torch()
    rs = np.random.RandomState(13)
    plan = ops.RaggedPlan(SIZES, "cuda")
    C, lo = (19, 2) if many else (3, 1)                                            # many: 18 classes + background next to one class
    imgs = dev(rs.standard_normal((2, 3, 16, 16)).astype(np.float32))
    masks = dev(pitched(rs, plan, C))
    nch = np.array([lo, C])
    nchan = dev(nch.astype(np.int32))
    m_all, m_used = dev(pitched_mask(plan, C)), dev(pitched_mask(plan, C, nch))

    def fn():
        need = ops.lib().excel_par_ragged_workspace_bytes(plan.total_pix, C)
        own, ws = torch.empty(masks.shape, dtype=torch.float32, device="cuda"), torch.empty(need, dtype=torch.uint8, device="cuda")
        return dict(all=ops.par_forward_ragged(imgs, masks, plan, C, num_iter=2), nchan=ops.par_forward_ragged(imgs, masks, plan, C, num_iter=2, nchan=nchan),
                    own=ops.par_forward_ragged(imgs, masks, plan, C, num_iter=2, nchan=nchan, out=own, ws=ws))
    return Case(fn, lambda path, t: t[m_all if "all" in path else m_used], n_ws=2)


def _crf_image(rs, H, W):
    img = (rs.rand(H, W, 3) * 255).astype(np.uint8)
    img[:, : W // 2] = (img[:, : W // 2] * 0.15 + 140).astype(np.uint8)           # a smooth half and a noisy half
    return img


def _crf_prob(rs, C, H, W):
    p = rs.rand(C, H, W).astype(np.float32) ** 2 + 1e-3
    return p / p.sum(0, keepdims=True)


def _dcrf(ops):
    torch = _torch()
    rs = np.random.RandomState(14)
    H, W = SIZES[1]
    img, p = dev(_crf_image(rs, H, W), torch.uint8), dev(_crf_prob(rs, 3, H, W))
    return Case(lambda: dict(q=ops.dcrf_inference(img, p, *CRF_PARAMS), q0=ops.dcrf_inference(img, p, 0, *CRF_PARAMS[1:])), n_ws=2)


def _dcrf_ragged(ops):
    torch = _torch()
    rs = np.random.RandomState(15)
    plan = ops.RaggedPlan(SIZES, "cuda")
    imgs = dev(np.concatenate([_crf_image(rs, H, W).reshape(-1) for H, W in SIZES]), torch.uint8)
    unary = dev(np.concatenate([_crf_prob(rs, 3, H, W).reshape(-1) for H, W in SIZES]))
    one = ops.dcrf_ragged_workspace_bytes(SIZES[1:], 3)

    def fn():
        return dict(group=ops.dcrf_inference_ragged(imgs, plan, unary, 3, *CRF_PARAMS, want_labels=True, want_q=True),
                    split=ops.dcrf_inference_ragged(imgs, plan, unary, 3, *CRF_PARAMS, want_labels=True, want_q=True, budget_bytes=one))
    return Case(fn, n_ws=2)


def _dcrf_lam(ops):
    """q: "torch.empty: only planes < nchan[b] and columns < W_b are written" (ops.dcrf_lam_ragged)."""
    torch = _torch()
    rs = np.random.RandomState(16)
    plan = ops.RaggedPlan(SIZES, "cuda")
    imgs = dev(np.concatenate([_crf_image(rs, H, W).reshape(-1) for H, W in SIZES]), torch.uint8)
    cams = dev(pitched(rs, plan, 3, 0.01, 1.0))
    nch = np.array([1, 3], np.int32)
    cls_idx = dev(np.array([[4, 0], [1, 7]], np.int32))
    m_used = dev(pitched_mask(plan, 3, nch))
    fn = lambda: ops.dcrf_lam_ragged(imgs, plan, cams, 3, dev(nch), nch, cls_idx, *CRF_PARAMS, want_labels=True, want_q=True)
    return Case(fn, lambda path, t: t[m_used] if t.dtype == torch.float32 else t, lambda r: [r[1][~m_used]], n_ws=1)


def _train_augment(ops):
    torch = _torch()
    rs = np.random.RandomState(17)
    hw, S = [(40, 52), (30, 25)], 32
    plan = ops.RaggedPlan(hw, "cuda")
    imgs = dev(np.concatenate([rs.randint(0, 256, (h, w, 3)).astype(np.uint8).reshape(-1) for h, w in hw]), torch.uint8)
    labs = np.concatenate([rs.randint(0, 6, (h, w)).astype(np.uint8).reshape(-1) for h, w in hw])
    labs[rs.rand(labs.size) < 0.1] = 255
    labs = dev(labs, torch.uint8)
    params = aug_params(ops, hw, S, [0.75, 1.5], [1, 0], rs)                       # both resize passes run, shrinking and enlarging
    return Case(lambda: dict(voc=ops.train_augment(imgs, plan, labs, params, S), coco=ops.train_augment_image(imgs, plan, params, S)), n_ws=2)


def _png(ops):
    torch = _torch()
    rs = np.random.RandomState(18)
    plan = ops.RaggedPlan(SIZES, "cuda")
    labels = rs.randint(0, 4, plan.total_label_pix).astype(np.uint8)
    labels[: SIZES[0][1] * 3] = 7                                                  # a few long runs
    labels = dev(labels, torch.uint8)

    def fn():
        need = ops.png_labels_arena_bytes(SIZES)
        arena = torch.empty(need + 100, dtype=torch.uint8, device="cuda")
        ws = torch.empty(int(ops.lib().excel_png_labels_workspace_bytes(2, 40)), dtype=torch.uint8, device="cuda")
        return dict(fresh=ops.png_encode_labels_ragged(labels, plan), own=ops.png_encode_labels_ragged(labels, plan, out=arena, ws=ws), tail=arena[need:])
    # the returned view out[:need] is written in full (the arena is cleared up to the bound); the caller's bytes behind it are not touched
    return Case(fn, lambda path, t: t[:0] if "tail" in path else t, lambda r: [r["tail"]], n_ws=1)


def _jpeg(ops):
    """"the files lie back to back, file i = bytes[off_i:off_i + size_i]" (ops.jpeg_encode_rgb_ragged): the arena bytes behind the last
    file are not part of the result."""
    torch = _torch()
    rs = np.random.RandomState(19)
    items, off, rgb = [], 0, []
    for H, W in SIZES:
        rgb.append(np.clip(rs.randint(0, 256, (H, W, 3)) * 0.3 + np.linspace(0, 170, W)[None, :, None], 0, 255).astype(np.uint8).reshape(-1))
        items.append((off, H, W))
        off += 3 * H * W
    rgb = dev(np.concatenate(rgb), torch.uint8)

    def files(out, table):
        t = table.cpu().numpy()
        assert (t[:, 1] > 0).all()
        end = int(t[-1, 0] + t[-1, 1])
        return dict(bytes=out[:end], table=table, tail=out[end:])

    def fn():
        arena = torch.empty(ops.jpeg_rgb_arena_bytes(SIZES), dtype=torch.uint8, device="cuda")
        ws = torch.empty(ops.jpeg_rgb_workspace_bytes(SIZES), dtype=torch.uint8, device="cuda")
        return dict(fresh=files(*ops.jpeg_encode_rgb_ragged(rgb, items)), own=files(*ops.jpeg_encode_rgb_ragged(rgb, items, out=arena, ws=ws)))
    return Case(fn, lambda path, t: t[:0] if "tail" in path else t, lambda r: [r["fresh"]["tail"], r["own"]["tail"]], n_ws=1)


def _vit_f32(ops):
    """The exact-fp32 ViT (a_sum with pitch NP as the K tail of A_sum.V): S = 80 -> g = 5, N = 26.  The handle caches its workspace per
    stream, so it is poisoned in place like the attention test does."""
    from oracle.vit import VitConfig, make_vit_weights
    cfg = VitConfig(width=128, layers=8, heads=2, patch=16, out_dim=64, input_resolution=64, n_surgery=5)
    h = ops.VitHandle(make_vit_weights(cfg, seed=11), cfg.width, cfg.layers, cfg.heads, cfg.patch, cfg.out_dim, n_surgery=cfg.n_surgery, gemm_mode="f32")
    rs = np.random.RandomState(20)
    imgs = dev(rs.standard_normal((3, 3, 80, 80)).astype(np.float32))
    ex = dev(rs.rand(3, 25, 25).astype(np.float32) * 0.1)

    def fn():
        from _scratch import current_byte
        h.workspace(3, 80)[0].fill_(current_byte())
        r = h.forward(imgs, want_w_aff=True, aff_layers=6, n_attn_out=8, want_feats=True, want_raw=True)
        h.workspace(3, 80)[0].fill_(current_byte())
        return dict(plain=r, lvc=h.forward(imgs, want_w_aff=True, aff_layers=6, n_attn_out=2, want_feats=True, want_raw=True, ex_attn=ex,
                                           feats_as_reference=True))
    return Case(fn)


def _seg_ops(ops):
    rs = np.random.RandomState(21)
    plan = ops.RaggedPlan(SIZES, "cuda")
    dst = ops.RaggedPlan([(21, 35), (33, 27)], "cuda")
    nc = 5
    segs = [dev(rs.standard_normal((4, nc, g, g)).astype(np.float32)) for g in (5, 3, 7)]
    tight = dev(rs.standard_normal((2, nc, 5, 7)).astype(np.float32))

    def fn():
        planes, labels = ops.seg_msc_fuse_ragged(segs, [False, True, True], plan, want_planes=True, want_labels=True, label_hw=plan.hw)
        return dict(planes=planes, labels=labels, resized=ops.seg_resize_argmax_ragged(planes, plan, dst, nc),
                    uniform=ops.seg_resize_argmax_uniform(tight, dst), prob=ops.seg_softmax_resize(planes, plan, 1, nc, 33, 27),
                    prob_same=ops.seg_softmax_resize(planes, plan, 0, nc, *SIZES[0]), probs=ops.seg_softmax_resize_ragged(planes, plan, dst, nc))
    # seg_msc_fuse_ragged's planes: "the pad columns get the value of the clamped sample" (segeval.hip) - written, so nothing is masked
    return Case(fn)


def _input_ops(ops):
    torch = _torch()
    rs = np.random.RandomState(22)
    plan = ops.RaggedPlan(SIZES, "cuda")
    hwc = dev(rs.randint(0, 256, 3 * plan.total_label_pix).astype(np.uint8), torch.uint8)

    def fn():
        own = torch.empty((2, 3, 30, 30), dtype=torch.float32, device="cuda")
        own2 = torch.empty((4, 3, 30, 30), dtype=torch.float32, device="cuda")
        return dict(one=ops.normalize_resize_u8_ragged(hwc, plan, 30), one_own=ops.normalize_resize_u8_ragged(hwc, plan, 30, out=own),
                    mirror=ops.normalize_resize_u8_ragged_mirror(hwc, plan, 30), mirror_own=ops.normalize_resize_u8_ragged_mirror(hwc, plan, 30, out=own2))
    return Case(fn)


def _label_ops(ops):
    """cam_overlay_ragged, mode "max": "the bytes of an image with k_b = 0 are left unwritten" (ops.cam_overlay_ragged)."""
    torch = _torch()
    rs = np.random.RandomState(23)
    sizes = SIZES + [(9, 6)]
    plan = ops.RaggedPlan(sizes, "cuda")
    onehot = np.zeros((3, 6), np.float32)
    onehot[0, [1, 4]] = 1
    onehot[2, [0, 3, 5]] = 1                                                       # image 1 has no class: k_b = 0
    idx, ncls, nchan = ops.cls_compact(dev(onehot), 3, want_nchan=True)
    k = np.array([2, 0, 3])
    cams = dev(pitched(rs, plan, 4))
    tight = dev(rs.rand(3, 4, 17, 29).astype(np.float32))
    hwc = dev(rs.randint(0, 256, 3 * plan.total_label_pix).astype(np.uint8), torch.uint8)
    one = dev(rs.randint(0, 256, (17, 29, 3)).astype(np.uint8), torch.uint8)
    lo, hi = 3 * int(plan.loff[1]), 3 * int(plan.loff[2])
    cls = dev((rs.rand(3, 4) < 0.6).astype(np.float32))
    gt = dev(rs.randint(0, 8, plan.total_label_pix).astype(np.uint8), torch.uint8)

    def fn():
        lab = ops.argmax_label_ragged(cams, plan, 4, nchan, idx)
        own = torch.empty((plan.total_label_pix,), dtype=torch.uint8, device="cuda")
        return dict(ragged=lab, ragged_own=ops.argmax_label_ragged(cams, plan, 4, nchan, idx, out=own), tight=ops.argmax_label(tight, nchan, idx, want_i64=True), plain=ops.argmax_label(tight),
                    ov_max=ops.cam_overlay_ragged(hwc, cams, plan, 4, k, mode="max")[0], ov_cls=ops.cam_overlay_ragged(hwc, cams, plan, 4, k, mode="per_class")[0],
                    one_max=ops.cam_overlay(one, tight[0, :3], mode="max"), one_cls=ops.cam_overlay(one, tight[0, :3], mode="per_class"),
                    lam=ops.lam_to_label(tight, cls, img_box=np.array([[0, 17, 0, 29], [2, 9, 1, 20], [0, 4, 5, 29]], np.int32), high_thre=0.7,
                                         low_thre=0.25, ignore_mid=True),
                    lam_plain=ops.lam_to_label(tight, cls), hist=ops.confusion_accumulate(gt, lab, 8))

    def defined(path, t):
        return torch.cat([t[:lo], t[hi:]]) if "ov_max" in path else t
    return Case(fn, defined, lambda r: [r["ov_max"][lo:hi]])


def _train_panels(ops):
    torch = _torch()
    rs = np.random.RandomState(24)
    B, F, g, S = 3, 4, 3, 46                                                       # an odd batch (one empty grid cell), S % 4 != 0
    x = dev(rs.standard_normal((B, 3, S, S)).astype(np.float32))
    attr = dev(rs.uniform(-0.1, 1.1, (B, g * g, F)).astype(np.float32))
    cls = np.zeros((B, F), np.float32)
    for b in range(B):
        cls[b, [b % F, (b + 2) % F]] = 1
    labs = {n: dev(rs.randint(0, 21, (B, S, S)).astype(np.uint8), torch.uint8) for n in ("pseu_aff", "seg_gt", "seg_pred")}
    labs["pseu_mid"] = dev(rs.randint(0, 21, (B, g, g)).astype(np.uint8), torch.uint8)
    return Case(lambda: ops.train_panels(inputs=x, attr_maps_raw=attr, cls_label=dev(cls), **labs).buffer)


CASES = {
    "decoder": _decoder, "text": _text, "feature_affinity": _feature_affinity, "feature_affinity_grouped": _feature_affinity_grouped,
    "attn_means": _attn_means, "trans_mat": _trans_mat, "refine": _refine, "cam_upsample": _cam_upsample,
    "cam_upsample_ragged": _cam_upsample_ragged, "clip_feature_surgery": _clip_feature_surgery, "patch_text_cam": _patch_text_cam,
    "par_forward": _par_forward, "par_forward_ragged": _par_forward_ragged, "dcrf": _dcrf, "dcrf_ragged": _dcrf_ragged, "dcrf_lam": _dcrf_lam,
    "train_augment": _train_augment, "png": _png, "jpeg": _jpeg, "vit_f32": _vit_f32,
    # the same ops at the COCO class counts (Smax = 18, Cmax = 19; mixed counts with 18 and 1)
    "refine_many": lambda ops: _refine(ops, many=True), "cam_upsample_many": lambda ops: _cam_upsample(ops, many=True),
    "cam_upsample_ragged_many": lambda ops: _cam_upsample_ragged(ops, many=True), "par_forward_many": lambda ops: _par_forward(ops, many=True),
    "par_forward_ragged_many": lambda ops: _par_forward_ragged(ops, many=True),
    # no workspace: outputs only
    "seg_ops": _seg_ops, "input_ops": _input_ops, "label_ops": _label_ops, "train_panels": _train_panels,
}
