"""Case table of tests/test_gpu_stream_contract.py (importable without a GPU: the host completeness test reads STREAM_COVERS).

Every function or method of excel_amd/ops.py that passes _stream() to the library is named in STREAM_COVERS with the cases that run it.
The workspace users and the output-only ops of tests/_scratch_cases.py are reused as they are; the cases below add the remaining
launchers.  A case is build(ops) -> Case(fn, defined): build uploads seeded inputs and creates handles and plans on the default
stream, fn() only calls ops (and the torch copies that put a handle's state back) and returns a tree of device tensors.  Shapes
are the smallest the op accepts that still make it launch every kernel it has (g = 5 or 6, images of SIZES, nc = 21, B = 2-4; the
GEMMs at the first two shapes of test_gemm_bf16x3): a case takes milliseconds.

Documented host reads (the op synchronises ITS OWN stream, which the contract allows): pack_f16 returns the inexact count as a Python
int (gemm_family); lam_to_label and dcrf_lam_ragged's case upload small host arrays from pageable memory."""
import numpy as np

from _scratch_cases import CASES as SCRATCH_CASES
from _scratch_cases import SIZES, Case, decoder_handle, decoder_weights, dev, pitched, pitched_mask

STREAM_COVERS = {
    # ---- the cases of tests/_scratch_cases.py
    "DecoderHandle.forward": ["decoder"],
    "TextHandle.encode": ["text"],
    "feature_affinity": ["feature_affinity"],
    "feature_affinity_grouped": ["feature_affinity_grouped"],
    "attn_select_mean": ["attn_means"],
    "attn_layer_mean": ["attn_means"],
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
    "VitHandle.forward": ["vit_f32", "vit_split"],
    "seg_msc_fuse_ragged": ["seg_ops"],
    "seg_resize_argmax_ragged": ["seg_ops"],
    "seg_resize_argmax_uniform": ["seg_ops"],
    "seg_softmax_resize": ["seg_ops"],
    "seg_softmax_resize_ragged": ["seg_ops"],
    "normalize_resize_u8_ragged": ["input_ops"],
    "normalize_resize_u8_ragged_mirror": ["input_ops"],
    "argmax_label_ragged": ["label_ops"],
    "argmax_label": ["label_ops"],
    "cam_overlay_ragged": ["label_ops"],
    "cam_overlay": ["label_ops"],
    "lam_to_label": ["label_ops"],
    "confusion_accumulate": ["label_ops"],
    "train_panels": ["train_panels"],
    # ---- the cases below
    "gemm": ["gemm_family"],
    "split_bf16": ["gemm_family"],
    "gemm_bf16x3": ["gemm_family"],
    "pack_f16": ["gemm_family"],
    "gemm_f16x2": ["gemm_family"],
    "layernorm": ["gemm_family"],
    "prompt_ensemble": ["text_attr"],
    "attr_aggregate": ["text_attr"],
    "normalize_img_u8": ["image_io"],
    "denormalize_img": ["image_io"],
    "seg_scale_accumulate": ["image_io"],
    "bilinear_resize": ["image_io"],
    "pos_embed_resize": ["image_io"],
    "cls_compact": ["cam_misc"],
    "scoremap_box_mask": ["cam_misc"],
    "flip_max_normalize": ["cam_misc"],
    "lam_scale_accumulate": ["cam_misc"],
    "plane_minmax_normalize_": ["cam_misc"],
    "lam_tta_fuse": ["cam_misc"],
    "conf_planes_ragged": ["conf_labels"],
    "conf_merge_ragged": ["conf_labels"],
    "confusion_accumulate_masked": ["scores"],
    "nonfinite_count": ["scores"],
    "clip_tags": ["scores"],
    "image_scores": ["scores"],
    "boundary_scores": ["scores"],
    "DecoderHandle.forward_train": ["train"],
    "DecoderHandle.train_attn_fts": ["train"],
    "DecoderHandle.backward": ["train"],
    "DecoderHandle.adamw_step": ["train"],
    "train_losses": ["train"],
}

GEMM_SHAPES = [(128, 128, 32), (300, 64, 512)]          # the first two of test_gemm_bf16x3: one tile, and a ragged M with a long K


def _torch():
    import torch
    return torch


def _gemm_family(ops):
    """Every building block at both shapes: the exact-fp32 GEMM (NT, and batched NN with a shared B), both split types, the three- and
    the two-product GEMM with every epilogue (plain, bias + QuickGELU + residual, split output), pack_f16 (whose count is read on the
    host: the op synchronises its own stream) and LayerNorm."""
    rs = np.random.RandomState(30)
    ins = []
    for M, N, K in GEMM_SHAPES:
        A = dev(rs.standard_normal((M, K)).astype(np.float32))
        W = dev((rs.standard_normal((N, K)) * 0.05).astype(np.float16).astype(np.float32))          # fp16-valued: gemm_f16x2's precondition
        ins.append((A, W, dev(rs.standard_normal(N).astype(np.float32)), dev(rs.standard_normal((M, N)).astype(np.float32)),
                    dev(rs.standard_normal((2, M, K)).astype(np.float32)), dev(rs.standard_normal((2, K, N)).astype(np.float32)),
                    dev(1 + 0.1 * rs.standard_normal(K).astype(np.float32)), dev(rs.standard_normal(K).astype(np.float32))))

    def fn():
        r = {}
        for (M, N, K), (A, W, bias, res, A3, Bkn, lw, lb) in zip(GEMM_SHAPES, ins):
            r[M, "f32"] = ops.gemm(A, W, bias=bias, residual=res, act=1)
            r[M, "f32_batched_nn"] = ops.gemm(A3, Bkn, b_kmajor=False)
            r[M, "ln"] = ops.layernorm(A, lw, lb)
            for f16 in (False, True):
                As, Ws = ops.split_bf16(A, f16=f16), ops.split_bf16(W, f16=f16)
                r[M, f16, "As"], r[M, f16, "Ws"] = As, Ws
                r[M, f16, "plain"] = ops.gemm_bf16x3(As, Ws, f16=f16)
                r[M, f16, "epi"] = ops.gemm_bf16x3(As, Ws, bias=bias, residual=res, act=1, f16=f16)
                r[M, f16, "split"] = ops.gemm_bf16x3(As, Ws, bias=bias, split_out=True, f16=f16)
            Wh, inexact = ops.pack_f16(W)
            assert inexact == 0
            r[M, "Wh"] = Wh
            r[M, "x2"] = ops.gemm_f16x2(As, Ws, bias=bias, residual=res, act=1)
            r[M, "x2_half"] = ops.gemm_f16x2(As, Ws, W_half=Wh)
            r[M, "x2_split"] = ops.gemm_f16x2(As, Ws, W_half=Wh, bias=bias, split_out=True)
        return r
    return Case(fn)


def _text_attr(ops):
    rs = np.random.RandomState(31)
    emb = dev(rs.standard_normal((7, 32)).astype(np.float32))
    text = rs.standard_normal((9, 32)).astype(np.float32)
    text = dev(text / np.linalg.norm(text, axis=1, keepdims=True))
    bank = rs.standard_normal((32, 16)).astype(np.float32)
    bank = dev(bank / np.linalg.norm(bank, axis=0, keepdims=True))
    return Case(lambda: dict(ensemble=ops.prompt_ensemble(emb), attr=ops.attr_aggregate(text, bank, 4)))


def _image_io(ops):
    torch = _torch()
    rs = np.random.RandomState(32)
    H, W = SIZES[0]
    u8 = dev(rs.randint(0, 256, (2, 11, 7, 3)).astype(np.uint8), torch.uint8)
    x = dev(rs.standard_normal((2, 3, 9, 13)).astype(np.float32))
    segs = dev(rs.standard_normal((4, 21, 5, 5)).astype(np.float32))                # [2B, nc, g, g]
    segs3 = dev(rs.standard_normal((4, 21, 3, 3)).astype(np.float32))
    small = dev(rs.standard_normal((2, 3, 5, 7)).astype(np.float32))
    pos = dev(rs.standard_normal((4 * 4 + 1, 8)).astype(np.float32))

    def fn():
        acc = ops.seg_scale_accumulate(segs, None, H, W, flip_mean=True, init=True)
        first = acc.clone()
        return dict(norm=ops.normalize_img_u8(u8), denorm=ops.denormalize_img(x), denorm_f=ops.denormalize_img(x, as_float=True),
                    first=first, acc=ops.seg_scale_accumulate(segs3, acc, H, W, flip_mean=False, init=False, scale=0.5),
                    up=ops.bilinear_resize(small, H, W), up_ac=ops.bilinear_resize(small, H, W, align_corners=True),
                    down=ops.bilinear_resize(small, 3, 4), pos=ops.pos_embed_resize(pos, 5))
    return Case(fn)


def _cam_misc(ops):
    rs = np.random.RandomState(33)
    H, W = SIZES[0]
    onehot = np.zeros((3, 6), np.float32)
    onehot[0, [1, 4]] = 1
    onehot[1, [2]] = 1
    onehot[2, [0, 3, 5]] = 1
    onehot = dev(onehot)
    attr = dev(rs.rand(3, 25, 6).astype(np.float32))
    m5 = dev(rs.rand(6, 25, 4).astype(np.float32))                                 # [2B, P, F]: image, then its mirrored input
    m3 = dev(rs.rand(6, 9, 4).astype(np.float32))

    def fn():
        idx, ncls, nchan = ops.cls_compact(onehot, 3, want_nchan=True)
        idx2, ncls2 = ops.cls_compact(onehot, 3)
        acc = ops.lam_scale_accumulate(m5, None, 5, H, W, init=True)
        first = acc.clone()
        acc = ops.lam_scale_accumulate(m3, acc, 3, H, W, init=False)
        return dict(idx=idx, ncls=ncls, nchan=nchan, idx2=idx2, ncls2=ncls2, box=ops.scoremap_box_mask(attr, idx, ncls, 5, want_mask=True),
                    box_plain=ops.scoremap_box_mask(attr, idx, ncls, 5)[0], flip=ops.flip_max_normalize(m5, 5), first=first, acc=acc,
                    normed=ops.plane_minmax_normalize_(acc.clone()), tta=ops.lam_tta_fuse([m5, m3], (5, 3), 5, True),
                    tta_noflip=ops.lam_tta_fuse([m5, m3], (5, 3), 5, False))
    return Case(fn)


def _conf_labels(ops):
    """conf_planes_ragged: "Planes >= nchan2[b] and the pad columns are not written" (ops.conf_planes_ragged): the hole of its output.
    conf_merge_ragged reads exactly the written part (planes < 2 nchan[b], columns < W_b), so it takes the planes as they are."""
    rs = np.random.RandomState(34)
    smax = 3
    sizes = SIZES + [(9, 6)]
    plan = ops.RaggedPlan(sizes, "cuda")
    half = ops.conf_half_plan(plan)
    counts = np.array([2, 1, 3], np.int32)
    onehot = np.zeros((3, 6), np.float32)
    onehot[0, [1, 4]] = 1
    onehot[1, [2]] = 1
    onehot[2, [0, 3, 5]] = 1
    idx, _ = ops.cls_compact(dev(onehot), smax)
    cams = dev(pitched(rs, plan, smax + 1))
    nchan = dev(counts + 1)
    box = dev(np.array([[0, 17, 0, 29], [2, 30, 1, 20], [0, 4, 2, 6]], np.int32))
    written = dev(pitched_mask(half, 2 * (smax + 1), 2 * (counts + 1)))

    def fn():
        planes, nchan2 = ops.conf_planes_ragged(cams, plan, half, smax, nchan, 0.7, 0.25)
        raw, _ = ops.conf_planes_ragged(cams, plan, half, smax, nchan, 0.7, 0.25, softmax=False)
        return dict(planes=planes, nchan2=nchan2, raw_first_group=raw, merged=ops.conf_merge_ragged(planes, half, plan, smax, nchan, idx, img_box=box),
                    merged_plain=ops.conf_merge_ragged(planes, half, plan, smax, nchan))

    first_group = dev(pitched_mask(half, 2 * (smax + 1), counts + 1))

    def defined(path, t):
        if "'planes'" in path:
            return t[written]
        return t[first_group] if "'raw_first_group'" in path else t
    return Case(fn, defined)


def _scores(ops):
    torch = _torch()
    rs = np.random.RandomState(35)
    nc = 21
    sizes = SIZES + [(9, 6)]
    plan = ops.RaggedPlan(sizes, "cuda")
    gt = rs.randint(0, nc, plan.total_label_pix).astype(np.uint8)
    gt[rs.rand(gt.size) < 0.1] = 255
    pred = np.where(rs.rand(gt.size) < 0.7, gt, rs.randint(0, nc, gt.size)).astype(np.uint8)
    gt, pred = dev(gt, torch.uint8), dev(pred, torch.uint8)
    ugt, upred = dev(rs.randint(0, nc, (3, 17, 29)).astype(np.uint8), torch.uint8), dev(rs.randint(0, nc, (3, 17, 29)).astype(np.uint8), torch.uint8)
    skip = dev(np.array([0, 1, 0], np.int32))
    radii = dev(np.array([2, 1, 3], np.int32))
    x = rs.standard_normal((3, 26, 32)).astype(np.float32)
    bad = x.copy()
    bad[1, 3, 5], bad[2, 0, 0], bad[2, 25, 31] = np.nan, np.inf, -np.inf
    x, bad = dev(x), dev(bad)
    text = dev(rs.standard_normal((9, 32)).astype(np.float32))

    def fn():
        count = ops.nonfinite_count(bad)
        first = count.clone()
        return dict(first=first, count=ops.nonfinite_count(x, out=count, init=False), tags=ops.clip_tags(x, text, 4, kmax=3),
                    tags_compact=ops.clip_tags(x[:, 0].contiguous(), text, 4, kmax=2, want_scores=False)[0],
                    hist=ops.confusion_accumulate_masked(gt, pred, nc, skip, plan=plan), hist_u=ops.confusion_accumulate_masked(ugt, upred, nc, skip),
                    scores=ops.image_scores(gt, pred, nc, skip=skip, plan=plan), scores_u=ops.image_scores(ugt, upred, nc),
                    band=ops.boundary_scores(gt, pred, nc, [2, 1, 3], skip=skip, plan=plan), band_dev=ops.boundary_scores(gt, pred, nc, radii, plan=plan),
                    band_u=ops.boundary_scores(ugt, upred, nc, 2))
    return Case(fn)


def _vit_split(ops):
    """VitHandle.forward in a split-plane mode (bf16x3: the strip attention kernel and the split GEMMs; the table's other ViT case is
    exact fp32), S = 80 -> g = 5, N = 26, with and without the LVC cue.  The handle caches its workspace per stream, so it is poisoned
    in place as in the vit_f32 case."""
    from oracle.vit import VitConfig, make_vit_weights
    cfg = VitConfig(width=128, layers=8, heads=2, patch=16, out_dim=64, input_resolution=64, n_surgery=5)
    h = ops.VitHandle(make_vit_weights(cfg, seed=11), cfg.width, cfg.layers, cfg.heads, cfg.patch, cfg.out_dim, n_surgery=cfg.n_surgery, gemm_mode="bf16x3")
    assert h.gemm_mode() == "bf16x3"
    rs = np.random.RandomState(36)
    imgs = dev(rs.standard_normal((3, 3, 80, 80)).astype(np.float32))
    ex = dev(rs.rand(3, 25, 25).astype(np.float32) * 0.1)

    def fn():
        from _scratch import current_byte
        h.workspace(3, 80)[0].fill_(current_byte())
        r = h.forward(imgs, want_w_aff=True, aff_layers=6, n_attn_out=8, want_feats=True, want_raw=True)
        h.workspace(3, 80)[0].fill_(current_byte())
        return dict(plain=r, lvc=h.forward(imgs, want_w_aff=True, aff_layers=6, n_attn_out=2, want_feats=True, want_raw=True, ex_attn=ex,
                                           feats_as_reference=True), raw_only=h.forward(imgs, want_w_aff=False, want_raw=True, want_features=False))
    return Case(fn)


def _train(ops):
    """One training iteration of the decoder head: forward_train (Dropout2d on), train_losses, train_attn_fts, backward, adamw_step, at
    g = 6 (P = 36, P % 4 == 0).  adamw_step changes the handle's parameters and moments, and backward writes into the handle's one
    gradient buffer, so fn() first puts all three back to where the reference run found them (torch copies on the current stream) and
    returns clones of what the handle keeps."""
    torch = _torch()
    rs = np.random.RandomState(37)
    h = decoder_handle(ops, decoder_weights(rs))                                   # L = 3, D = 64, E = 32, nc = 21, 2 blocks, 8 heads
    B, g = 2, 6
    feats = dev(rs.standard_normal((3, B, g * g + 1, 64)).astype(np.float32))
    pseudo = np.repeat(np.repeat(rs.randint(0, 4, (B, g, g)), 16, 1), 16, 2).astype(np.uint8)      # class blobs on the token grid ...
    pseudo[:, ::7, ::5] = 255                                                                        # ... and scattered ignored pixels
    pseudo = dev(pseudo, torch.uint8)
    w0 = {k: v.clone() for k, v in h.t.items()}
    h._grad_table()

    def fn():
        from _scratch import current_byte, fill_bytes
        for k, v in h.t.items():
            v.copy_(w0[k])
        if getattr(h, "_adam", None) is not None:
            for m, v in h._adam.values():
                m.zero_()
                v.zero_()
        fill_bytes(h.grad_flat, current_byte())                                    # backward writes every gradient: none keeps this byte
        seg, ap, ctx = h.forward_train(feats, dropout_p=0.1, dropout_seed=3)
        losses, d_seg, d_ap = ops.train_losses(seg, ap, pseudo, radius=3)
        fts = h.train_attn_fts(ctx)
        grads = {k: v.clone() for k, v in h.backward(ctx, d_seg, d_ap).items()}
        h.adamw_step(1e-3, 1)
        return dict(seg=seg, attn_pred=ap, losses=losses, d_seg=d_seg, d_attn_pred=d_ap, attn_fts=fts, grads=grads,
                    params={k: v.clone() for k, v in h.t.items()}, moments={k: (m.clone(), v.clone()) for k, (m, v) in h._adam.items()})
    return Case(fn)


CASES = dict(SCRATCH_CASES)
CASES.update({"gemm_family": _gemm_family, "text_attr": _text_attr, "image_io": _image_io, "cam_misc": _cam_misc, "conf_labels": _conf_labels,
              "scores": _scores, "vit_split": _vit_split, "train": _train})
