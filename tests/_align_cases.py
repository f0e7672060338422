"""Alignment table of tests/test_gpu_align_contract.py and tests/test_host_align_contract.py (importable without a GPU).

The third library-wide contract beside scratch memory (tests/_scratch_cases.py) and streams (tests/_stream_cases.py): where a tensor
starts in memory does not change a result.

  ops layer   every tensor argument of every function or method of excel_amd/ops.py that hands a pointer to the library may be a
              contiguous view that starts one element into its storage (buf[1:1 + n].view(shape)); the result has the bits of the
              call on freshly allocated tensors.  An argument the op WRITES either gives the same bits or is refused with a ValueError
              that names it, before anything is launched.
  C ABI       an entry called with a pointer below the alignment its comment in include/excel_hip.h states returns EXCEL_ERR_ARG, the
              error text names the argument, and nothing was launched.
  kernels     no kernel is launched on a pointer below the alignment its code assumes.

ALIGN has one row per op.  Row.args: entry -> {pointer argument: (bytes, the widest access made through it)}, found by reading the
launchers and kernels (file:line of the access, csrc/ relative).  "by element" means every access through the pointer is a plain
element access, so the element type's own alignment is all it needs; 16 / 8 above the element size means a vector cast, a 16-byte DMA
into LDS, a 64-bit atomic or a wider type carved from a workspace.  "guarded" names the run-time branch that keeps the wide access away
from a pointer that is not aligned.  Row.written: argument of the ops function that the op writes -> "same_bits" | "refused".
Row.parent: what held before the contract was pinned - "safe" (scalar or self-guarding kernels), "checked" (the library refused
the pointer already; ops passed the refusal on as a RuntimeError), "unguarded" (a misaligned pointer reached a vector access)."""
import contextlib
from collections import namedtuple

import _scratch_cases as SC
from _stream_cases import CASES, STREAM_COVERS  # noqa: F401  (the cases this contract runs: those of the stream contract)

Row = namedtuple("Row", "args written parent", defaults=({}, "safe"))

E = "by element"
WS4 = (4, "fp32 / int32 regions carved from it")


def _f(*names, why=E):
    """fp32 / int32 pointers that are touched by element"""
    return {n: (4, why) for n in names}


def _b(*names, why=E):
    """uint8 pointers: any byte"""
    return {n: (1, why) for n in names}


_WEIGHTS = (16, "GEMM B operand f32x4 (gemm.hip:70), ln_row f32x4 (norm.hip:34-35), split / pack kernels f32x4 (gemm_bf16x3.hip:429,448)")
_VIT_FWD = {"img": (16, "f32x4 load, norm.hip im2col_kernel:167"), "workspace": (16, "GEMM operands, 16 B LDS DMA (attn.hip, attn_strip.hip, gemm_bf16x3.hip:282)"),
            "image_features": (16, "f32x4 store, norm.hip token_axis_scale_kernel:151"),
            "x_raw": (16, "f32x4 store gemm_bf16x3.hip:174, f32x4 load norm.hip:145"),
            **_f("w_aff", "attn_out", "ex_attn", why="by element: attn.hip:471-498, attn_strip.hip:470-510, attn_f32.hip:268-292"),
            "feats_out": (4, "hipMemcpyAsync, vit.hip:388,426")}
_SPLIT_GEMM = {"A_split": (16, "16 B LDS DMA, gemm_bf16x3.hip:282"), "W_split": (16, "16 B LDS DMA, gemm_bf16x3.hip:282"),
               "C": (16, "f32x4 / 2 x 8 B stores, gemm_bf16x3.hip:174-192"), "bias": (16, "f32x4 load, gemm_bf16x3.hip:107"),
               "residual": (16, "f32x4 load, gemm_bf16x3.hip:147")}
_LABEL_PAIR = {**_b("gt", "pred", why="guarded: scalar head in front of the uint4 body, label_maps.h:17-28"), **_f("table", "skip")}
_DEC_WS = (16, "GEMM operands and LayerNorm rows carved from it")

ALIGN = {
    # ---- building blocks
    "gemm": Row({"excel_gemm_f32": {"A": (16, "f32x4 load, gemm.hip load_tile:61"), "Bm": (16, "f32x4 load, gemm.hip load_tile:70,80"),
                                    **_f("C", "bias", "residual", why="by element, gemm.hip:156-179")}}, parent="checked"),
    "split_bf16": Row({e: {"in": (16, "f32x4 load, gemm_bf16x3.hip split_bf16_kernel:429"), "out": (8, "8 B plane stores, gemm_bf16x3.hip:437-438")}
                       for e in ("excel_split_bf16", "excel_split_f16")}, parent="unguarded"),
    "pack_f16": Row({"excel_pack_f16": {"in": (16, "f32x4 load, gemm_bf16x3.hip pack_hi_kernel:448"), "out": (8, "8 B store, gemm_bf16x3.hip:455"),
                                        "inexact_dev": (8, "64-bit atomic counter")}}, parent="unguarded"),
    "gemm_bf16x3": Row({"excel_gemm_bf16x3": _SPLIT_GEMM, "excel_gemm_f16x3": _SPLIT_GEMM}, parent="unguarded"),
    "gemm_f16x2": Row({"excel_gemm_f16x2": {**_SPLIT_GEMM, "W_half": (2, "guarded: gemm_half_ok leaves a half matrix below 16 B unused, gemm_bf16x3.hip:530")}},
                      parent="unguarded"),
    "layernorm": Row({"excel_layernorm": {n: (16, "f32x4, norm.hip ln_row:17-45") for n in "xwby"}}, parent="unguarded"),
    # ---- handles
    "VitHandle.forward": Row({"excel_vit_create": {"weights": _WEIGHTS}, "excel_vit_forward_ex": _VIT_FWD}, parent="unguarded"),
    "DecoderHandle.forward": Row({"excel_decoder_create": {"weights": _WEIGHTS},
                                  "excel_decoder_forward": {"all_feats": (16, "GEMM A operand read in place, decoder.hip:158"), "workspace": _DEC_WS,
                                                            **_f("attn_fts_out", "seg_out", why="by element, decoder.hip dec_transpose")}},
                                 parent="checked"),
    "DecoderHandle.forward_train": Row({"excel_decoder_forward_train": {"all_feats": (16, "GEMM A operand read in place, train.hip:521"),
                                                                        "workspace": _DEC_WS, **_f("seg_out", "attn_pred_out")}}, parent="checked"),
    "DecoderHandle.train_attn_fts": Row({"excel_decoder_train_attn_fts": {"workspace": _DEC_WS, **_f("attn_fts_out")}}),
    "DecoderHandle.backward": Row({"excel_decoder_backward": {"all_feats": (4, "hipMemcpy2DAsync, train.hip:727"), "workspace": _DEC_WS,
                                                              **_f("d_seg", "d_attn_pred", "grads", why="by element: dec_transpose, tr_sigmoid_bwd, GEMM C stores")}}),
    "DecoderHandle.adamw_step": Row({"excel_adamw_step": _f("param", "grad", "exp_avg", "exp_avg_sq")}),
    "TextHandle.encode": Row({"excel_text_create": {"weights": _WEIGHTS},
                              "excel_text_encode": {"workspace": _DEC_WS, **_f("tokens", "out", why="by element, decoder.hip:196-205, GEMM C store")}}),
    "prompt_ensemble": Row({"excel_prompt_ensemble": _f("emb", "out", why="by element, decoder.hip prompt_ensemble_kernel")}),
    "train_losses": Row({"excel_train_losses": {**_f("seg", "attn_pred", "losses", "d_seg", "d_attn_pred"), **_b("pseudo", "aff_labels"),
                                                "workspace": (8, "double partial sums, train.hip:173")}}),
    # ---- image / label plumbing (attr.hip, par.hip argmax, camviz.hip, trainviz.hip: no vector access)
    "lam_to_label": Row({"excel_lam_to_label": {**_f("cam", "cls_label", "img_box", "valid_cam"), **_b("label")}}),
    "normalize_img_u8": Row({"excel_normalize_img_u8": {**_b("hwc"), **_f("out")}}),
    "denormalize_img": Row({"excel_denormalize_img": {**_f("img", "out_f32"), **_b("out_u8")}}),
    "seg_scale_accumulate": Row({"excel_seg_scale_accumulate": _f("segs", "acc")}, {"acc": "same_bits"}),
    "seg_msc_fuse_ragged": Row({"excel_seg_msc_fuse_ragged": {**_f("segs", "table"), "planes": (16, "f32x4 store, segeval.hip:95"), **_b("labels_u8")}},
                               parent="checked"),
    "seg_resize_argmax_ragged": Row({"excel_seg_resize_argmax_ragged": {**_f("planes", "src_table", "dst_table"), **_b("labels_u8")}}),
    "seg_resize_argmax_uniform": Row({"excel_seg_resize_argmax_uniform": {**_f("segs", "dst_table"), **_b("labels_u8")}}),
    "seg_softmax_resize": Row({"excel_seg_softmax_resize": _f("planes", "prob")}),
    "seg_softmax_resize_ragged": Row({"excel_seg_softmax_resize_ragged": _f("planes", "src_table", "dst_table", "prob")}),
    # ---- CAM
    "clip_feature_surgery": Row({"excel_clip_feature_surgery": {"image_features": (16, "GEMM A operand f32x4, gemm.hip:61"),
                                                                "text": (16, "GEMM B operand f32x4, gemm.hip:70"), "workspace": (16, "S: GEMM C, rows of ldT % 4 == 0"),
                                                                **_f("out_full", "out_slice", why="by element, cam.hip cam_epilogue_kernel")}}, parent="checked"),
    "patch_text_cam": Row({"excel_patch_text_cam": {"x_raw": (16, "f32x4 load, cam.hip:327"), "text": (16, "f32x4 load, cam.hip:153,253"),
                                                    "image_features": (16, "f32x4 store, cam.hip:388"), "workspace": (16, "16 B LDS DMA of the split text, cam.hip:340"),
                                                    **_f("out_full", "out_slice", why="by element, cam.hip patch_text_finish_kernel")}}, parent="checked"),
    # ---- affinity random walk (aff.hip, lvc.hip, abi.hip: no vector access; the GEMMs run on workspace buffers)
    "attn_layer_mean": Row({"excel_attn_layer_mean": _f("attn", "w_aff")}),
    "attn_select_mean": Row({"excel_attn_select_mean": {**_f("attn", "seg_attn", "w_out"), "workspace": (8, "double partial sums, lvc.hip:293")}}),
    "feature_affinity": Row({"excel_feature_affinity": {**_f("feats", "out"), "workspace": (16, "fn: both GEMM operands, lvc.hip:118; double partials")}}),
    "feature_affinity_grouped": Row({"excel_feature_affinity_grouped": {**_f("feats", "out"), "workspace": (16, "fn: both GEMM operands, lvc.hip:118")}},
                                    {"out": "same_bits"}),
    "compute_trans_mat": Row({"excel_compute_trans_mat": {**_f("w_aff", "trans_out"), "workspace": (16, "Tsym: both GEMM operands, abi.hip compute_trans_mat")}}),
    "cls_compact": Row({"excel_cls_compact": _f("onehot", "cls_idx", "ncls", "nchan")}),
    "scoremap_box_mask": Row({"excel_scoremap_box_mask": {**_f("attr", "cls_idx", "ncls", "v_out"), **_b("mask_out")}}),
    "refine_cams_with_aff_batched": Row({"excel_refine_cams_with_aff": {**_f("attr", "w_aff", "cls_idx", "ncls", "refined"), "workspace": WS4}}),
    "cam_upsample_bkg": Row({"excel_cam_upsample_bkg": {**_f("refined", "ncls", "cams"), "workspace": WS4}}, {"out": "same_bits"}),
    # ---- PAR / labels / metric
    "par_forward": Row({"excel_par_forward": {**_f("imgs", "masks", "out", why="guarded: aligned16 plans the streamed-plane kernels, abi.hip par_forward, par_plan.hip:39"),
                                              **_f("nchan"), "workspace": WS4}}, {"out": "same_bits", "ws": "refused"}),
    "par_forward_ragged": Row({"excel_par_forward_ragged": {**_f("imgs", "nchan", "table"), "masks": (16, "16 B buffer DMA into LDS, par.hip:253"),
                                                            "out": (16, "ping-pong partner of masks, par.hip:253"),
                                                            "workspace": (16, "statistics and guide staged 16 B at a time, par.hip:253,451")}},
                              {"out": "refused", "ws": "refused"}, parent="checked"),
    "argmax_label": Row({"excel_argmax_label": {**_f("cams", "nchan", "cls_idx"), **_b("labels_u8"), "labels_i64": (8, "by element (int64)")}}),
    "argmax_label_ragged": Row({"excel_argmax_label_ragged": {**_f("cams", "nchan", "cls_idx", "table"), **_b("labels_u8")}}, {"out": "same_bits"}),
    "confusion_accumulate": Row({"excel_confusion_accumulate": {**_b("gt", "pred", why=_LABEL_PAIR["gt"][1]), "hist": (8, "64-bit atomic adds (int64)")}},
                                {"hist": "same_bits"}),
    "confusion_accumulate_masked": Row({"excel_confusion_accumulate_masked": {**_LABEL_PAIR, "hist": (8, "64-bit atomic adds (int64)")}}, {"hist": "same_bits"}),
    # (the helper of the three ops above: it hands the plan's table to whichever of their entries the caller runs)
    "_label_pair": Row({e: _f("table") for e in ("excel_confusion_accumulate_masked", "excel_image_scores", "excel_boundary_scores")}),
    "nonfinite_count": Row({"excel_nonfinite_count": {"x": (4, "guarded: scalar head in front of the uint4 body, guard.hip:24-33"), **_f("count")}},
                           {"out": "same_bits"}),
    "clip_tags": Row({"excel_clip_tags": {"x_cls": (16, "float4 load, tag.hip:50"), "text": (16, "float4 load, tag.hip:61"), **_f("onehot_out", "scores_out")}},
                     parent="checked"),
    "image_scores": Row({"excel_image_scores": {**_LABEL_PAIR, **_f("counts")}}, {"out": "same_bits"}),
    "boundary_scores": Row({"excel_boundary_scores": {**_b("gt", "pred", why="guarded: rows staged from their own 4-byte boundary, boundary.hip:72-84"),
                                                      **_f("table", "radius", "skip", "counts")}}, {"out": "same_bits"}),
    # ---- ragged batches
    "normalize_resize_u8_ragged": Row({"excel_normalize_resize_u8_ragged": {**_b("hwc"), **_f("table", "out")}}, {"out": "same_bits"}),
    "normalize_resize_u8_ragged_mirror": Row({"excel_normalize_resize_u8_ragged_mirror": {**_b("hwc"), **_f("table", "out")}}, {"out": "same_bits"}),
    "cam_upsample_bkg_ragged": Row({"excel_cam_upsample_bkg_ragged": {**_f("refined", "ncls", "table"), "cams": (16, "the pitched layout's premise: every row on a 16 B boundary"),
                                                                      "workspace": WS4}}, {"out": "refused"}, parent="checked"),
    "conf_planes_ragged": Row({"excel_conf_planes_ragged": _f("cams", "nchan", "src_table", "half_table", "planes", "nchan2")}, {"out": "same_bits"}),
    "conf_merge_ragged": Row({"excel_conf_merge_ragged": {**_f("planes", "nchan", "cls_idx", "half_table", "dst_table", "img_box"), **_b("labels_u8")}},
                             {"out": "same_bits"}),
    "cam_overlay_ragged": Row({"excel_cam_overlay_ragged": {**_b("hwc", "out"), **_f("cams", "ncls", "table"), "out_off": (8, "by element (int64)"),
                                                            "tables": (8, "by element (double)")}}),
    "cam_overlay": Row({"excel_cam_overlay": {**_b("hwc", "out"), **_f("cams"), "tables": (8, "by element (double)")}}),
    "train_panels": Row({"excel_train_panels": {**_f("img", "attr", "cls_label"), **_b("pseu_aff", "pseu_mid", "seg_gt", "seg_pred", "palette", "out"),
                                                "jet": (8, "by element (double)")}}),
    "png_encode_labels_ragged": Row({"excel_png_encode_labels_ragged": {**_b("labels", "palette"), **_f("table"), "arena": (4, "cleared and filled in 32-bit words, png.hip:351"),
                                                                        "out_table": (8, "by element (int64)"), "workspace": (8, "uint2 row records, png.hip:345")}},
                                    {"out": "refused", "ws": "refused"}, parent="checked"),
    "jpeg_encode_rgb_ragged": Row({"excel_jpeg_encode_rgb_ragged": {**_b("rgb", "arena"), "out_table": (8, "by element (int64)"),
                                                                    "workspace": (16, "uint4 chunks of stream words, jpeg.hip:421")}},
                                  {"out": "same_bits", "ws": "refused"}, parent="checked"),
    "train_augment": Row({"excel_train_augment": {**_b("hwc", "labels", "label"), **_f("table", "img", "img_box"), "workspace": WS4}}),
    "train_augment_image": Row({"excel_train_augment_image": {**_b("hwc"), **_f("table", "img", "img_box"), "workspace": WS4}}),
    # ---- DenseCRF (crf.hip: no vector access; the batch entries take slices of the batch's tensors)
    "dcrf_inference": Row({"excel_dcrf_inference": {**_b("rgb_hwc"), **_f("prob", "q_out"), "workspace": (8, "64-bit accumulators, crf.hip:439")}}),
    "dcrf_inference_ragged": Row({"excel_dcrf_inference_ragged": {**_b("hwc", "labels_u8"), **_f("unary", "table", "q_out"),
                                                                  "workspace": (8, "64-bit accumulators, crf.hip:439")}}),
    "dcrf_lam_ragged": Row({"excel_dcrf_lam_ragged": {**_b("hwc", "labels_u8"), **_f("cams", "nchan", "cls_idx", "table", "q_out"),
                                                      "workspace": (8, "64-bit accumulators, crf.hip:439")}}),
    # ---- one-time / auxiliary (attr.hip, vit.hip pos_resize, tta.hip: no vector access)
    "attr_aggregate": Row({"excel_attr_aggregate": _f("text", "bank", "out")}),
    "bilinear_resize": Row({"excel_bilinear_resize": _f("in", "out")}),
    "pos_embed_resize": Row({"excel_pos_embed_resize": _f("pos", "out")}),
    "flip_max_normalize": Row({"excel_flip_max_normalize": _f("attr", "out")}),
    "lam_scale_accumulate": Row({"excel_lam_scale_accumulate": _f("maps", "acc")}, {"acc": "same_bits"}),
    "plane_minmax_normalize_": Row({"excel_plane_minmax_normalize": _f("lam")}, {"lam": "same_bits"}),
    "lam_tta_fuse": Row({"excel_lam_tta_fuse": _f("maps", "out")}, {"out": "same_bits"}),
}

GUARDED = "guarded"      # a reason that starts with this word: a run-time branch, not a refusal, keeps the wide access away


def above_4():
    """[(entry, argument, bytes)]: every pointer ALIGN holds to more than 4 bytes, which its entry refuses when it is 4 bytes (2 for
    the 16-bit planes, 1 for the uint8 workspaces) further on; the guarded ones are left out.  "weights" stands for every pointer of a
    *_create entry's weight table."""
    out = []
    for row in ALIGN.values():
        for entry, args in row.args.items():
            for name, (nbytes, why) in args.items():
                if nbytes > 4 and not why.startswith(GUARDED) and (entry, name, nbytes) not in out:
                    out.append((entry, name, nbytes))
    return out


# ------------------------------------------------------------------ tensors one element into their storage
def shifted(t, device=None):
    """A copy of `t` that is a contiguous view starting at element 1 of a fresh buffer of numel + 1 elements of t's dtype: the buffer is
    aligned to 16 bytes or more, so the view starts itemsize bytes past a 16-byte boundary.  The bytes are compared after the copy."""
    import torch
    device = t.device if device is None else torch.device(device)
    t = t.contiguous()
    buf = torch.empty(t.numel() + 1, dtype=t.dtype, device=device)
    assert buf.data_ptr() % 16 == 0, "a fresh allocation is expected on a 16-byte boundary"
    v = buf[1:].view(t.shape)
    v.copy_(t)
    assert v.is_contiguous() and v.shape == t.shape and v.dtype == t.dtype
    assert v.data_ptr() % 16 == t.element_size() % 16, (v.data_ptr() % 16, t.element_size())
    same = lambda a: a.cpu().contiguous().view(-1).view(torch.uint8)
    assert torch.equal(same(v), same(t)), "the shifted upload changed the bytes"
    return v


@contextlib.contextmanager
def shifted_uploads():
    """While the block is active, the cases' uploader (tests/_scratch_cases.py dev, which pitched / pitched_mask and tests/_stream_cases.py
    go through) returns shifted() tensors.  Outside it the builds are what the scratch and stream tests run."""
    SC.UPLOADER.append(shifted)
    try:
        yield
    finally:
        SC.UPLOADER.pop()
