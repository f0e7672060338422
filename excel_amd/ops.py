"""torch.Tensor-facing wrappers of the C ABI (device memory + stream plumbing only).

Every function here hands raw device pointers of CUDA(=HIP) tensors to
libexcel_hip; nothing is computed with torch ops.  Tensors must be fp32,
contiguous and on the GPU; outputs are fresh tensors.
"""
import ctypes as C
import os

import torch

from . import _lib
from ._lib import check, lib

PAR_DILATIONS = (1, 2, 4, 8, 12, 24)


def _p(t, dtype=torch.float32):
    if t is None:
        return None
    if not t.is_cuda:
        raise RuntimeError("excel_amd ops need GPU tensors (the HIP library is the only compute path)")
    if t.dtype != dtype:
        raise TypeError(f"expected {dtype}, got {t.dtype}")
    if not t.is_contiguous():
        raise ValueError("tensor must be contiguous")
    return C.c_void_p(t.data_ptr())


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _ws(nbytes, device):
    return torch.empty(max(int(nbytes), 256), dtype=torch.uint8, device=device)


def _realign(t, align=16):
    """An INPUT of an op whose kernels read `align` bytes at a time (the per-op audit is tests/_align_cases.py): `t` itself when it
    starts on such a boundary - one integer test, nothing else - and otherwise a copy in fresh storage, which the allocator aligns to
    256 bytes or more.  A contiguous view into a pooled buffer (buf[1:1 + n].view(shape)) is the case: same values, same kernels, same
    bits.  The copy is queued on the current stream like the launch that reads it."""
    if t is None or t.data_ptr() % align == 0:
        return t
    return t.clone(memory_format=torch.contiguous_format)


def _written(t, who, name, align=16):
    """An argument the op WRITES cannot be copied: one that starts below the alignment the kernels assume is refused here, by name,
    before anything is allocated or launched."""
    if t is not None and t.data_ptr() % align:
        raise ValueError(f"{who}: {name} must be {align}-byte aligned (it starts {t.data_ptr() % align} bytes past a {align}-byte boundary: "
                         "a view into a larger buffer?); the kernels write it in wider pieces and it cannot be copied")
    return t


def f32c(t, align=4):
    """fp32 and contiguous; align=16 for the inputs of ops whose kernels read 16 bytes at a time (_realign)."""
    t = t.to(dtype=torch.float32).contiguous()
    return t if align <= 4 else _realign(t, align)


# ------------------------------------------------------------------ building blocks
def gemm(A, Bm, bias=None, residual=None, act=0, b_kmajor=True):
    """C = act(A @ op(B) + bias) + residual.  A [M,K] (or [batch,M,K]); B [N,K] if b_kmajor else [K,N]."""
    batched = A.dim() == 3
    A3 = _realign(A if batched else A[None])         # both operands are loaded 16 bytes at a time; C, bias and residual by element
    B3 = _realign(Bm if Bm.dim() == 3 else Bm[None])
    batch, M, K = A3.shape
    N = B3.shape[1] if b_kmajor else B3.shape[2]
    out = torch.empty((batch, M, N), dtype=torch.float32, device=A.device)
    sB = 0 if B3.shape[0] == 1 else B3.stride(0)
    check(lib().excel_gemm_f32(_p(A3), _p(B3), _p(out), _p(bias), _p(residual), M, N, K, A3.stride(1), B3.stride(1), N,
                               N, 1 if b_kmajor else 0, act, batch, A3.stride(0), sB, M * N, M * N, _stream()), "excel_gemm_f32")
    return out if batched else out[0]


GEMM_MODES = {"f32": 0, "bf16x3": 1, "f16x3": 2, "f16x2": 3}      # excel_vit_set_gemm_mode (include/excel_hip.h)


def split_bf16(x, f16=False):
    """fp32 [R,K] -> split operand [R,2,K] (bf16 - or, with f16, IEEE-half - bit patterns in an int16 tensor)."""
    x = f32c(x, 16)
    R, K = x.shape
    out = torch.empty((R, 2, K), dtype=torch.int16, device=x.device)
    fn = lib().excel_split_f16 if f16 else lib().excel_split_bf16
    check(fn(_p(x), _p(out, torch.int16), R, K, _stream()), "excel_split_f16" if f16 else "excel_split_bf16")
    return out


def gemm_bf16x3(A_split, W_split, bias=None, residual=None, act=0, split_out=False, f16=False):
    """C = act(A . W^T + bias) + residual from two split operands (three 16-bit MFMAs per product); f16: IEEE-half planes (split_bf16(f16=True))."""
    # 16-byte DMA of the operands into LDS; the epilogue reads bias and residual 16 bytes at a time
    A_split, W_split, bias, residual = _realign(A_split), _realign(W_split), _realign(bias), _realign(residual)
    M, _, K = A_split.shape
    N = W_split.shape[0]
    out = torch.empty((M, N), dtype=torch.float32, device=A_split.device)
    fn = lib().excel_gemm_f16x3 if f16 else lib().excel_gemm_bf16x3
    check(fn(_p(A_split, torch.int16), _p(W_split, torch.int16), _p(out), _p(bias), _p(residual), M, N, K, act,
             1 if split_out else 0, _stream()), "excel_gemm_f16x3" if f16 else "excel_gemm_bf16x3")
    return out.view(torch.int16).view(M, 2, N) if split_out else out


def pack_f16(x):
    """fp32 [R,K] -> (the hi plane as a plain IEEE-half matrix [R,K] (int16 bit patterns), number of elements NOT representable in
    half).  The second value is 0 exactly when `x` is fp16-valued - the precondition of gemm_f16x2 (every published CLIP archive)."""
    x = f32c(x, 16)
    R, K = x.shape
    out = torch.empty((R, K), dtype=torch.int16, device=x.device)
    cnt = torch.zeros(1, dtype=torch.int64, device=x.device)
    check(lib().excel_pack_f16(_p(x), _p(out, torch.int16), R, K, _p(cnt, torch.int64), _stream()), "excel_pack_f16")
    return out, int(cnt.item())


def gemm_f16x2(A_split, W_split, W_half=None, bias=None, residual=None, act=0, split_out=False):
    """gemm_bf16x3(..., f16=True) for fp16-VALUED weights (the lo plane of W_split is all zero): two MFMAs per product, the same bits.
    W_half (pack_f16 of the same weights) lets the large-tile kernel stream half the weight bytes."""
    # as gemm_bf16x3; W_half goes as it is: the library leaves a half matrix below 16 bytes unused (the split weights serve, same bits)
    A_split, W_split, bias, residual = _realign(A_split), _realign(W_split), _realign(bias), _realign(residual)
    M, _, K = A_split.shape
    N = W_split.shape[0]
    out = torch.empty((M, N), dtype=torch.float32, device=A_split.device)
    check(lib().excel_gemm_f16x2(_p(A_split, torch.int16), _p(W_split, torch.int16), _p(W_half, torch.int16) if W_half is not None else None,
                                 _p(out), _p(bias), _p(residual), M, N, K, act, 1 if split_out else 0, _stream()), "excel_gemm_f16x2")
    return out.view(torch.int16).view(M, 2, N) if split_out else out


GEMM_PLAN_KERNELS = ("8wave", "8wave_mixed", "w4", "w4_mix")       # excel_gemm_plan (include/excel_hip.h)
GEMM_OUT_MODES = {"plain": 0, "qkv": 1, "split": 2}


def gemm_plan(M, N, K, n_cu, mode="bf16x3", batch=1, out="plain", residual=False, half=False):
    """The kernel instance and grid the split-plane GEMM of `mode` runs this problem on with n_cu compute units (host arithmetic only):
    out "plain" / "qkv" (the ViT's head-major in_proj) / "split"; half: the f16x2 call passes W_half."""
    plan = (C.c_int32 * 10)()
    check(lib().excel_gemm_plan(M, N, K, batch, GEMM_OUT_MODES[out], int(residual), GEMM_MODES[mode], int(half), n_cu, plan), "excel_gemm_plan")
    keys = ("kernel", "tile", "nt_m", "x2", "tall", "shrt", "second", "grid_x", "grid_y", "block")
    d = dict(zip(keys, plan))
    d["kernel"] = GEMM_PLAN_KERNELS[d["kernel"]]
    return d


ATTN_PLAN_PATHS = ("strip", "twopass_split", "twopass_f32")       # excel_attn_plan (include/excel_hip.h)


def attn_plan(B, H, N, mode="bf16x3", surgery=True, want_w=True):
    """The kernels one ViT layer's attention runs on for B images of N tokens and H heads in `mode` (host arithmetic only): the path,
    the strip kernel's instance (ntw key tiles per wave on `waves` waves, `waves_full` of them with ntw tiles), the row pass's score
    types and the grids.  surgery: one of the last n_surgery layers; want_w: w_aff / attn_out cover the layer."""
    plan = (C.c_int32 * 14)()
    check(lib().excel_attn_plan(B, H, N, GEMM_MODES[mode], int(surgery), int(want_w), plan), "excel_attn_plan")
    v = list(plan)
    return dict(path=ATTN_PLAN_PATHS[v[0]], ntiles=v[1], ntw=v[2], waves=v[3], waves_full=v[4], rowpass_ntypes=v[5], rowpass_grid=tuple(v[6:9]),
                grid=tuple(v[9:12]), block=v[12], split_c=v[13])


CAM_PLAN_KERNELS = ("narrow", "wide")                             # excel_patch_text_cam_plan (include/excel_hip.h)


def cam_plan(B, N, C_, T, mode="bf16x3"):
    """The kernels patch_text_cam runs B images of N tokens x C_ columns against T text rows on in `mode` (host arithmetic only): the
    similarity kernel ("narrow": T <= 128, instance <split, ct class tiles of 32, tlds = text bank staged in LDS>; "wide": class chunks,
    ct = 0), the workgroups per image and the grids of the prep / similarity / finish launches, the pitch of the min / max table."""
    plan = (C.c_int32 * 14)()
    check(lib().excel_patch_text_cam_plan(B, N, C_, T, GEMM_MODES[mode], plan), "excel_patch_text_cam_plan")
    v = list(plan)
    return dict(kernel=CAM_PLAN_KERNELS[v[0]], split=bool(v[1]), ct=v[2], tlds=bool(v[3]), groups=v[4], prep_grid=tuple(v[5:8]),
                sim_grid=tuple(v[8:10]), block=v[10], finish_grid=tuple(v[11:13]), finish_pitch=v[13])


def layernorm(x, w, b, eps=1e-5):
    x, w, b = _realign(x), _realign(w), _realign(b)      # a row, the weight and the bias are read 16 bytes at a time
    D = x.shape[-1]
    y = torch.empty_like(x)
    check(lib().excel_layernorm(_p(x), _p(w), _p(b), _p(y), x.numel() // D, D, eps, _stream()), "excel_layernorm")
    return y


# ------------------------------------------------------------------ ViT
class VitHandle:
    """Owns device copies of the ViT weights (state_dict naming of the reference's VisionTransformer,
    clip/clip_surgery_model.py:374-394) and the C handle bound to them."""

    def __init__(self, state_dict, width, layers, heads, patch, out_dim, n_surgery=5, device="cuda", prefix="", gemm_mode=None):
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise RuntimeError("excel_amd.VitHandle needs a GPU device: the HIP library is the only compute path")
        g = lambda k: _realign(f32c(torch.as_tensor(state_dict[prefix + k])).to(self.device))      # excel_vit_create: 16-byte aligned weights
        self.cfg = dict(width=width, layers=layers, heads=heads, patch=patch, out_dim=out_dim, n_surgery=n_surgery)
        self.t = {}
        top = {"conv1_w": "conv1.weight", "class_emb": "class_embedding", "pos_emb": "positional_embedding",
               "ln_pre_w": "ln_pre.weight", "ln_pre_b": "ln_pre.bias", "ln_post_w": "ln_post.weight",
               "ln_post_b": "ln_post.bias", "proj": "proj"}
        for f, k in top.items():
            self.t[f] = g(k)
        pos_rows = self.t["pos_emb"].shape[0]
        pos_grid = int(round((pos_rows - 1) ** 0.5))
        assert pos_grid * pos_grid + 1 == pos_rows
        self.blocks = (_lib.VitBlockWeights * layers)()
        for i in range(layers):
            p = f"transformer.resblocks.{i}."
            # surgery blocks of a reloaded reference model carry attn.qkv/attn.proj instead of in_proj/out_proj (:401-404)
            def pick(*names):
                for n in names:
                    if prefix + p + n in state_dict:
                        return g(p + n)
                raise KeyError(p + names[0])
            fields = {
                "ln1_w": pick("ln_1.weight"), "ln1_b": pick("ln_1.bias"),
                "in_proj_w": pick("attn.in_proj_weight", "attn.qkv.weight"),
                "in_proj_b": pick("attn.in_proj_bias", "attn.qkv.bias"),
                "out_proj_w": pick("attn.out_proj.weight", "attn.proj.weight"),
                "out_proj_b": pick("attn.out_proj.bias", "attn.proj.bias"),
                "ln2_w": pick("ln_2.weight"), "ln2_b": pick("ln_2.bias"),
                "fc1_w": pick("mlp.c_fc.weight"), "fc1_b": pick("mlp.c_fc.bias"),
                "fc2_w": pick("mlp.c_proj.weight"), "fc2_b": pick("mlp.c_proj.bias"),
            }
            for f, t in fields.items():
                self.t[f"{i}.{f}"] = t
                setattr(self.blocks[i], f, t.data_ptr())
        w = _lib.VitWeights()
        for f in top:
            setattr(w, f, self.t[f].data_ptr())
        w.blocks = self.blocks
        cfg = _lib.VitConfig(width, layers, heads, patch, out_dim, n_surgery, pos_grid)
        self._h = C.c_void_p()
        with torch.cuda.device(self.device):
            check(lib().excel_vit_create(C.byref(cfg), C.byref(w), C.byref(self._h)), "excel_vit_create")
            # numerics of the linear layers and attention scores: "bf16x3" (default; fp32 operands as bf16 hi+lo, 3 bf16
            # MFMAs per product, CAM error ~1e-5 against exact fp32 on well-conditioned weights), "f16x3" (IEEE-half planes: fp32-grade
            # results, ~2.5 % slower), "f16x2" (f16x3 with two MFMAs per product in the nn.Linear GEMMs - needs fp16-VALUED weights, which
            # every published CLIP archive has: bit-identical to f16x3 there and faster than bf16x3) or "f32" (exact fp32 MFMA).
            # Default ("auto"): f16x2 when the weights allow it, else bf16x3.  EXCEL_GEMM_MODE overrides.
            # The f16 modes hold activations (LayerNorm / QuickGELU outputs, q|k|v) in IEEE half: beyond 65 504 they turn into NaNs on
            # purpose.  Nothing in the forward pass looks for them; the overflow guard (nonfinite_count + confusion_accumulate_masked,
            # pipeline guard=, infer_lam --overflow_guard) is what catches such an image and re-runs it in "f32".
            mode = gemm_mode or os.environ.get("EXCEL_GEMM_MODE", "auto")
            if mode != "f32" and (width % 32 or (3 * patch * patch) % 32):
                mode = "f32"
            if mode == "auto":
                mode = "f16x2" if self.weights_fp16_exact() else "bf16x3"
            self.set_gemm_mode(mode)
        self._ws = {}          # one workspace per launch stream: the same weights can serve concurrent streams

    def __del__(self):
        try:
            if getattr(self, "_h", None):
                lib().excel_vit_destroy(self._h)
                self._h = None
        except Exception:
            pass

    def set_gemm_mode(self, mode):
        """'f32' (exact fp32 MFMA), 'bf16x3' (split-bf16 operands, 3 bf16 MFMAs per product), 'f16x3' (IEEE-half planes) or 'f16x2'
        (f16x3 with two-product weight GEMMs; raises unless weights_fp16_exact())."""
        check(lib().excel_vit_set_gemm_mode(self._h, GEMM_MODES[mode]), "excel_vit_set_gemm_mode")

    def weights_fp16_exact(self):
        """True when every GEMM weight of this handle is exactly representable in IEEE half (clip/build_model.py:72 loads the published
        fp16 archive into the fp32 model unchanged, so real CLIP weights are)."""
        rc = lib().excel_vit_weights_fp16_exact(self._h)
        if rc < 0:
            check(rc, "excel_vit_weights_fp16_exact")
        return rc == 1

    def gemm_mode(self):
        return {v: k for k, v in GEMM_MODES.items()}[lib().excel_vit_get_gemm_mode(self._h)]

    def workspace(self, B, S):
        need = lib().excel_vit_workspace_bytes(self._h, B, S)
        if need == 0:
            raise ValueError(f"bad ViT input shape B={B} S={S}")
        key = torch.cuda.current_stream().cuda_stream
        ws = self._ws.get(key)
        if ws is None or ws.numel() < need:
            self._ws.pop(key, None)
            ws = None
            ws = self._ws[key] = torch.empty(need, dtype=torch.uint8, device=self.device)
        return ws, need

    def forward(self, imgs, want_w_aff=True, aff_layers=6, n_attn_out=0, want_feats=False, want_raw=False, ex_attn=None,
                feats_as_reference=False, want_features=True):
        """-> dict(image_features [B,N,C], w_aff [B,P,P]|None, attn [n,B,N,N]|None, feats [L,B,N,D]|None, x_raw|None)
        ex_attn [B,P,P]: LVC cue added to every head of every surgery block (clip_surgery_model.py:127-141).
        feats_as_reference: `feats` as the reference's decoder receives them (in-place aliasing quirk, include/excel_hip.h)."""
        imgs = f32c(imgs, 16)          # im2col reads 16 bytes at a time; ex_attn is read by element
        B, _, S, S2 = imgs.shape
        assert S == S2
        c = self.cfg
        g = S // c["patch"]
        N = g * g + 1
        dev = imgs.device
        if not (want_features or want_raw):
            raise ValueError("VitHandle.forward: want_features or want_raw")
        # want_features=False: only x_raw (the fused CAM kernel normalises over the token axis itself)
        f = torch.empty((B, N, c["out_dim"]), dtype=torch.float32, device=dev) if want_features else None
        raw = torch.empty((B, N, c["out_dim"]), dtype=torch.float32, device=dev) if want_raw else None
        w_aff = torch.empty((B, N - 1, N - 1), dtype=torch.float32, device=dev) if want_w_aff else None
        attn = torch.empty((n_attn_out, B, N, N), dtype=torch.float32, device=dev) if n_attn_out else None
        feats = torch.empty((c["layers"], B, N, c["width"]), dtype=torch.float32, device=dev) if want_feats else None
        ws, need = self.workspace(B, S)
        if ex_attn is not None:
            ex_attn = f32c(ex_attn)
            if tuple(ex_attn.shape) != (B, N - 1, N - 1):
                raise ValueError(f"ex_attn must be [B,P,P] = {(B, N - 1, N - 1)}, got {tuple(ex_attn.shape)}")
        check(lib().excel_vit_forward_ex(self._h, _p(imgs), B, S, _p(ws, torch.uint8), need, _p(f), _p(raw), _p(w_aff),
                                         aff_layers, _p(attn), n_attn_out, _p(feats), _p(ex_attn), 1 if feats_as_reference else 0, _stream()),
              "excel_vit_forward")
        return dict(image_features=f, w_aff=w_aff, attn=attn, feats=feats, x_raw=raw)


class DecoderHandle:
    """Device copies of the decoder head's weights + the C handle (SegFormerHead fuse: model/segformer_head.py:47-77;
    DecoderTransformer: model/decoder/TransDecoder.py:105-124).  `fuse_sd` / `dec_sd` use the reference modules' state_dict keys."""

    def __init__(self, fuse_sd, dec_sd, heads=8, device="cuda"):
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise RuntimeError("excel_amd.DecoderHandle needs a GPU device: the HIP library is the only compute path")
        g = lambda sd, k: _realign(f32c(torch.as_tensor(sd[k])).to(self.device))       # excel_decoder_create: 16-byte aligned weights
        self.t = {}
        L = 0
        while f"linears_modulelist.{L}.proj.weight" in fuse_sd:
            L += 1
        nl = 0
        while f"transformer.resblocks.{nl}.ln_1.weight" in dec_sd:
            nl += 1
        E, D = fuse_sd["linears_modulelist.0.proj.weight"].shape
        nc = dec_sd["linear_pred.weight"].shape[0]
        self.cfg = dict(vit_layers=L, vit_width=int(D), embed=int(E), dec_layers=nl, heads=heads, num_classes=int(nc))
        self.fuse = (_lib.FuseLayerWeights * L)()
        for l in range(L):
            for f, k in (("proj_w", "proj.weight"), ("proj_b", "proj.bias"), ("proj2_w", "proj_2.weight"), ("proj2_b", "proj_2.bias")):
                t = self.t[f"fuse{l}.{f}"] = g(fuse_sd, f"linears_modulelist.{l}.{k}")
                setattr(self.fuse[l], f, t.data_ptr())
        self.blocks = (_lib.DecoderBlockWeights * max(nl, 1))()
        names = {"ln1_w": "ln_1.weight", "ln1_b": "ln_1.bias", "in_proj_w": "attn.in_proj_weight", "in_proj_b": "attn.in_proj_bias",
                 "out_proj_w": "attn.out_proj.weight", "out_proj_b": "attn.out_proj.bias", "ln2_w": "ln_2.weight", "ln2_b": "ln_2.bias",
                 "fc1_w": "mlp.c_fc.weight", "fc1_b": "mlp.c_fc.bias", "fc2_w": "mlp.c_proj.weight", "fc2_b": "mlp.c_proj.bias"}
        for l in range(nl):
            for f, k in names.items():
                t = self.t[f"blk{l}.{f}"] = g(dec_sd, f"transformer.resblocks.{l}.{k}")
                setattr(self.blocks[l], f, t.data_ptr())
        w = _lib.DecoderWeights()
        w.fuse, w.blocks = self.fuse, self.blocks
        for f, (sd, k) in {"fuse_w": (fuse_sd, "linear_fuse.weight"), "fuse_b": (fuse_sd, "linear_fuse.bias"),
                           "pred_w": (dec_sd, "linear_pred.weight"), "pred_b": (dec_sd, "linear_pred.bias")}.items():
            t = self.t[f] = g(sd, k).reshape(sd[k].shape[0], -1).contiguous() if f.endswith("_w") else g(sd, k)
            setattr(w, f, t.data_ptr())
        cfg = _lib.DecoderConfig(L, int(D), int(E), nl, heads, int(nc))
        self._h = C.c_void_p()
        with torch.cuda.device(self.device):
            check(lib().excel_decoder_create(C.byref(cfg), C.byref(w), C.byref(self._h)), "excel_decoder_create")

    def __del__(self):
        try:
            if getattr(self, "_h", None):
                lib().excel_decoder_destroy(self._h)
                self._h = None
        except Exception:
            pass

    def state_dicts(self):
        """-> (fuse_sd, dec_sd) with the reference modules' state_dict keys and shapes (1x1 conv weights as [out,in,1,1]): what
        torch.save(model.state_dict()) of the reference holds for the head, so a head trained here loads back there."""
        c = self.cfg
        fuse, dec = {}, {}
        for l in range(c["vit_layers"]):
            for f, k in (("proj_w", "proj.weight"), ("proj_b", "proj.bias"), ("proj2_w", "proj_2.weight"), ("proj2_b", "proj_2.bias")):
                fuse[f"linears_modulelist.{l}.{k}"] = self.t[f"fuse{l}.{f}"].detach().clone()
        fuse["linear_fuse.weight"] = self.t["fuse_w"].detach().clone()[:, :, None, None]
        fuse["linear_fuse.bias"] = self.t["fuse_b"].detach().clone()
        for l in range(c["dec_layers"]):
            for f, k in _BLOCK_KEYS.items():
                dec[f"transformer.resblocks.{l}.{k}"] = self.t[f"blk{l}.{f}"].detach().clone()
        dec["linear_pred.weight"] = self.t["pred_w"].detach().clone()[:, :, None, None]
        dec["linear_pred.bias"] = self.t["pred_b"].detach().clone()
        return fuse, dec

    def _ref_layout(self):
        """{name in self.t: (0 = fuse_sd | 1 = dec_sd, the reference module's key, its shape there)}: state_dicts() read backwards."""
        c = self.cfg
        out = {}
        for l in range(c["vit_layers"]):
            for f, k in (("proj_w", "proj.weight"), ("proj_b", "proj.bias"), ("proj2_w", "proj_2.weight"), ("proj2_b", "proj_2.bias")):
                out[f"fuse{l}.{f}"] = (0, f"linears_modulelist.{l}.{k}")
        out["fuse_w"], out["fuse_b"] = (0, "linear_fuse.weight"), (0, "linear_fuse.bias")
        for l in range(c["dec_layers"]):
            for f, k in _BLOCK_KEYS.items():
                out[f"blk{l}.{f}"] = (1, f"transformer.resblocks.{l}.{k}")
        out["pred_w"], out["pred_b"] = (1, "linear_pred.weight"), (1, "linear_pred.bias")
        return {n: (w, k, tuple(self.t[n].shape) + ((1, 1) if n in ("fuse_w", "pred_w") else ())) for n, (w, k) in out.items()}

    def load_weights(self, fuse_sd, dec_sd):
        """The inverse of state_dicts(): copies `fuse_sd` / `dec_sd` (the reference modules' keys and shapes, 1x1 conv weights as
        [out,in,1,1]) into the EXISTING device tensors.  The C handle and the gradient table hold raw pointers into self.t, so nothing
        is reallocated; everything is checked before the first byte is copied (ValueError naming the key: missing, or another shape)."""
        sds = (fuse_sd, dec_sd)
        layout = self._ref_layout()
        for n, (w, k, shape) in layout.items():
            if k not in sds[w]:
                raise ValueError(f"DecoderHandle.load_weights: missing key {('decoder_fts_fuse.', 'decoder.')[w]}{k}")
            got = tuple(torch.as_tensor(sds[w][k]).shape)
            if got != shape:
                raise ValueError(f"DecoderHandle.load_weights: {('decoder_fts_fuse.', 'decoder.')[w]}{k} has shape {got}, the head's is {shape}")
        with torch.no_grad():
            for n, (w, k, _) in layout.items():
                self.t[n].copy_(torch.as_tensor(sds[w][k]).detach().to(torch.float32).reshape(self.t[n].shape))

    def optimizer_state(self):
        """AdamW's moments as CPU copies, {"exp_avg": {name: tensor}, "exp_avg_sq": {name: tensor}} keyed like self.t (torch.optim.AdamW's
        names for the two buffers; its `step` is the caller's counter, see adamw_step).  None before the first adamw_step."""
        if getattr(self, "_adam", None) is None:
            return None
        return {"exp_avg": {k: m.detach().cpu().clone() for k, (m, _) in self._adam.items()},
                "exp_avg_sq": {k: v.detach().cpu().clone() for k, (_, v) in self._adam.items()}}

    def check_optimizer_state(self, state):
        """load_optimizer_state's refusals alone: ValueError naming the key on a missing or extra key, another shape or a dtype other
        than float32."""
        parts = ("exp_avg", "exp_avg_sq")
        if not isinstance(state, dict) or set(state) != set(parts):
            bad = sorted(set(parts) ^ set(state)) if isinstance(state, dict) else list(parts)
            raise ValueError(f"DecoderHandle.load_optimizer_state: expected the keys {list(parts)}, missing or extra: {bad[0]}")
        for part in parts:
            for k in self.t:
                if k not in state[part]:
                    raise ValueError(f"DecoderHandle.load_optimizer_state: missing key {part}.{k}")
            for k, v in state[part].items():
                if k not in self.t:
                    raise ValueError(f"DecoderHandle.load_optimizer_state: extra key {part}.{k}")
                if not torch.is_tensor(v) or v.dtype != torch.float32:
                    raise ValueError(f"DecoderHandle.load_optimizer_state: {part}.{k} is {getattr(v, 'dtype', type(v).__name__)}, "
                                     "expected a torch.float32 tensor")
                if tuple(v.shape) != tuple(self.t[k].shape):
                    raise ValueError(f"DecoderHandle.load_optimizer_state: {part}.{k} has shape {tuple(v.shape)}, "
                                     f"the parameter's is {tuple(self.t[k].shape)}")

    def load_optimizer_state(self, state):
        """What optimizer_state() returned -> the moments of the next adamw_step (created if no step ran yet).  Everything is checked
        (check_optimizer_state) before anything is copied."""
        self.check_optimizer_state(state)
        if getattr(self, "_adam", None) is None:
            self._adam = {k: (torch.zeros_like(v), torch.zeros_like(v)) for k, v in self.t.items()}
        with torch.no_grad():
            for k, (m, v) in self._adam.items():
                m.copy_(state["exp_avg"][k])
                v.copy_(state["exp_avg_sq"][k])

    # ------------------------------------------------------------------ training iteration
    def _grad_table(self):
        """Gradient tensors shaped like the parameters + the C table pointing at them (built once)."""
        if getattr(self, "_grads", None) is None:
            # one flat buffer (each parameter's gradient is a 16-byte aligned view): a data-parallel step is ONE all-reduce
            offs, total = {}, 0
            for k, v in self.t.items():
                offs[k] = total
                total += (v.numel() + 3) // 4 * 4
            self.grad_flat = torch.zeros(total, dtype=torch.float32, device=self.device)
            self._grads = {k: self.grad_flat[offs[k]:offs[k] + v.numel()].view(v.shape) for k, v in self.t.items()}
            c = self.cfg
            self._gfuse = (_lib.FuseLayerWeights * c["vit_layers"])()
            for l in range(c["vit_layers"]):
                for f in ("proj_w", "proj_b", "proj2_w", "proj2_b"):
                    setattr(self._gfuse[l], f, self._grads[f"fuse{l}.{f}"].data_ptr())
            self._gblocks = (_lib.DecoderBlockWeights * max(c["dec_layers"], 1))()
            for l in range(c["dec_layers"]):
                for f in _BLOCK_KEYS:
                    setattr(self._gblocks[l], f, self._grads[f"blk{l}.{f}"].data_ptr())
            g = _lib.DecoderWeights()
            g.fuse, g.blocks = self._gfuse, self._gblocks
            for f in ("fuse_w", "fuse_b", "pred_w", "pred_b"):
                setattr(g, f, self._grads[f].data_ptr())
            self._gtable = g
        return self._grads, self._gtable

    def _check_feats(self, L, N, D, g):
        """all_feats [L,B,N,D] must match the head's configuration: the kernels index by it (a wrong shape would read out of bounds)."""
        c = self.cfg
        if L != c["vit_layers"] or D != c["vit_width"]:
            raise ValueError(f"all_feats must be [{c['vit_layers']},B,N,{c['vit_width']}], got L={L}, D={D}")
        if g * g + 1 != N:
            raise ValueError("all_feats must hold cls + a square grid of patch tokens")

    def forward_train(self, all_feats, dropout_p=0.0, dropout_seed=0):
        """-> (seg [B,nc,g,g], attn_pred [B,P,P], ctx) ; ctx goes to backward().  dropout_p: the head's Dropout2d (0.1 in the reference)."""
        all_feats = f32c(all_feats, 16)        # read in place as the A operand of the fuse GEMMs
        L, B, N, D = all_feats.shape
        g = int(round((N - 1) ** 0.5))
        c = self.cfg
        self._check_feats(L, N, D, g)
        dev = all_feats.device
        seg = torch.empty((B, c["num_classes"], g, g), dtype=torch.float32, device=dev)
        ap = torch.empty((B, g * g, g * g), dtype=torch.float32, device=dev)
        need = lib().excel_decoder_train_workspace_bytes(self._h, B, g)
        ws = _ws(need, dev)
        check(lib().excel_decoder_forward_train(self._h, _p(all_feats), B, g, _p(ws, torch.uint8), need, _p(seg), _p(ap), float(dropout_p),
                                                int(dropout_seed) & 0xFFFFFFFF, _stream()), "excel_decoder_forward_train")
        return seg, ap, (all_feats, B, g, ws, need, float(dropout_p), int(dropout_seed) & 0xFFFFFFFF)

    def train_attn_fts(self, ctx):
        """attn_fts [B,E,g,g] of the forward_train that produced `ctx`: the post-Dropout2d fused features (the LVC cue of the
        training loop, scripts/train_voc.py:186-189)."""
        all_feats, B, g, ws, need, _, _ = ctx
        fts = torch.empty((B, self.cfg["embed"], g, g), dtype=torch.float32, device=all_feats.device)
        check(lib().excel_decoder_train_attn_fts(self._h, B, g, _p(ws, torch.uint8), need, _p(fts), _stream()), "excel_decoder_train_attn_fts")
        return fts

    def backward(self, ctx, d_seg, d_attn_pred=None):
        """-> dict of gradients keyed like self.t (fuse{l}.proj_w ..., blk{l}.fc1_w ..., fuse_w, pred_w ...)."""
        all_feats, B, g, ws, need, dp, dseed = ctx
        grads, table = self._grad_table()
        check(lib().excel_decoder_backward(self._h, _p(all_feats), B, g, _p(ws, torch.uint8), need, _p(f32c(d_seg)),
                                           _p(f32c(d_attn_pred)) if d_attn_pred is not None else None, C.byref(table), dp, dseed, _stream()),
              "excel_decoder_backward")
        return grads

    def adamw_step(self, lr, step, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2):
        """torch.optim.AdamW over every parameter with the gradients of the last backward(); `step` counts from 1."""
        grads, _ = self._grad_table()
        if getattr(self, "_adam", None) is None:
            self._adam = {k: (torch.zeros_like(v), torch.zeros_like(v)) for k, v in self.t.items()}
        for k, p in self.t.items():
            m, v = self._adam[k]
            check(lib().excel_adamw_step(_p(p), _p(grads[k]), _p(m), _p(v), p.numel(), float(lr), float(betas[0]), float(betas[1]), float(eps),
                                         float(weight_decay), int(step), _stream()), "excel_adamw_step")

    def forward(self, all_feats, want_seg=True):
        """all_feats [L,B,N,D] -> (attn_fts [B,E,g,g], seg [B,nc,g,g] | None)"""
        all_feats = f32c(all_feats, 16)
        L, B, N, D = all_feats.shape
        c = self.cfg
        g = int(round((N - 1) ** 0.5))
        self._check_feats(L, N, D, g)
        dev = all_feats.device
        fts = torch.empty((B, c["embed"], g, g), dtype=torch.float32, device=dev)
        seg = torch.empty((B, c["num_classes"], g, g), dtype=torch.float32, device=dev) if want_seg else None
        need = lib().excel_decoder_workspace_bytes(self._h, B, g)
        ws = _ws(need, dev)
        check(lib().excel_decoder_forward(self._h, _p(all_feats), B, g, _p(ws, torch.uint8), need, _p(fts), _p(seg), _stream()),
              "excel_decoder_forward")
        return fts, seg


_BLOCK_KEYS = {"ln1_w": "ln_1.weight", "ln1_b": "ln_1.bias", "in_proj_w": "attn.in_proj_weight", "in_proj_b": "attn.in_proj_bias",
               "out_proj_w": "attn.out_proj.weight", "out_proj_b": "attn.out_proj.bias", "ln2_w": "ln_2.weight", "ln2_b": "ln_2.bias",
               "fc1_w": "mlp.c_fc.weight", "fc1_b": "mlp.c_fc.bias", "fc2_w": "mlp.c_proj.weight", "fc2_b": "mlp.c_proj.bias"}


class TextHandle:
    """CLIP text tower (encode_text, clip/clip_surgery_model.py:551-564) over the HIP library.  `sd`: the CLIP state_dict keys of
    the text side (token_embedding.weight, positional_embedding, transformer.resblocks.*, ln_final.*, text_projection)."""

    def __init__(self, sd, heads, device="cuda"):
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise RuntimeError("excel_amd.TextHandle needs a GPU device: the HIP library is the only compute path")
        g = lambda k: _realign(f32c(torch.as_tensor(sd[k])).to(self.device))           # excel_text_create: 16-byte aligned weights
        self.t = {}
        nl = 0
        while f"transformer.resblocks.{nl}.ln_1.weight" in sd:
            nl += 1
        self.blocks = (_lib.DecoderBlockWeights * max(nl, 1))()
        for l in range(nl):
            for f, k in _BLOCK_KEYS.items():
                t = self.t[f"blk{l}.{f}"] = g(f"transformer.resblocks.{l}.{k}")
                setattr(self.blocks[l], f, t.data_ptr())
        w = _lib.TextWeights()
        for f, k in (("token_embedding", "token_embedding.weight"), ("positional_embedding", "positional_embedding"),
                     ("ln_final_w", "ln_final.weight"), ("ln_final_b", "ln_final.bias"), ("text_projection", "text_projection")):
            t = self.t[f] = g(k)
            setattr(w, f, t.data_ptr())
        w.blocks = self.blocks
        vocab, width = self.t["token_embedding"].shape
        ctx = self.t["positional_embedding"].shape[0]
        embed = self.t["text_projection"].shape[1]
        self.cfg = dict(vocab_size=int(vocab), context_length=int(ctx), width=int(width), layers=nl, heads=heads, embed_dim=int(embed))
        cfg = _lib.TextConfig(int(vocab), int(ctx), int(width), nl, heads, int(embed))
        self._h = C.c_void_p()
        with torch.cuda.device(self.device):
            check(lib().excel_text_create(C.byref(cfg), C.byref(w), C.byref(self._h)), "excel_text_create")

    def __del__(self):
        try:
            if getattr(self, "_h", None):
                lib().excel_text_destroy(self._h)
                self._h = None
        except Exception:
            pass

    def encode(self, tokens):
        """tokens [B, context_length] (any integer dtype) -> [B, embed_dim] f32"""
        tok = torch.as_tensor(tokens).to(device=self.device, dtype=torch.int32).contiguous()
        B, ctx = tok.shape
        if ctx != self.cfg["context_length"]:
            raise ValueError(f"tokens must be [B,{self.cfg['context_length']}], got {tuple(tok.shape)}")
        out = torch.empty((B, self.cfg["embed_dim"]), dtype=torch.float32, device=self.device)
        need = lib().excel_text_workspace_bytes(self._h, B)
        ws = _ws(need, self.device)
        check(lib().excel_text_encode(self._h, _p(tok, torch.int32), B, _p(out), _p(ws, torch.uint8), need, _stream()), "excel_text_encode")
        return out


def prompt_ensemble(class_embeddings):
    """clip/clip.py:262-266: [n,E] -> unit-norm mean of the unit-norm rows [E]."""
    e = f32c(class_embeddings)
    n, E = e.shape
    out = torch.empty((E,), dtype=torch.float32, device=e.device)
    check(lib().excel_prompt_ensemble(_p(e), n, E, _p(out), _stream()), "excel_prompt_ensemble")
    return out


def train_losses(seg, attn_pred, pseudo_u8, radius=8, ignore_index=255, w_seg=1.0, w_diver=0.1, aff_labels_u8=None):
    """scripts/train_voc.py:202-215 -> (losses [2] = (seg_loss, diver_loss), d_seg, d_attn_pred).
    aff_labels_u8: the map the affinity labels come from (default: the pseudo labels; :210 switches to the seg arg-max later on)."""
    seg, attn_pred = f32c(seg), f32c(attn_pred)
    B, nc, gh, gw = seg.shape
    H, W = pseudo_u8.shape[-2:]
    losses = torch.empty((2,), dtype=torch.float32, device=seg.device)
    d_seg, d_ap = torch.empty_like(seg), torch.empty_like(attn_pred)
    ws = _ws(lib().excel_train_losses_workspace_bytes(B, nc, H, W), seg.device)
    check(lib().excel_train_losses(_p(seg), _p(attn_pred), _p(pseudo_u8.contiguous(), torch.uint8),
                                   _p(aff_labels_u8.contiguous(), torch.uint8) if aff_labels_u8 is not None else None, B, nc, gh, gw, H, W, radius, ignore_index,
                                   float(w_seg), float(w_diver), _p(losses), _p(d_seg), _p(d_ap), _p(ws, torch.uint8), _stream()), "excel_train_losses")
    return losses, d_seg, d_ap


def lam_to_label(cam, cls_label, img_box=None, bkg_thre=0.5, high_thre=None, low_thre=None, ignore_mid=False, ignore_index=255):
    """utils/camutils.py:123-145 -> (valid_cam [B,F,H,W], pseudo_label uint8 [B,H,W])."""
    cam, cls_label = f32c(cam), f32c(cls_label)
    B, F_, H, W = cam.shape
    valid = torch.empty_like(cam)
    lab = torch.empty((B, H, W), dtype=torch.uint8, device=cam.device)
    box = None if img_box is None else torch.as_tensor(img_box).to(device=cam.device, dtype=torch.int32).contiguous()
    check(lib().excel_lam_to_label(_p(cam), _p(cls_label), _p(box, torch.int32), B, F_, H, W, float(bkg_thre), float(high_thre or 0.0),
                                   float(low_thre or 0.0), 1 if ignore_mid else 0, int(ignore_index), _p(valid), _p(lab, torch.uint8), _stream()),
          "excel_lam_to_label")
    return valid, lab


def normalize_img_u8(hwc_u8, mean=(123.675, 116.28, 103.53), std=(58.395, 57.12, 57.375)):
    """datasets/transforms.normalize_img + HWC->CHW on the device: uint8 [B,H,W,3] -> f32 [B,3,H,W] (3 B/pixel over PCIe instead of 12)."""
    x = hwc_u8.contiguous()
    B, H, W, Cc = x.shape
    assert Cc == 3 and x.dtype == torch.uint8
    out = torch.empty((B, 3, H, W), dtype=torch.float32, device=x.device)
    m, s = (C.c_double * 3)(*mean), (C.c_double * 3)(*std)
    check(lib().excel_normalize_img_u8(_p(x, torch.uint8), B, H, W, m, s, _p(out), _stream()), "excel_normalize_img_u8")
    return out


def denormalize_img(imgs, mean=(123.675, 116.28, 103.53), std=(58.395, 57.12, 57.375), as_float=False):
    """utils/imutils.py:11-25: [B,3,H,W] normalised f32 -> uint8 image (denormalize_img) or that / 255 as f32 (denormalize_img2)."""
    imgs = f32c(imgs)
    B, Cc, H, W = imgs.shape
    assert Cc == 3
    out = torch.empty((B, 3, H, W), dtype=torch.float32 if as_float else torch.uint8, device=imgs.device)
    m, s = (C.c_float * 3)(*mean), (C.c_float * 3)(*std)
    check(lib().excel_denormalize_img(_p(imgs), B, H, W, m, s, None if as_float else _p(out, torch.uint8), _p(out) if as_float else None,
                                      _stream()), "excel_denormalize_img")
    return out


def seg_scale_accumulate(segs, acc, H, W, flip_mean, init, scale=1.0):
    """tools/infer_seg_voc.py:66-82 for one scale: segs [2B,nc,h,w] -> acc [B,nc,H,W] (allocated when None)."""
    segs = f32c(segs)
    B2, nc, h, w = segs.shape
    B = B2 // 2
    if acc is None:
        acc = torch.empty((B, nc, H, W), dtype=torch.float32, device=segs.device)
        init = True
    check(lib().excel_seg_scale_accumulate(_p(segs), _p(acc), B, nc, h, w, H, W, 1 if flip_mean else 0, 1 if init else 0, float(scale),
                                           _stream()), "excel_seg_scale_accumulate")
    return acc


SEG_MAX_SCALES = 8


def seg_msc_fuse_ragged(segs, flip_mean, plan, want_planes=True, want_labels=False, label_hw=None):
    """tools/infer_seg_voc.py:63-82 (coco :62-80) for a ragged batch, all scales in one launch (excel_seg_msc_fuse_ragged).
    segs: the decoder logits of every scale, [2B,nc,g_s,g_s] each (image b, then its flipped copy at B + b), in the reference's order
    (scale 1.0 first); flip_mean: one flag per scale; plan: RaggedPlan of the fuse sizes (h_b, w_b).
    -> (planes, labels): nc pitched planes per image (want_planes) and tight uint8 arg-max labels (want_labels), None where not wanted.
    Labels are the reference's only where the label size is the fuse size: `label_hw` ([B,2], the label sizes) is checked against the
    plan when labels are asked for, and a mismatch is refused (use seg_resize_argmax_ragged there)."""
    import numpy as np
    segs = [f32c(x) for x in segs]
    ns = len(segs)
    if not 1 <= ns <= SEG_MAX_SCALES:
        raise ValueError(f"seg_msc_fuse_ragged: {ns} scales, need 1..{SEG_MAX_SCALES}")
    if len(flip_mean) != ns:
        raise ValueError("seg_msc_fuse_ragged: one flip_mean flag per scale")
    if not (want_planes or want_labels):
        raise ValueError("seg_msc_fuse_ragged: ask for planes, labels or both")
    nc = int(segs[0].shape[1]) if segs[0].dim() == 4 else 0
    for x in segs:
        if x.dim() != 4 or x.shape[0] != 2 * plan.B or x.shape[1] != nc or x.shape[2] != x.shape[3] or x.shape[2] < 1:
            raise ValueError(f"seg_msc_fuse_ragged: every scale must be [2B={2 * plan.B}, nc={nc}, g, g], got {tuple(x.shape)}")
    if nc < 1:
        raise ValueError("seg_msc_fuse_ragged: nc >= 1")
    if want_labels:
        if label_hw is None:
            raise ValueError("seg_msc_fuse_ragged: labels need label_hw (the label sizes) to check them against the fuse sizes")
        if not np.array_equal(np.asarray(label_hw, np.int64).reshape(-1, 2), plan.hw.astype(np.int64)):
            raise ValueError("seg_msc_fuse_ragged: label sizes differ from the fuse sizes: fuse planes and use seg_resize_argmax_ragged")
    dev = segs[0].device
    planes = torch.empty((nc * plan.total_pix,), dtype=torch.float32, device=dev) if want_planes else None
    labels = torch.empty((plan.total_label_pix,), dtype=torch.uint8, device=dev) if want_labels else None
    ptrs = (C.c_void_p * ns)(*[x.data_ptr() for x in segs])
    for x in segs:
        _p(x)
    g = (C.c_int32 * ns)(*[int(x.shape[2]) for x in segs])
    fl = (C.c_int32 * ns)(*[1 if f else 0 for f in flip_mean])
    check(lib().excel_seg_msc_fuse_ragged(ptrs, g, fl, ns, nc, _p(plan.table, torch.int32), C.byref(plan.info), _p(planes),
                                          _p(labels, torch.uint8), _stream()), "excel_seg_msc_fuse_ragged")
    return planes, labels


def seg_resize_argmax_ragged(planes, src_plan, dst_plan, nc):
    """tools/infer_seg_coco.py:86-87: nc pitched planes per image at src_plan's sizes -> tight uint8 arg-max labels at dst_plan's sizes,
    without the resized logits in memory (excel_seg_resize_argmax_ragged)."""
    if src_plan.B != dst_plan.B:
        raise ValueError(f"seg_resize_argmax_ragged: plans of {src_plan.B} and {dst_plan.B} images")
    if planes.numel() != nc * src_plan.total_pix:
        raise ValueError(f"seg_resize_argmax_ragged: planes must hold nc * total_pix = {nc * src_plan.total_pix} floats")
    lab = torch.empty((dst_plan.total_label_pix,), dtype=torch.uint8, device=planes.device)
    check(lib().excel_seg_resize_argmax_ragged(_p(planes), _p(src_plan.table, torch.int32), C.byref(src_plan.info), _p(dst_plan.table, torch.int32),
                                               C.byref(dst_plan.info), int(nc), _p(lab, torch.uint8), _stream()), "excel_seg_resize_argmax_ragged")
    return lab


def seg_resize_argmax_uniform(segs, dst_plan):
    """engine/validatation_engine.py:27,37 for a ragged batch: the decoder's seg logits segs [B,nc,h,w] (tight, any h, w) -> bilinear to
    every image's label size (dst_plan) -> arg-max -> tight uint8 labels, one launch (excel_seg_resize_argmax_uniform; the bits of
    bilinear_resize + argmax_label per image)."""
    segs = f32c(segs)
    if segs.dim() != 4 or segs.shape[0] != dst_plan.B:
        raise ValueError(f"seg_resize_argmax_uniform: segs must be [B={dst_plan.B}, nc, h, w], got {tuple(segs.shape)}")
    B, nc, h, w = segs.shape
    lab = torch.empty((dst_plan.total_label_pix,), dtype=torch.uint8, device=segs.device)
    check(lib().excel_seg_resize_argmax_uniform(_p(segs), int(B), int(h), int(w), int(nc), _p(dst_plan.table, torch.int32),
                                                C.byref(dst_plan.info), _p(lab, torch.uint8), _stream()), "excel_seg_resize_argmax_uniform")
    return lab


def seg_softmax_resize(planes, plan, b, nc, H, W):
    """The CRF's input for image b of a packed nc-plane pitched tensor (tools/infer_seg_voc.py:146-147, coco :144-145): bilinear to
    (H, W) (skipped at the same size), softmax over classes -> tight [nc, H, W] (excel_seg_softmax_resize)."""
    h, w = int(plan.hw[b, 0]), int(plan.hw[b, 1])
    wp = (w + 3) // 4 * 4
    o = nc * int(plan.poff[b])
    if planes.numel() != nc * plan.total_pix:
        raise ValueError(f"seg_softmax_resize: planes must hold nc * total_pix = {nc * plan.total_pix} floats")
    src = planes[o:o + nc * h * wp]
    prob = torch.empty((nc, int(H), int(W)), dtype=torch.float32, device=planes.device)
    check(lib().excel_seg_softmax_resize(_p(src), h, w, int(nc), int(H), int(W), _p(prob), _stream()), "excel_seg_softmax_resize")
    return prob


def seg_softmax_resize_ragged(planes, src_plan, dst_plan, nc):
    """seg_softmax_resize for every image of a ragged batch in one launch (excel_seg_softmax_resize_ragged): nc pitched planes per
    image at src_plan's sizes -> tight [nc, H_b, W_b] probabilities per image at dst_plan's sizes, image b at nc * loff_b (flat)."""
    if src_plan.B != dst_plan.B:
        raise ValueError(f"seg_softmax_resize_ragged: plans of {src_plan.B} and {dst_plan.B} images")
    if planes.numel() != nc * src_plan.total_pix:
        raise ValueError(f"seg_softmax_resize_ragged: planes must hold nc * total_pix = {nc * src_plan.total_pix} floats")
    prob = torch.empty((nc * dst_plan.total_label_pix,), dtype=torch.float32, device=planes.device)
    check(lib().excel_seg_softmax_resize_ragged(_p(planes), _p(src_plan.table, torch.int32), C.byref(src_plan.info), _p(dst_plan.table, torch.int32),
                                                C.byref(dst_plan.info), int(nc), _p(prob), _stream()), "excel_seg_softmax_resize_ragged")
    return prob


# ------------------------------------------------------------------ CAM
def clip_feature_surgery(image_features, text_features, num_fg=None, t=2.0, want_full=True):
    """image_features [B,N,C], text_features [T,C] -> (full [B,N,T] | None, slice [B,N-1,F] | None)."""
    image_features = f32c(image_features, 16)      # the operands of the similarity GEMM
    text_features = f32c(text_features, 16)
    B, N, Cc = image_features.shape
    T = text_features.shape[0]
    dev = image_features.device
    full = torch.empty((B, N, T), dtype=torch.float32, device=dev) if want_full else None
    F_ = T if num_fg is None else num_fg
    sl = torch.empty((B, N - 1, F_), dtype=torch.float32, device=dev) if num_fg is not None else None
    ws = _ws(lib().excel_cam_workspace_bytes(B, N, T), dev)
    check(lib().excel_clip_feature_surgery(_p(image_features), _p(text_features), B, N, Cc, T, F_, float(t), _p(full), _p(sl),
                                           _p(ws, torch.uint8), _stream()), "excel_clip_feature_surgery")
    return full, sl


def patch_text_cam(x_raw, text_features, num_fg=None, t=2.0, want_full=False, want_features=False, mode="bf16x3"):
    """Fused path (excel_patch_text_cam): un-normalised token features x_raw [B,N,C] (VitHandle.forward(want_raw=True)) + text [T,C]
    -> (full [B,N,T] | None, slice [B,N-1,F] | None, image_features [B,N,C] | None): clip.py:353 + :288-310 (column-norm pass, similarity tiles, finish)."""
    x_raw = f32c(x_raw, 16)
    text_features = f32c(text_features, 16)
    B, N, Cc = x_raw.shape
    T = text_features.shape[0]
    dev = x_raw.device
    full = torch.empty((B, N, T), dtype=torch.float32, device=dev) if want_full else None
    F_ = T if num_fg is None else num_fg
    sl = torch.empty((B, N - 1, F_), dtype=torch.float32, device=dev) if num_fg is not None else None
    feats = torch.empty_like(x_raw) if want_features else None
    if full is None and sl is None:
        raise ValueError("patch_text_cam: nothing to compute (want_full=False and num_fg=None)")
    ws = _ws(lib().excel_patch_text_cam_workspace_bytes(B, N, Cc, T), dev)
    check(lib().excel_patch_text_cam(_p(x_raw), _p(text_features), B, N, Cc, T, F_, float(t), GEMM_MODES["f16x3" if mode == "f16x2" else mode], _p(full), _p(sl),
                                     _p(feats), _p(ws, torch.uint8), _stream()), "excel_patch_text_cam")
    return full, sl, feats


# ------------------------------------------------------------------ affinity random walk
def attn_layer_mean(attn, n_layers=6):
    """attn [Lw,B,N,N] -> mean of the last n_layers of attn[:, :, 1:, 1:]  -> [B,P,P]"""
    attn = f32c(attn)
    Lw, B, N, _ = attn.shape
    n = min(n_layers, Lw)
    out = torch.empty((B, N - 1, N - 1), dtype=torch.float32, device=attn.device)
    check(lib().excel_attn_layer_mean(_p(attn), Lw, B, N, Lw - n, n, _p(out), _stream()), "excel_attn_layer_mean")
    return out


def attn_select_mean(attn, seg_attn, n_layers=6):
    """seg_attn branch of refine_cams_with_aff (affutils.py:182-195): attn [Lw,B,N,N], seg_attn [B,P,P] -> [B,P,P]."""
    attn = f32c(attn)
    seg_attn = f32c(seg_attn)
    Lw, B, N, _ = attn.shape
    n = min(n_layers, Lw)
    if tuple(seg_attn.shape) != (B, N - 1, N - 1):
        raise ValueError(f"seg_attn must be [B,P,P] = {(B, N - 1, N - 1)}, got {tuple(seg_attn.shape)}")
    out = torch.empty((B, N - 1, N - 1), dtype=torch.float32, device=attn.device)
    ws = _ws(lib().excel_attn_select_workspace_bytes(B, n), attn.device)
    check(lib().excel_attn_select_mean(_p(attn), Lw, B, N, Lw - n, n, _p(seg_attn), _p(out), _p(ws, torch.uint8), _stream()),
          "excel_attn_select_mean")
    return out


def feature_affinity(feats, mode, beta=1.0, gamma=3.0):
    """feats [B,C,g,g] | [B,C,P] -> [B,P,P].  mode "sigmoid": attn_pred (model_excel.py:70-76);
    mode "mask_softmax": ex_attn of the LVC branch (clip_surgery_model.py:128-137)."""
    feats = f32c(feats)
    feats = feats.reshape(feats.shape[0], feats.shape[1], -1)
    B, Cc, P = feats.shape
    out = torch.empty((B, P, P), dtype=torch.float32, device=feats.device)
    ws = _ws(lib().excel_feature_affinity_workspace_bytes(B, Cc, P), feats.device)
    check(lib().excel_feature_affinity(_p(feats), B, Cc, P, float(beta), float(gamma), {"sigmoid": 0, "mask_softmax": 1}[mode],
                                       _p(out), _p(ws, torch.uint8), _stream()), "excel_feature_affinity")
    return out


def feature_affinity_grouped(feats, mode, group, member_stride=1, beta=1.0, gamma=3.0, out=None):
    """feature_affinity with the mean taken per group of images (include/excel_hip.h): member m of group j is image
    (j // member_stride) * group * member_stride + j % member_stride + m * member_stride.  group=1: per image (attn_pred of a batch);
    group=2, member_stride=B over a [2B] stack [x; flip x]: per (x_j, flip x_j) pair (ex_attn).  Every group equals a standalone
    feature_affinity call on its images bit for bit."""
    feats = f32c(feats)
    feats = feats.reshape(feats.shape[0], feats.shape[1], -1)
    B, Cc, P = feats.shape
    out = _out(out, (B, P, P), torch.float32, feats.device)
    ws = _ws(lib().excel_feature_affinity_grouped_workspace_bytes(B, Cc, P, int(group)), feats.device)
    check(lib().excel_feature_affinity_grouped(_p(feats), B, Cc, P, int(group), int(member_stride), float(beta), float(gamma),
                                               {"sigmoid": 0, "mask_softmax": 1}[mode], _p(out), _p(ws, torch.uint8), _stream()),
          "excel_feature_affinity_grouped")
    return out


def compute_trans_mat(w_aff):
    """[B,P,P] (or [P,P]) -> trans_mat, same shape (utils/affutils.py:8-24)."""
    single = w_aff.dim() == 2
    w = f32c(w_aff[None] if single else w_aff)
    B, P, _ = w.shape
    out = torch.empty_like(w)
    ws = _ws(lib().excel_trans_mat_workspace_bytes(B, P), w.device)
    check(lib().excel_compute_trans_mat(_p(w), B, P, _p(out), _p(ws, torch.uint8), _stream()), "excel_compute_trans_mat")
    return out[0] if single else out


def cls_compact(onehot, smax, want_nchan=False):
    """one-hot [B,F] -> (cls_idx [B,smax] int32, ncls [B] int32[, nchan = ncls+1])."""
    onehot = f32c(onehot)
    B, F_ = onehot.shape
    idx = torch.empty((B, smax), dtype=torch.int32, device=onehot.device)
    n = torch.empty((B,), dtype=torch.int32, device=onehot.device)
    nch = torch.empty((B,), dtype=torch.int32, device=onehot.device) if want_nchan else None
    check(lib().excel_cls_compact(_p(onehot), B, F_, smax, _p(idx, torch.int32), _p(n, torch.int32), _p(nch, torch.int32),
                                  _stream()), "excel_cls_compact")
    return (idx, n, nch) if want_nchan else (idx, n)


def scoremap_box_mask(attr, cls_idx, ncls, g, caa_thre=0.79, want_mask=False):
    attr = f32c(attr)
    B, P, F_ = attr.shape
    smax = cls_idx.shape[1]
    v = torch.zeros((B, smax, P), dtype=torch.float32, device=attr.device)
    m = torch.zeros((B, smax, P), dtype=torch.uint8, device=attr.device) if want_mask else None
    check(lib().excel_scoremap_box_mask(_p(attr), _p(cls_idx, torch.int32), _p(ncls, torch.int32), B, g, F_, smax, float(caa_thre),
                                        _p(v), _p(m, torch.uint8), _stream()), "excel_scoremap_box_mask")
    return v, m


def refine_cams_with_aff_batched(attr, w_aff, cls_idx, ncls, g, caa_thre=0.79):
    """attr [B,P,F], w_aff [B,P,P] -> refined [B,Smax,P] (rows >= ncls[b] are zero)."""
    attr = f32c(attr)
    w_aff = f32c(w_aff)
    B, P, F_ = attr.shape
    smax = cls_idx.shape[1]
    out = torch.zeros((B, smax, P), dtype=torch.float32, device=attr.device)
    ws = _ws(lib().excel_refine_workspace_bytes(B, P, smax), attr.device)
    check(lib().excel_refine_cams_with_aff(_p(attr), _p(w_aff), _p(cls_idx, torch.int32), _p(ncls, torch.int32), B, g, F_, smax,
                                           float(caa_thre), _p(out), _p(ws, torch.uint8), _stream()), "excel_refine_cams_with_aff")
    return out


def _out(out, shape, dtype, device, zero=False):
    """A caller-provided output buffer (the pipeline keeps its buffers across steps: no allocator traffic, no fill launches) or a fresh one."""
    if out is not None:
        if tuple(out.shape) != tuple(shape) or out.dtype != dtype or not out.is_contiguous():
            raise ValueError(f"out= must be a contiguous {dtype} tensor of shape {tuple(shape)}, got {out.dtype} {tuple(out.shape)}")
        return out
    return (torch.zeros if zero else torch.empty)(shape, dtype=dtype, device=device)


def cam_upsample_bkg(refined, ncls, g, H, W, out=None, zero_unused=True):
    """refined [B,Smax,P] -> cams [B,Smax+1,H,W] (channel 0 background; channels > ncls[b] are zero unless zero_unused=False:
    nothing on the path reads them)."""
    refined = f32c(refined)
    B, smax, P = refined.shape
    cams = _out(out, (B, smax + 1, H, W), torch.float32, refined.device)
    ws = _ws(B * smax * P * 4, refined.device)
    check(lib().excel_cam_upsample_bkg(_p(refined), _p(ncls, torch.int32), B, g, smax, H, W, _p(cams), _p(ws, torch.uint8),
                                       1 if zero_unused else 0, _stream()), "excel_cam_upsample_bkg")
    return cams


# ------------------------------------------------------------------ PAR / labels / metric
def par_forward(imgs, masks, dilations=PAR_DILATIONS, num_iter=20, nchan=None, w1=0.3, w2=0.01, stream_affinities=False, out=None, ws=None):
    """stream_affinities: stream the 8*ndil affinity planes instead of recomputing them per step (bit-identical outputs; the
    reference form of the recomputing kernel, and what shapes / dilation sets outside its envelope use anyway).
    Channels >= nchan[b] of `out` are not written (zero in a fresh tensor)."""
    # imgs, masks and out go as they are: the library plans the streamed-plane kernels when one of them is not 16-byte aligned (same
    # bits); the workspace is carved into fp32 planes
    _written(ws, "par_forward", "ws", 4)
    imgs = f32c(imgs)
    masks = f32c(masks)
    B, Cmax, H, W = masks.shape
    assert imgs.shape[0] == B and imgs.shape[1] == 3
    h, w = imgs.shape[-2:]
    out = _out(out, masks.shape, torch.float32, masks.device, zero=nchan is not None)
    dil = (C.c_int32 * len(dilations))(*dilations)
    need = lib().excel_par_workspace_bytes(B, Cmax, H, W, len(dilations))
    if ws is None or ws.numel() < need:
        ws = _ws(need, masks.device)
    check(lib().excel_par_forward(_p(imgs), h, w, _p(masks), _p(nchan, torch.int32), B, Cmax, H, W, dil, len(dilations), num_iter,
                                  w1, w2, _p(out), _p(ws, torch.uint8), 1 if stream_affinities else 0, _stream()), "excel_par_forward")
    return out


PAR_PLAN_STATS = ("tile", "pointwise_compact", "pointwise_planes")   # excel_par_plan (include/excel_hip.h)
PAR_PLAN_STEPS = ("none", "recompute", "stream")
PAR_PLAN_REFUSALS = (None, "n_iter", "dilations", "alignment", "size")


def par_plan(B, Cmax, H, W, dilations=PAR_DILATIONS, num_iter=20, guide_hw=None, stream_affinities=False, ragged=False, aligned16=True):
    """The kernels par_forward (ragged=False) or par_forward_ragged (ragged=True: B images of H x W each) runs on (host arithmetic
    only): whether the guide (guide_hw, default (H, W)) is resized, the statistics kernel ("tile" / "pointwise_compact" /
    "pointwise_planes") and its instance nd, the step kernel ("none" / "recompute" / "stream"), both grids and block sizes, the interior
    and border tiles of one image (tile kernels), and for a ragged request the library does not take, `refused` = the reason."""
    h, w = (H, W) if guide_hw is None else guide_hw
    dil = (C.c_int32 * len(dilations))(*dilations)
    plan = (C.c_int32 * 15)()
    check(lib().excel_par_plan(B, Cmax, h, w, H, W, dil, len(dilations), num_iter, 1 if stream_affinities else 0, int(ragged), int(aligned16),
                               plan), "excel_par_plan")
    v = list(plan)
    return dict(resize=bool(v[0]), stats=PAR_PLAN_STATS[v[1]], nd=v[2], step=PAR_PLAN_STEPS[v[3]], stats_grid=tuple(v[4:7]), stats_block=v[7],
                step_grid=tuple(v[8:11]), step_block=v[11], tiles_interior=v[12], tiles_border=v[13], refused=PAR_PLAN_REFUSALS[v[14]])


# ------------------------------------------------------------------ ragged batches (images of different label sizes in one launch)
class RaggedPlan:
    """Tile map + offsets of a batch of images with different (H_b, W_b) (include/excel_hip.h, "ragged batches").
    `hw`: sequence of (H, W).  The table is built on the host by the library (excel_ragged_plan) and copied to the device once."""

    def __init__(self, hw, device):
        import numpy as np
        hw = np.ascontiguousarray(np.asarray(hw, np.int32).reshape(-1, 2))
        self.hw = hw
        self.B = int(hw.shape[0])
        self.info = _lib.RaggedInfo()
        ptr = hw.ctypes.data_as(C.POINTER(C.c_int32))
        check(lib().excel_ragged_plan(ptr, self.B, C.byref(self.info), None), "excel_ragged_plan")
        table = np.empty(int(self.info.table_ints), np.int32)
        check(lib().excel_ragged_plan(ptr, self.B, C.byref(self.info), table.ctypes.data_as(C.POINTER(C.c_int32))), "excel_ragged_plan")
        self.table_host = table
        rec = table[:8 * (self.B + 1)].reshape(self.B + 1, 8)
        self.poff = rec[:, 2].astype(np.int64)          # [B+1] element offsets of the images in a one-plane pitched tensor
        self.loff = rec[:, 4].astype(np.int64)          # [B+1] pixel offsets in a tight u8 map
        self.total_pix = int(self.info.total_pix)
        self.total_label_pix = int(self.info.total_label_pix)
        self.total_tiles = int(self.info.total_tiles)
        self.table = torch.from_numpy(table).to(device, non_blocking=True) if device is not None else None

    def planes(self, packed, b, K):
        """View of image b of a packed K-plane pitched tensor: [K, H_b, W_b] (the row padding sliced off)."""
        H, W = int(self.hw[b, 0]), int(self.hw[b, 1])
        Wp = (W + 3) // 4 * 4
        o = K * int(self.poff[b])
        return packed[o:o + K * H * Wp].view(K, H, Wp)[:, :, :W]

    def label(self, packed_u8, b):
        H, W = int(self.hw[b, 0]), int(self.hw[b, 1])
        o = int(self.loff[b])
        return packed_u8[o:o + H * W].view(H, W)


def normalize_resize_u8_ragged(hwc_packed, plan, S, mean=(123.675, 116.28, 103.53), std=(58.395, 57.12, 57.375), out=None):
    """decoded uint8 HWC images of different sizes, packed back to back -> normalised, bilinearly resized network input [B,3,S,S]
    (datasets/transforms.normalize_img + tools/infer_lam.py:74)."""
    if hwc_packed.dtype != torch.uint8 or hwc_packed.numel() != 3 * plan.total_label_pix:
        raise ValueError(f"hwc_packed must hold {3 * plan.total_label_pix} uint8 values")
    out = _out(out, (plan.B, 3, S, S), torch.float32, hwc_packed.device)
    m, s = (C.c_double * 3)(*mean), (C.c_double * 3)(*std)
    check(lib().excel_normalize_resize_u8_ragged(_p(hwc_packed, torch.uint8), _p(plan.table, torch.int32), plan.B, S, m, s, _p(out), _stream()),
          "excel_normalize_resize_u8_ragged")
    return out


def normalize_resize_u8_ragged_mirror(hwc_packed, plan, S, mean=(123.675, 116.28, 103.53), std=(58.395, 57.12, 57.375), out=None):
    """normalize_resize_u8_ragged and its mirror along W in one pass -> [2B,3,S,S] = [x; flip(x)] (utils/camutils.py:15)."""
    if hwc_packed.dtype != torch.uint8 or hwc_packed.numel() != 3 * plan.total_label_pix:
        raise ValueError(f"hwc_packed must hold {3 * plan.total_label_pix} uint8 values")
    out = _out(out, (2 * plan.B, 3, S, S), torch.float32, hwc_packed.device)
    m, s = (C.c_double * 3)(*mean), (C.c_double * 3)(*std)
    check(lib().excel_normalize_resize_u8_ragged_mirror(_p(hwc_packed, torch.uint8), _p(plan.table, torch.int32), plan.B, S, m, s, _p(out),
                                                        _stream()), "excel_normalize_resize_u8_ragged_mirror")
    return out


# ------------------------------------------------------------------ CAM overlay images (include/excel_hip.h, camviz.hip)
CAM_OVERLAY_MODES = {"max": 0, "per_class": 1}
_CAM_TABLES = {}


def cam_overlay_tables(alpha, device, mean=(123.675, 116.28, 103.53), std=(58.395, 57.12, 57.375)):
    """Device copy (float64 [2,768], built once per alpha / normalisation / device) of utils.imutils.cam_overlay_tables."""
    key = (float(alpha), tuple(mean), tuple(std), str(device))
    t = _CAM_TABLES.get(key)
    if t is None:
        from .utils import imutils
        t = _CAM_TABLES[key] = torch.from_numpy(imutils.cam_overlay_tables(alpha, mean, std)).to(device)
    return t


def _pinned_upload(a, dtype, device):
    """small host array -> device, through pinned memory (a pageable copy would make the host wait for the stream)"""
    import numpy as np
    h = torch.from_numpy(np.ascontiguousarray(a)).to(dtype).pin_memory()
    return h.to(device, non_blocking=True)


def cam_overlay_ragged(hwc_packed, cams, plan, Cmax, ncls, mode="max", alpha=None, mean=(123.675, 116.28, 103.53),
                       std=(58.395, 57.12, 57.375)):
    """tools/infer_lam.py:97-111 for a ragged batch: the jet-coloured CAM blended over the photo, every image at its own size.
    hwc_packed = the decoded uint8 images (image b at byte 3 * loff_b), cams = Cmax pitched planes per image (plane 0 = background;
    the pipeline's step buffer may be passed as it is: only x < W_b and planes 1..k_b are read), ncls = the HOST array of k_b (present
    classes per image, from the batch's one-hot rows).  mode "max": alpha 0.5, one overlay per image with k_b >= 1; "per_class":
    alpha 0.6, k_b overlays per image.  -> (out: flat uint8 device tensor, off: host int64 [B] byte offset of image b's first overlay);
    overlay c of image b is out[off_b + 3*c*H_b*W_b :][: 3*H_b*W_b] as [H_b, W_b, 3]; in "max" mode the bytes of an image with k_b = 0
    are left unwritten."""
    import numpy as np
    if mode not in CAM_OVERLAY_MODES:
        raise ValueError(f"mode must be one of {sorted(CAM_OVERLAY_MODES)}, got {mode!r}")
    if alpha is None:
        alpha = 0.5 if mode == "max" else 0.6
    ncls = np.asarray(ncls, np.int64).reshape(-1)
    if ncls.shape[0] != plan.B or (ncls < 0).any() or (ncls > Cmax - 1).any():
        raise ValueError(f"ncls: need {plan.B} values in [0, Cmax - 1 = {Cmax - 1}], got {ncls.tolist()}")
    if hwc_packed.dtype != torch.uint8 or hwc_packed.numel() != 3 * plan.total_label_pix:
        raise ValueError(f"hwc_packed must hold {3 * plan.total_label_pix} uint8 values")
    if cams.numel() < Cmax * plan.total_pix:
        raise ValueError(f"cams must hold Cmax * total_pix = {Cmax * plan.total_pix} floats, got {cams.numel()}")
    dev = hwc_packed.device
    hw = plan.hw.astype(np.int64)
    if mode == "max":
        off = 3 * plan.loff[:plan.B]
        nbytes = 3 * plan.total_label_pix
    else:
        sizes = 3 * ncls * hw[:, 0] * hw[:, 1]
        off = np.concatenate([[0], np.cumsum(sizes)])[:plan.B]
        nbytes = int(sizes.sum())
    out = torch.empty(max(int(nbytes), 1), dtype=torch.uint8, device=dev)[:int(nbytes)]
    if nbytes == 0:
        return out, off
    n_dev = _pinned_upload(ncls, torch.int32, dev)
    off_dev = _pinned_upload(off, torch.int64, dev) if mode == "per_class" else None
    tabs = cam_overlay_tables(alpha, dev, mean, std)
    check(lib().excel_cam_overlay_ragged(_p(hwc_packed, torch.uint8), _p(cams[:Cmax * plan.total_pix]), Cmax, _p(n_dev, torch.int32),
                                         _p(off_dev, torch.int64), _p(plan.table, torch.int32), C.byref(plan.info), CAM_OVERLAY_MODES[mode],
                                         _p(tabs, torch.float64), _p(out, torch.uint8), _stream()), "excel_cam_overlay_ragged")
    return out, off


def cam_overlay(hwc, cams, mode="max", alpha=None, mean=(123.675, 116.28, 103.53), std=(58.395, 57.12, 57.375)):
    """One image (the per-image path): hwc uint8 [H,W,3], cams tight f32 [1+k,H,W] (refine_cams_with_bkg_weclip's normed maps) ->
    "max": [H,W,3] (None when k == 0); "per_class": [k,H,W,3]."""
    if mode not in CAM_OVERLAY_MODES:
        raise ValueError(f"mode must be one of {sorted(CAM_OVERLAY_MODES)}, got {mode!r}")
    if alpha is None:
        alpha = 0.5 if mode == "max" else 0.6
    cams = f32c(cams)
    k, H, W = cams.shape[0] - 1, cams.shape[1], cams.shape[2]
    if hwc.dtype != torch.uint8 or tuple(hwc.shape) != (H, W, 3):
        raise ValueError(f"hwc must be uint8 [{H},{W},3], got {hwc.dtype} {tuple(hwc.shape)}")
    if mode == "max" and k == 0:
        return None
    out = torch.empty((H, W, 3) if mode == "max" else (k, H, W, 3), dtype=torch.uint8, device=cams.device)
    if out.numel() == 0:
        return out
    tabs = cam_overlay_tables(alpha, cams.device, mean, std)
    check(lib().excel_cam_overlay(_p(hwc.contiguous(), torch.uint8), _p(cams), k, H, W, CAM_OVERLAY_MODES[mode], _p(tabs, torch.float64),
                                  _p(out, torch.uint8), _stream()), "excel_cam_overlay")
    return out


# ------------------------------------------------------------------ training-progress panels (include/excel_hip.h, trainviz.hip)
TRAIN_PANELS = ("img1", "cam1", "pseu_aff", "pseu_mid", "seg_gt", "seg_pred")     # bit k of the C ABI's panel_mask; the reference's tag order
TB_MEAN, TB_STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)                     # utils/tbutils.py:28
_PANEL_TABLES = {}


def train_panels_plan(B, S, g, panels=TRAIN_PANELS, nrow=2):
    """excel_train_panels_plan (host only) -> ({name: (Hg, Wg, byte offset)} of the requested panels in panel order, total bytes)."""
    unknown = [n for n in panels if n not in TRAIN_PANELS]
    if unknown:
        raise ValueError(f"unknown panels {unknown}; known: {list(TRAIN_PANELS)}")
    mask = sum(1 << TRAIN_PANELS.index(n) for n in set(panels))
    out = (C.c_int64 * (3 * len(TRAIN_PANELS) + 1))()
    check(lib().excel_train_panels_plan(int(B), int(nrow), int(S), int(g), mask, out), "excel_train_panels_plan")
    plan = {n: (int(out[3 * k]), int(out[3 * k + 1]), int(out[3 * k + 2])) for k, n in enumerate(TRAIN_PANELS) if (mask >> k) & 1}
    return plan, int(out[3 * len(TRAIN_PANELS)])


class TrainPanels(dict):
    """panel name -> uint8 [Hg,Wg,3] device view; `buffer` is the one flat uint8 tensor the views share and `plan` their
    (Hg, Wg, byte offset), so a caller that wants the panels on the host makes ONE copy (host())."""
    buffer = None
    plan = None

    def host(self):
        """-> {name: numpy uint8 [Hg,Wg,3]} from one device-to-host copy of the shared buffer"""
        buf = self.buffer.cpu().numpy()
        return {n: buf[off:off + 3 * Hg * Wg].reshape(Hg, Wg, 3) for n, (Hg, Wg, off) in self.plan.items()}


def _panel_tables(device):
    """(0.5 * (jet * 255) as float64 [256,3], the VOC palette uint8 [256,3]) on the device, built once per device"""
    t = _PANEL_TABLES.get(str(device))
    if t is None:
        from .utils import imutils
        t = _PANEL_TABLES[str(device)] = (torch.from_numpy(imutils.jet_lut() * 255 * 0.5).contiguous().to(device),
                                          torch.from_numpy(imutils.colormap()).contiguous().to(device))
    return t


def train_panels(inputs=None, attr_maps_raw=None, cls_label=None, pseu_aff=None, pseu_mid=None, seg_gt=None, seg_pred=None, nrow=2,
                 panels=None, S=None, g=None):
    """The image grids of scripts/train_voc.py:233-246 (utils/tbutils.py make_grid_image / make_grid_label) for one training batch in
    one launch: inputs f32 [B,3,S,S] normalised, attr_maps_raw f32 [B,P,F] (P = g*g), cls_label [B,F], label maps uint8 [B,S,S]
    (pseu_mid: [B,g,g]).  `panels` defaults to every panel whose inputs were given (img1 needs inputs; cam1 inputs, attr_maps_raw and
    cls_label).  S / g are taken from the tensors.  -> TrainPanels: name -> uint8 [Hg,Wg,3] views of one device buffer."""
    given = dict(pseu_aff=pseu_aff, pseu_mid=pseu_mid, seg_gt=seg_gt, seg_pred=seg_pred)
    if panels is None:
        panels = [n for n in TRAIN_PANELS if (n == "img1" and inputs is not None)
                  or (n == "cam1" and inputs is not None and attr_maps_raw is not None and cls_label is not None)
                  or given.get(n) is not None]
    if not panels:
        raise ValueError("train_panels: nothing to render")
    ref = inputs if inputs is not None else next((t for n, t in given.items() if n != "pseu_mid" and t is not None), None)
    B = int((ref if ref is not None else pseu_mid).shape[0])
    S = int(ref.shape[-1]) if ref is not None else int(S or 1)
    if ref is not None and tuple(ref.shape[-2:]) != (S, S):
        raise ValueError(f"train_panels needs square crops, got {tuple(ref.shape[-2:])}")
    F_ = P = 0
    if attr_maps_raw is not None:
        attr_maps_raw = f32c(attr_maps_raw)
        P, F_ = int(attr_maps_raw.shape[1]), int(attr_maps_raw.shape[2])
        g = int(round(P ** 0.5)) if g is None else int(g)
        cls_label = f32c(cls_label) if cls_label is not None else None
        if cls_label is not None and tuple(cls_label.shape) != (B, F_):
            raise ValueError(f"cls_label must be [{B},{F_}], got {tuple(cls_label.shape)}")
    elif pseu_mid is not None:
        g = int(pseu_mid.shape[-1])
    g = int(g or 1)
    dev = (ref if ref is not None else pseu_mid).device
    labs = []
    for n, side in (("pseu_aff", S), ("pseu_mid", g), ("seg_gt", S), ("seg_pred", S)):
        t = given[n]
        if t is not None:
            if t.dtype != torch.uint8 or tuple(t.shape) != (B, side, side):
                raise ValueError(f"{n} must be uint8 [{B},{side},{side}], got {t.dtype} {tuple(t.shape)}")
            t = t.contiguous()
        labs.append(t)
    if inputs is not None:
        inputs = f32c(inputs)
        if tuple(inputs.shape) != (B, 3, S, S):
            raise ValueError(f"inputs must be [B,3,S,S], got {tuple(inputs.shape)}")
    plan, total = train_panels_plan(B, S, g, panels, nrow)
    mask = sum(1 << TRAIN_PANELS.index(n) for n in plan)
    out = torch.empty(total, dtype=torch.uint8, device=dev)
    jet, pal = _panel_tables(dev)
    m, s = (C.c_float * 3)(*TB_MEAN), (C.c_float * 3)(*TB_STD)
    check(lib().excel_train_panels(_p(inputs), _p(attr_maps_raw), _p(cls_label), *[_p(t, torch.uint8) for t in labs], B, F_, P, g, S, int(nrow),
                                   mask, m, s, _p(jet, torch.float64), _p(pal, torch.uint8), _p(out, torch.uint8), total, _stream()),
          "excel_train_panels")
    res = TrainPanels((n, out[off:off + 3 * Hg * Wg].view(Hg, Wg, 3)) for n, (Hg, Wg, off) in plan.items())
    res.buffer, res.plan = out, plan
    return res


# ------------------------------------------------------------------ label PNG files (include/excel_hip.h, png.hip)
_PNG_PALETTES = {}


def png_labels_bound_bytes(H, W):
    """Bytes that bound the PNG file of one H x W label map (excel_png_labels_bound_bytes); also the size of its slot in the arena."""
    return int(lib().excel_png_labels_bound_bytes(int(H), int(W)))


def png_labels_arena_bytes(hw):
    """Arena bytes png_encode_labels_ragged needs for images of the sizes `hw` [(H, W)]: the sum of their bounds."""
    return sum(png_labels_bound_bytes(h, w) for h, w in hw)


def _png_palette(palette, device):
    """uint8 [256,3] (None: utils.imutils.colormap(), the VOC colour map of SegmentationClassAug) -> flat device tensor, cached per device."""
    import numpy as np
    from .utils import imutils
    pal = imutils.colormap() if palette is None else np.asarray(palette)
    if pal.dtype != np.uint8 or pal.size != 768:
        raise ValueError(f"palette must hold 256 RGB uint8 entries, got {pal.dtype} {pal.shape}")
    key = (pal.tobytes(), str(device))
    t = _PNG_PALETTES.get(key)
    if t is None:
        if len(_PNG_PALETTES) > 16:
            _PNG_PALETTES.clear()
        t = _PNG_PALETTES[key] = torch.from_numpy(np.ascontiguousarray(pal).reshape(-1).copy()).to(device)
    return t


def png_encode_labels_ragged(labels_flat, plan, palette=None, out=None, ws=None):
    """tools/infer_lam.py:95 / tools/training_free_attr.py:225 for a ragged batch, on the device: the flat uint8 label maps
    argmax_label_ragged writes (or a uniform [B,H,W] uint8 tensor with plan=None: the same entry over a plan of equal sizes) -> one
    complete palette PNG file per image.  palette: uint8 [256,3], None = imutils.colormap() (the VOC colour map).
    -> (bytes: flat uint8 device tensor, table: int64 device tensor [B,2] of (offset, size)); file b = bytes[off_b:off_b + size_b], and
    off_b = the sum of png_labels_bound_bytes over the images in front, which the host knows without the table.
    out: a flat uint8 device tensor of at least png_labels_arena_bytes(plan.hw) bytes to encode into (a view of it is returned);
    ws: a uint8 device tensor for the row records (grown when too small is the caller's business: too small is an error)."""
    import numpy as np
    if plan is None:
        if labels_flat.dim() != 3:
            raise ValueError("plan=None needs a uniform [B,H,W] label tensor")
        Bn, H, W = labels_flat.shape
        plan = RaggedPlan([(H, W)] * Bn, labels_flat.device)
    if labels_flat.dtype != torch.uint8 or labels_flat.numel() != plan.total_label_pix:
        raise ValueError(f"labels must hold {plan.total_label_pix} uint8 values, got {labels_flat.dtype} x {labels_flat.numel()}")
    dev = labels_flat.device
    hw = np.ascontiguousarray(plan.hw, np.int32)
    need = png_labels_arena_bytes(hw)
    if out is None:
        out = torch.empty(need, dtype=torch.uint8, device=dev)
    elif out.dtype != torch.uint8 or out.dim() != 1 or not out.is_contiguous():
        raise ValueError("out= must be a flat contiguous uint8 tensor")
    _written(out, "png_encode_labels_ragged", "out", 4)      # the arena is cleared and filled in 32-bit words
    _written(ws, "png_encode_labels_ragged", "ws", 8)        # 8-byte row records
    ws_need = int(lib().excel_png_labels_workspace_bytes(plan.B, int(hw[:, 0].max())))
    if ws is None:
        ws = _ws(ws_need, dev)
    table = torch.empty((plan.B, 2), dtype=torch.int64, device=dev)
    check(lib().excel_png_encode_labels_ragged(_p(labels_flat.contiguous().view(-1), torch.uint8), _p(plan.table, torch.int32), C.byref(plan.info),
                                               hw.ctypes.data_as(C.POINTER(C.c_int32)), _p(_png_palette(palette, dev), torch.uint8),
                                               _p(out, torch.uint8), out.numel(), _p(table, torch.int64), _p(ws, torch.uint8), ws.numel(),
                                               _stream()), "excel_png_encode_labels_ragged")
    return out[:need], table


# ------------------------------------------------------------------ CAM overlay JPEG files (include/excel_hip.h, jpeg.hip)
JPEG_HEADER_BYTES = 623          # SOI .. SOS; a file is this, the entropy-coded segment and the 2 bytes of EOI


def _jpeg_items(items):
    import numpy as np
    it = np.asarray(items, np.int64).reshape(-1, 3)
    if it.shape[0] < 1:
        raise ValueError("jpeg_encode_rgb_ragged needs at least one image")
    return np.ascontiguousarray(it[:, 0]), np.ascontiguousarray(it[:, 1:].astype(np.int32))


def jpeg_rgb_arena_bytes(hw):
    """Arena bytes that bound the files of RGB images of the sizes `hw` [(H, W)]: 625 + 3 H W each (excel_jpeg_rgb_arena_bytes)."""
    import numpy as np
    hw = np.ascontiguousarray(np.asarray(hw, np.int32).reshape(-1, 2))
    return int(lib().excel_jpeg_rgb_arena_bytes(hw.ctypes.data_as(C.POINTER(C.c_int32)), hw.shape[0]))


def jpeg_rgb_workspace_bytes(hw):
    """Workspace bytes of jpeg_encode_rgb_ragged for images of the sizes `hw` [(H, W)] (excel_jpeg_rgb_workspace_bytes)."""
    import numpy as np
    hw = np.ascontiguousarray(np.asarray(hw, np.int32).reshape(-1, 2))
    return int(lib().excel_jpeg_rgb_workspace_bytes(hw.ctypes.data_as(C.POINTER(C.c_int32)), hw.shape[0]))


def jpeg_encode_rgb_ragged(rgb_flat, items, quality=75, out=None, ws=None):
    """tools/infer_lam.py:104,111 for a ragged batch, on the device: rgb_flat = the flat uint8 buffer cam_overlay_ragged writes, items =
    [(byte offset, H, W)] of the tight [H,W,3] images in it -> one complete baseline JPEG file per image, the bytes Pillow writes at
    `quality`.  -> (bytes: flat uint8 device tensor, table: int64 device tensor [n,2] of (offset, size)); the files lie back to back,
    file i = bytes[off_i:off_i + size_i].  size -1: the file would have ended behind the arena and was not written (encode that image
    on the host).  out: a flat uint8 device tensor to encode into, of any size (None: jpeg_rgb_arena_bytes, which the files are
    expected to stay below); ws: a uint8 device tensor of at least jpeg_rgb_workspace_bytes (too small is an error)."""
    off, hw = _jpeg_items(items)
    if rgb_flat.dtype != torch.uint8 or rgb_flat.dim() != 1 or not rgb_flat.is_contiguous():
        raise ValueError("rgb_flat must be a flat contiguous uint8 tensor")
    ends = off + 3 * hw[:, 0].astype("int64") * hw[:, 1].astype("int64")
    if (off < 0).any() or int(ends.max()) > rgb_flat.numel():
        raise ValueError(f"items reach byte {int(ends.max())} of a buffer of {rgb_flat.numel()} bytes (or hold a negative offset)")
    dev = rgb_flat.device
    n = int(hw.shape[0])
    hw_p, off_p = hw.ctypes.data_as(C.POINTER(C.c_int32)), off.ctypes.data_as(C.POINTER(C.c_int64))
    if out is None:
        out = torch.empty(max(int(lib().excel_jpeg_rgb_arena_bytes(hw_p, n)), 1), dtype=torch.uint8, device=dev)
    elif out.dtype != torch.uint8 or out.dim() != 1 or not out.is_contiguous():
        raise ValueError("out= must be a flat contiguous uint8 tensor")
    _written(ws, "jpeg_encode_rgb_ragged", "ws")             # records, coefficients and 16-byte chunks of stream words
    if ws is None:
        ws = _ws(max(int(lib().excel_jpeg_rgb_workspace_bytes(hw_p, n)), 1), dev)
    table = torch.empty((n, 2), dtype=torch.int64, device=dev)
    check(lib().excel_jpeg_encode_rgb_ragged(_p(rgb_flat, torch.uint8), off_p, hw_p, n, int(quality), _p(out, torch.uint8), out.numel(),
                                             _p(table, torch.int64), _p(ws, torch.uint8), ws.numel(), _stream()), "excel_jpeg_encode_rgb_ragged")
    return out, table


# ------------------------------------------------------------------ training augmentation (include/excel_hip.h, aug.hip)
AUG_CANDIDATES = 10
# one record per image, laid out like excel_aug_params (C alignment: 104 bytes)
AUG_PARAMS_DTYPE = None


def aug_params_dtype():
    import numpy as np
    global AUG_PARAMS_DTYPE
    if AUG_PARAMS_DTYPE is None:
        AUG_PARAMS_DTYPE = np.dtype([("ratio", "<f8"), ("flip", "<i4"), ("h_pad", "<i4"), ("w_pad", "<i4"),
                                     ("cand_h", "<i4", (AUG_CANDIDATES,)), ("cand_w", "<i4", (AUG_CANDIDATES,))], align=True)
        assert AUG_PARAMS_DTYPE.itemsize == C.sizeof(_lib.AugParams)
    return AUG_PARAMS_DTYPE


class TrainAugPlan:
    """Host half of ops.train_augment: excel_train_aug_plan checks every size and parameter and builds the table of Pillow's
    BILINEAR coefficients and NEAREST indices (a host function, no device work); `table` is its device copy when `device` is given."""

    def __init__(self, hw, params, S, device):
        import numpy as np
        hw = np.ascontiguousarray(np.asarray(hw, np.int32).reshape(-1, 2))
        params = np.ascontiguousarray(params, dtype=aug_params_dtype())
        if params.shape != (hw.shape[0],):
            raise ValueError(f"params: {params.shape[0] if params.ndim else 0} records for {hw.shape[0]} images")
        self.B, self.S = int(hw.shape[0]), int(S)
        self.hw, self.params = hw, params
        self.info = _lib.TrainAugInfo()
        hp = hw.ctypes.data_as(C.POINTER(C.c_int32))
        pp = params.ctypes.data_as(C.POINTER(_lib.AugParams))
        check(lib().excel_train_aug_plan(hp, pp, self.B, self.S, C.byref(self.info), None), "excel_train_aug_plan")
        table = np.empty(int(self.info.table_ints), np.int32)
        check(lib().excel_train_aug_plan(hp, pp, self.B, self.S, C.byref(self.info), table.ctypes.data_as(C.POINTER(C.c_int32))),
              "excel_train_aug_plan")
        self.table_host = table
        self.workspace_bytes = int(lib().excel_train_augment_workspace_bytes(C.byref(self.info)))
        self.table = None
        if device is not None:        # pinned source: the copy is queued on the current stream, the host does not wait for it
            self.table = torch.from_numpy(table).pin_memory().to(device, non_blocking=True)


def train_augment(images_u8, plan, labels_u8, params, crop_size, mean=(123.675, 116.28, 103.53), std=(58.395, 57.12, 57.375),
                  aug_plan=None):
    """VOC12ClsDataset(aug=True)'s transform (datasets/voc.py:110-117) on the device for a ragged batch: packed uint8 HWC images and
    uint8 label maps (RaggedPlan layout), `params` = one ops.aug_params_dtype() record per image (the host's random draws)
    -> (img [B,3,S,S] f32 normalised, label [B,S,S] u8 (255 = pad), img_box [B,4] int32).  Queued on the current stream; no host
    synchronisation.  `aug_plan` = a TrainAugPlan built ahead for the same batch and params (e.g. by a staging thread)."""
    S = int(crop_size)
    if S <= 0:
        raise ValueError("crop_size must be positive")
    dev = images_u8.device
    if aug_plan is None:
        aug_plan = TrainAugPlan(plan.hw, params, S, dev)
    if aug_plan.S != S or aug_plan.B != plan.B or aug_plan.table is None:
        raise ValueError("aug_plan was built for another batch / crop size, or without a device table")
    n = int(aug_plan.info.total_label_pix)
    if images_u8.dtype != torch.uint8 or images_u8.numel() != 3 * n:
        raise ValueError(f"images_u8 must hold {3 * n} uint8 values")
    if labels_u8.dtype != torch.uint8 or labels_u8.numel() != n:
        raise ValueError(f"labels_u8 must hold {n} uint8 values")
    B = plan.B
    img = torch.empty((B, 3, S, S), dtype=torch.float32, device=dev)
    label = torch.empty((B, S, S), dtype=torch.uint8, device=dev)
    box = torch.empty((B, 4), dtype=torch.int32, device=dev)
    ws = _ws(aug_plan.workspace_bytes, dev)
    m, s = (C.c_double * 3)(*mean), (C.c_double * 3)(*std)
    check(lib().excel_train_augment(_p(images_u8, torch.uint8), _p(labels_u8, torch.uint8), _p(aug_plan.table, torch.int32),
                                    C.byref(aug_plan.info), m, s, _p(img), _p(label, torch.uint8), _p(box, torch.int32),
                                    _p(ws, torch.uint8), _stream()), "excel_train_augment")
    return img, label, box


def train_augment_image(images_u8, plan, params, crop_size, aug_plan=None, mean=(123.675, 116.28, 103.53), std=(58.395, 57.12, 57.375)):
    """CocoClsDataset(aug=True)'s transform (datasets/coco.py:112-142) on the device for a ragged batch of packed uint8 HWC images that
    carry no label map: as train_augment, but the crop is candidate 0 of each record (get_random_cropbox's first draw when the label
    is None) -> (img [B,3,S,S] f32 normalised, img_box [B,4] int32).  Queued on the current stream; no host synchronisation."""
    S = int(crop_size)
    if S <= 0:
        raise ValueError("crop_size must be positive")
    dev = images_u8.device
    if aug_plan is None:
        aug_plan = TrainAugPlan(plan.hw, params, S, dev)
    if aug_plan.S != S or aug_plan.B != plan.B or aug_plan.table is None:
        raise ValueError("aug_plan was built for another batch / crop size, or without a device table")
    n = int(aug_plan.info.total_label_pix)
    if images_u8.dtype != torch.uint8 or images_u8.numel() != 3 * n:
        raise ValueError(f"images_u8 must hold {3 * n} uint8 values")
    B = plan.B
    img = torch.empty((B, 3, S, S), dtype=torch.float32, device=dev)
    box = torch.empty((B, 4), dtype=torch.int32, device=dev)
    ws = _ws(aug_plan.workspace_bytes, dev)
    m, s = (C.c_double * 3)(*mean), (C.c_double * 3)(*std)
    check(lib().excel_train_augment_image(_p(images_u8, torch.uint8), _p(aug_plan.table, torch.int32), C.byref(aug_plan.info), m, s,
                                          _p(img), _p(box, torch.int32), _p(ws, torch.uint8), _stream()), "excel_train_augment_image")
    return img, box


def cam_upsample_bkg_ragged(refined, ncls, g, plan, out=None, zero_unused=True):
    """refined [B,Smax,P] -> packed cams: (Smax+1) pitched planes per image at its own (H_b, W_b).  The pad columns (x >= W_b) of the
    pitched rows are not written, and with zero_unused=False neither are the planes > ncls[b]: every consumer stops at W_b and nchan[b]."""
    _written(out, "cam_upsample_bkg_ragged", "out")      # pitched planes: every row starts on a 16-byte boundary
    refined = f32c(refined)
    B, smax, P = refined.shape
    assert B == plan.B
    cams = _out(out, ((smax + 1) * plan.total_pix,), torch.float32, refined.device)
    ws = _ws(B * smax * P * 4, refined.device)
    check(lib().excel_cam_upsample_bkg_ragged(_p(refined), _p(ncls, torch.int32), _p(plan.table, torch.int32), C.byref(plan.info), g, smax,
                                              _p(cams), _p(ws, torch.uint8), 1 if zero_unused else 0, _stream()), "excel_cam_upsample_bkg_ragged")
    return cams


def par_forward_ragged(imgs, masks, plan, Cmax, dilations=PAR_DILATIONS, num_iter=20, nchan=None, w1=0.3, w2=0.01, out=None, ws=None):
    """imgs [B,3,h,w] (uniform), masks = Cmax pitched planes per image -> refined masks, same layout."""
    # only the tile kernel exists for ragged batches: it stages masks, out and the workspace in 16-byte pieces
    _written(out, "par_forward_ragged", "out")
    _written(ws, "par_forward_ragged", "ws")
    imgs = f32c(imgs)
    masks = _realign(masks)
    assert imgs.shape[0] == plan.B and imgs.shape[1] == 3 and masks.numel() == Cmax * plan.total_pix
    h, w = imgs.shape[-2:]
    out = _out(out, masks.shape, torch.float32, masks.device, zero=True)
    dil = (C.c_int32 * len(dilations))(*dilations)
    need = lib().excel_par_ragged_workspace_bytes(plan.total_pix, Cmax)
    if ws is None or ws.numel() < need:
        ws = _ws(need, masks.device)
    check(lib().excel_par_forward_ragged(_p(imgs), h, w, _p(masks), _p(nchan, torch.int32), _p(plan.table, torch.int32), C.byref(plan.info), Cmax,
                                         dil, len(dilations), num_iter, w1, w2, _p(out), _p(ws, torch.uint8), _stream()), "excel_par_forward_ragged")
    return out


def argmax_label_ragged(cams, plan, Cmax, nchan=None, cls_idx=None, out=None):
    """packed cams (Cmax pitched planes per image) -> tight uint8 labels [sum H_b*W_b], valid_key lookup applied."""
    smax = cls_idx.shape[1] if cls_idx is not None else Cmax - 1
    lab = _out(out, (plan.total_label_pix,), torch.uint8, cams.device)
    check(lib().excel_argmax_label_ragged(_p(cams), _p(nchan, torch.int32), _p(cls_idx, torch.int32), _p(plan.table, torch.int32), C.byref(plan.info),
                                          smax, Cmax, _p(lab, torch.uint8), _stream()), "excel_argmax_label_ragged")
    return lab


# ------------------------------------------------------------------ confident labels (include/excel_hip.h, "confident labels")
def conf_half_plan(plan, down_scale=2, names=None):
    """The half plan of utils/affutils.py:113: (H_b // ds, W_b // ds) for every image of `plan`.  An image whose half size would be
    empty is refused here, on the host, by name."""
    ds = int(down_scale)
    if ds < 1:
        raise ValueError(f"down_scale must be at least 1 (got {down_scale})")
    hw = [(int(H) // ds, int(W) // ds) for H, W in plan.hw]
    for b, (h, w) in enumerate(hw):
        if h < 1 or w < 1:
            who = str(names[b]) if names is not None else f"image {b}"
            raise ValueError(f"{who}: {int(plan.hw[b, 0])} x {int(plan.hw[b, 1])} pixels leave nothing at down_scale {ds}")
    return RaggedPlan(hw, plan.table.device if plan.table is not None else None)


def conf_planes_ragged(cams, plan, half_plan, smax, nchan, high_thre, low_thre, out=None, softmax=True):
    """utils/affutils.py:115-141 for a ragged batch: cams (smax + 1 pitched planes per image on `plan`; plane 0 is not read),
    nchan [B] = k_b + 1 -> (planes, nchan2): 2 (smax + 1) pitched planes per image on `half_plan`, the softmax over
    [high_thre, m_1 .. m_k] then the one over [low_thre, m_1 .. m_k], and nchan2 = 2 (k_b + 1) for par_forward_ragged.
    Planes >= nchan2[b] and the pad columns are not written.  softmax=False (tests): the resized values alone, in the first group."""
    if plan.B != half_plan.B:
        raise ValueError(f"conf_planes_ragged: plans of {plan.B} and {half_plan.B} images")
    if cams.numel() != (smax + 1) * plan.total_pix:
        raise ValueError(f"conf_planes_ragged: cams must hold (smax + 1) * total_pix = {(smax + 1) * plan.total_pix} floats")
    if nchan.numel() != plan.B:
        raise ValueError(f"conf_planes_ragged: nchan holds {nchan.numel()} counts for {plan.B} images")
    planes = _out(out, (2 * (smax + 1) * half_plan.total_pix,), torch.float32, cams.device)
    nchan2 = torch.empty((plan.B,), dtype=torch.int32, device=cams.device)
    check(lib().excel_conf_planes_ragged(_p(cams), _p(nchan, torch.int32), _p(plan.table, torch.int32), C.byref(plan.info),
                                         _p(half_plan.table, torch.int32), C.byref(half_plan.info), int(smax), float(high_thre), float(low_thre),
                                         1 if softmax else 0, _p(planes), _p(nchan2, torch.int32), _stream()), "excel_conf_planes_ragged")
    return planes, nchan2


def conf_merge_ragged(planes, half_plan, plan, smax, nchan, cls_idx=None, img_box=None, ignore_index=255, out=None):
    """utils/affutils.py:94-96 for both groups, :146-156 for a ragged batch: planes (2 (smax + 1) pitched planes per image on
    `half_plan`, PAR's output) -> tight uint8 labels on `plan`: per group bilinear + first-maximum arg-max + key lookup, then
    lab_h where it is a class, 0 where both groups say background, ignore_index between.  img_box: int32 [B,4] (y0, y1, x0, x1) on
    the device; pixels outside get ignore_index."""
    if plan.B != half_plan.B:
        raise ValueError(f"conf_merge_ragged: plans of {half_plan.B} and {plan.B} images")
    if planes.numel() != 2 * (smax + 1) * half_plan.total_pix:
        raise ValueError(f"conf_merge_ragged: planes must hold 2 * (smax + 1) * total_pix = {2 * (smax + 1) * half_plan.total_pix} floats")
    if nchan.numel() != plan.B:
        raise ValueError(f"conf_merge_ragged: nchan holds {nchan.numel()} counts for {plan.B} images")
    if cls_idx is not None and tuple(cls_idx.shape) != (plan.B, smax):
        raise ValueError(f"conf_merge_ragged: cls_idx must be [B={plan.B}, smax={smax}], got {tuple(cls_idx.shape)}")
    if img_box is not None and (tuple(img_box.shape) != (plan.B, 4) or img_box.dtype != torch.int32):
        raise ValueError(f"conf_merge_ragged: img_box must be int32 [B={plan.B}, 4], got {img_box.dtype} {tuple(img_box.shape)}")
    lab = _out(out, (plan.total_label_pix,), torch.uint8, planes.device)
    check(lib().excel_conf_merge_ragged(_p(planes), _p(nchan, torch.int32), _p(cls_idx, torch.int32), _p(half_plan.table, torch.int32),
                                        C.byref(half_plan.info), _p(plan.table, torch.int32), C.byref(plan.info), int(smax),
                                        _p(img_box, torch.int32), int(ignore_index), _p(lab, torch.uint8), _stream()), "excel_conf_merge_ragged")
    return lab


def argmax_label(cams, nchan=None, cls_idx=None, want_i64=False):
    """cams [B,Cmax,H,W] -> labels u8 [B,H,W] (and int64 copy if asked), valid_key lookup applied."""
    cams = f32c(cams)
    B, Cmax, H, W = cams.shape
    smax = cls_idx.shape[1] if cls_idx is not None else Cmax - 1
    l8 = torch.empty((B, H, W), dtype=torch.uint8, device=cams.device)
    l64 = torch.empty((B, H, W), dtype=torch.int64, device=cams.device) if want_i64 else None
    check(lib().excel_argmax_label(_p(cams), _p(nchan, torch.int32), _p(cls_idx, torch.int32), B, smax, Cmax, H * W,
                                   _p(l8, torch.uint8), _p(l64, torch.int64), _stream()), "excel_argmax_label")
    return (l8, l64) if want_i64 else l8


def confusion_accumulate(gt_u8, pred_u8, num_classes, hist=None):
    """hist (int64 [nc,nc], device) += bincount(nc*gt + pred) over gt < nc."""
    gt = gt_u8.contiguous().view(-1)
    pr = pred_u8.contiguous().view(-1)
    assert gt.numel() == pr.numel()
    if hist is None:
        hist = torch.zeros((num_classes, num_classes), dtype=torch.int64, device=gt.device)
    check(lib().excel_confusion_accumulate(_p(gt, torch.uint8), _p(pr, torch.uint8), gt.numel(), num_classes,
                                           _p(hist, torch.int64), _stream()), "excel_confusion_accumulate")
    return hist


# ------------------------------------------------------------------ overflow guard of the f16 modes (include/excel_hip.h, "overflow guard")
def nonfinite_count(x, out=None, init=True):
    """x: float32 [B, ...] (first dimension = the image; contiguous, 4-byte aligned is enough) -> int32 [B]: per image the number of
    +-inf / NaN values.  init=False ADDS to `out`, so the tensors of one step share one counter.  No workspace, no synchronisation."""
    B = int(x.shape[0])
    if out is None:
        if not init:
            raise ValueError("nonfinite_count: init=False adds to an existing counter: pass out=")
        out = torch.empty((B,), dtype=torch.int32, device=x.device)
    if out.numel() != B:
        raise ValueError(f"nonfinite_count: out holds {out.numel()} counters for {B} images")
    check(lib().excel_nonfinite_count(_p(x), B, x.numel() // B, _p(out, torch.int32), 1 if init else 0, _stream()), "excel_nonfinite_count")
    return out


# ------------------------------------------------------------------ image tags (include/excel_hip.h, "image tags")
def clip_tags(x, text_rows, num_fg, scale=100.0, thre=0.2, kmax=6, want_scores=True):
    """CLIP's zero-shot tags of B images -> (onehot [B,num_fg] f32, scores [B,num_fg] f32 or None): the rows cls_compact reads.
    x: [B,N,C] (row 0 of every image is used where it lies: the tower's x_raw, whose class-token row is CLIP's image embedding) or a
    compact [B,C]; text_rows [T,C], the num_fg foreground rows first.  scores = the softmax over ALL T rows of scale * cosine; a class is
    tagged when it is among the kmax best foreground scores and reaches thre times the best one (the best is always tagged; a tie goes to
    the lower index).  A row with a non-finite logit gets class 0 alone and NaN scores.  One launch, no scratch memory, no synchronisation."""
    if x.dim() not in (2, 3):
        raise ValueError(f"clip_tags: x must be [B,N,C] or [B,C], got {tuple(x.shape)}")
    x = f32c(x, 16)                 # the kernel reads both 16 bytes at a time
    text_rows = f32c(text_rows, 16)
    B, C_ = int(x.shape[0]), int(x.shape[-1])
    stride = int(x.shape[1]) * C_ if x.dim() == 3 else C_
    T = int(text_rows.shape[0])
    if text_rows.dim() != 2 or int(text_rows.shape[1]) != C_:
        raise ValueError(f"clip_tags: text_rows must be [T,{C_}], got {tuple(text_rows.shape)}")
    onehot = torch.empty((B, int(num_fg)), dtype=torch.float32, device=x.device)
    scores = torch.empty((B, int(num_fg)), dtype=torch.float32, device=x.device) if want_scores else None
    check(lib().excel_clip_tags(_p(x), stride, _p(text_rows), B, C_, T, int(num_fg), float(scale), float(thre), int(kmax), _p(onehot),
                                _p(scores), _stream()), "excel_clip_tags")
    return onehot, scores


def _label_pair(who, gt_u8, pred_u8, plan, skip):
    """What the ops over (gt, pred, plan, skip) share -> (gt, pred, B, table pointer, info pointer): contiguous maps of equal size, B from
    the plan or the first dimension, the pixel count the plan holds, one skip flag per image."""
    gt = gt_u8.contiguous()
    pr = pred_u8.contiguous()
    if gt.numel() != pr.numel():
        raise ValueError(f"{who}: gt holds {gt.numel()} pixels, pred {pr.numel()}")
    B = plan.B if plan is not None else (int(gt.shape[0]) if gt.dim() > 0 else 0)
    if plan is not None and gt.numel() != plan.total_label_pix:
        raise ValueError(f"{who}: {gt.numel()} pixels, the plan holds {plan.total_label_pix}")
    if skip is not None and skip.numel() != B:
        raise ValueError(f"{who}: skip holds {skip.numel()} flags for {B} images")
    return gt, pr, B, _p(plan.table, torch.int32) if plan is not None else None, C.byref(plan.info) if plan is not None else None


def confusion_accumulate_masked(gt_u8, pred_u8, num_classes, skip, hist=None, plan=None):
    """confusion_accumulate over the images with skip[b] == 0 (skip: int32 [B], device - e.g. nonfinite_count's counters).
    plan=None: gt / pred are uniform [B,H,W] maps; with a RaggedPlan they are its tight label maps back to back."""
    assert gt_u8.numel() == pred_u8.numel()
    gt, pr, B, table, info = _label_pair("confusion_accumulate_masked", gt_u8, pred_u8, plan, skip)
    if hist is None:
        hist = torch.zeros((num_classes, num_classes), dtype=torch.int64, device=gt.device)
    check(lib().excel_confusion_accumulate_masked(_p(gt, torch.uint8), _p(pr, torch.uint8), B, gt.numel() // B, table, info,
                                                  _p(skip, torch.int32), num_classes, _p(hist, torch.int64), _stream()),
          "excel_confusion_accumulate_masked")
    return hist


# ------------------------------------------------------------------ per-image scores (include/excel_hip.h, "per-image scores")
def image_scores(gt_u8, pred_u8, num_classes, skip=None, plan=None, out=None):
    """-> int32 [B,3,nc] (device): per image the ground-truth area, the predicted area and the intersection of every class over the pixels
    with gt < nc and pred < nc - the margins of the image's own confusion matrix (utils/evaluate.image_score_rows turns them into IoU,
    mIoU and pixel accuracy).  plan=None: gt / pred are uniform [B,H,W] maps; with a RaggedPlan they are its tight label maps back to
    back.  skip: int32 [B] (device) or None - the rows of an image with skip[b] != 0 are zero.  out: a buffer of B*3*nc int32, fully
    overwritten.  One launch, no scratch memory, no synchronisation."""
    nc = int(num_classes)
    if not 1 <= nc <= 256:
        raise ValueError(f"image_scores: num_classes = {nc} is outside [1, 256]")
    gt, pr, B, table, info = _label_pair("image_scores", gt_u8, pred_u8, plan, skip)
    if B < 1:
        raise ValueError(f"image_scores: B = {B}: at least one image is needed (gt {tuple(gt.shape)})")
    if out is not None and (out.numel() != B * 3 * nc or out.dtype != torch.int32):
        raise ValueError(f"image_scores: out must hold {B * 3 * nc} int32 (got {out.numel()} {out.dtype})")
    counts = torch.empty((B, 3, nc), dtype=torch.int32, device=gt.device) if out is None else out.view(B, 3, nc)
    check(lib().excel_image_scores(_p(gt, torch.uint8), _p(pr, torch.uint8), B, gt.numel() // B, table, info, _p(skip, torch.int32), nc,
                                   _p(counts, torch.int32), _stream()), "excel_image_scores")
    return counts


# ------------------------------------------------------------------ boundary scores (include/excel_hip.h, "boundary scores")
BOUNDARY_TILE = (16, 64)            # (TH, TW) of boundary_scores_kernel: one workgroup per tile, its halo sized by the largest radius


def boundary_max_radius():
    """The largest radius this build's boundary_scores accepts (72: 2 % of a 3600-pixel diagonal)."""
    return int(lib().excel_boundary_max_radius())


def boundary_scores(gt_u8, pred_u8, num_classes, radius, skip=None, plan=None, out=None, max_radius=None):
    """-> int32 [B,3,nc] (device): image_scores restricted to the contour bands - per image and class the valid pixels of the ground truth
    in the ground truth's band, those of the prediction in the prediction's band, and the pixels where both agree and both bands meet
    (Boundary IoU's counts; utils/evaluate.image_score_rows / boundary_scores_from_counts turn them into scores).  A pixel is in the
    band of a map iff its (2d+1) x (2d+1) window leaves the image or holds another raw value.  plan=None: gt / pred are uniform [B,H,W]
    maps; with a RaggedPlan they are its tight label maps back to back.  radius: an int (every image), a host sequence of B ints
    (utils/image_scores.boundary_radius per image; uploaded without a wait) or a device int32 tensor [B] - then `max_radius` may bound
    it (default: the build's maximum), and an image whose radius is < 1 or beyond the bound gets -1 in all its entries.  Host radii
    outside [1, boundary_max_radius()] are refused here, naming the image.  skip / out as in image_scores.  One launch, no scratch
    memory, no synchronisation."""
    nc = int(num_classes)
    if not 1 <= nc <= 256:
        raise ValueError(f"boundary_scores: num_classes = {nc} is outside [1, 256]")
    if plan is None and gt_u8.dim() != 3:
        raise ValueError(f"boundary_scores: uniform maps must be [B,H,W] (gt {tuple(gt_u8.shape)}); a ragged batch needs its plan")
    gt, pr, B, table, info = _label_pair("boundary_scores", gt_u8, pred_u8, plan, skip)
    if plan is None:
        H, W = int(gt.shape[1]), int(gt.shape[2])
        hw = lambda b: (H, W)
    else:
        H, W = 0, 0
        hw = lambda b: (int(plan.hw[b, 0]), int(plan.hw[b, 1]))
    if B < 1 or gt.numel() < 1:
        raise ValueError(f"boundary_scores: at least one image with a pixel is needed (gt {tuple(gt.shape)})")
    if out is not None and (out.numel() != B * 3 * nc or out.dtype != torch.int32):
        raise ValueError(f"boundary_scores: out must hold {B * 3 * nc} int32 (got {out.numel()} {out.dtype})")
    top = boundary_max_radius()
    if isinstance(radius, torch.Tensor):
        if radius.dtype != torch.int32 or radius.numel() != B or radius.device != gt.device:
            raise ValueError(f"boundary_scores: a radius tensor must hold {B} int32 on {gt.device} (got {radius.numel()} {radius.dtype} on {radius.device})")
        rad, bound = radius.contiguous(), top if max_radius is None else int(max_radius)
    else:
        import numpy as np
        host = np.full(B, int(radius), np.int32) if np.ndim(radius) == 0 else np.asarray([int(r) for r in radius], np.int32)
        if host.shape != (B,):
            raise ValueError(f"boundary_scores: {host.size} radii for {B} images")
        for b in np.nonzero((host < 1) | (host > top))[0]:
            h, w = hw(int(b))
            raise ValueError(f"boundary_scores: image {int(b)} ({h} x {w}) has radius {int(host[b])}, outside [1, {top}] "
                             "(ops.boundary_max_radius())")
        bound = int(host.max()) if max_radius is None or np.ndim(radius) == 0 else int(max_radius)
        rad = None if np.ndim(radius) == 0 else torch.from_numpy(host).to(gt.device, non_blocking=True)
    if not 1 <= bound <= top:
        raise ValueError(f"boundary_scores: max_radius = {bound} is outside [1, {top}]")
    counts = torch.empty((B, 3, nc), dtype=torch.int32, device=gt.device) if out is None else out.view(B, 3, nc)
    check(lib().excel_boundary_scores(_p(gt, torch.uint8), _p(pr, torch.uint8), B, H, W, table, info, _p(rad, torch.int32), bound,
                                      _p(skip, torch.int32), nc, _p(counts, torch.int32), _stream()), "excel_boundary_scores")
    return counts


# ------------------------------------------------------------------ one-time / auxiliary
def attr_aggregate(text_features, bank, num_fg, topK=0.9):
    """text [T,C], bank [C,K] -> text_attr [C,T] (model/load_attr.py:86-119)."""
    text_features = f32c(text_features)
    bank = f32c(bank)
    T, Cc = text_features.shape
    K = bank.shape[1]
    out = torch.empty((Cc, T), dtype=torch.float32, device=text_features.device)
    check(lib().excel_attr_aggregate(_p(text_features), _p(bank), num_fg, T, Cc, K, float(topK), _p(out), _stream()),
          "excel_attr_aggregate")
    return out


def bilinear_resize(x, H, W, align_corners=False):
    """x [..., h, w] -> [..., H, W]  (F.interpolate mode='bilinear')."""
    x = f32c(x)
    h, w = x.shape[-2:]
    planes = x.numel() // (h * w)
    out = torch.empty(x.shape[:-2] + (H, W), dtype=torch.float32, device=x.device)
    check(lib().excel_bilinear_resize(_p(x), _p(out), planes, h, w, H, W, 1 if align_corners else 0, _stream()),
          "excel_bilinear_resize")
    return out


def pos_embed_resize(pos, g):
    pos = f32c(pos)
    side = int(round((pos.shape[0] - 1) ** 0.5))
    D = pos.shape[1]
    out = torch.empty((g * g + 1, D), dtype=torch.float32, device=pos.device)
    check(lib().excel_pos_embed_resize(_p(pos), side, g, D, _p(out), _stream()), "excel_pos_embed_resize")
    return out


def flip_max_normalize(attr, g):
    """attr [2B,P,F] (second half from flipped inputs) -> [B,P,F] (utils/camutils.py:21-26)."""
    attr = f32c(attr)
    B2, P, F_ = attr.shape
    out = torch.empty((B2 // 2, P, F_), dtype=torch.float32, device=attr.device)
    check(lib().excel_flip_max_normalize(_p(attr), _p(out), B2 // 2, g, F_, _stream()), "excel_flip_max_normalize")
    return out


def lam_scale_accumulate(maps, acc, g, H, W, init):
    """maps [2B,P,F] of one scale -> resize to (H,W), flip-max, (+)= into acc [B,F,H,W]."""
    maps = f32c(maps)
    B2, P, F_ = maps.shape
    if acc is None:
        acc = torch.empty((B2 // 2, F_, H, W), dtype=torch.float32, device=maps.device)
        init = True
    check(lib().excel_lam_scale_accumulate(_p(maps), _p(acc), B2 // 2, g, F_, H, W, 1 if init else 0, _stream()),
          "excel_lam_scale_accumulate")
    return acc


def plane_minmax_normalize_(lam):
    """in place: lam -= min_hw ; lam /= max_hw + 1e-5 for every [..., H, W] plane."""
    H, W = lam.shape[-2:]
    check(lib().excel_plane_minmax_normalize(_p(lam), lam.numel() // (H * W), H * W, _stream()), "excel_plane_minmax_normalize")
    return lam


TTA_MAX_SCALES = 8
TTA_MAX_GRID = 48


def lam_tta_fuse(maps, grids, g_out, flip, out=None):
    """Flip and multi-scale LAM fuse at the patch grid (excel_lam_tta_fuse; utils/camutils.py:8-63).
    maps: per scale the model's attribute maps [2B if flip else B, g_s*g_s, F] (image B + b = the mirrored input of image b), in the
    order they are summed; grids: the g_s -> [B, g_out*g_out, F], what refine_cams_with_aff_batched reads: per (b, f) plane the
    bilinear resize to the g_out grid, the max with the mirrored half (flip), the sum over scales, min-max normalised.  Bit-equal to
    lam_scale_accumulate per scale + plane_minmax_normalize_ (flip) for finite inputs; a plane that a non-finite value reaches is NaN
    as a whole.  Two launches; `out` holds the sums in between, so nothing else is allocated."""
    maps = [f32c(m) for m in maps]
    grids = [int(g) for g in grids]
    ns = len(maps)
    if not 1 <= ns <= TTA_MAX_SCALES:
        raise ValueError(f"lam_tta_fuse: {ns} scales, need 1..{TTA_MAX_SCALES}")
    if len(grids) != ns:
        raise ValueError("lam_tta_fuse: one grid size per scale")
    g_out = int(g_out)
    if not 1 <= g_out <= TTA_MAX_GRID:
        raise ValueError(f"lam_tta_fuse: g_out = {g_out} outside [1, {TTA_MAX_GRID}]")
    nb = int(maps[0].shape[0]) if maps[0].dim() == 3 else 0
    F_ = int(maps[0].shape[2]) if maps[0].dim() == 3 else 0
    if flip and nb % 2:
        raise ValueError(f"lam_tta_fuse: flip needs [2B, P, F] maps (image, then mirrored image), got {nb} images")
    B = nb // 2 if flip else nb
    if B < 1 or F_ < 1:
        raise ValueError(f"lam_tta_fuse: need B >= 1 and F >= 1, got maps of shape {tuple(maps[0].shape)}")
    for m, g in zip(maps, grids):
        if not 1 <= g <= TTA_MAX_GRID:
            raise ValueError(f"lam_tta_fuse: grid {g} outside [1, {TTA_MAX_GRID}]")
        if tuple(m.shape) != (nb, g * g, F_):
            raise ValueError(f"lam_tta_fuse: the maps of grid {g} must be [{nb}, {g * g}, {F_}], got {tuple(m.shape)}")
    if out is None:
        out = torch.empty((B, g_out * g_out, F_), dtype=torch.float32, device=maps[0].device)
    elif tuple(out.shape) != (B, g_out * g_out, F_):
        raise ValueError(f"lam_tta_fuse: out must be [{B}, {g_out * g_out}, {F_}], got {tuple(out.shape)}")
    ptrs = (C.c_void_p * ns)(*[_p(m).value for m in maps])
    gs = (C.c_int32 * ns)(*grids)
    check(lib().excel_lam_tta_fuse(ptrs, gs, ns, 1 if flip else 0, B, F_, g_out, _p(out), _stream()), "excel_lam_tta_fuse")
    return out


# ------------------------------------------------------------------ live kernel timing (HIP events on the launch stream)
def prof_enable(on=True, categories=None, every=1):
    """categories: iterable of category names to bracket (None = all); every: bracket every n-th launch of a category
    (each event pair costs ~10 us of GPU idle time, so the timed region samples)."""
    check(lib().excel_prof_set_sampling(int(every)), "excel_prof_set_sampling")
    mask = (1 << 64) - 1
    if categories is not None:
        names = [lib().excel_prof_category_name(i).decode() for i in range(lib().excel_prof_num_categories())]
        mask = 0
        for c in categories:
            mask |= 1 << names.index(c)
    check(lib().excel_prof_set_mask(mask), "excel_prof_set_mask")
    check(lib().excel_prof_enable(1 if on else 0), "excel_prof_enable")


def dcrf_inference(image_u8, prob, iters, pos_w, pos_xy_std, bi_w, bi_xy_std, bi_rgb_std, is_energy=False):
    """image [H,W,3] uint8, prob [C,H,W] f32 (probabilities, or unary energies when is_energy) -> Q [C,H,W] (excel_dcrf_inference)."""
    prob = f32c(prob)
    if image_u8.dtype != torch.uint8 or not image_u8.is_contiguous():
        image_u8 = image_u8.to(torch.uint8).contiguous()
    Cn, H, W = prob.shape
    assert tuple(image_u8.shape) == (H, W, 3), (tuple(image_u8.shape), (H, W, 3))
    out = torch.empty_like(prob)
    ws = _ws(lib().excel_dcrf_workspace_bytes(H, W, Cn), prob.device)
    check(lib().excel_dcrf_inference(_p(image_u8, torch.uint8), _p(prob), 1 if is_energy else 0, H, W, Cn, int(iters), float(pos_w), float(pos_xy_std),
                                     float(bi_w), float(bi_xy_std), float(bi_rgb_std), _p(out), _p(ws, torch.uint8), _stream()), "excel_dcrf_inference")
    return out


_dcrf_budget_warned = False


def dcrf_ragged_workspace_bytes(hw, C_):
    """Workspace of excel_dcrf_inference_ragged for a group of images of sizes hw = [(H, W), ...] and C_ classes (host only).
    RuntimeError where the library refuses the group (more lattice vertices than its 32-bit indices hold)."""
    total = sum(int(h) * int(w) for h, w in hw)
    out = C.c_size_t(0)
    check(lib().excel_dcrf_ragged_workspace_bytes(total, int(C_), C.byref(out)), "excel_dcrf_ragged_workspace_bytes")
    return int(out.value)


def dcrf_groups(hw, C_, budget_bytes):
    """Split a batch into consecutive runs [(start, stop), ...] for excel_dcrf_inference_ragged (host only): images are added to a run
    while its workspace stays within budget_bytes (and the library accepts it); an image that alone exceeds the budget is a run of its
    own.  Every image is in exactly one run, in order."""
    sizes = [(int(h), int(w)) for h, w in hw]
    runs, start = [], 0
    for b in range(1, len(sizes) + 1):
        if b == len(sizes):
            runs.append((start, b))
            break
        try:
            fits = dcrf_ragged_workspace_bytes(sizes[start:b + 1], C_) <= budget_bytes
        except RuntimeError:
            fits = False
        if not fits:
            runs.append((start, b))
            start = b
    return runs


def dcrf_inference_ragged(images_u8, plan, unary, C_, iters, pos_w, pos_xy_std, bi_w, bi_xy_std, bi_rgb_std, is_energy=False, want_labels=True,
                          want_q=False, budget_bytes=None):
    """dcrf_inference (+ argmax_label) for a ragged batch, a group of images per chain of launches (excel_dcrf_inference_ragged).
    images_u8: the packed uint8 HWC images (image b at 3 * loff_b); unary: flat, tight [C_, H_b, W_b] per image at C_ * loff_b
    (seg_softmax_resize_ragged's output; energies when is_energy).  budget_bytes caps the workspace: the batch is cut into
    dcrf_groups and the groups run one after another in one workspace (None: the whole batch is one group).
    -> (labels, q): tight uint8 labels [total_label_pix] and flat marginals (layout of `unary`), None where not wanted.  Every image
    has the bits of dcrf_inference / argmax_label on it alone, whatever the grouping."""
    if not (want_labels or want_q):
        raise ValueError("dcrf_inference_ragged: ask for labels, q or both")
    n = plan.total_label_pix
    if images_u8.dtype != torch.uint8 or images_u8.numel() != 3 * n:
        raise ValueError(f"dcrf_inference_ragged: images_u8 must hold {3 * n} uint8 values")
    if unary.dtype != torch.float32 or unary.numel() != C_ * n:
        raise ValueError(f"dcrf_inference_ragged: unary must hold C * total_label_pix = {C_ * n} float32 values")
    images_u8, unary = images_u8.view(-1), unary.view(-1)
    dev = unary.device
    labels = torch.empty((n,), dtype=torch.uint8, device=dev) if want_labels else None
    q = torch.empty((C_ * n,), dtype=torch.float32, device=dev) if want_q else None
    groups = [(0, plan.B)] if budget_bytes is None else dcrf_groups(plan.hw, C_, budget_bytes)
    need = max(dcrf_ragged_workspace_bytes(plan.hw[s:e], C_) for s, e in groups)
    global _dcrf_budget_warned
    if budget_bytes is not None and need > budget_bytes and not _dcrf_budget_warned:
        _dcrf_budget_warned = True
        import warnings
        warnings.warn(f"dcrf_inference_ragged: one image alone needs a workspace of {need} bytes, over the budget of {budget_bytes}; "
                      "it runs as a group of its own (said once)")
    ws = _ws(need, dev)
    for s, e in groups:
        sub = plan if (s, e) == (0, plan.B) else RaggedPlan(plan.hw[s:e], dev)
        lo, hi = int(plan.loff[s]), int(plan.loff[e])
        check(lib().excel_dcrf_inference_ragged(_p(images_u8[3 * lo:3 * hi], torch.uint8), _p(unary[C_ * lo:C_ * hi]), 1 if is_energy else 0,
                                                _p(sub.table, torch.int32), C.byref(sub.info), int(C_), int(iters), float(pos_w), float(pos_xy_std),
                                                float(bi_w), float(bi_xy_std), float(bi_rgb_std),
                                                _p(labels[lo:hi], torch.uint8) if want_labels else None, _p(q[C_ * lo:C_ * hi]) if want_q else None,
                                                _p(ws, torch.uint8), _stream()), "excel_dcrf_inference_ragged")
    return labels, q


def _lam_counts(hw, nchan):
    import numpy as np
    hw = np.ascontiguousarray(np.asarray(hw, np.int32).reshape(-1, 2))
    nchan = np.ascontiguousarray(np.asarray(nchan, np.int32).reshape(-1))
    if len(hw) != len(nchan):
        raise ValueError(f"{len(hw)} sizes but {len(nchan)} class counts")
    return hw, nchan


def dcrf_lam_ragged_workspace_bytes(hw, nchan):
    """Workspace of excel_dcrf_lam_ragged for a group of images of sizes hw = [(H, W), ...] with nchan[b] classes each (host only):
    that of dcrf_ragged_workspace_bytes(hw, max(nchan)) plus one int32 per lattice vertex (9 per pixel; two arrays, each rounded up to
    256 bytes).  RuntimeError where the library refuses the group."""
    hw, nchan = _lam_counts(hw, nchan)
    out = C.c_size_t(0)
    i32 = C.POINTER(C.c_int32)
    check(lib().excel_dcrf_lam_ragged_workspace_bytes(hw.ctypes.data_as(i32), nchan.ctypes.data_as(i32), len(nchan), C.byref(out)),
          "excel_dcrf_lam_ragged_workspace_bytes")
    return int(out.value)


def dcrf_lam_groups(hw, nchan, budget_bytes):
    """dcrf_groups for excel_dcrf_lam_ragged (host only): consecutive runs [(start, stop), ...] whose workspace stays within
    budget_bytes; an image that alone exceeds the budget is a run of its own.  Every image is in exactly one run, in order."""
    hw, nchan = _lam_counts(hw, nchan)
    runs, start = [], 0
    for b in range(1, len(nchan) + 1):
        if b == len(nchan):
            runs.append((start, b))
            break
        try:
            fits = dcrf_lam_ragged_workspace_bytes(hw[start:b + 1], nchan[start:b + 1]) <= budget_bytes
        except RuntimeError:
            fits = False
        if not fits:
            runs.append((start, b))
            start = b
    return runs


def dcrf_lam_ragged(images_u8, plan, cams, Cmax, nchan, nchan_host, cls_idx, iters, pos_w, pos_xy_std, bi_w, bi_xy_std, bi_rgb_std,
                    want_labels=True, want_q=False, budget_bytes=None):
    """The DenseCRF stage of tools/infer_lam.py:179-237 for a ragged batch of LAMs with their own class counts (excel_dcrf_lam_ragged).
    images_u8: the packed uint8 HWC images; cams: Cmax pitched planes per image (image b at Cmax * poff_b: pipeline.last_cams), read
    in place (planes >= nchan[b] and pad columns are never touched); nchan (device int32 [B]) / nchan_host (host, same values) = the
    class counts; cls_idx (device int32 [B, smax] or None) maps the arg-max to the labels (0, cls_idx + 1).  budget_bytes caps the
    workspace: the batch is cut into dcrf_lam_groups, which run one after another in one workspace (None: one group).
    -> (labels, q): tight uint8 labels [total_label_pix] and marginals in the layout of `cams` (torch.empty: only planes < nchan[b] and
    columns < W_b are written), None where not wanted.  Every image has the bits of dcrf_inference on its own planes + argmax_label."""
    import numpy as np
    if not (want_labels or want_q):
        raise ValueError("dcrf_lam_ragged: ask for labels, q or both")
    Cmax = int(Cmax)
    n = plan.total_label_pix
    hw, nchan_host = _lam_counts(plan.hw, nchan_host)
    if images_u8.dtype != torch.uint8 or images_u8.numel() != 3 * n:
        raise ValueError(f"dcrf_lam_ragged: images_u8 must hold {3 * n} uint8 values")
    if cams.dtype != torch.float32 or cams.numel() != Cmax * plan.total_pix:
        raise ValueError(f"dcrf_lam_ragged: cams must hold Cmax * total_pix = {Cmax * plan.total_pix} float32 values")
    if nchan.dtype != torch.int32 or nchan.numel() != plan.B:
        raise ValueError(f"dcrf_lam_ragged: nchan must be int32 [{plan.B}]")
    smax = Cmax - 1
    if cls_idx is not None:
        if cls_idx.dtype != torch.int32 or cls_idx.dim() != 2 or cls_idx.shape[0] != plan.B or not cls_idx.is_contiguous():
            raise ValueError(f"dcrf_lam_ragged: cls_idx must be contiguous int32 [{plan.B}, smax]")
        smax = int(cls_idx.shape[1])
    images_u8, cams, nchan = images_u8.view(-1), cams.view(-1), nchan.view(-1)
    dev = cams.device
    labels = torch.empty((n,), dtype=torch.uint8, device=dev) if want_labels else None
    q = torch.empty((Cmax * plan.total_pix,), dtype=torch.float32, device=dev) if want_q else None
    groups = [(0, plan.B)] if budget_bytes is None else dcrf_lam_groups(hw, nchan_host, budget_bytes)
    sizes = [dcrf_lam_ragged_workspace_bytes(hw[s:e], nchan_host[s:e]) for s, e in groups]
    need = max(sizes)
    global _dcrf_budget_warned
    if budget_bytes is not None and need > budget_bytes and not _dcrf_budget_warned:
        _dcrf_budget_warned = True
        import warnings
        warnings.warn(f"dcrf_lam_ragged: one image alone needs a workspace of {need} bytes, over the budget of {budget_bytes}; "
                      "it runs as a group of its own (said once)")
    dcrf_lam_ragged.last_groups, dcrf_lam_ragged.last_workspace_bytes = len(groups), need
    ws = _ws(need, dev)
    i32 = C.POINTER(C.c_int32)
    for s, e in groups:
        sub = plan if (s, e) == (0, plan.B) else RaggedPlan(hw[s:e], dev)
        lo, hi = int(plan.loff[s]), int(plan.loff[e])
        po, pe = Cmax * int(plan.poff[s]), Cmax * int(plan.poff[e])
        host = np.ascontiguousarray(nchan_host[s:e])
        check(lib().excel_dcrf_lam_ragged(_p(images_u8[3 * lo:3 * hi], torch.uint8), _p(cams[po:pe]), _p(nchan[s:e], torch.int32),
                                          host.ctypes.data_as(i32), _p(cls_idx[s:e], torch.int32) if cls_idx is not None else None,
                                          _p(sub.table, torch.int32), C.byref(sub.info), smax, Cmax, int(iters), float(pos_w),
                                          float(pos_xy_std), float(bi_w), float(bi_xy_std), float(bi_rgb_std),
                                          _p(labels[lo:hi], torch.uint8) if want_labels else None, _p(q[po:pe]) if want_q else None,
                                          _p(ws, torch.uint8), _stream()), "excel_dcrf_lam_ragged")
    return labels, q


def prof_collect():
    """-> {category: dict(ms=summed elapsed, launches=count, work=algorithmic FLOPs or 0)} and clears the log."""
    n = lib().excel_prof_num_categories()
    ms = (C.c_double * n)()
    cnt = (C.c_longlong * n)()
    work = (C.c_double * n)()
    check(lib().excel_prof_collect(ms, cnt, work), "excel_prof_collect")
    return {lib().excel_prof_category_name(i).decode(): dict(ms=ms[i], launches=cnt[i], work=work[i]) for i in range(n)}
