// The CLIP-surgery ViT of the C ABI (include/excel_hip.h, excel_vit_*): the handle, its weight preparation for the split-plane modes,
// the workspace layout and the forward driver.  Compiled once: the launchers that depend on the 16-bit split type are called through
// the SplitApi table of the handle's mode (excel_internal.h); no excel_launch_* name of those is visible unqualified here.
#include "../../include/excel_hip.h"
#include "common.h"
#include "excel_internal.h"

#include <map>
#include <vector>

// ------------------------------------------------------------------------------------ small helper kernels
__global__ void transpose_kernel(const float* __restrict__ in, float* __restrict__ out, int R, int Cc) {
    __shared__ float t[32][33];
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    const int r0 = blockIdx.y * 32, c0 = blockIdx.x * 32;
    for (int k = ty; k < 32; k += 8)
        if (r0 + k < R && c0 + tx < Cc) t[k][tx] = in[(long long)(r0 + k) * Cc + c0 + tx];
    __syncthreads();
    for (int k = ty; k < 32; k += 8)
        if (c0 + k < Cc && r0 + tx < R) out[(long long)(c0 + k) * R + r0 + tx] = t[tx][k];
}

// positional grid resize, F.interpolate(bilinear, align_corners=False) on [1,D,side,side] (clip_surgery_model.py:430-433)
__global__ void pos_resize_kernel(const float* __restrict__ pos, float* __restrict__ out, int side, int g, int D) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    const long long total = (long long)(g * g + 1) * D;
    if (i >= total) return;
    const int d = (int)(i % D);
    const int n = (int)(i / D);
    if (n == 0) { out[i] = pos[d]; return; }
    const int y = (n - 1) / g, x = (n - 1) % g;
    const BilinearTap t = bilinear_tap(x, y, side, side, g, g, 0);
    auto at = [&](int yy, int xx) { return pos[(long long)(1 + yy * side + xx) * D + d]; };
    out[i] = bilinear_blend(t, at(t.y0, t.x0), at(t.y0, t.x1), at(t.y1, t.x0), at(t.y1, t.x1));
}

extern "C" int excel_pos_embed_resize(const float* pos, int side, int g, int D, float* out, void* stream) {
    EXCEL_CHECK_ARG(pos && out && side > 0 && g > 0, "pos_embed_resize: bad argument");
    hipLaunchKernelGGL(pos_resize_kernel, dim3((unsigned)cdivl((long long)(g * g + 1) * D, 256)), dim3(256), 0, ST(stream), pos, out, side, g, D);
    EXCEL_CHECK_LAUNCH("pos_resize");
    return EXCEL_OK;
}

// ------------------------------------------------------------------------------------ ViT handle
struct SplitBlockW {
    unsigned short *in_proj, *out_proj, *fc1, *fc2;             // split planes [N][2][K]
    unsigned short *h_in_proj, *h_out_proj, *h_fc1, *h_fc2;     // plain half matrices [N][K] (mode 3, "f16x2"), else null
};
struct excel_vit {
    excel_vit_config cfg;
    excel_vit_weights w;
    std::vector<excel_vit_block_weights> blocks;
    float* projT = nullptr;             // [C, D]
    std::map<int, float*> pos_cache;    // g -> [1+g*g, D]
    int gemm_mode = 0;                  // 0: exact fp32 MFMA, 1: bf16x3 (split bf16, 3 MFMAs per product), 2: f16x3 (split IEEE half), 3: f16x2 (2 + fp16-valued weights)
    int split_type = 0;                 // what the split weights hold: 0 nothing yet, 1 bf16 planes, 2 f16 planes
    unsigned short* split_arena = nullptr;   // all split weights in one allocation
    std::vector<SplitBlockW> sblocks;
    unsigned short *s_conv1 = nullptr, *s_projT = nullptr;
    // "f16x2": the weights as plain half matrices (one allocation) and whether they are all fp16-valued (-1: not examined yet)
    unsigned short* half_arena = nullptr;
    unsigned short *h_conv1 = nullptr, *h_projT = nullptr;
    int fp16_exact = -1;
};

// Every weight matrix a GEMM of the forward reads, in the order both arenas hold them:
// visit(fp32 source, rows, K, the handle's pointer to its split planes, the handle's pointer to its plain half matrix)
template <class Visit>
static void vit_gemm_weights(excel_vit* h, Visit visit) {
    const excel_vit_config& c = h->cfg;
    const size_t D = c.width, Kc = (size_t)3 * c.patch * c.patch;
    if (h->sblocks.size() != (size_t)c.layers) h->sblocks.assign(c.layers, SplitBlockW{});
    for (int l = 0; l < c.layers; ++l) {
        const excel_vit_block_weights& bw = h->blocks[l];
        SplitBlockW& sb = h->sblocks[l];
        visit(bw.in_proj_w, 3 * D, D, sb.in_proj, sb.h_in_proj);
        visit(bw.out_proj_w, D, D, sb.out_proj, sb.h_out_proj);
        visit(bw.fc1_w, 4 * D, D, sb.fc1, sb.h_fc1);
        visit(bw.fc2_w, D, 4 * D, sb.fc2, sb.h_fc2);
    }
    visit(h->w.conv1_w, D, Kc, h->s_conv1, h->h_conv1);
    visit(h->projT, (size_t)c.out_dim, D, h->s_projT, h->h_projT);
}
static size_t vit_gemm_weight_elems(excel_vit* h) {
    size_t total = 0;
    vit_gemm_weights(h, [&](const float*, size_t rows, size_t K, unsigned short*&, unsigned short*&) { total += rows * K; });
    return total;
}

static int vit_prepare_split_weights(excel_vit* h, int type) {
    if (h->split_arena && h->split_type == type) return EXCEL_OK;
    float* arena = (float*)h->split_arena;
    if (!arena) {
        if (hipMalloc(&arena, vit_gemm_weight_elems(h) * sizeof(float)) != hipSuccess) {      // hi + lo plane: 4 bytes per element
            excel_set_error("excel_vit: hipMalloc(split weights) failed");
            return EXCEL_ERR_ALLOC;
        }
    } else if (hipDeviceSynchronize() != hipSuccess) {      // re-splitting for the other type: nothing may still read the old planes
        excel_set_error("excel_vit: device synchronize failed");
        return EXCEL_ERR_LAUNCH;
    }
    h->split_arena = (unsigned short*)arena;
    h->split_type = 0;               // the arena holds nothing usable until every split kernel has finished (set below, after the sync)
    const SplitApi& k = split_api(type == 2 ? 2 : 1);
    float* cur = arena;
    int put_rc = EXCEL_OK;
    vit_gemm_weights(h, [&](const float* src, size_t rows, size_t K, unsigned short*& split, unsigned short*&) {
        split = (unsigned short*)cur;
        const int rc = k.split_bf16(src, split, (long long)rows, (int)K, 0);
        if (rc != EXCEL_OK && put_rc == EXCEL_OK) put_rc = rc;
        cur += rows * K;
    });
    // (one-time set-up on the legacy stream 0, which every blocking stream orders against; the device-wide sync above / this one make it
    // safe for callers on non-blocking streams too)
    if (put_rc != EXCEL_OK) return put_rc;
    if (hipStreamSynchronize(0) != hipSuccess) {
        excel_set_error("excel_vit: splitting weights failed: %s", hipGetErrorString(hipGetLastError()));
        return EXCEL_ERR_LAUNCH;
    }
    h->split_type = type;            // only now: a failed re-split leaves split_type 0, so the next set_gemm_mode splits again
    return EXCEL_OK;
}

// Packs every GEMM weight as a plain half matrix (the compact operand of the two-product GEMM) and counts the elements that are not
// exactly representable: fp16_exact = (count == 0).  One pass, once per handle.
static int vit_prepare_half_weights(excel_vit* h) {
    if (h->fp16_exact >= 0) return EXCEL_OK;
    const size_t total = vit_gemm_weight_elems(h);        // halfs
    unsigned short* arena = nullptr;
    unsigned long long* cnt = nullptr;
    if (hipMalloc(&arena, total * sizeof(unsigned short) + 256) != hipSuccess) {
        excel_set_error("excel_vit: hipMalloc(half weights) failed");
        return EXCEL_ERR_ALLOC;
    }
    cnt = (unsigned long long*)((char*)arena + align_up(total * sizeof(unsigned short), 16));
    if (hipMemsetAsync(cnt, 0, sizeof(unsigned long long), 0) != hipSuccess) { hipFree(arena); excel_set_error("excel_vit: memset failed"); return EXCEL_ERR_LAUNCH; }
    const SplitApi& k = split_api(2);
    unsigned short* cur = arena;
    int put_rc = EXCEL_OK;
    vit_gemm_weights(h, [&](const float* src, size_t rows, size_t K, unsigned short*&, unsigned short*& half) {
        half = cur;
        const int rc = k.pack_hi(src, half, (long long)rows, (int)K, cnt, 0);
        if (rc != EXCEL_OK && put_rc == EXCEL_OK) put_rc = rc;
        cur += rows * K;
    });
    auto drop = [&] {
        vit_gemm_weights(h, [](const float*, size_t, size_t, unsigned short*&, unsigned short*& half) { half = nullptr; });
        hipFree(arena);
    };
    unsigned long long n_bad = 1;
    if (put_rc != EXCEL_OK || hipMemcpy(&n_bad, cnt, sizeof(n_bad), hipMemcpyDeviceToHost) != hipSuccess) {       // (synchronises)
        drop();
        if (put_rc != EXCEL_OK) return put_rc;
        excel_set_error("excel_vit: packing half weights failed: %s", hipGetErrorString(hipGetLastError()));
        return EXCEL_ERR_LAUNCH;
    }
    h->fp16_exact = n_bad == 0 ? 1 : 0;
    if (h->fp16_exact) h->half_arena = arena;
    else drop();                       // full-mantissa weights: the packed matrices are of no use (the two-product mode is refused)
    return EXCEL_OK;
}

extern "C" int excel_vit_weights_fp16_exact(excel_vit_t h) {
    EXCEL_CHECK_ARG(h, "excel_vit_weights_fp16_exact: null handle");
    if ((h->cfg.width % 32) != 0 || ((3 * h->cfg.patch * h->cfg.patch) % 32) != 0) return 0;      // no split-plane mode for this shape at all
    TRY(vit_prepare_half_weights(h));
    return h->fp16_exact;
}

extern "C" int excel_vit_set_gemm_mode(excel_vit_t h, int mode) {
    EXCEL_CHECK_ARG(h && mode >= 0 && mode <= 3, "excel_vit_set_gemm_mode: mode must be 0 (f32), 1 (bf16x3), 2 (f16x3) or 3 (f16x2)");
    if (mode >= 1) {
        EXCEL_CHECK_ARG((h->cfg.width % 32) == 0 && ((3 * h->cfg.patch * h->cfg.patch) % 32) == 0,
                        "the split-plane modes need width and 3*patch^2 to be multiples of 32");
        if (mode == 3) {
            TRY(vit_prepare_half_weights(h));
            EXCEL_CHECK_ARG(h->fp16_exact == 1, "excel_vit_set_gemm_mode: mode 3 (f16x2) needs fp16-valued weights (excel_vit_weights_fp16_exact); use 2 (f16x3)");
        }
        TRY(vit_prepare_split_weights(h, mode == 3 ? 2 : mode));
    }
    h->gemm_mode = mode;
    return EXCEL_OK;
}
extern "C" int excel_vit_get_gemm_mode(excel_vit_t h) { return h ? h->gemm_mode : -1; }

extern "C" int excel_vit_create(const excel_vit_config* cfg, const excel_vit_weights* w, excel_vit_t* out) {
    EXCEL_CHECK_ARG(cfg && w && out, "excel_vit_create: null argument");
    EXCEL_CHECK_ARG(cfg->heads > 0 && cfg->width == cfg->heads * 64, "excel_vit_create: head_dim must be 64 (width=%d heads=%d)", cfg->width, cfg->heads);
    EXCEL_CHECK_ARG(cfg->layers >= 1 && cfg->n_surgery >= 0 && cfg->n_surgery <= cfg->layers, "excel_vit_create: bad layer counts");
    EXCEL_CHECK_ARG((cfg->out_dim % 4) == 0 && (cfg->patch % 4) == 0, "excel_vit_create: out_dim and patch must be multiples of 4");
    // every weight is read 16 bytes at a time somewhere on the path: matrices by the GEMMs' operand loads and the split / pack kernels,
    // LayerNorm weights, class_emb and pos_emb by ln_row, biases by the split-plane GEMM's epilogue
    EXCEL_CHECK_ARG(w->blocks, "excel_vit_create: null argument");
    {
        const void* top[] = {w->conv1_w, w->class_emb, w->pos_emb, w->ln_pre_w, w->ln_pre_b, w->ln_post_w, w->ln_post_b, w->proj};
        const char* top_name[] = {"conv1_w", "class_emb", "pos_emb", "ln_pre_w", "ln_pre_b", "ln_post_w", "ln_post_b", "proj"};
        for (int i = 0; i < 8; ++i) EXCEL_CHECK_ALIGN(top[i], 16, "excel_vit_create", top_name[i]);
        TRY(check_block_weights_aligned("excel_vit_create", w->blocks, cfg->layers));
    }
    excel_vit* h = new excel_vit();
    h->cfg = *cfg;
    h->w = *w;
    h->blocks.assign(w->blocks, w->blocks + cfg->layers);
    h->w.blocks = h->blocks.data();
    if (hipMalloc(&h->projT, sizeof(float) * cfg->out_dim * cfg->width) != hipSuccess) {
        delete h;
        excel_set_error("excel_vit_create: hipMalloc failed");
        return EXCEL_ERR_ALLOC;
    }
    hipLaunchKernelGGL(transpose_kernel, dim3(cdiv(cfg->out_dim, 32), cdiv(cfg->width, 32)), dim3(256), 0, 0, w->proj, h->projT,
                       cfg->width, cfg->out_dim);
    if (hipStreamSynchronize(0) != hipSuccess) {
        excel_set_error("excel_vit_create: transpose failed: %s", hipGetErrorString(hipGetLastError()));
        hipFree(h->projT);
        delete h;
        return EXCEL_ERR_LAUNCH;
    }
    *out = h;
    const char* mode = getenv("EXCEL_GEMM_MODE");     // default numerics of new handles: "f32" | "bf16x3" | "f16x3" | "f16x2"
    if (mode && (!strcmp(mode, "bf16x3") || !strcmp(mode, "f16x3") || !strcmp(mode, "f16x2")) && (cfg->width % 32) == 0 && ((3 * cfg->patch * cfg->patch) % 32) == 0) {
        int rc = excel_vit_set_gemm_mode(h, !strcmp(mode, "f16x2") ? 3 : !strcmp(mode, "f16x3") ? 2 : 1);
        if (rc) return rc;
    }
    return EXCEL_OK;
}

extern "C" void excel_vit_destroy(excel_vit_t h) {
    if (!h) return;
    if (h->projT) hipFree(h->projT);
    if (h->split_arena) hipFree(h->split_arena);
    if (h->half_arena) hipFree(h->half_arena);
    for (auto& kv : h->pos_cache) hipFree(kv.second);
    delete h;
}

struct VitWs {
    float *x, *xo, *y, *ao, *qkvh, *qkvs, *hbuf, *stats, *a_sum, *vt, *fraw, *ss;
    int NP, KP;
    size_t total;
};

static VitWs vit_ws_layout(const excel_vit_config& c, int B, int S, char* base) {
    const int g = S / c.patch, N = g * g + 1;
    const size_t M = (size_t)B * N, D = c.width;
    VitWs w;
    w.NP = (N + 3) / 4 * 4;
    w.KP = (N + 31) / 32 * 32;            // K of the bf16x3 A_sum.V GEMM (zero padded)
    Workspace ws(base);
    w.x = ws.take<float>(M * D);
    w.xo = ws.take<float>(M * D);
    w.y = ws.take<float>(M * D);
    w.ao = ws.take<float>(M * D);                   // also the patch-embed GEMM output [B*P, D]
    w.qkvh = ws.take<float>(M * 3 * D);
    w.qkvs = ws.take<float>(M * 3 * D);             // split-bf16 copy of q|k|v for the bf16x3 attention scores (bf16x3 mode)
    {   // MLP hidden [M,4D]; also holds the im2col matrix [B*P, 3*ps*ps]
        const size_t col = (size_t)B * (N - 1) * 3 * c.patch * c.patch;
        w.hbuf = ws.take<float>(M * 4 * D > col ? M * 4 * D : col);
    }
    w.stats = ws.take<float>((size_t)B * c.heads * 4 * N * 2);
    w.a_sum = ws.take<float>((size_t)B * N * w.KP);              // fp32 [B,N,NP] or split bf16 [B,N][2*KP]
    w.vt = ws.take<float>((size_t)B * D * w.KP);                 // V^T split [B][D][2*KP] (bf16x3 mode)
    w.fraw = ws.take<float>(M * c.out_dim);
    w.ss = ws.take<float>((size_t)B * c.out_dim);
    w.total = ws.total();
    return w;
}

extern "C" size_t excel_vit_workspace_bytes(excel_vit_t h, int B, int S) {
    if (!h || B <= 0 || S <= 0 || S % h->cfg.patch) return 0;
    return vit_ws_layout(h->cfg, B, S, nullptr).total;
}

// ------------------------------------------------------------------------------------ the surgery forward
// One host driver for all four modes.  k = split_api(h->gemm_mode): the launchers over the mode's 16-bit split type (mode 0 uses only
// their fp32-output paths); excel_launch_gemm and the *_f32 attention launchers are the exact-fp32 kernels, built once.
static int vit_forward(const SplitApi& k, excel_vit_t h, const float* img, int B, int S, void* workspace, size_t workspace_bytes,
                       float* image_features, float* x_raw, float* w_aff, int aff_layers, float* attn_out, int n_attn_out, float* feats_out,
                       const float* ex_attn, int flags, void* stream) {
    const bool aliased_feats = feats_out && (flags & EXCEL_VIT_FEATS_AS_REFERENCE);
    EXCEL_CHECK_ARG(h && img && workspace && (image_features || x_raw), "excel_vit_forward: null argument (image_features or x_raw is required)");
    const excel_vit_config& c = h->cfg;
    EXCEL_CHECK_ARG(B > 0 && S > 0 && S % c.patch == 0, "excel_vit_forward: S must be a positive multiple of the patch size");
    const int ps = c.patch, g = S / ps, P = g * g, N = P + 1, D = c.width, H = c.heads, L = c.layers, C = c.out_dim;
    EXCEL_CHECK_ARG(n_attn_out >= 0 && n_attn_out <= L && (n_attn_out == 0 || attn_out), "excel_vit_forward: bad attn_out request");
    EXCEL_CHECK_ARG(!w_aff || (aff_layers >= 1 && aff_layers <= L), "excel_vit_forward: bad aff_layers");
    // img: im2col reads f32x4; x_raw: the projection GEMM's f32x4 stores and token_axis_scale's f32x4 loads; image_features: its f32x4
    // stores; the workspace holds every GEMM operand.  w_aff, attn_out and ex_attn are touched one element at a time and feats_out by
    // copies: 4 bytes.
    EXCEL_CHECK_ALIGN(img, 16, "excel_vit_forward", "img");
    EXCEL_CHECK_ALIGN(workspace, 16, "excel_vit_forward", "workspace");
    EXCEL_CHECK_ALIGN(image_features, 16, "excel_vit_forward", "image_features");
    EXCEL_CHECK_ALIGN(x_raw, 16, "excel_vit_forward", "x_raw");
    hipStream_t st = ST(stream);
    VitWs ws = vit_ws_layout(c, B, S, (char*)workspace);
    EXCEL_CHECK_ARG(workspace_bytes >= ws.total, "excel_vit_forward: workspace too small (%zu < %zu)", workspace_bytes, ws.total);
    const int M = B * N;
    const float eps = 1e-5f;
    const float scale = 0.125f;   // head_dim^-0.5 with head_dim = 64 (clip_surgery_model.py:82)

    // positional embedding for this grid (cached)
    const float* pos = h->w.pos_emb;
    if (g != c.pos_grid) {
        auto it = h->pos_cache.find(g);
        if (it == h->pos_cache.end()) {
            float* buf = nullptr;
            if (hipMalloc(&buf, sizeof(float) * (size_t)N * D) != hipSuccess) {
                excel_set_error("excel_vit_forward: hipMalloc(pos) failed");
                return EXCEL_ERR_ALLOC;
            }
            hipLaunchKernelGGL(pos_resize_kernel, dim3((unsigned)cdivl((long long)N * D, 256)), dim3(256), 0, st, h->w.pos_emb, buf, c.pos_grid, g, D);
            EXCEL_CHECK_LAUNCH("pos_resize");
            // one-time per grid size: the cached table may be read from OTHER streams by later calls
            if (hipStreamSynchronize(st) != hipSuccess) {
                excel_set_error("excel_vit_forward: pos_resize failed");
                return EXCEL_ERR_LAUNCH;
            }
            it = h->pos_cache.emplace(g, buf).first;
        }
        pos = it->second;
    }

    const bool bf = h->gemm_mode >= 1;                  // split-plane modes: 1 = bf16x3, 2 = f16x3, 3 = f16x2
    const bool x2 = h->gemm_mode == 3;                  // fp16-valued weights (checked by set_gemm_mode): two-product weight GEMMs
    // patch embedding: im2col -> GEMM (conv1 weight is [D, 3*ps*ps] K-major) -> +cls/pos, ln_pre
    TRY(k.im2col(img, ws.hbuf, B, S, ps, st, bf ? 1 : 0));
    {
        const int Kc = 3 * ps * ps;
        if (bf) {
            GemmBfArgs ga = gemm_bf_args(ws.hbuf, h->s_conv1, ws.ao, nullptr, nullptr, nullptr, B * P, D, Kc, D, 0, GEMM_ACT_NONE, GEMM_OUT_PLAIN);
            if (x2) { ga.w_lo_zero = 1; ga.Bh = h->h_conv1; ga.ldbh = Kc; }
            TRY(k.gemm_bf16x3(ga, st));
        } else {
            GemmArgs ga = gemm_args(ws.hbuf, h->w.conv1_w, ws.ao, nullptr, nullptr, B * P, D, Kc, Kc, Kc, D, 0, GEMM_ACT_NONE);
            TRY(excel_launch_gemm(ga, true, 1, st));
        }
    }
    TRY(k.assemble_ln_pre(ws.ao, h->w.class_emb, pos, h->w.ln_pre_w, h->w.ln_pre_b, ws.x, B, N, D, eps, st));

    // linear layer helper: C = act(A . W^T + bias) + res, A produced in the mode's operand format.
    // rows/lda_f/ldc/ldr default to the dense [M, .] case; the last block uses them to touch only the cls rows.
    auto linear_ex = [&](const float* A, const float* Wf, const unsigned short* Ws, const unsigned short* Wh, const float* bias, const float* res, float* Cout,
                         int rows, int Nout, int K, long long lda_f, int ldc, int ldr, int act, int out_mode) -> int {
        if (bf) {
            GemmBfArgs ga = gemm_bf_args(A, Ws, Cout, Cout, bias, res, rows, Nout, K, ldc, ldr, act, out_mode);
            ga.lda = (int)(2 * lda_f);
            if (x2) { ga.w_lo_zero = 1; ga.Bh = Wh; ga.ldbh = K; }
            if (out_mode == GEMM_OUT_QKV_HEADMAJOR) { ga.tokN = N; ga.heads = H; ga.hd = 64; ga.qkv_split = (unsigned short*)ws.qkvs; }
            return k.gemm_bf16x3(ga, st);
        }
        GemmArgs ga = gemm_args(A, Wf, Cout, bias, res, rows, Nout, K, (int)lda_f, K, ldc, ldr, act);
        if (out_mode == GEMM_OUT_QKV_HEADMAJOR) { ga.out_mode = GEMM_OUT_QKV_HEADMAJOR; ga.tokN = N; ga.heads = H; ga.hd = 64; }
        return excel_launch_gemm(ga, true, 1, st);
    };
    auto linear = [&](const float* A, const float* Wf, const unsigned short* Ws, const unsigned short* Wh, const float* bias, const float* res, float* Cout,
                      int Nout, int K, int act, int out_mode) -> int {
        return linear_ex(A, Wf, Ws, Wh, bias, res, Cout, M, Nout, K, K, Nout, Nout, act, out_mode);
    };
    const int mid_mode = bf ? GEMM_OUT_SPLIT_BF16 : GEMM_OUT_PLAIN;   // format of GEMM->GEMM intermediates (MLP hidden)
    const SplitBlockW nosplit{};

    const int first_surgery = L - c.n_surgery;
    for (int l = 0; l < L; ++l) {
        const excel_vit_block_weights& bw = h->blocks[l];
        const SplitBlockW& sw = bf ? h->sblocks[l] : nosplit;
        const bool surgery = l >= first_surgery;
        float* src = (surgery && l > first_surgery) ? ws.xo : ws.x;   // :315 vs :323
        TRY(k.layernorm(src, nullptr, 1, bw.ln1_w, bw.ln1_b, ws.y, M, D, eps, st, bf, 0));
        TRY(linear(ws.y, bw.in_proj_w, sw.in_proj, sw.h_in_proj, bw.in_proj_b, nullptr, ws.qkvh, 3 * D, D, GEMM_ACT_NONE, GEMM_OUT_QKV_HEADMAJOR));
        const unsigned short* qkvs = (const unsigned short*)ws.qkvs;    // split modes: the q|k|v planes the in-proj GEMM just wrote
        // last block: its original-path output feeds only x[0] = x_ori[0] (:442) -> attention output, out-proj and MLP are
        // needed for the cls rows alone (the reference computes all rows; all_feats consumers still get them on request)
        const bool cls_only = surgery && l == L - 1 && !feats_out;
        if (bf && surgery)   // V^T in split format: B operand of A_sum.V (the row pass reads V through the LDS transpose read)
            TRY(k.vt_from_planes(qkvs, (unsigned short*)ws.vt, B, H, N, ws.KP, st));
        const bool in_aff = w_aff && l >= L - aff_layers;
        float* attn_l = (n_attn_out && l >= L - n_attn_out) ? attn_out + (size_t)(l - (L - n_attn_out)) * B * N * N : nullptr;
        // bf16x3 mode: the strip-resident kernel (attn_strip.hip) owns the softmax statistics of q.q / k.k / v.v and of the
        // q.k weights, so the row pass only runs its flash part (attention output of the original path)
        const AttnPlan ap = attn_plan(B, H, N, h->gemm_mode, surgery ? 1 : 0, (in_aff || attn_l) ? 1 : 0);
        const bool f32 = ap.path == ATTN_TWOPASS_F32;
        const int flash_nq = cls_only ? 1 : (1 << 30);
        if (f32) TRY(excel_launch_attn_rowpass_f32(ws.qkvh, ws.ao, ws.stats, B, H, N, 64, scale, ap, st, flash_nq));
        else TRY(k.attn_rowpass(qkvs, ws.ao, ws.stats, B, H, N, 64, scale, ap, st, flash_nq));
        if (surgery || in_aff || attn_l) {
            if (ap.path == ATTN_STRIP) {
                TRY(k.attn_strip(qkvs, surgery ? (unsigned short*)ws.a_sum : nullptr, in_aff ? w_aff : nullptr, attn_l, B, H, N, ws.KP,
                                 64, scale, surgery ? 1 : 0, surgery ? 1.f : 1.f / (float)H, 1.f / (float)aff_layers,
                                 (l == L - aff_layers) ? 1 : 0, ex_attn, ap, st, ws.stats));   // (the row pass above left the q.k row statistics in ws.stats)
            } else if (f32) {
                TRY(excel_launch_attn_accum_f32(ws.qkvh, ws.stats, surgery ? ws.a_sum : nullptr, in_aff ? w_aff : nullptr, attn_l, B, H, N,
                                                ws.NP, 64, scale, surgery ? 1 : 0, surgery ? 1.f : 1.f / (float)H,
                                                1.f / (float)aff_layers, (l == L - aff_layers) ? 1 : 0, ap, st, ex_attn));
            } else {
                TRY(k.attn_accum(qkvs, ws.stats, surgery ? ws.a_sum : nullptr, in_aff ? w_aff : nullptr, attn_l, B, H, N,
                                 ws.KP, 64, scale, surgery ? 1 : 0, surgery ? 1.f : 1.f / (float)H,
                                 1.f / (float)aff_layers, (l == L - aff_layers) ? 1 : 0, ap, st, ex_attn));
            }
        }
        if (!surgery) {
            TRY(linear(ws.ao, bw.out_proj_w, sw.out_proj, sw.h_out_proj, bw.out_proj_b, ws.x, ws.x, D, D, GEMM_ACT_NONE, GEMM_OUT_PLAIN));   // x += out_proj(attn)
            TRY(k.layernorm(ws.x, nullptr, 1, bw.ln2_w, bw.ln2_b, ws.y, M, D, eps, st, bf, 0));
            TRY(linear(ws.y, bw.fc1_w, sw.fc1, sw.h_fc1, bw.fc1_b, nullptr, ws.hbuf, 4 * D, D, GEMM_ACT_QUICKGELU, mid_mode));
            TRY(linear(ws.hbuf, bw.fc2_w, sw.fc2, sw.h_fc2, bw.fc2_b, ws.x, ws.x, D, 4 * D, GEMM_ACT_NONE, GEMM_OUT_PLAIN));           // x += mlp(ln_2(x))
            if (feats_out) hipMemcpyAsync(feats_out + (size_t)l * M * D, ws.x, sizeof(float) * (size_t)M * D, hipMemcpyDeviceToDevice, st);
        } else {
            // new path: (A_sum . V_h) for every head, heads concatenated -> y   (:149)
            if (bf) {
                // one bf16x3 NT GEMM per image: y[b] (split) = A_sum[b] [N x KP] . (V^T[b] [D x KP])^T
                GemmBfArgs ga = gemm_bf_args(ws.a_sum, (const unsigned short*)ws.vt, ws.y, ws.y, nullptr, nullptr, N, D, ws.KP, D, 0,
                                             GEMM_ACT_NONE, GEMM_OUT_SPLIT_BF16);
                ga.batch = B;
                ga.sA = (long long)N * 2 * ws.KP; ga.sB = (long long)D * 2 * ws.KP; ga.sC = 0; ga.sCs = (long long)N * 2 * D;
                TRY(k.gemm_bf16x3(ga, st));
            } else {   // exact fp32: batched NN GEMM over (b,h)
                GemmArgs ga = gemm_args(ws.a_sum, ws.qkvh + (size_t)2 * H * N * 64, ws.y, nullptr, nullptr, N, 64, N, ws.NP, 64, D, 0, GEMM_ACT_NONE);
                ga.Kld = ws.NP;
                ga.zdiv = H;
                ga.sA = (long long)N * ws.NP; ga.sA2 = 0;
                ga.sB = (long long)3 * H * N * 64; ga.sB2 = (long long)N * 64;
                ga.sC = (long long)N * D; ga.sC2 = 64;
                TRY(excel_launch_gemm(ga, false, B * H, st));
            }
            // original path residual first (x_ori = src + proj(attn_ori.v), :317/:326), then the new path (x += proj(.), :319/:329)
            if (cls_only) {
                const long long rs = (long long)N * D;       // row stride between consecutive cls tokens
                TRY(linear_ex(ws.ao, bw.out_proj_w, sw.out_proj, sw.h_out_proj, bw.out_proj_b, src, ws.xo, B, D, D, rs, (int)rs, (int)rs, GEMM_ACT_NONE, GEMM_OUT_PLAIN));
                TRY(linear(ws.y, bw.out_proj_w, sw.out_proj, sw.h_out_proj, bw.out_proj_b, ws.x, ws.x, D, D, GEMM_ACT_NONE, GEMM_OUT_PLAIN));
                TRY(k.layernorm(ws.xo, nullptr, 1, bw.ln2_w, bw.ln2_b, ws.y, B, D, eps, st, bf, rs));        // compact [B, D]
                TRY(linear_ex(ws.y, bw.fc1_w, sw.fc1, sw.h_fc1, bw.fc1_b, nullptr, ws.hbuf, B, 4 * D, D, D, 4 * D, 0, GEMM_ACT_QUICKGELU, mid_mode));
                TRY(linear_ex(ws.hbuf, bw.fc2_w, sw.fc2, sw.h_fc2, bw.fc2_b, ws.xo, ws.xo, B, D, 4 * D, 4 * D, (int)rs, (int)rs, GEMM_ACT_NONE, GEMM_OUT_PLAIN));
            } else {
                TRY(linear(ws.ao, bw.out_proj_w, sw.out_proj, sw.h_out_proj, bw.out_proj_b, src, ws.xo, D, D, GEMM_ACT_NONE, GEMM_OUT_PLAIN));
                // quirk Q4 (what the reference's decoder really sees): the previous block's all_feats entry is a view of
                // x_ori, and this block's `x_ori += x_ori_res` (:317) mutates it before the name is re-bound (:318)
                if (aliased_feats && l > L - c.n_surgery)
                    hipMemcpyAsync(feats_out + (size_t)(l - 1) * M * D, ws.xo, sizeof(float) * (size_t)M * D, hipMemcpyDeviceToDevice, st);
                TRY(linear(ws.y, bw.out_proj_w, sw.out_proj, sw.h_out_proj, bw.out_proj_b, ws.x, ws.x, D, D, GEMM_ACT_NONE, GEMM_OUT_PLAIN));
                TRY(k.layernorm(ws.xo, nullptr, 1, bw.ln2_w, bw.ln2_b, ws.y, M, D, eps, st, bf, 0));
                TRY(linear(ws.y, bw.fc1_w, sw.fc1, sw.h_fc1, bw.fc1_b, nullptr, ws.hbuf, 4 * D, D, GEMM_ACT_QUICKGELU, mid_mode));
                TRY(linear(ws.hbuf, bw.fc2_w, sw.fc2, sw.h_fc2, bw.fc2_b, ws.xo, ws.xo, D, 4 * D, GEMM_ACT_NONE, GEMM_OUT_PLAIN));         // x_ori += mlp(ln_2(x_ori))
            }
            if (feats_out) hipMemcpyAsync(feats_out + (size_t)l * M * D, ws.xo, sizeof(float) * (size_t)M * D, hipMemcpyDeviceToDevice, st);
        }
    }
    if (aliased_feats && c.n_surgery > 0 && c.n_surgery < L) {
        // quirk Q4: the last single-path block's entry aliases the new-path x: all `x += x_res` (:319,:329) and the cls
        // swap (:442) land in it
        float* dst = feats_out + (size_t)(L - c.n_surgery - 1) * M * D;
        hipMemcpyAsync(dst, ws.x, sizeof(float) * (size_t)M * D, hipMemcpyDeviceToDevice, st);
        hipMemcpy2DAsync(dst, sizeof(float) * (size_t)N * D, ws.xo, sizeof(float) * (size_t)N * D, sizeof(float) * D, B,
                         hipMemcpyDeviceToDevice, st);
    }
    // x[0] = x_ori[0] (:442) fused into ln_post (:445), then @ proj (:446)
    TRY(k.layernorm(ws.x, c.n_surgery > 0 ? ws.xo : nullptr, N, h->w.ln_post_w, h->w.ln_post_b, ws.y, M, D, eps, st, bf, 0));
    float* fraw = x_raw ? x_raw : ws.fraw;
    g_excel_prof_gemm_cat = PROF_CAM_PROJ;                     // the CAM's projection GEMM is reported on its own (bench.py roofline_sim_gemm)
    const int rc_proj = linear(ws.y, h->projT, h->s_projT, h->h_projT, nullptr, nullptr, fraw, C, D, GEMM_ACT_NONE, GEMM_OUT_PLAIN);
    g_excel_prof_gemm_cat = -1;
    TRY(rc_proj);
    if (image_features) TRY(k.token_axis_normalize(fraw, ws.ss, image_features, B, N, C, st));   // clip.py:353 (the fused CAM kernel does it itself)
    return EXCEL_OK;
}

extern "C" int excel_vit_forward_ex(excel_vit_t h, const float* img, int B, int S, void* workspace, size_t workspace_bytes,
                                    float* image_features, float* x_raw, float* w_aff, int aff_layers, float* attn_out,
                                    int n_attn_out, float* feats_out, const float* ex_attn, int flags, void* stream) {
    EXCEL_CHECK_ARG(h, "excel_vit_forward: null handle");
    return vit_forward(split_api(h->gemm_mode), h, img, B, S, workspace, workspace_bytes, image_features, x_raw, w_aff, aff_layers, attn_out,
                       n_attn_out, feats_out, ex_attn, flags, stream);
}

extern "C" int excel_vit_forward(excel_vit_t h, const float* img, int B, int S, void* workspace, size_t workspace_bytes,
                                 float* image_features, float* x_raw, float* w_aff, int aff_layers, float* attn_out,
                                 int n_attn_out, float* feats_out, void* stream) {
    return excel_vit_forward_ex(h, img, B, S, workspace, workspace_bytes, image_features, x_raw, w_aff, aff_layers, attn_out, n_attn_out,
                                feats_out, nullptr, 0, stream);
}
