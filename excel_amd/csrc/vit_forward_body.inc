// Body of the ViT surgery forward (abi.hip: vit_forward_bf16 / vit_forward_f16).  Included twice: the unqualified launcher names bind to
// namespace excel_bf16 (default) or, through block-scope using-declarations, to excel_f16 - the same host code over either split type.
    const bool aliased_feats = feats_out && (flags & EXCEL_VIT_FEATS_AS_REFERENCE);
    EXCEL_CHECK_ARG(h && img && workspace && (image_features || x_raw), "excel_vit_forward: null argument (image_features or x_raw is required)");
    const excel_vit_config& c = h->cfg;
    EXCEL_CHECK_ARG(B > 0 && S > 0 && S % c.patch == 0, "excel_vit_forward: S must be a positive multiple of the patch size");
    const int ps = c.patch, g = S / ps, P = g * g, N = P + 1, D = c.width, H = c.heads, L = c.layers, C = c.out_dim;
    EXCEL_CHECK_ARG(n_attn_out >= 0 && n_attn_out <= L && (n_attn_out == 0 || attn_out), "excel_vit_forward: bad attn_out request");
    EXCEL_CHECK_ARG(!w_aff || (aff_layers >= 1 && aff_layers <= L), "excel_vit_forward: bad aff_layers");
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

    const bool bf = h->gemm_mode >= 1;                  // split-plane modes: 1 = bf16x3, 2 = f16x3, 3 = f16x2 (this body is compiled once per type)
    const bool x2 = h->gemm_mode == 3;                  // fp16-valued weights (checked by set_gemm_mode): two-product weight GEMMs
    // patch embedding: im2col -> GEMM (conv1 weight is [D, 3*ps*ps] K-major) -> +cls/pos, ln_pre
    TRY(excel_launch_im2col(img, ws.hbuf, B, S, ps, st, bf ? 1 : 0));
    {
        const int Kc = 3 * ps * ps;
        if (bf) {
            GemmBfArgs ga = gemm_bf_args(ws.hbuf, h->s_conv1, ws.ao, nullptr, nullptr, nullptr, B * P, D, Kc, D, 0, GEMM_ACT_NONE, GEMM_OUT_PLAIN);
            if (x2) { ga.w_lo_zero = 1; ga.Bh = h->h_conv1; ga.ldbh = Kc; }
            TRY(excel_launch_gemm_bf16x3(ga, st));
        } else {
            GemmArgs ga = gemm_args(ws.hbuf, h->w.conv1_w, ws.ao, nullptr, nullptr, B * P, D, Kc, Kc, Kc, D, 0, GEMM_ACT_NONE);
            TRY(excel_launch_gemm(ga, true, 1, st));
        }
    }
    TRY(excel_launch_assemble_ln_pre(ws.ao, h->w.class_emb, pos, h->w.ln_pre_w, h->w.ln_pre_b, ws.x, B, N, D, eps, st));

    // linear layer helper: C = act(A . W^T + bias) + res, A produced in the mode's operand format.
    // rows/lda_f/ldc/ldr default to the dense [M, .] case; the last block uses them to touch only the cls rows.
    auto linear_ex = [&](const float* A, const float* Wf, const unsigned short* Ws, const unsigned short* Wh, const float* bias, const float* res, float* Cout,
                         int rows, int Nout, int K, long long lda_f, int ldc, int ldr, int act, int out_mode) -> int {
        if (bf) {
            GemmBfArgs ga = gemm_bf_args(A, Ws, Cout, Cout, bias, res, rows, Nout, K, ldc, ldr, act, out_mode);
            ga.lda = (int)(2 * lda_f);
            if (x2) { ga.w_lo_zero = 1; ga.Bh = Wh; ga.ldbh = K; }
            if (out_mode == GEMM_OUT_QKV_HEADMAJOR) { ga.tokN = N; ga.heads = H; ga.hd = 64; ga.qkv_split = (unsigned short*)ws.qkvs; }
            return excel_launch_gemm_bf16x3(ga, st);
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
        TRY(excel_launch_layernorm(src, nullptr, 1, bw.ln1_w, bw.ln1_b, ws.y, M, D, eps, st, bf));
        TRY(linear(ws.y, bw.in_proj_w, sw.in_proj, sw.h_in_proj, bw.in_proj_b, nullptr, ws.qkvh, 3 * D, D, GEMM_ACT_NONE, GEMM_OUT_QKV_HEADMAJOR));
        const unsigned short* qkvs = (const unsigned short*)ws.qkvs;    // split modes: the q|k|v planes the in-proj GEMM just wrote
        // last block: its original-path output feeds only x[0] = x_ori[0] (:442) -> attention output, out-proj and MLP are
        // needed for the cls rows alone (the reference computes all rows; all_feats consumers still get them on request)
        const bool cls_only = surgery && l == L - 1 && !feats_out;
        if (bf && surgery)   // V^T in split format: B operand of A_sum.V (the row pass reads V through the LDS transpose read)
            TRY(excel_launch_vt_from_planes(qkvs, (unsigned short*)ws.vt, B, H, N, ws.KP, st));
        const bool in_aff = w_aff && l >= L - aff_layers;
        float* attn_l = (n_attn_out && l >= L - n_attn_out) ? attn_out + (size_t)(l - (L - n_attn_out)) * B * N * N : nullptr;
        // bf16x3 mode: the strip-resident kernel (attn_strip.hip) owns the softmax statistics of q.q / k.k / v.v and of the
        // q.k weights, so the row pass only runs its flash part (attention output of the original path)
        const AttnPlan ap = attn_plan(B, H, N, h->gemm_mode, surgery ? 1 : 0, (in_aff || attn_l) ? 1 : 0);
        const bool f32 = ap.path == ATTN_TWOPASS_F32;
        const int flash_nq = cls_only ? 1 : (1 << 30);
        if (f32) TRY(excel_launch_attn_rowpass_f32(ws.qkvh, ws.ao, ws.stats, B, H, N, 64, scale, ap, st, flash_nq));
        else TRY(excel_launch_attn_rowpass(qkvs, ws.ao, ws.stats, B, H, N, 64, scale, ap, st, flash_nq));
        if (surgery || in_aff || attn_l) {
            if (ap.path == ATTN_STRIP) {
                TRY(excel_launch_attn_strip(qkvs, surgery ? (unsigned short*)ws.a_sum : nullptr, in_aff ? w_aff : nullptr, attn_l, B, H, N, ws.KP,
                                            64, scale, surgery ? 1 : 0, surgery ? 1.f : 1.f / (float)H, 1.f / (float)aff_layers,
                                            (l == L - aff_layers) ? 1 : 0, ex_attn, ap, st, ws.stats));   // (the row pass above left the q.k row statistics in ws.stats)
            } else if (f32) {
                TRY(excel_launch_attn_accum_f32(ws.qkvh, ws.stats, surgery ? ws.a_sum : nullptr, in_aff ? w_aff : nullptr, attn_l, B, H, N,
                                                ws.NP, 64, scale, surgery ? 1 : 0, surgery ? 1.f : 1.f / (float)H,
                                                1.f / (float)aff_layers, (l == L - aff_layers) ? 1 : 0, ap, st, ex_attn));
            } else {
                TRY(excel_launch_attn_accum(qkvs, ws.stats, surgery ? ws.a_sum : nullptr, in_aff ? w_aff : nullptr, attn_l, B, H, N,
                                            ws.KP, 64, scale, surgery ? 1 : 0, surgery ? 1.f : 1.f / (float)H,
                                            1.f / (float)aff_layers, (l == L - aff_layers) ? 1 : 0, ap, st, ex_attn));
            }
        }
        if (!surgery) {
            TRY(linear(ws.ao, bw.out_proj_w, sw.out_proj, sw.h_out_proj, bw.out_proj_b, ws.x, ws.x, D, D, GEMM_ACT_NONE, GEMM_OUT_PLAIN));   // x += out_proj(attn)
            TRY(excel_launch_layernorm(ws.x, nullptr, 1, bw.ln2_w, bw.ln2_b, ws.y, M, D, eps, st, bf));
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
                TRY(excel_launch_gemm_bf16x3(ga, st));
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
                TRY(excel_launch_layernorm(ws.xo, nullptr, 1, bw.ln2_w, bw.ln2_b, ws.y, B, D, eps, st, bf, rs));        // compact [B, D]
                TRY(linear_ex(ws.y, bw.fc1_w, sw.fc1, sw.h_fc1, bw.fc1_b, nullptr, ws.hbuf, B, 4 * D, D, D, 4 * D, 0, GEMM_ACT_QUICKGELU, mid_mode));
                TRY(linear_ex(ws.hbuf, bw.fc2_w, sw.fc2, sw.h_fc2, bw.fc2_b, ws.xo, ws.xo, B, D, 4 * D, 4 * D, (int)rs, (int)rs, GEMM_ACT_NONE, GEMM_OUT_PLAIN));
            } else {
                TRY(linear(ws.ao, bw.out_proj_w, sw.out_proj, sw.h_out_proj, bw.out_proj_b, src, ws.xo, D, D, GEMM_ACT_NONE, GEMM_OUT_PLAIN));
                // quirk Q4 (what the reference's decoder really sees): the previous block's all_feats entry is a view of
                // x_ori, and this block's `x_ori += x_ori_res` (:317) mutates it before the name is re-bound (:318)
                if (aliased_feats && l > L - c.n_surgery)
                    hipMemcpyAsync(feats_out + (size_t)(l - 1) * M * D, ws.xo, sizeof(float) * (size_t)M * D, hipMemcpyDeviceToDevice, st);
                TRY(linear(ws.y, bw.out_proj_w, sw.out_proj, sw.h_out_proj, bw.out_proj_b, ws.x, ws.x, D, D, GEMM_ACT_NONE, GEMM_OUT_PLAIN));
                TRY(excel_launch_layernorm(ws.xo, nullptr, 1, bw.ln2_w, bw.ln2_b, ws.y, M, D, eps, st, bf));
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
    TRY(excel_launch_layernorm(ws.x, c.n_surgery > 0 ? ws.xo : nullptr, N, h->w.ln_post_w, h->w.ln_post_b, ws.y, M, D, eps, st, bf));
    float* fraw = x_raw ? x_raw : ws.fraw;
    g_excel_prof_gemm_cat = PROF_CAM_PROJ;                     // the CAM's projection GEMM is reported on its own (bench.py roofline_sim_gemm)
    const int rc_proj = linear(ws.y, h->projT, h->s_projT, h->h_projT, nullptr, nullptr, fraw, C, D, GEMM_ACT_NONE, GEMM_OUT_PLAIN);
    g_excel_prof_gemm_cat = -1;
    TRY(rc_proj);
    if (image_features) TRY(excel_launch_token_axis_normalize(fraw, ws.ss, image_features, B, N, C, st));   // clip.py:353 (the fused CAM kernel does it itself)
    return EXCEL_OK;
