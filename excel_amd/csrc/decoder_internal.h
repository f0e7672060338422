// Shared between decoder.hip (inference) and train.hip (training iteration).
#pragma once
#include <string.h>
#include <vector>
#include "common.h"
#include "excel_internal.h"
#include "../../include/excel_hip.h"

struct excel_decoder {
    excel_decoder_config cfg;
    std::vector<excel_fuse_layer_weights> fuse;
    std::vector<excel_decoder_block_weights> blocks;
    excel_decoder_weights w;
};

// decoder.hip
int excel_launch_dec_softmax(float* s, long long rows, int P, int Pp, int causal, hipStream_t st);
// [B, R, Cc] (row pitch ld) -> [B, Cc, Rp]: out[b][c][r] = in[b][r][c]; columns r in [R, Rp) are zero-filled
int excel_launch_dec_transpose(const float* in, float* out, int B, int R, int Cc, int ld, int Rp, hipStream_t st);
// The attention core of a pre-LN block (nn.MultiheadAttention): qkv [B,3,H,P,hd] head-major -> scores[b,h] = q k^T / sqrt(hd)
// ([B*H, P, Pp], left holding the probabilities), row softmax (causal: keys 0..q), attn_out[b, :, h*hd..] = P[b,h] . v[b,h] ([B*P, E])
int excel_launch_dec_attention(const float* qkv, float* scores, float* attn_out, int B, int P, int Pp, int E, int H, int causal, hipStream_t st);
