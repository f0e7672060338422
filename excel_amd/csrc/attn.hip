// Self-attention kernels of the ExCEL "surgery" ViT (clip/clip_surgery_model.py:95-159, :307) for the split-plane modes (bf16x3 /
// f16x3 / f16x2): scores and P.V as three products of 16-bit hi / lo planes on the matrix core, softmax in fp32.  The exact-fp32
// kernels, whose header describes the design both share (head-major q|k|v, transposed score tiles with a query row in one lane, a
// row pass for the statistics and the attention output, a second pass that reduces the probabilities over heads in registers),
// are in attn_f32.hip; up to 40 key tiles the second pass is the strip-resident kernel of attn_strip.hip.
#include <stdlib.h>
#include "common.h"
#include "excel_internal.h"

namespace EXCEL_SPLIT_NS {     // compiled once per 16-bit split type (excel_internal.h, build.py)

#define HD 64

// ------------------------------------------------------------------------------------------------ rowpass
struct RowpassArgs {
    float* out;          // split tensor [B*N][2][H*64]: attention output of type 0 (pre out-proj), A operand of the out-proj GEMM
    float2* stats;       // [B,H,4,N] {row max (scaled scores, log2 units), 1/row sum}
    int B, H, N;
    float scale;
    const unsigned short* qkvs;   // q|k|v head-major in split format [B,3,H,N][2][64]
    int flash_nq;        // q-blocks >= flash_nq of type 0 only produce row stats (last block: only the cls row's output is consumed)
    int xcd_local;       // 1: workgroups of one (image, head) on one XCD
    int tail_grp;        // (image, head) groups per chunk of the XCD-local order: their full q-blocks, then their partial last q-blocks
};

typedef unsigned short u16;

// ------------------------------------------------------------------------------------------------ rowpass, bf16x3 pipeline
// Production variant of the row pass (bf16x3 scores AND bf16x3 P.V): K (split q|k|v rows) and V^T tiles stream through a
// 3-stage LDS ring filled by global_load_lds (no VGPR round trip), two key tiles in flight behind a counted s_waitcnt
// vmcnt + raw s_barrier, exactly like gemm_bf16x3_kernel<4,3>: the register-staged version waited for each tile's global
// loads inside the step that issued them.  LDS images are lane-linear, so both swizzles are applied to the SOURCE address:
//   K tile   [32 keys][16 chunks of 16 B = hi 64 | lo 64]   chunk c at slot c ^ (key & 15)      (conflict-free b128)
//   V tile   8 sub-tiles (hi d 0-15, 16-31, 32-47, 48-63, then lo) of [32 keys][16 d] bf16, 1 KB each, 1152 B apart: the P.V operand
//            (lane = d, 4 consecutive keys) is read with ds_read_b64_tr_b16 - the hardware transposes a [4 keys][16 d] block per 16
//            lanes, each lane supplying the address of one 8-byte row segment - straight from the row-major q|k|v planes.  Rounds 1-3
//            read it from a V^T copy that a separate transpose kernel wrote per block (0.39 ms per step, 2-way LDS conflicts).
template <bool FLASH>
__device__ __forceinline__ void rowpass_body_bf(const RowpassArgs& p, float* smem, int b, int h, int type, int qblk) {
    constexpr int KT_EL = 32 * 128;                      // u16 elements of a K tile (8 KB)
    constexpr int VSUB = 1152;                           // bytes between V sub-tiles: 1 KB + 128 (the two sub-tiles a half-wave reads sit in complementary banks)
    constexpr int VT_EL = 8 * VSUB / 2;                  // u16 elements of a V tile (9 KB)
    constexpr int STAGE_EL = KT_EL + (FLASH ? VT_EL : 0);
    constexpr int PER_WAVE = FLASH ? 4 : 2;              // 1-KB global_load_lds per wave per key tile
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int r = lane & 31, kh = lane >> 5;
    const int N = p.N;
    const int tx = (type == 0 || type == 1) ? 0 : (type == 2 ? 1 : 2);
    const int ty = (type == 0) ? 1 : tx;
    const u16* Xsp = p.qkvs + (((long long)b * 3 + tx) * p.H + h) * (long long)N * 128;
    const u16* Ysp = p.qkvs + (((long long)b * 3 + ty) * p.H + h) * (long long)N * 128;
    const u16* Vsp = p.qkvs + (((long long)b * 3 + 2) * p.H + h) * (long long)N * 128;
    u16* ring = reinterpret_cast<u16*>(smem);            // [3][K tile | V^T tile]
    const unsigned ring_b = __builtin_amdgcn_readfirstlane(lds_addr(ring));      // (provably wave-uniform: it goes into m0)

    const int q0 = qblk * 128 + wave * 32;
    const int qrow = min(q0 + r, N - 1);
    splitx8 xh[4], xl[4];
#pragma unroll
    for (int s4 = 0; s4 < 4; ++s4) {
        xh[s4] = *reinterpret_cast<const splitx8*>(Xsp + (long long)qrow * 128 + s4 * 16 + kh * 8);
        xl[s4] = *reinterpret_cast<const splitx8*>(Xsp + (long long)qrow * 128 + 64 + s4 * 16 + kh * 8);
    }

    // consume the query fragments once BEFORE any LDS-DMA is in flight: the compiler then places its wait for these ordinary loads
    // here and not (as vmcnt(0), draining the DMA queue) in front of their first use inside the key loop
    asm volatile("" : "+v"(xh[0]), "+v"(xh[1]), "+v"(xh[2]), "+v"(xh[3]), "+v"(xl[0]), "+v"(xl[1]), "+v"(xl[2]), "+v"(xl[3]));
    // LDS-DMA through buffer descriptors over this (image, head)'s key plane and V^T rows: the per-lane byte offsets are loop invariant
    // (2 + 2 VGPRs), the tile position goes into the scalar offset - no per-lane 64-bit address arithmetic and no row clamp inside the key
    // loop (it was ~14 VALU instructions per key tile in a loop that is bound by instruction issue).  Key rows past the end of the plane
    // read the next plane / the descriptor's out-of-range zeros: finite, and masked to -inf below; V^T is zero padded to vt_kp keys.
    typedef __attribute__((address_space(3))) unsigned char* lds_bptr;
    const long long kplane_bytes = (long long)N * 256;
    const long long kavail = ((((long long)p.B * 3 - ((long long)b * 3 + ty)) * p.H - h) * kplane_bytes);      // bytes from this plane to the end of qkvs
    const __amdgpu_buffer_rsrc_t rs_k = __builtin_amdgcn_make_buffer_rsrc((void*)Ysp, 0, (int)(kavail < (1LL << 31) - 1 ? kavail : (1LL << 31) - 1), 0x00020000);
    const long long vavail = ((((long long)p.B * 3 - ((long long)b * 3 + 2)) * p.H - h) * kplane_bytes);       // ... from the v plane to the end of qkvs
    const __amdgpu_buffer_rsrc_t rs_v = __builtin_amdgcn_make_buffer_rsrc((void*)Vsp, 0, FLASH ? (int)(vavail < (1LL << 31) - 1 ? vavail : (1LL << 31) - 1) : 0, 0x00020000);
    int koffb[2], voffb[2];
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const int krow = wave * 8 + j * 4 + (lane >> 4);                 // row of the tile this lane loads a chunk of
        koffb[j] = krow * 256 + (((lane & 15) ^ (krow & 15)) * 16);
        const int sub = wave * 2 + j;                                    // V sub-tile this lane loads 16 B of: key lane >> 1, d half lane & 1
        voffb[j] = (lane >> 1) * 256 + (sub >> 2) * 128 + (((sub & 3) * 16 + (lane & 1) * 8) * 2);
    }
    // piece idx of this wave's PER_WAVE 1-KB loads of key tile kt: 0, 1 = K rows, 2, 3 = V^T rows (flash only)
    auto issue_piece = [&](int kt, int stage, int idx) {
        unsigned dstk = __builtin_amdgcn_readfirstlane(ring_b + stage * (STAGE_EL * 2));     // wave-uniform (it goes into m0); also keeps
        asm volatile("" : "+s"(dstk));                                                         // the per-piece destinations out of hoisted SGPRs
        if (idx < 2) {
            __builtin_amdgcn_raw_ptr_buffer_load_lds(rs_k, (lds_bptr)(unsigned long long)(dstk + (wave * 8 + idx * 4) * 256), 16, koffb[idx], kt * (32 * 256), 0, 0);
        } else if (FLASH) {
            const int j = idx - 2;
            __builtin_amdgcn_raw_ptr_buffer_load_lds(rs_v, (lds_bptr)(unsigned long long)(dstk + KT_EL * 2 + (wave * 2 + j) * VSUB), 16, voffb[j], kt * (32 * 256), 0, 0);
        }
    };
    auto issue = [&](int kt, int stage) {
#pragma unroll
        for (int idx = 0; idx < PER_WAVE; ++idx) issue_piece(kt, stage, idx);
    };

    const float c2 = p.scale * 1.4426950408889634f;     // scores enter the softmax in log2 units
    float m = -INFINITY, l = 0.f;                         // m: running row max in log2 units
    f32x16 oT[2];
#pragma unroll
    for (int e = 0; e < 16; ++e) { oT[0][e] = 0.f; oT[1][e] = 0.f; }

    const int nkt = (N + 31) / 32;
    issue(0, 0);
    if (nkt > 1) issue(1, 1);
    int stage = 0;
    for (int kt = 0; kt < nkt; ++kt) {
        if (kt + 1 < nkt) {
            if (PER_WAVE == 4) asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
            else asm volatile("s_waitcnt vmcnt(2)" ::: "memory");
        } else {
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        }
        __builtin_amdgcn_s_barrier();
        const int rstage = stage == 0 ? 2 : stage - 1;                       // slot of tile kt-1, free since the barrier: tile kt+2 goes there
        const bool refill = kt + 2 < nkt;
        if (q0 >= N) {                                                        // wave-uniform: all 32 query rows are padding -> only keep the ring moving
            if (refill) issue(kt + 2, rstage);
            stage = (stage == 2) ? 0 : stage + 1;
            continue;
        }
        // LDS reads as inline asm (common.h): a compiler-visible ds_read behind pending LDS-DMA gets an s_waitcnt vmcnt(0) in front of
        // it, which drained the two key tiles in flight on every step
        const unsigned kr = ring_b + (stage * STAGE_EL + r * 128) * 2;
        f32x16 s;
#pragma unroll
        for (int e = 0; e < 16; ++e) s[e] = 0.f;
        {
            splitx8 yh[4], yl[4];
#pragma unroll
            for (int s4 = 0; s4 < 4; ++s4) {
                yh[s4] = lds_read16(kr + (((s4 * 2 + kh) ^ (r & 15)) * 16));
                yl[s4] = lds_read16(kr + (((8 + s4 * 2 + kh) ^ (r & 15)) * 16));
            }
            lds_wait8(yh, yl);
            // the refill is issued one piece per k-step between the score MFMAs (back to back, the pieces of all waves queue up in the CU's
            // one address path and each wave sits behind its own before it reaches its MFMAs)
#pragma unroll
            for (int s4 = 0; s4 < 4; ++s4) {
                if (refill && s4 < PER_WAVE) issue_piece(kt + 2, rstage, s4);
                s = EXCEL_MFMA16(yl[s4], xh[s4], s, 0, 0, 0);
                s = EXCEL_MFMA16(yh[s4], xl[s4], s, 0, 0, 0);
                s = EXCEL_MFMA16(yh[s4], xh[s4], s, 0, 0, 0);
                __builtin_amdgcn_sched_barrier(0);
            }
        }
        // softmax bookkeeping in log2 units: p = exp2(s*c2 - m2), c2 = scale*log2(e)  (one fma + one v_exp per element);
        // only the last key tile can contain keys >= N, so the mask lives in a uniform branch.
        if (kt == nkt - 1) {
#pragma unroll
            for (int e = 0; e < 16; ++e)
                if (kt * 32 + c32_row(e, lane) >= N) s[e] = -INFINITY;
        }
        float mx = s[0];
#pragma unroll
        for (int e = 1; e < 16; ++e) mx = fmaxf(mx, s[e]);
        {
            float mlo, mhi;
            wave_halves(mx, mlo, mhi);
            mx = fmaxf(mlo, mhi) * c2;
        }
        const float m_new = fmaxf(m, mx);
        const bool grew = m_new > m;
        const float alpha = __builtin_amdgcn_exp2f(m - m_new);            // 1.0 exactly when the running max did not move
        float ps = 0.f;
#pragma unroll
        for (int e = 0; e < 16; ++e) {
            s[e] = __builtin_amdgcn_exp2f(fmaf(s[e], c2, -m_new));
            ps += s[e];
        }
        {
            float plo, phi;
            wave_halves(ps, plo, phi);
            ps = plo + phi;
        }
        l = l * alpha + ps;
        m = m_new;
        if (FLASH) {
            if (__any(grew)) {                           // wave-uniform: after the first few tiles the max rarely moves
#pragma unroll
                for (int e = 0; e < 16; ++e) { oT[0][e] *= alpha; oT[1][e] *= alpha; }
            }
            // P (this lane: keys (e&3)+8(e>>2)+4kh of query r) -> bf16 hi/lo; MFMA k-step ks takes e = 8ks..8ks+7, i.e. keys
            // {16ks+4kh+0..3, 16ks+8+4kh+0..3}: the V operand (lane = d) takes exactly those two groups of 4 consecutive keys.
            // hi = p truncated to bf16 (bit mask), lo = bf16(p - hi): p - hi is exact, so hi + lo keeps 16 mantissa bits.
            splitx8 ph[2], pl[2];
#ifdef EXCEL_SPLIT_F16
            {   // IEEE half: probabilities need neither the saturation nor the NaN test of split_hi (common.h: split_pair_bounded)
                unsigned phu[2][4], plu[2][4];
#pragma unroll
                for (int e = 0; e < 16; e += 2) split_pair_bounded(s[e], s[e + 1], phu[e >> 3][(e & 7) >> 1], plu[e >> 3][(e & 7) >> 1]);
#pragma unroll
                for (int q = 0; q < 2; ++q) {
                    ph[q] = __builtin_bit_cast(splitx8, uint4{phu[q][0], phu[q][1], phu[q][2], phu[q][3]});
                    pl[q] = __builtin_bit_cast(splitx8, uint4{plu[q][0], plu[q][1], plu[q][2], plu[q][3]});
                }
            }
#else
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                const float hf = __uint_as_float(__float_as_uint(s[e]) & 0xFFFF0000u);
                ph[e >> 3][e & 7] = split_hi(hf);
                pl[e >> 3][e & 7] = split_hi(s[e] - hf);
            }
#endif
            // lane (d = 32 dt + r, kh): sub-tile 2 dt + (r >> 4), its column r & 15; the 16 lanes of a group address the 16 row segments
            // (key = k0 + i / 4, d quarter i % 4) of the [4 keys][16 d] block whose column they receive
            const unsigned vb = ring_b + (stage * STAGE_EL + KT_EL) * 2 + ((lane >> 4) & 1) * VSUB + (4 * kh + ((lane & 15) >> 2)) * 32 + (lane & 3) * 8;
#pragma unroll
            for (int dt = 0; dt < 2; ++dt) {
                splitx4 vq[8];                                   // [ks][h0 h1 l0 l1]
                const unsigned vbd = vb + dt * 2 * VSUB;        // (one address per d tile; everything else is the instruction's immediate)
                vq[0] = lds_read8h_tr<0>(vbd);
                vq[1] = lds_read8h_tr<256>(vbd);
                vq[2] = lds_read8h_tr<4 * VSUB>(vbd);
                vq[3] = lds_read8h_tr<4 * VSUB + 256>(vbd);
                vq[4] = lds_read8h_tr<512>(vbd);
                vq[5] = lds_read8h_tr<512 + 256>(vbd);
                vq[6] = lds_read8h_tr<4 * VSUB + 512>(vbd);
                vq[7] = lds_read8h_tr<4 * VSUB + 512 + 256>(vbd);
                asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(vq[0]), "+v"(vq[1]), "+v"(vq[2]), "+v"(vq[3]), "+v"(vq[4]), "+v"(vq[5]), "+v"(vq[6]), "+v"(vq[7])::"memory");
#pragma unroll
                for (int ks = 0; ks < 2; ++ks) {
                    const splitx4 h0 = vq[ks * 4], h1 = vq[ks * 4 + 1], l0 = vq[ks * 4 + 2], l1 = vq[ks * 4 + 3];
                    const splitx8 vh = {h0[0], h0[1], h0[2], h0[3], h1[0], h1[1], h1[2], h1[3]};
                    const splitx8 vl = {l0[0], l0[1], l0[2], l0[3], l1[0], l1[1], l1[2], l1[3]};
                    oT[dt] = EXCEL_MFMA16(vl, ph[ks], oT[dt], 0, 0, 0);
                    oT[dt] = EXCEL_MFMA16(vh, pl[ks], oT[dt], 0, 0, 0);
                    oT[dt] = EXCEL_MFMA16(vh, ph[ks], oT[dt], 0, 0, 0);
                }
            }
        }
        stage = (stage == 2) ? 0 : stage + 1;
    }

    const float linv = 1.f / l;
    if (kh == 0 && q0 + r < N)
        p.stats[(((long long)b * p.H + h) * 4 + type) * N + q0 + r] = make_float2(m, linv);   // m in LOG2 units (bf16x3 accum expects that)

    if (FLASH) {
        __syncthreads();     // every wave has finished reading the ring: reuse it for the output transpose
        float* ob = smem + wave * (32 * 65);
#pragma unroll
        for (int dt = 0; dt < 2; ++dt)
#pragma unroll
            for (int e = 0; e < 16; ++e) ob[r * 65 + dt * 32 + c32_row(e, lane)] = oT[dt][e] * linv;
        __builtin_amdgcn_s_waitcnt(0xc07f);
        for (int qq = 0; qq < 32; ++qq) {
            const int q = q0 + qq;
            if (q >= N) break;
            const float v = ob[qq * 65 + lane];
            const split_t hi = split_hi(v);
            split_t* o = reinterpret_cast<split_t*>(p.out) + ((long long)b * N + q) * 2 * (p.H * HD) + split_off(h * HD + lane, 0);
            o[0] = hi;
            o[32] = split_hi(v - (float)hi);
        }
    }
}

__global__ __launch_bounds__(256, 2) void attn_rowpass_kernel(RowpassArgs p) {
    __shared__ __attribute__((aligned(1024))) float smem[3 * (2048 + 2304)];   // 51 KB: 3-stage ring of (K tile 8 KB + V tile 9 KB)
    int bh, qb;
    rowpass_block_map(p.N, p.xcd_local, p.tail_grp, bh, qb);
    const int b = bh / p.H, h = bh % p.H;
    const int type = blockIdx.z;
    if (type == 0 && qb < p.flash_nq) rowpass_body_bf<true>(p, smem, b, h, 0, qb);
    else rowpass_body_bf<false>(p, smem, b, h, type, qb);
}

// ------------------------------------------------------------------------------------------------ accum
struct AccumArgs {
    const float2* stats;  // [B,H,4,N]
    float* a_sum;         // split tensor [B,N][2*NP] (NP % 32 == 0; surgery only): head-sum of (qq+kk+vv softmaxes)/3, zero in columns
                          // [N,NP) - A operand of the A_sum.V GEMM
    float* w_aff;         // [B,P,P]   running layer-mean of W[1:,1:]   (may be null)
    float* attn_out;      // [B,N,N]   W of this layer (may be null)
    int B, H, N, NP;
    float scale;
    float w_scale;        // 1/H for nn.MultiheadAttention blocks (head-mean), 1 for surgery blocks (head-sum)
    float aff_scale;      // 1/attn_layers
    int aff_init;         // 1: w_aff = ..., 0: w_aff += ...
    const unsigned short* qkvs;   // q|k|v head-major in split format [B,3,H,N][2][64]
    int dbg;              // dev: bit0 skip scoring, bit1 skip tile loads, bit2 skip the output epilogue
    const float* ex_attn; // [B,P,P] LVC cue added to every head's attn[1:,1:] of a surgery block (may be null)
    float ex_scale;       // = H (the head sum of a per-head constant)
};

// ------------------------------------------------------------------------------------------------ accum, bf16x3 pipeline
// The accumulate pass (attn_f32.hip: attn_accum) of the split modes beyond the strip kernel's reach, restructured after measuring it:
//   * workgroup = 128 queries x 64 keys, 8 waves (4 x 2, one 32x32 score tile each): two waves per SIMD, so one wave's
//     exp/accumulate VALU work overlaps the other's MFMAs, and 25 % fewer operand bytes per score than 64 x 64;
//   * the six operand tiles (q|k|v rows of the query tile X: 32 KB each, of the key tile Y: 16 KB each) and the row stats
//     are streamed by global_load_lds on a ROLLING schedule, so the tiles of head h+1 land while head h is scored.
// Per head, 4 steps, one raw s_barrier each (X tile = 4, Y tile = 2, stats = 2 wave-instructions per wave):
//     step 0  qq (XQ,YQ)  issue XV,YV(h)                 wait XQ,YQ,stats(h): newest XK,YK(h)          -> vmcnt(6)
//     step 1  qk (XQ,YK)  issue YQ,stats(h+1)            wait YK(h):          newest XV,YV(h)          -> vmcnt(6)
//     step 2  kk (XK,YK)  issue XQ(h+1)                  (barrier only: frees XQ)
//     step 3  vv (XV,YV)  issue XK,YK(h+1)               wait XV,YV(h):       newest YQ,stats,XQ(h+1)  -> vmcnt(8) / (0) last
// A slot is refilled only after the barrier that follows its last reader; vmcnt retires loads in issue order.  There is
// no ordinary global load inside the loop (it would force a vmcnt(0) drain of the LDS-DMA queue).
template <bool SURGERY>
__global__ __launch_bounds__(512, 2) void attn_accum_bf_kernel(AccumArgs p) {
    constexpr int XT = 128 * 128, YT = 64 * 128;                    // u16 elements of an X tile (32 KB) / Y tile (16 KB)
    constexpr int NTYPE = SURGERY ? 4 : 1;
    // surgery: XQ XK XV | YQ YK YV ; else double-buffered (XQ, YK)
    constexpr int TILES_EL = SURGERY ? 3 * XT + 3 * YT : 2 * (XT + YT);
    __shared__ __attribute__((aligned(1024))) u16 tiles[TILES_EL];
    __shared__ __attribute__((aligned(1024))) float2 lstats[2 * NTYPE * 128 + 32];   // [buffer][type][128 q] + a dump slot
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int r = lane & 31, kh = lane >> 5;
    const int wq = wave >> 1, wk = wave & 1;
    int kt = blockIdx.x, qt = blockIdx.y, b = blockIdx.z;
    if (EXCEL_DBG(p.dbg) & 8) {      // experiment: XCD-contiguous tile order (workgroups sharing X / Y tiles on one L2)
        const int lin = blockIdx.x + gridDim.x * (blockIdx.y + gridDim.y * blockIdx.z);
        const int id = xcd_remap(lin, gridDim.x * gridDim.y * gridDim.z);
        kt = id % gridDim.x; qt = (id / gridDim.x) % gridDim.y; b = id / (gridDim.x * gridDim.y);
    }
    const int N = p.N;

    // staging: the tile image is lane-linear (one wave-instruction = 1 KB = 4 rows x 16 chunks), so the swizzle
    // (chunk c at slot c ^ (row & 15)) is applied to the source address.  X: wave w rows 16w..16w+15 (4 instr);
    // Y: rows 8w..8w+7 (2 instr).
    int rowx[4], coffx[4], rowy[2], coffy[2];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int row_l = wave * 16 + j * 4 + (lane >> 4);
        coffx[j] = ((lane & 15) ^ (row_l & 15)) * 8;
        rowx[j] = min(qt * 128 + row_l, N - 1);
    }
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const int row_l = wave * 8 + j * 4 + (lane >> 4);
        coffy[j] = ((lane & 15) ^ (row_l & 15)) * 8;
        rowy[j] = min(kt * 64 + row_l, N - 1);
    }
    auto issue_x = [&](int off, int typ, int h) {
        const u16* src = p.qkvs + (((long long)b * 3 + typ) * p.H + h) * (long long)N * 128;
#pragma unroll
        for (int j = 0; j < 4; ++j)
            __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(src + (long long)rowx[j] * 128 + coffx[j]),
                                             (__attribute__((address_space(3))) void*)(tiles + off + (wave * 16 + j * 4) * 128), 16, 0, 0);
    };
    auto issue_y = [&](int off, int typ, int h) {
        const u16* src = p.qkvs + (((long long)b * 3 + typ) * p.H + h) * (long long)N * 128;
#pragma unroll
        for (int j = 0; j < 2; ++j)
            __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(src + (long long)rowy[j] * 128 + coffy[j]),
                                             (__attribute__((address_space(3))) void*)(tiles + off + (wave * 8 + j * 4) * 128), 16, 0, 0);
    };
    // row stats of head h: NTYPE x 128 float2 = NTYPE KB; every wave moves 2 x 256 B (global_load_lds_dword)
    auto issue_stats = [&](int h) {
        float* dst = reinterpret_cast<float*>(lstats + (h & 1) * NTYPE * 128);
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int piece = wave * 2 + j;                          // 16 pieces of 64 floats (= 32 float2)
            if (SURGERY || piece < 4) {
                const int ty = piece >> 2, q32 = (piece & 3) * 32 + (lane >> 1);
                const float* src = reinterpret_cast<const float*>(p.stats + (((long long)b * p.H + h) * 4 + ty) * N + min(qt * 128 + q32, N - 1)) + (lane & 1);
                __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)src,
                                                 (__attribute__((address_space(3))) void*)(dst + piece * 64), 4, 0, 0);
            } else {   // keep the per-wave instruction count uniform (counted vmcnt): harmless reload of piece 0
                const float* src = reinterpret_cast<const float*>(p.stats + (((long long)b * p.H + h) * 4) * N + min(qt * 128 + (lane >> 1), N - 1)) + (lane & 1);
                __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)src,
                                                 (__attribute__((address_space(3))) void*)(reinterpret_cast<float*>(lstats) + 2 * NTYPE * 256), 4, 0, 0);
            }
        }
    };

    f32x16 accW, accA;
#pragma unroll
    for (int e = 0; e < 16; ++e) { accW[e] = 0.f; accA[e] = 0.f; }
    const float c2 = p.scale * 1.4426950408889634f;               // row stats are in log2 units (rowpass_body_bf)
    const bool last_kt = kt * 64 + wk * 32 + 32 > N;              // wave-uniform: only the last key tile holds keys >= N

    // wave-uniform: this wave's 32 x 32 tile lies entirely in the padding (N = 785 leaves 3 of the 4 query sub-tiles of the last
    // query tile and half of the last key tile empty): nothing to score, the wave only keeps the staging and barriers going
    const bool tile_oob = (qt * 128 + wq * 32 >= N) || (kt * 64 + wk * 32 >= N);
    auto score = [&](int offY, int offX, int type, int h, f32x16& acc) {
        if ((EXCEL_DBG(p.dbg) & 1) || tile_oob) return;
        const float2 ml = lstats[((h & 1) * NTYPE + type) * 128 + wq * 32 + r];
        const u16* y16 = tiles + offY + (wk * 32 + r) * 128;
        const u16* x16 = tiles + offX + (wq * 32 + r) * 128;
        f32x16 s;
#pragma unroll
        for (int e = 0; e < 16; ++e) s[e] = 0.f;
#pragma unroll
        for (int s4 = 0; s4 < 4; ++s4) {
            const int ch = ((s4 * 2 + kh) ^ (r & 15)) * 8, cl = ((8 + s4 * 2 + kh) ^ (r & 15)) * 8;
            const splitx8 yh = *reinterpret_cast<const splitx8*>(y16 + ch), yl = *reinterpret_cast<const splitx8*>(y16 + cl);
            const splitx8 xh = *reinterpret_cast<const splitx8*>(x16 + ch), xl = *reinterpret_cast<const splitx8*>(x16 + cl);
            s = EXCEL_MFMA16(yl, xh, s, 0, 0, 0);
            s = EXCEL_MFMA16(yh, xl, s, 0, 0, 0);
            s = EXCEL_MFMA16(yh, xh, s, 0, 0, 0);
        }
        if (last_kt) {
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                const int key = kt * 64 + wk * 32 + c32_row(e, lane);
                const float pr = __builtin_amdgcn_exp2f(fmaf(s[e], c2, -ml.x));
                acc[e] += (key < N) ? pr * ml.y : 0.f;
            }
        } else {
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[e] = fmaf(__builtin_amdgcn_exp2f(fmaf(s[e], c2, -ml.x)), ml.y, acc[e]);
        }
    };

    if (SURGERY) {
        constexpr int XQ = 0, XK = XT, XV = 2 * XT, YQ = 3 * XT, YK = 3 * XT + YT, YV = 3 * XT + 2 * YT;
        issue_y(YQ, 0, 0);
        issue_stats(0);
        issue_x(XQ, 0, 0);
        issue_x(XK, 1, 0);
        issue_y(YK, 1, 0);
        for (int h = 0; h < p.H; ++h) {
            const bool more = h + 1 < p.H && !(EXCEL_DBG(p.dbg) & 2);
            asm volatile("s_waitcnt vmcnt(6)" ::: "memory");          // YQ,stats,XQ(h) landed (XK,YK(h) may be in flight)
            __builtin_amdgcn_s_barrier();
            if (!(EXCEL_DBG(p.dbg) & 2) || h == 0) { issue_x(XV, 2, h); issue_y(YV, 2, h); }
            score(YQ, XQ, 1, h, accA);                                // q.q
            if (!(EXCEL_DBG(p.dbg) & 2) || h == 0) asm volatile("s_waitcnt vmcnt(6)" ::: "memory");   // XK,YK(h) landed (XV,YV in flight)
            __builtin_amdgcn_s_barrier();
            if (more) { issue_y(YQ, 0, h + 1); issue_stats(h + 1); }
            score(YK, XQ, 0, h, accW);                                // q.k
            __builtin_amdgcn_s_barrier();                             // everyone is done with XQ(h)
            if (more) issue_x(XQ, 0, h + 1);
            score(YK, XK, 2, h, accA);                                // k.k
            if (more) asm volatile("s_waitcnt vmcnt(8)" ::: "memory");   // XV,YV(h) landed (YQ,stats,XQ(h+1) in flight)
            else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            __builtin_amdgcn_s_barrier();
            if (more) { issue_x(XK, 1, h + 1); issue_y(YK, 1, h + 1); }
            score(YV, XV, 3, h, accA);                                // v.v
        }
    } else {
        // head-mean weights of an nn.MultiheadAttention block: only q.k; (XQ, YK, stats) double buffered
        issue_x(0, 0, 0);
        issue_y(XT, 1, 0);
        issue_stats(0);
        for (int h = 0; h < p.H; ++h) {
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            __builtin_amdgcn_s_barrier();
            const int cur = (h & 1) * (XT + YT), nxt = (XT + YT) - cur;
            if (h + 1 < p.H) { issue_x(nxt, 0, h + 1); issue_y(nxt + XT, 1, h + 1); issue_stats(h + 1); }
            score(cur + XT, cur, 0, h, accW);
        }
    }
    __syncthreads();
    if (EXCEL_DBG(p.dbg) & 4) { if (accA[0] + accW[0] == 12345.f) p.a_sum[0] = 1.f; return; }

    // transpose each wave's [key][q] tile through LDS (pitch 33) and store rows of q with consecutive keys
    float* tb = reinterpret_cast<float*>(tiles) + wave * (32 * 33);
    const int qbase = qt * 128 + wq * 32, kbase = kt * 64 + wk * 32;
    auto emit = [&](const f32x16& acc, int which) {
#pragma unroll
        for (int e = 0; e < 16; ++e) tb[r * 33 + c32_row(e, lane)] = acc[e];
        __builtin_amdgcn_s_waitcnt(0xc07f);
        // unrolled: the 16 read-modify-write round trips on w_aff must be in flight together, not one after the other
        float oldw[16];
        if (which == 1 && p.w_aff && !p.aff_init) {
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                const int qg = qbase + 2 * i + kh, kg = kbase + r;
                const long long P = N - 1;
                oldw[i] = (qg < N && qg >= 1 && kg >= 1 && kg < N) ? p.w_aff[((long long)b * P + (qg - 1)) * P + (kg - 1)] : 0.f;
            }
        } else {
#pragma unroll
            for (int i = 0; i < 16; ++i) oldw[i] = 0.f;
        }
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const int qq = 2 * i + kh;
            const int qg = qbase + qq, kg = kbase + r;
            const float v = tb[qq * 33 + r];
            if (qg >= N) continue;
            if (which == 0) {
                if (kg < p.NP) {
                    float av = v * (1.f / 3.f);
                    // LVC branch (clip_surgery_model.py:140-141): every head's attn[1:,1:] += ex_attn -> head-sum gains H x ex_attn
                    if (p.ex_attn && qg >= 1 && kg >= 1 && kg < N) av += p.ex_scale * p.ex_attn[((long long)b * (N - 1) + (qg - 1)) * (N - 1) + (kg - 1)];
                    split_t* o = reinterpret_cast<split_t*>(p.a_sum) + ((long long)b * N + qg) * 2 * p.NP + split_off(kg, 0);
                    const split_t hi = split_hi(av);
                    o[0] = hi;
                    o[32] = split_hi(av - (float)hi);
                }
            } else {
                const float pw = v * p.w_scale;
                if (p.attn_out && kg < N) p.attn_out[((long long)b * N + qg) * N + kg] = pw;
                if (p.w_aff && qg >= 1 && kg >= 1 && kg < N) {
                    const long long P = N - 1;
                    p.w_aff[((long long)b * P + (qg - 1)) * P + (kg - 1)] = oldw[i] + pw * p.aff_scale;
                }
            }
        }
        __builtin_amdgcn_s_waitcnt(0xc07f);
    };
    if (SURGERY) emit(accA, 0);
    emit(accW, 1);
}

int excel_launch_attn_rowpass(const unsigned short* qkvs, float* out, float* stats, int B, int H, int N, int hd, float scale,
                              const AttnPlan& pl, hipStream_t st, int flash_nq) {
    ProfScope prof__(PROF_ATTN_ROWPASS, st);
    EXCEL_CHECK_ARG(hd == HD, "attention: head_dim must be 64 (got %d)", hd);
    EXCEL_CHECK_ARG(pl.rp_ntypes == 1 || pl.rp_ntypes == 4, "attention: ntypes must be 1 or 4");
    EXCEL_CHECK_ARG(pl.path != ATTN_TWOPASS_F32 && qkvs, "attention: the plan is of another mode");
    RowpassArgs a{out, reinterpret_cast<float2*>(stats), B, H, N, scale, qkvs, flash_nq, 1, 1 << 20};
#ifdef EXCEL_DEV
    { static const int x = getenv("EXCEL_ROWPASS_XCD") ? atoi(getenv("EXCEL_ROWPASS_XCD")) : 1; a.xcd_local = x; }
    { static const int g = getenv("EXCEL_ROWPASS_GRP") ? atoi(getenv("EXCEL_ROWPASS_GRP")) : 0; if (g > 0) a.tail_grp = g; }
#endif
    hipLaunchKernelGGL(attn_rowpass_kernel, dim3(pl.rp_grid[0], pl.rp_grid[1], pl.rp_grid[2]), dim3(256), 0, st, a);
    EXCEL_CHECK_LAUNCH("attn_rowpass");
    return EXCEL_OK;
}

int excel_launch_attn_accum(const unsigned short* qkvs, const float* stats, float* a_sum, float* w_aff, float* attn_out, int B, int H,
                            int N, int NP, int hd, float scale, int surgery, float w_scale, float aff_scale, int aff_init,
                            const AttnPlan& pl, hipStream_t st, const float* ex_attn) {
    ProfScope prof__(PROF_ATTN_ACCUM, st);
    EXCEL_CHECK_ARG(hd == HD, "attention: head_dim must be 64 (got %d)", hd);
    EXCEL_CHECK_ARG(pl.path == ATTN_TWOPASS_SPLIT && pl.block > 0 && qkvs, "attn_accum: the plan names another path");
    EXCEL_CHECK_ARG(!surgery || (a_sum && NP >= N && NP <= cdiv(N, 64) * 64), "attn_accum: bad a_sum/NP");
    AccumArgs a{reinterpret_cast<const float2*>(stats), a_sum, w_aff, attn_out, B, H, N, NP, scale, w_scale, aff_scale, aff_init, qkvs, 0, surgery ? ex_attn : nullptr, (float)H};
    const dim3 grid(pl.grid[0], pl.grid[1], pl.grid[2]), block(pl.block);       // 128 x 64 tiles, 512 threads
#ifdef EXCEL_DEV
    { static const char* d = getenv("EXCEL_ACCUM_DBG"); if (d) a.dbg = atoi(d); }
#endif
    if (surgery) hipLaunchKernelGGL((attn_accum_bf_kernel<true>), grid, block, 0, st, a);
    else hipLaunchKernelGGL((attn_accum_bf_kernel<false>), grid, block, 0, st, a);
    EXCEL_CHECK_LAUNCH("attn_accum");
    return EXCEL_OK;
}

}  // namespace EXCEL_SPLIT_NS
