// Kernel selection of the ViT attention: which kernels one layer's attention runs on for a token count N, with their grids (the row pass
// of attn.hip, then the strip-resident kernel of attn_strip.hip or the accumulate kernels of attn.hip).  Pure host arithmetic on integers -
// no pointers, no device calls, no state - so one function serves the launchers, the ViT forward (vit_forward_body.inc) and the host
// query of the C ABI (excel_attn_plan), and can be tested without a GPU.
#include "common.h"
#include "excel_internal.h"

AttnPlan attn_plan(int B, int H, int N, int gemm_mode, int surgery, int want_w) {
    AttnPlan pl = {};
    pl.ntiles = cdiv(N, 32);
    // split modes: the strip-resident kernel up to 8 waves x 5 key tiles; beyond that, and in exact fp32, the two-pass kernels
    pl.path = gemm_mode == 0 ? ATTN_TWOPASS_F32 : (pl.ntiles <= ATTN_STRIP_MAX_TILES ? ATTN_STRIP : ATTN_TWOPASS_SPLIT);
    // the strip kernel owns the statistics of q.q / k.k / v.v: its row pass only runs the flash part (q.k)
    pl.rp_ntypes = (surgery && pl.path != ATTN_STRIP) ? 4 : 1;
    pl.rp_grid[0] = cdiv(N, 128); pl.rp_grid[1] = B * H; pl.rp_grid[2] = pl.rp_ntypes;
    if (pl.path == ATTN_STRIP) {
        pl.ntw = cdiv(pl.ntiles, 8);
        pl.nw = cdiv(pl.ntiles, pl.ntw);                          // 25 tiles: 7 waves x (4,4,4,4,3,3,3)
        const int tb = pl.ntiles / pl.nw;                         // (the kernel's own split: the first ntiles - tb * nw waves own tb + 1)
        pl.nw_full = tb == pl.ntw ? pl.nw : pl.ntiles - tb * pl.nw;
    }
    if (!surgery && !want_w) return pl;
    if (pl.path == ATTN_STRIP) {
        // Both sweeps wanted: one workgroup per (strip, sweep).  A strip workgroup fills a CU (148 KB LDS), so B x nstrips = 800 uniform
        // workgroups on 256 CUs are 3.125 rounds = 4 rounds of 4H phases; split, the 3H-phase workgroups go first and the H-phase ones
        // level the tail: 150-156 phase-times per CU instead of 192.
        const int nstrips = pl.ntiles;
        if (surgery && want_w) pl.split_c = cdiv(B * nstrips, 8);
        pl.grid[0] = pl.split_c ? 8 * 2 * pl.split_c : B * nstrips; pl.grid[1] = 1; pl.grid[2] = 1;
        pl.block = pl.nw * 64;
    } else {
        pl.grid[0] = cdiv(N, 64); pl.grid[1] = cdiv(N, pl.path == ATTN_TWOPASS_SPLIT ? 128 : 64); pl.grid[2] = B;
        pl.block = pl.path == ATTN_TWOPASS_SPLIT ? 512 : 256;
    }
    return pl;
}
