"""The ViT attention's kernel selection (excel_attn_plan, attn_plan.hip) is host arithmetic: it is pinned here, on the CPU, for every
patch grid from 1x1 to 48x48 and at every boundary of the token count N the launchers dispatch on.  The expected values are the table
tests/_attn_shapes.py writes out by hand from these formulae (cdiv(a, b) = ceil(a / b)), not a recording of the code under test:

    tiles = cdiv(N, 32)
    split modes (bf16x3, f16x3, f16x2), tiles <= 40 (N <= 1280): flash row pass (1 score type) + attn_strip_kernel<ntw>,
        ntw = cdiv(tiles, 8) key tiles per wave, nw = cdiv(tiles, ntw) waves, tiles - nw * (ntw - 1) of them with ntw tiles, the others
        with ntw - 1; block = 64 * nw; grid = B * tiles strips, or - both sweeps wanted (surgery layer and weights) - 16 * split_c with
        split_c = cdiv(B * tiles, 8)
    split modes, tiles > 40: row pass (4 score types on a surgery layer, else 1) + attn_accum_bf_kernel, grid (cdiv(N, 64), cdiv(N, 128), B)
        of 512 threads
    f32, any N: row pass (4 / 1 score types) + attn_accum_kernel, grid (cdiv(N, 64), cdiv(N, 64), B) of 256 threads
    row pass: grid (cdiv(N, 128), B * H, score types); no second kernel when the layer is neither a surgery layer nor asked for weights

The second half checks the GPU sweep's own comparison functions (tests/_attn_shapes.py) on the oracle alone: they accept the fp32
oracle and reject an attention matrix with one key dropped from one row, and one with a wrongly admitted key in every row."""
import numpy as np
import pytest

import _attn_shapes as A
from excel_amd import ops

SPLIT_MODES = ("bf16x3", "f16x3", "f16x2")


def cdiv(a, b):
    return -(-a // b)


def test_dispatch_table_is_consistent():
    """The hand-written table against its own defining properties (no library involved)."""
    for g, (N, tiles, ntw, nw, full, last) in A.DISPATCH.items():
        assert N == g * g + 1 and 32 * (tiles - 1) < N <= 32 * tiles and last == N - 32 * (tiles - 1)
        if tiles <= 40:
            assert 8 * (ntw - 1) < tiles <= 8 * ntw and ntw * (nw - 1) < tiles <= ntw * nw and nw <= 8
            assert full * ntw + (nw - full) * (ntw - 1) == tiles and 1 <= full <= nw
        else:
            assert (ntw, nw, full) == (0, 0, 0)


@pytest.mark.parametrize("mode", SPLIT_MODES)
def test_attn_plan_every_grid_side_split_modes(mode):
    B, H = 3, 2
    for g, (N, tiles, ntw, nw, full, _) in A.DISPATCH.items():
        for surgery in (False, True):
            for want_w in (False, True):
                p = ops.attn_plan(B, H, N, mode=mode, surgery=surgery, want_w=want_w)
                strip = tiles <= 40
                second = surgery or want_w
                want = dict(path="strip" if strip else "twopass_split", ntiles=tiles, ntw=ntw, waves=nw, waves_full=full,
                            rowpass_ntypes=4 if (surgery and not strip) else 1, split_c=0)
                want["rowpass_grid"] = (cdiv(N, 128), B * H, want["rowpass_ntypes"])
                if not second:
                    want.update(grid=(0, 0, 0), block=0)
                elif strip:
                    if surgery and want_w:
                        want["split_c"] = cdiv(B * tiles, 8)
                        want.update(grid=(16 * want["split_c"], 1, 1))
                    else:
                        want.update(grid=(B * tiles, 1, 1))
                    want["block"] = 64 * nw
                else:
                    want.update(grid=(cdiv(N, 64), cdiv(N, 128), B), block=512)
                assert p == want, (g, surgery, want_w)


def test_attn_plan_every_grid_side_f32():
    B, H = 2, 12
    for g, (N, tiles, _, _, _, _) in A.DISPATCH.items():
        for surgery in (False, True):
            for want_w in (False, True):
                p = ops.attn_plan(B, H, N, mode="f32", surgery=surgery, want_w=want_w)
                nt = 4 if surgery else 1
                second = surgery or want_w
                assert p == dict(path="twopass_f32", ntiles=tiles, ntw=0, waves=0, waves_full=0, rowpass_ntypes=nt,
                                 rowpass_grid=(cdiv(N, 128), B * H, nt), grid=(cdiv(N, 64), cdiv(N, 64), B) if second else (0, 0, 0),
                                 block=256 if second else 0, split_c=0), (g, surgery, want_w)


# N: (instance, waves, waves with `instance` tiles) - by hand: 256 = 8 tiles -> 8 waves x 1; 257 = 9 tiles -> 2 per wave, 5 waves (2,2,2,2,1);
# 512 = 16 -> 8 x 2; 513 = 17 -> 3 per wave, 6 waves (3,3,3,3,3,2); 768 = 24 -> 8 x 3; 769 = 25 -> 4 per wave, 7 waves (4,4,4,4,3,3,3);
# 1024 = 32 -> 8 x 4; 1025 = 33 -> 5 per wave, 7 waves (5,5,5,5,5,4,4); 1280 = 40 -> 8 x 5; 1281 = 41 tiles -> two-pass
BOUNDARIES = {256: (1, 8, 8), 257: (2, 5, 4), 512: (2, 8, 8), 513: (3, 6, 5), 768: (3, 8, 8), 769: (4, 7, 4), 1024: (4, 8, 8),
              1025: (5, 7, 5), 1280: (5, 8, 8), 1281: (0, 0, 0)}


@pytest.mark.parametrize("mode", SPLIT_MODES)
def test_attn_plan_boundaries(mode):
    for N, (ntw, nw, full) in BOUNDARIES.items():
        p = ops.attn_plan(1, 12, N, mode=mode)
        assert (p["ntw"], p["waves"], p["waves_full"]) == (ntw, nw, full), N
        assert p["path"] == ("strip" if ntw else "twopass_split") and p["rowpass_ntypes"] == (1 if ntw else 4), N
        assert p["ntiles"] == cdiv(N, 32)
        if ntw:
            assert p["block"] == 64 * nw and p["split_c"] == cdiv(p["ntiles"], 8) and p["grid"] == (16 * p["split_c"], 1, 1)


def test_attn_plan_strip_precondition_holds_in_the_whole_envelope():
    """excel_launch_attn_strip refuses a launch unless every wave owns ntw or ntw - 1 tiles (tiles // waves >= ntw - 1) and the kernel is
    instantiated for 1..5 tiles per wave on at most 8 waves: true for every N the plan sends there."""
    for N in range(1, 1281):
        p = ops.attn_plan(1, 1, N)
        t = p["ntiles"]
        assert p["path"] == "strip" and 1 <= p["ntw"] <= 5 and 1 <= p["waves"] <= 8
        assert t // p["waves"] >= p["ntw"] - 1 and p["ntw"] * p["waves"] >= t
        assert p["waves_full"] * p["ntw"] + (p["waves"] - p["waves_full"]) * (p["ntw"] - 1) == t and p["waves_full"] >= 1
    assert ops.attn_plan(1, 1, 1281)["path"] == "twopass_split"


def test_attn_plan_rejects_bad_arguments():
    for bad in ((0, 2, 65), (1, 0, 65), (1, 2, 0), (1, 2, -5), (1, 2, (1 << 20) + 1), (70000, 1, 65)):
        with pytest.raises(RuntimeError, match="attn_plan"):
            ops.attn_plan(*bad)
    from excel_amd._lib import lib
    import ctypes as C
    plan = (C.c_int32 * 14)()
    assert lib().excel_attn_plan(1, 2, 65, 4, 1, 1, plan) != 0          # no such gemm_mode
    assert lib().excel_attn_plan(1, 2, 65, -1, 1, 1, plan) != 0
    assert lib().excel_attn_plan(1, 2, 65, 1, 2, 1, plan) != 0          # flags are 0 / 1
    assert lib().excel_attn_plan(1, 2, 65, 1, 1, -1, plan) != 0
    assert lib().excel_attn_plan(1, 2, 65, 1, 1, 1, None) != 0
    assert lib().excel_attn_plan(1, 2, 65, 1, 1, 1, plan) == 0


# ---------------------------------------------------------------------------------------------------- the sweep's gates, on the oracle alone
@pytest.mark.parametrize("g", [16, 42])
def test_masking_gate_rejects_one_wrong_key(g):
    """Flat net (attn_gain 0.25): the regime is there (every key holds >= 0.3 of a uniform share, fp32 noise far below the gate); the fp32
    oracle passes the masking and the numerics gate; one key dropped from one row (row renormalised), and one wrongly admitted unit-score
    key in every row (what a padded, all-zero key row contributes: exp(0 - max) / sum), are both rejected."""
    N = g * g + 1
    ref, o, pmin = A.reference("flat", g, 1)
    assert not A.masking_precondition(o, pmin, N), A.masking_precondition(o, pmin, N)
    w = A.net_weights("flat", g)
    x32, attn32, feats32 = A.oracle.vit.vit_forward(A.images(g, 1), w, A.TINY)
    clean = dict(attn=attn32, feats=feats32, x_raw=x32, image_features=A.token_normalize(x32), w_aff=attn32[-6:, :, 1:, 1:].mean(0))
    err = A.errors(clean, ref)
    assert not A.masking_failures(err, pmin) and not A.numerics_failures(err, o, "f32")
    for l in (0, A.TINY.layers - 1):                                  # a plain layer and a surgery layer
        # the last valid key (the one a wrong tile mask would lose) dropped from one row of the last query block, the row renormalised
        dropped = dict(clean, attn=attn32.copy())
        row = dropped["attn"][l, 0, N - 2]
        s = row.sum(dtype=np.float64)
        row[N - 1] = 0.0
        row *= np.float32(s / row.sum(dtype=np.float64))
        bad = A.masking_failures(A.errors(dropped, ref), pmin)
        assert any(m.startswith(f"attn{l}:") for m in bad), (l, bad)
        assert not any(m.startswith("rowsum") for m in bad)           # (renormalised: only the per-element gate can see it)
        # one extra key of score 0 admitted into every row's softmax: its mass leaves the valid keys.  The flat net's scores are small, so
        # such a key weighs about as much as a real one: rows scale by (1 - 1 / (N + 1))
        admitted = dict(clean, attn=attn32.copy())
        admitted["attn"][l] *= np.float32(1.0 - 1.0 / (N + 1))
        bad = A.masking_failures(A.errors(admitted, ref), pmin)
        assert any(m.startswith(f"rowsum{l}:") for m in bad), (l, bad)
