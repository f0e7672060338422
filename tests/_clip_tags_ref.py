"""The definition of excel_clip_tags (include/excel_hip.h, "image tags") restated in numpy, and the case table of its tests.

clip_tags_ref evaluates the definition in the dtype it is given: float64 is the reference the kernel is compared with, float32 is the
yardstick of the score tolerance (the kernel is allowed 16 times the float32 evaluation's own error against float64, and never more
than score_bound)."""
import numpy as np

# (B, C, T, F, scale, thre, kmax)
CASES = {
    "voc": (3, 512, 45, 20, 100.0, 0.2, 6),
    "widest": (2, 512, 512, 254, 100.0, 0.2, 18),
    "smallest": (2, 32, 1, 1, 100.0, 0.2, 1),
    "no_bkg_cut": (3, 64, 5, 5, 100.0, 0.0, 3),
    "top1": (3, 768, 103, 80, 100.0, 1.0, 4),
    "flat": (2, 512, 45, 20, 10.0, 0.5, 2),
}
MIN_MARGIN = 1e-3
SEED = 7


def make_case(name):
    """-> (x [B,C] f32, text [T,C] f32, F, scale, thre, kmax): RandomState(SEED), x = 3 randn(B,C), then text = randn(T,C)"""
    B, C, T, F, scale, thre, kmax = CASES[name]
    rs = np.random.RandomState(SEED)
    x = (3.0 * rs.standard_normal((B, C))).astype(np.float32)
    text = rs.standard_normal((T, C)).astype(np.float32)
    return x, text, F, scale, thre, kmax


def clip_tags_ref(x, text, F, scale, thre, kmax, dtype=np.float64):
    """x [B,C], text [T,C] -> (onehot [B,F] float32, scores [B,F] dtype).  A row whose logits are not all finite: class 0, NaN scores."""
    x, text = np.asarray(x, dtype), np.asarray(text, dtype)
    B = x.shape[0]
    onehot = np.zeros((B, F), np.float32)
    scores = np.zeros((B, F), dtype)
    scale, thre = dtype(scale), dtype(thre)
    with np.errstate(all="ignore"):
        tn = np.sqrt((text * text).sum(1))
        for b in range(B):
            cos = (text @ x[b]) / (np.sqrt((x[b] * x[b]).sum()) * tn)
            logit = scale * cos
            if not np.isfinite(logit).all():
                onehot[b, 0] = 1.0
                scores[b] = np.nan
                continue
            e = np.exp(logit - logit.max())
            p = e / e.sum()
            s = p[:F]
            scores[b] = s
            pmax = s.max()
            for f in range(F):
                rank = int((s > s[f]).sum() + (s[:f] == s[f]).sum())
                onehot[b, f] = 1.0 if rank < kmax and (rank == 0 or s[f] >= thre * pmax) else 0.0
    return onehot, scores


def margin(scores, thre, kmax):
    """The smallest relative distance of a decision of the definition to its boundary over the rows of `scores` [B,F] (float64): of any
    score to thre * pmax, and of the two scores either side of the kmax cut - exact ties excepted (the index decides those, and a score
    that equals thre * pmax exactly, as pmax itself does at thre = 1, is decided by equality).  At thre = 0 the threshold decides
    nothing (every score, also one that underflows to 0, passes `>= 0`), so only the cut counts there.  Rows of NaNs are skipped."""
    m = np.inf
    for s in np.asarray(scores, np.float64):
        if not np.isfinite(s).all():
            continue
        pmax = s.max()
        d = np.abs(s - thre * pmax) / pmax
        d = d[d != 0]
        if d.size and thre > 0:
            m = min(m, float(d.min()))
        if kmax < s.size:
            o = np.sort(s)[::-1]
            if o[kmax - 1] != o[kmax]:
                m = min(m, float((o[kmax - 1] - o[kmax]) / o[kmax - 1]))
    return m


def score_error(scores, ref):
    """max |scores - ref| over the finite rows of `ref`, relative to each row's top score; NaN rows must be NaN in both"""
    scores, ref = np.asarray(scores, np.float64), np.asarray(ref, np.float64)
    err = 0.0
    for a, r in zip(scores, ref):
        if not np.isfinite(r).all():
            assert np.isnan(a).all() and np.isnan(r).all()
            continue
        err = max(err, float(np.abs(a - r).max() / r.max()))
    return err


def score_bound(scale, C):
    """The derived worst case of a float32 evaluation, relative to the top score: a cosine of C products summed in float32 is off by at
    most about C * 2^-24 (each of the three sums), scale turns that into a logit error, and a softmax probability moves by at most twice
    the largest logit error in relative terms: 6 * scale * C * 2^-24."""
    return 6.0 * scale * C * 2.0 ** -24
