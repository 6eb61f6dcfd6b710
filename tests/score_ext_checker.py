"""Float64 statement of the "scores, extended" section of include/gtcrn_micro_hip.h, written from the header and
independent of the kernels: ESTOI (Jensen & Taal 2016, the structure pystoi's stoi(..., extended=True) follows) on the
envelopes of score_checker.stoi_stages, and segmental SNR as the header states it, frame by frame.

Not a test module: tests/test_score_ext_checker.py pins it (a second formulation of each metric, ESTOI's properties,
seeded wrong definitions), tests/test_gpu_score_ext.py holds the kernels to it.
"""
import numpy as np

import score_checker as SC

EPS = SC.EPS
SEG, NBANDS = SC.SEG, SC.NBANDS
SNR_FRAME, SNR_HOP = 480, 120
SNR_LO, SNR_HI = -10.0, 35.0

_refs = {}


# ---- ESTOI ------------------------------------------------------------------------------------------------------------
def _row_col_normalise(a, columns=True):
    """Rows lose their mean and are divided by (their norm + EPS), then the columns of the result the same way."""
    a = a - a.mean(axis=1, keepdims=True)
    a = a / (np.linalg.norm(a, axis=1, keepdims=True) + EPS)
    if columns:
        a = a - a.mean(axis=0, keepdims=True)
        a = a / (np.linalg.norm(a, axis=0, keepdims=True) + EPS)
    return a


def estoi_from_envelopes(X, Y):
    """(estoi, segments) of two (15, M) envelope sets: one segment after the other, as the header words it."""
    X = np.asarray(X, np.float64)
    Y = np.asarray(Y, np.float64)
    M = X.shape[1]
    if M < SEG:
        return 1e-5, 0
    S = M - SEG + 1
    d = np.empty(S)
    for s in range(S):
        xn = _row_col_normalise(X[:, s:s + SEG])
        yn = _row_col_normalise(Y[:, s:s + SEG])
        d[s] = np.sum(xn * yn) / SEG
    return float(d.mean()), S


def estoi_from_envelopes_vectorised(X, Y):
    """The same number from all segments at once: a (S, 15, 30) stack, the sums written with einsum."""
    X = np.asarray(X, np.float64)
    Y = np.asarray(Y, np.float64)
    M = X.shape[1]
    if M < SEG:
        return 1e-5, 0
    S = M - SEG + 1
    idx = np.arange(S)[:, None] + np.arange(SEG)[None, :]

    def norm(E):
        a = E[:, idx].transpose(1, 0, 2)                                     # (S, 15, 30)
        a = a - np.einsum("sjt->sj", a)[:, :, None] / SEG
        a = a / (np.sqrt(np.einsum("sjt,sjt->sj", a, a))[:, :, None] + EPS)
        a = a - np.einsum("sjt->st", a)[:, None, :] / NBANDS
        return a / (np.sqrt(np.einsum("sjt,sjt->st", a, a))[:, None, :] + EPS)

    return float(np.einsum("sjt,sjt->", norm(X), norm(Y)) / (SEG * S)), S


def estoi(ref, inf):
    st = SC.stoi_stages(np.asarray(ref, np.float32), np.asarray(inf, np.float32))
    return estoi_from_envelopes(st["env_ref"], st["env_inf"])[0]


# ---- segmental SNR ------------------------------------------------------------------------------------------------------
def segsnr_frames(n):
    n = int(n)
    return (n - SNR_FRAME) // SNR_HOP + 1 if n >= SNR_FRAME else 0


def segsnr_window():
    return 0.5 * (1.0 - np.cos(2.0 * np.pi * np.arange(1, SNR_FRAME + 1) / (SNR_FRAME + 1)))


def segsnr(ref, inf):
    """(segsnr, F): a loop over the frames that fit, in ascending order."""
    r = np.asarray(ref, np.float32).astype(np.float64)
    y = np.asarray(inf, np.float32).astype(np.float64)
    w = segsnr_window()
    F = segsnr_frames(r.size)
    if F == 0:
        return float("nan"), 0
    total = 0.0
    for f in range(F):
        s = f * SNR_HOP
        rr, dd = w * r[s:s + SNR_FRAME], w * (r[s:s + SNR_FRAME] - y[s:s + SNR_FRAME])
        v = 10.0 * np.log10(np.sum(rr ** 2) / (np.sum(dd ** 2) + EPS) + EPS)
        total += min(max(v, SNR_LO), SNR_HI)
    return total / F, F


def segsnr_vectorised(ref, inf):
    """The same number from a strided view of all frames."""
    r = np.asarray(ref, np.float32).astype(np.float64)
    y = np.asarray(inf, np.float32).astype(np.float64)
    F = segsnr_frames(r.size)
    if F == 0:
        return float("nan"), 0
    idx = SNR_HOP * np.arange(F)[:, None] + np.arange(SNR_FRAME)[None, :]
    w2 = segsnr_window() ** 2
    num, den = (r[idx] ** 2) @ w2, ((r - y)[idx] ** 2) @ w2
    return float(np.clip(10.0 * np.log10(num / (den + EPS) + EPS), SNR_LO, SNR_HI).mean()), F


# ---- the record ---------------------------------------------------------------------------------------------------------
def score_ext(ref, inf):
    """What gtcrn_score_ext adds to score_checker.score's record for one pair (float32 samples in)."""
    ref = np.asarray(ref, np.float32)
    inf = np.asarray(inf, np.float32)
    base = SC.score(ref, inf)
    e, S = estoi_from_envelopes(base["stages"]["env_ref"], base["stages"]["env_inf"])
    assert S == base["segments"]
    v, F = segsnr(ref, inf)
    return dict(base, estoi=e, segsnr=v, segsnr_frames=F)


def case_reference(spec):
    """score_ext() of one clip of SC.GPU_CASES on top of SC.case_reference, computed once and shared."""
    if spec not in _refs:
        base = SC.case_reference(spec)
        ref, inf = SC.case_pair(spec)
        e, _ = estoi_from_envelopes(base["stages"]["env_ref"], base["stages"]["env_inf"])
        v, F = segsnr(ref, inf)
        _refs[spec] = dict(base, estoi=e, segsnr=v, segsnr_frames=F)
    return _refs[spec]


# ---- seeded wrong definitions (tests/test_score_ext_checker.py: each moves the score far beyond the GPU ceiling) ----------
def estoi_wrong(X, Y, bug):
    """bug = "no_columns": the column normalisation omitted; "clipped": STOI's alpha and clipping left in front."""
    X = np.asarray(X, np.float64)
    Y = np.asarray(Y, np.float64)
    S = X.shape[1] - SEG + 1
    d = np.empty(S)
    for s in range(S):
        x, y = X[:, s:s + SEG], Y[:, s:s + SEG]
        if bug == "clipped":
            alpha = np.linalg.norm(x, axis=1, keepdims=True) / (np.linalg.norm(y, axis=1, keepdims=True) + EPS)
            y = np.minimum(alpha * y, x * SC.BETA_CLIP)
        cols = bug != "no_columns"
        d[s] = np.sum(_row_col_normalise(x, cols) * _row_col_normalise(y, cols)) / SEG
    return float(d.mean())


def segsnr_wrong(ref, inf, bug):
    """bug = "hop128": frames every 128 samples; "drop_last": the last frame left out."""
    r = np.asarray(ref, np.float32).astype(np.float64)
    y = np.asarray(inf, np.float32).astype(np.float64)
    w = segsnr_window()
    hop = 128 if bug == "hop128" else SNR_HOP
    F = (r.size - SNR_FRAME) // hop + 1 - (1 if bug == "drop_last" else 0)
    v = []
    for f in range(F):
        s = f * hop
        num, den = np.sum((w * r[s:s + SNR_FRAME]) ** 2), np.sum((w * (r[s:s + SNR_FRAME] - y[s:s + SNR_FRAME])) ** 2)
        v.append(min(max(10.0 * np.log10(num / (den + EPS) + EPS), SNR_LO), SNR_HI))
    return float(np.mean(v))
