"""The numpy statement of "reverberant speech: exact RIR convolution" (include/gtcrn_micro_hip.h): Philox block k = 2 for the
reverb plan, beside what tests/batch_checker.py states for k = 0 and 1, and the convolution as np.convolve on int64 over
the zero-extended clip, then the stated shift and clamp.  Written from the contract, not from the kernels: nothing here is
split into digits, tiled or shared with csrc/reverb.*."""
import numpy as np

import batch_checker as BC

REVERB_PLAN_DTYPE = np.dtype([("rir", "<i4"), ("reserved", "<i4")])
REVERB_RECORD_DTYPE = np.dtype([("rir", "<i4"), ("ntaps", "<i4"), ("saturated", "<i4"), ("reserved", "<i4")])
MAX_TAPS = 16384
TAP_MAX = 32639


def reverb_plan(n_rir, p_reverb, B, seed, step, item0=0):
    key = (seed & BC.M32, (seed >> 32) & BC.M32)
    out = np.zeros(B, REVERB_PLAN_DTYPE)
    for b in range(B):
        t = BC.philox4x32_10(((item0 + b) & BC.M32, step & BC.M32, (step >> 32) & BC.M32, 2), key)
        out[b] = (BC.mulhi(t[1], n_rir) if BC.unit(t[0]) < np.float32(p_reverb) else -1, 0)
    return out


def make_reverb_plan(rirs):
    out = np.zeros(len(rirs), REVERB_PLAN_DTYPE)
    out["rir"] = rirs
    return out


def clamp_plans(plan_, rplan, n_speech, n_rir):
    """The plans as the device uses them: sclip and rir clamped into their tables, a negative sstart as 0."""
    p, r = plan_.copy(), rplan.copy()
    p["sclip"] = np.clip(p["sclip"], 0, n_speech - 1)
    p["sstart"] = np.maximum(p["sstart"], 0)
    r["rir"] = np.where(r["rir"] < 0, -1, np.minimum(r["rir"], n_rir - 1))
    return p, r


def wet_row(clip, s0, L, h):
    """clip: the whole int16 clip; h: the int16 taps, or None for a dry row.  -> (int16 row of L samples, clamped count)."""
    x = clip.astype(np.int64)
    if h is None:
        w = np.zeros(L, np.int64)
        got = x[s0:s0 + L]
        w[:len(got)] = got
        return w.astype(np.int16), 0
    K = len(h)
    # x[j] for j = s0 - (K - 1) .. s0 + L - 1, zero outside the clip
    lo, hi = s0 - (K - 1), s0 + L
    ext = np.zeros(hi - lo, np.int64)
    a, e = max(lo, 0), min(hi, len(x))
    if e > a:
        ext[a - lo:e - lo] = x[a:e]
    acc = np.convolve(ext, h.astype(np.int64), mode="valid")             # acc[i] = sum_k h[k] ext[K - 1 + i - k]
    assert acc.dtype == np.int64 and len(acc) == L
    v = (acc + 16384) >> 15
    sat = int(((v < -32768) | (v > 32767)).sum())
    return np.clip(v, -32768, 32767).astype(np.int16), sat


def reverb(spcm, soff, taps, roff, plan_, rplan, L, stride):
    """-> (staged (B, stride) int16 with rows' tails zero, offsets int64[B + 1], staged plan, records)."""
    B = len(plan_)
    p, r = clamp_plans(plan_, rplan, len(soff) - 1, len(roff) - 1)
    staged = np.zeros((B, stride), np.int16)
    rec = np.zeros(B, REVERB_RECORD_DTYPE)
    for b in range(B):
        clip = spcm[int(soff[p["sclip"][b]]):int(soff[p["sclip"][b] + 1])]
        rir = int(r["rir"][b])
        h = None if rir < 0 else taps[int(roff[rir]):int(roff[rir + 1])]
        staged[b, :L], sat = wet_row(clip, int(p["sstart"][b]), L, h)
        rec[b] = (rir, 0 if h is None else len(h), sat, 0)
    splan = plan_.copy()
    splan["sclip"] = np.arange(B)
    splan["sstart"] = 0
    return staged, np.arange(B + 1, dtype=np.int64) * stride, splan, rec
