"""The numpy statement of "dereverberation targets: early or direct clean" (include/gtcrn_micro_hip.h): the split convolution
as two np.convolve calls on int64 -- of h[:E] and of h -- over the zero-extended clip, each with the stated shift and clamp,
and the mix with a target as tests/batch_checker.py's mix_item for noisy and record plus the one stated line for clean.
Written from the contract, not from the kernels: nothing here is split into digits, tiled, cut into segments or shared with
csrc/reverb.* or csrc/batch.*."""
import numpy as np

import batch_checker as BC
import reverb_checker as RC

SPLIT_RECORD_DTYPE = np.dtype([("rir", "<i4"), ("ntaps", "<i4"), ("saturated", "<i4"), ("split", "<i4"),
                               ("target_saturated", "<i4"), ("reserved", "<i4", (3,))])
f32 = np.float32


def clamp_split(split, roff):
    """The splits as the device uses them: clamped into 1 .. K_r."""
    lens = np.asarray(roff[1:], np.int64) - np.asarray(roff[:-1], np.int64)
    return np.clip(np.asarray(split, np.int64), 1, lens).astype(np.int32)


def split_for(responses, target_ms):
    """E_r = min(K_r, d_r + 1 + rint(16 target_ms)), d_r the first tap of the largest magnitude."""
    out = []
    for h in responses:
        a = np.abs(np.asarray(h, np.int64))
        d = next(k for k in range(a.size) if a[k] == a.max())
        out.append(min(a.size, d + 1 + int(np.rint(16.0 * target_ms))))
    return np.array(out, np.int32)


def split(spcm, soff, taps, roff, split_, plan_, rplan, L, stride):
    """-> (wet (B, stride) int16, target (B, stride) int16 -- rows' tails zero --, offsets int64[B + 1], staged plan, records)."""
    B = len(plan_)
    p, r = RC.clamp_plans(plan_, rplan, len(soff) - 1, len(roff) - 1)
    E = clamp_split(split_, roff)
    wet, tgt = np.zeros((B, stride), np.int16), np.zeros((B, stride), np.int16)
    rec = np.zeros(B, SPLIT_RECORD_DTYPE)
    for b in range(B):
        clip = spcm[int(soff[p["sclip"][b]]):int(soff[p["sclip"][b] + 1])]
        rir, s0 = int(r["rir"][b]), int(p["sstart"][b])
        if rir < 0:
            wet[b, :L], _ = RC.wet_row(clip, s0, L, None)
            tgt[b, :L] = wet[b, :L]
            rec[b] = (-1, 0, 0, 0, 0, (0, 0, 0))
            continue
        h = taps[int(roff[rir]):int(roff[rir + 1])]
        e = int(E[rir])
        wet[b, :L], sat = RC.wet_row(clip, s0, L, h)
        tgt[b, :L], tsat = RC.wet_row(clip, s0, L, h[:e])
        rec[b] = (rir, len(h), sat, e, tsat, (0, 0, 0))
    splan = plan_.copy()
    splan["sclip"] = np.arange(B)
    splan["sstart"] = 0
    return wet, tgt, np.arange(B + 1, dtype=np.int64) * stride, splan, rec


def mix_target(spcm, soff, npcm, noff, tpcm, plan_, L):
    """tpcm: the target corpus under soff.  -> (noisy, clean (B, L) float32, records): noisy and the record are the mix
    contract's on the speech side, clean = float32(Gf) * (t * 2^-15)."""
    B = len(plan_)
    noisy, clean, rec = np.zeros((B, L), f32), np.zeros((B, L), f32), np.zeros(B, BC.RECORD_DTYPE)
    for b, p in enumerate(plan_):
        s = BC.window(spcm, soff, int(p["sclip"]), int(p["sstart"]), L)
        t = BC.window(tpcm, soff, int(p["sclip"]), int(p["sstart"]), L)
        a, e = int(noff[p["nclip"]]), int(noff[p["nclip"] + 1])
        n = npcm[a + (int(p["nstart"]) + np.arange(L, dtype=np.int64)) % (e - a)]
        noisy[b], _, r = BC.mix_item(s, n, p["snr_amp"], p["lvl_amp"])
        rec[b] = r
        clean[b] = (f32(r[4]) * (t.astype(f32) * f32(2.0 ** -15))).astype(f32)
    return noisy, clean, rec
