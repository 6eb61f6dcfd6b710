"""The numpy statement of "telephone-channel rows: exact 8 kHz band + G.711" (include/gtcrn_micro_hip.h): the filter table from
tests/resample_checker.design, Philox block k = 3 for the phone plan beside what tests/batch_checker.py states for k = 0 and 1,
the two G.711 laws as the header's formulas, and steps 1 - 5 as two int64 matrix-free convolutions (np.convolve on the
zero-stuffed signal), the stated shifts and clips.  Written from the contract, not from csrc/phone.*: nothing here is paired,
chunked, split into polyphase halves or accumulated in 32 bits."""
import numpy as np

import batch_checker as BC
import resample_checker as RS

PHONE_PLAN_DTYPE = np.dtype([("codec", "<i4"), ("reserved", "<i4")])
PHONE_RECORD_DTYPE = np.dtype([("codec", "<i4"), ("saturated_down", "<i4"), ("saturated_up", "<i4"), ("reserved", "<i4")])
CODECS = {"pcm": 0, "ulaw": 1, "alaw": 2}
f32 = np.float32


def taps():
    """T[0 .. 128] as int64, and the float64 h it was rounded from."""
    up, down, half, h = RS.design(16000, 8000)
    assert (up, down, half, len(h)) == (1, 2, 64, 129)
    return np.rint(32768.0 * h).astype(np.int64), h


def phone_plan(p_phone, codec_mask, B, seed, step, item0=0):
    key = (seed & BC.M32, (seed >> 32) & BC.M32)
    bits = [c for c in range(3) if (codec_mask >> c) & 1]
    out = np.zeros(B, PHONE_PLAN_DTYPE)
    for b in range(B):
        t = BC.philox4x32_10(((item0 + b) & BC.M32, step & BC.M32, (step >> 32) & BC.M32, 3), key)
        out[b] = (bits[BC.mulhi(t[1], len(bits))] if BC.unit(t[0]) < np.float32(p_phone) else -1, 0)
    return out


def make_plan(codecs):
    out = np.zeros(len(codecs), PHONE_PLAN_DTYPE)
    out["codec"] = codecs
    return out


# ---- G.711, from the header's "G.711 payloads" formulas ---------------------------------------------------------------------
def _floor_log2(a):
    return np.floor(np.log2(a.astype(np.float64))).astype(np.int64)        # exact for integers below 2^53


def ulaw_encode(p):
    p = np.asarray(p, np.int64)
    s = np.where(p < 0, 0x80, 0)
    a = np.minimum(np.abs(p), 32635) + 132
    e = _floor_log2(a) - 7
    m = (a >> (e + 3)) & 15
    return ~(s | (e << 4) | m) & 0xFF


def ulaw_decode(c):
    u = ~np.asarray(c, np.int64) & 0xFF
    e, m = (u >> 4) & 7, u & 15
    mag = (((m << 3) + 132) << e) - 132
    return np.where(u & 0x80, -mag, mag)


def alaw_encode(p):
    p = np.asarray(p, np.int64)
    g = np.where(p >= 0, p, ~p)
    q = g >> 3
    s = np.where(q < 32, 0, _floor_log2(np.maximum(q, 1)) - 4)
    m = np.where(s < 2, (q >> 1) & 15, (q >> s) & 15)
    return (np.where(p >= 0, 0x80, 0) | (s << 4) | m) ^ 0x55


def alaw_decode(c):
    a = np.asarray(c, np.int64) ^ 0x55
    m, s = a & 15, (a >> 4) & 7
    t = np.where(s == 0, (m << 4) + 8, ((m << 4) + 264) << np.maximum(s - 1, 0))
    return np.where(a & 0x80, t, -t)


def codec(c, v):
    if c == 1:
        return ulaw_decode(ulaw_encode(v))
    if c == 2:
        return alaw_decode(alaw_encode(v))
    return np.asarray(v, np.int64)


# ---- steps 1 - 5 -----------------------------------------------------------------------------------------------------------------
def pcm16(r):
    return np.clip(np.rint(np.asarray(r, f32).astype(np.float64) * 32768.0), -32768, 32767).astype(np.int64)


def channel_row(r, c):
    """r: float32 row, c: codec 0 .. 2.  -> (float32 row, clips of step 2, clips of step 4, v, w)."""
    T, _ = taps()
    L = len(r)
    J = (L + 1) // 2
    p = pcm16(r)
    # step 2: full[n] = sum_i p_i T[n - i]; v_j wants the tap index 2j - i + 64, i.e. n = 2j + 64
    full = np.convolve(p, T)
    assert full.dtype == np.int64
    acc = full[64 + 2 * np.arange(J)]
    v = (acc + (1 << 14)) >> 15
    down = int(((v < -32768) | (v > 32767)).sum())
    v = np.clip(v, -32768, 32767)
    w = codec(c, v)
    # step 4: the zero-stuffed w (w_j at position 2j), z_i wants the tap index i - 2j + 64, i.e. n = i + 64
    stuffed = np.zeros(2 * J, np.int64)
    stuffed[::2] = w
    acc = np.convolve(stuffed, T)[64 + np.arange(L)]
    z = (acc + (1 << 13)) >> 14
    up = int(((z < -32768) | (z > 32767)).sum())
    z = np.clip(z, -32768, 32767)
    out = z.astype(f32) / f32(32768.0)
    return out, down, up, v, w


def phone(src_noisy, src_clean, plan, target):
    """src_*: (B, L) float32 (src_clean may be None); plan: PHONE_PLAN_DTYPE; target 0 narrow, 1 wide.
    -> (noisy, clean or None, records).  A plan entry outside -1 .. 2 counts as -1."""
    B = len(plan)
    noisy = np.array(src_noisy, f32, copy=True)
    clean = None if src_clean is None else np.array(src_clean, f32, copy=True)
    rec = np.zeros(B, PHONE_RECORD_DTYPE)
    for b in range(B):
        c = int(plan["codec"][b])
        if c < -1 or c > 2:
            c = -1
        rec[b] = (c, 0, 0, 0)
        if c < 0:
            continue
        noisy[b], down, up, _, _ = channel_row(src_noisy[b], c)
        rec[b] = (c, down, up, 0)
        if clean is not None and target == 0:
            clean[b] = channel_row(src_clean[b], 0)[0]
    return noisy, clean, rec


# ---- rows the host and the GPU tests share ------------------------------------------------------------------------------------
def full_scale(L):
    return (np.resize(np.array([32767] * 3 + [-32768] * 4, np.float32), L) / np.float32(32768.0)).astype(np.float32)


def rows_for(L, seed=0):
    """(noisy, clean) sources of six rows: random at -35 and at -6 dB, all zero, the int16 boundary values (and the floats
    that round onto and over them), the full-scale pattern, and a row that is loud enough to clip after the codec."""
    rng = np.random.default_rng(1000 * seed + L)
    edge = np.array([-32768, -32767, -32769, -129, -128, -1, 0, 1, 127, 128, 32766, 32767, 32768, 0.5, -0.5, 1.5, 2.5, -1.5,
                     32766.5, 32767.5, -32767.5, -32768.5, 40000, -40000], np.float64) / 32768.0
    n = np.stack([
        rng.standard_normal(L) * 10 ** (-35 / 20),
        rng.standard_normal(L) * 10 ** (-6 / 20),
        np.zeros(L),
        np.resize(edge, L),
        full_scale(L).astype(np.float64),
        np.clip(rng.standard_normal(L) * 2.0, -1.0, 1.0),
    ]).astype(np.float32)
    c = np.roll(n, 1, axis=0) * np.float32(0.5)
    return n, np.ascontiguousarray(c.astype(np.float32))
