"""The packet loss concealment contract of include/gtcrn_micro_hip.h ("packet loss concealment"), restated in numpy on a page:
int64 sums, float64 scores, float32 cross-fade, the G.711 maps of tests/g711_checker.py.  Independent of csrc/: nothing here
loads the library.  Used by tests/test_plc_host.py and tests/test_gpu_plc.py through tests/plc_cases.py."""
import numpy as np

import g711_checker as G

F = np.float32
RATES = (8000, 16000, 22050, 24000, 32000, 44100, 48000)


def params(fs, hold_ms=10, fade_ms=50, recover_ms=5):
    """The 8 parameter words {pmin, pmax, W, D, T0, T1, F, fs}."""
    assert fs in RATES
    return np.array([fs // 200, fs * 15 // 1000, fs // 50, max(1, fs // 8000), hold_ms * fs // 1000, fade_ms * fs // 1000,
                     max(1, recover_ms * fs // 1000), fs], np.int32)


def hist_len(prm):
    return int(prm[1]) + int(prm[2])


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def pcm_of(x):
    """clip(rint(32768 x), -32768, 32767) of float32 values, a NaN giving -32768."""
    with np.errstate(invalid="ignore", over="ignore"):
        v = np.asarray(x, F) * F(32768.0)
        v = np.where(v >= F(-32768.0), v, F(-32768.0))
        v = np.where(v <= F(32767.0), v, F(32767.0))
        return np.rint(v).astype(np.int64)


def int16_of(row, law):
    """The int16 (as int64) of a row's samples: float32, int16 or G.711 codes."""
    if row.dtype == np.float32:
        return pcm_of(row)
    if row.dtype == np.int16:
        return row.astype(np.int64)
    return G.decode_table(law).astype(np.int64)[row]


def stored(o, dtype, law):
    """How int16 values are written to a row."""
    if dtype == np.float32:
        return (o.astype(np.float64) / 32768.0).astype(F)
    if dtype == np.int16:
        return o.astype(np.int16)
    return G.encode(law, o)


def logical(ring, pos, Lh):
    """The history in logical order (newest last) of a ring whose write position is pos."""
    return np.roll(ring[:Lh], -pos).astype(np.int64)


def append(ring, pos, Lh, v):
    """Appends the int16 values v to the ring in place; returns the new write position."""
    n = len(v)
    j = np.arange(max(0, n - Lh), n)
    ring[(pos + j) % Lh] = v[j].astype(np.int16)
    return (pos + n) % Lh


def scores(a, Lh, lags, d, W):
    i = np.arange(0, W, d)
    a0 = a[Lh - 1 - i]
    a1 = a[(Lh - 1 - i)[None, :] - np.asarray(lags)[:, None]]
    c, e = (a1 * a0[None, :]).sum(1), (a1 * a1).sum(1)
    assert np.abs(c).max(initial=0) < 2 ** 30 and e.max(initial=0) < 2 ** 30, "the contract's int32 bound"
    cf, ef = c.astype(np.float64), e.astype(np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where((c > 0) & (e > 0), (cf * cf) / ef, 0.0)


def pick(lags, sc):
    """The largest score > 0, among equal scores the smallest lag; None without a positive score."""
    best = None
    for p, s in zip(lags, sc):
        if s > 0 and (best is None or s > best[1]):          # lags ascend: an equal score at a larger lag does not replace
            best = (int(p), s)
    return None if best is None else best[0]


def find_lag(h, prm):
    pmin, pmax, W, D = (int(v) for v in prm[:4])
    Lh = pmax + W
    m = int(np.abs(h).max())
    s = max(0, m.bit_length() - 10)
    a = h >> s
    coarse = np.arange(pmin, pmax + 1, D)
    p0 = pick(coarse, scores(a, Lh, coarse, D, W))
    if p0 is None:
        return pmax
    fine = np.arange(max(pmin, p0 - D + 1), min(pmax, p0 + D - 1) + 1)
    p = pick(fine, scores(a, Lh, fine, 1, W))
    return p0 if p is None else p


def gain(t, prm):
    T0, T1 = int(prm[4]), int(prm[5])
    t = np.asarray(t, np.int64)
    return np.where(t < T0, 32768, np.maximum(0, 32768 - ((t - T0) * 32768) // T1))


def synth(h, Lh, P, n):
    return h[Lh - P + np.arange(n) % P]


def conceal(x, lost, hist, rec, prm, slots=None, count=None, law=None):
    """One call on numpy arrays, in place: x (M, n) float32 / int16 / uint8 codes, lost (M,), hist (S, >= Lh) int16 rings,
    rec (S, 4) int32 {pos, lag, erased, events}, prm the 8 words."""
    M, n = x.shape
    S = rec.shape[0]
    Lh, T0, T1, Fr = hist_len(prm), int(prm[4]), int(prm[5]), int(prm[6])
    live = M if count is None else max(0, min(int(count), M))
    for i in range(live):
        slot = i if slots is None else int(slots[i])
        if not 0 <= slot < S:
            continue
        ring, row = hist[slot], x[i]
        pos, P, erased, events = (int(v) for v in rec[slot])
        if not lost[i] and erased == 0:
            rec[slot, 0] = append(ring, pos, Lh, int16_of(row, law))
            continue
        h = logical(ring, pos, Lh)
        if lost[i]:
            if erased == 0:
                P = find_lag(h, prm)
                events = (events & ~0xFFFF) | ((events + 1) & 0xFFFF)
            s = synth(h, Lh, P, n)
            o = (s * gain(erased + np.arange(n), prm) + 16384) >> 15
            row[:] = stored(o, x.dtype, law)
            pos = append(ring, pos, Lh, s)
            events = (events & 0xFFFF) | ((((events >> 16) + 1) & 0xFFFF) << 16)
            events = events - (1 << 32) if events >= 1 << 31 else events
            rec[slot] = (pos, P, min(erased + n, T0 + T1), events)
            continue
        f = min(Fr, n)
        k = np.arange(f)
        r = ((k + 1) * 32768) // f
        sa = (synth(h, Lh, P, f) * gain(erased + k, prm) + 16384) >> 15
        if x.dtype == np.float32:
            rf, saf = (r.astype(np.float64) / 32768.0).astype(F), (sa.astype(np.float64) / 32768.0).astype(F)
            with np.errstate(invalid="ignore", over="ignore"):
                row[:f] = (row[:f] * rf).astype(F) + (saf * (F(1.0) - rf).astype(F)).astype(F)
        else:
            row[:f] = stored((int16_of(row[:f], law) * r + sa * (32768 - r) + 16384) >> 15, x.dtype, law)
        pos = append(ring, pos, Lh, int16_of(row, law))
        rec[slot] = (pos, P, 0, events)


def history(hist, rec, prm):
    """(S, Lh) int16: the histories in logical order."""
    Lh = hist_len(prm)
    return np.stack([np.roll(hist[s, :Lh], -int(rec[s, 0])) for s in range(hist.shape[0])])
