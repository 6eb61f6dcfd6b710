"""The cases of the packet loss concealment that tests/test_plc_host.py runs through the host twins and tests/test_gpu_plc.py
through the kernel, each against tests/plc_checker.py, bit for bit.  A case is a dict: fs, n, S (streams), kw (the parameter
fields), ticks: a list of (rows (M, n) int16, lost (M,), slots (M,) or None, count or None); float cases carry float32 rows.
The histories and records are carried from tick to tick.  `run` turns the int16 rows into the row type under test."""
import os

import numpy as np

import g711_checker as G
import plc_checker as PK

F = np.float32
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
GUARD = {np.dtype(np.float32): F(12345.0), np.dtype(np.int16): np.int16(12345), np.dtype(np.uint8): np.uint8(0x5A)}
GUARD_H = np.int16(-21555)
KINDS = ("f32", "pcm16", "ulaw", "alaw")
LAW = {"f32": None, "pcm16": None, "ulaw": 0, "alaw": 1}
RATE_CASES = ((8000, 80), (8000, 160), (16000, 160), (16000, 320), (16000, 256), (22050, 441), (44100, 441), (48000, 480), (48000, 960))

_speech = None


def speech(fs, length, row):
    """An excerpt of the golden examples (16 kHz int16), every other sample at 8 kHz; other rates take it as it is."""
    global _speech
    if _speech is None:
        z = np.load(os.path.join(GOLDEN, "examples_full.npz"))
        _speech = np.concatenate([z["noisy"][:, 16000:76000], z["enh"][:, 16000:76000]], 0)
    v = _speech[row % len(_speech)]
    v = v[::2] if fs == 8000 else v
    return np.resize(v, length).astype(np.int16)


def periodic(P, length, amp=8000, phase=0):
    """An integer-period signal: four harmonics of period P samples, exactly periodic as int16."""
    t = (np.arange(P) + phase) % P
    cyc = sum(np.sin(2 * np.pi * k * t / P + 0.3 * k) / k for k in (1, 2, 3, 4))
    cyc = np.rint(amp * cyc / np.abs(cyc).max()).astype(np.int16)
    return np.resize(cyc, length)


def signals(fs, length, seed):
    """The named signals at rate fs, as a list of (name, int16 array)."""
    rng = np.random.default_rng(seed)
    prm = PK.params(fs)
    pmin, pmax, D = int(prm[0]), int(prm[1]), int(prm[3])
    P = pmin + D * 5                                            # P and 2 P in range, both on the coarse grid
    assert 2 * P <= pmax
    square = np.where((np.arange(length) // (pmin // 2 + 3)) % 2 == 0, -32768, 32767).astype(np.int16)
    return [("silence", np.zeros(length, np.int16)), ("full_scale", square),
            ("quiet", periodic(P + 7, length, amp=500)), ("periodic", periodic(P, length)),
            ("off_grid", periodic(P + D * 3 + (1 if D > 1 else 0), length, amp=12000)),
            ("speech", speech(fs, length, seed)), ("speech2", speech(fs, length, seed + 5)),
            ("noise", (rng.standard_normal(length) * 3000).astype(np.int16))]


def schedules(T, rng):
    """(T, 8) loss flags: single losses; bursts of 2 and 3; a burst of 8; the first packets; back to back with one good packet
    between; none; random; every other packet."""
    L = np.zeros((T, 8), bool)
    at = lambda f: min(T - 1, int(f * T))
    L[[at(0.35), at(0.7)], 0] = True
    L[at(0.4):at(0.4) + 2, 1] = True
    L[at(0.7):at(0.7) + 3, 1] = True
    L[at(0.4):at(0.4) + 8, 2] = True
    L[:2, 3] = True
    L[at(0.8), 3] = True
    L[[at(0.35), at(0.35) + 2], 4] = True
    L[:, 6] = rng.random(T) < 0.2
    L[1::2, 7] = True
    return L


def stream_case(fs, n, T=30, seed=0, shift=0, **kw):
    """Eight streams, the eight schedules, the eight signals rotated by `shift`, every stream in every tick."""
    rng = np.random.default_rng(seed)
    sig = signals(fs, T * n, seed)
    x = np.stack([sig[(k + shift) % len(sig)][1] for k in range(8)])
    L = schedules(T, rng)
    ticks = [(x[:, t * n:(t + 1) * n].copy(), L[t].astype(np.int32), None, None) for t in range(T)]
    return dict(fs=fs, n=n, S=8, kw=kw, ticks=ticks)


def slots_case(fs=16000, n=160, T=24, seed=3):
    """Nine streams, six rows a tick in a changing, unsorted order; an id out of range in some ticks (a no-op row, lost or not);
    the row count cycles through M, 2 and 0."""
    rng = np.random.default_rng(seed)
    sig = signals(fs, T * n, seed)
    ticks = []
    for t in range(T):
        ids = rng.permutation(9)[:6].astype(np.int32)
        rows = np.stack([sig[s % len(sig)][1][t * n:(t + 1) * n] for s in ids])
        if t % 5 == 2:
            ids[1] = 99 if t % 2 else -1
        lost = (rng.random(6) < 0.3).astype(np.int32) * 7
        ticks.append((rows, lost, ids, (None, 6, 2, 0, 6, 9)[t % 6]))
    return dict(fs=fs, n=n, S=9, kw={}, ticks=ticks)


def poison_case(poisoned=True, fs=16000, n=160, T=16):
    """Float rows.  Stream 2 carries NaN, +-Inf and 1e30 in received packets, in a recovery packet and (ignored) in a lost one."""
    c = stream_case(fs, n, T, seed=11, shift=3)
    ticks = []
    for t, (rows, lost, slots, count) in enumerate(c["ticks"]):
        rows = (rows.astype(np.float64) / 32768.0).astype(F)
        lost = lost.copy()
        lost[2] = int(t in (4, 5, 9))
        if poisoned:
            if t in (2, 3, 6, 10, 12, 14):                       # 6 and 10 are recovery packets
                rows[2, [0, 1, 5, n - 1]] = [np.nan, np.inf, -np.inf, 1e30]
                rows[2, 2] = -1e30
            if t == 4:
                rows[2, :] = np.nan
        ticks.append((rows, lost, slots, count))
    return dict(fs=fs, n=n, S=8, kw=c["kw"], ticks=ticks)


def all_cases():
    cases = [(f"{fs}_{n}", stream_case(fs, n, seed=i, shift=i)) for i, (fs, n) in enumerate(RATE_CASES)]
    p8 = PK.params(8000)
    pmin, pmax, Lh = int(p8[0]), int(p8[1]), PK.hist_len(p8)
    cases.append(("n_1", stream_case(8000, 1, T=2 * Lh + 90, seed=20, shift=1)))            # F > n: every recovery is one sample
    cases += [(f"n_{n}", stream_case(8000, n, T=30, seed=21 + i, shift=2 + i)) for i, n in enumerate((pmin - 1, pmin, pmax + 1, 1024))]
    cases.append(("n_1024_at_48000", stream_case(48000, 1024, T=12, seed=26, shift=4)))
    cases.append(("short_fades", stream_case(16000, 160, seed=27, shift=5, hold_ms=0, fade_ms=1, recover_ms=0)))
    cases.append(("long_fades", stream_case(16000, 160, seed=28, shift=6, hold_ms=200, fade_ms=200, recover_ms=200)))
    cases.append(("slots", slots_case()))
    return cases


def poison_cases():
    return [("poison", poison_case())]


def as_kind(rows, kind):
    """int16 rows as the row type under test (float32 rows stay float32: the float cases)."""
    if rows.dtype == np.float32:
        assert kind == "f32"
        return rows.copy()
    if kind == "f32":
        return (rows.astype(np.float64) / 32768.0).astype(F)
    if kind == "pcm16":
        return rows.copy()
    return G.encode(LAW[kind], rows)


def fresh(c, pad=3):
    """Zeroed histories (pitch Lh + pad, the pad holding guards), records and the parameter words of a case."""
    prm = PK.params(c["fs"], **c["kw"])
    Lh = PK.hist_len(prm)
    hist = np.zeros((c["S"], Lh + pad), np.int16)
    hist[:, Lh:] = GUARD_H
    return prm, hist, np.zeros((c["S"], 4), np.int32)


def filled(rows, lost, pad, rng):
    """The call's buffer: pitch n + pad, guards behind every row; a lost row holds junk of its type."""
    M, n = rows.shape
    buf = np.full((M, n + pad), GUARD[rows.dtype], rows.dtype)
    buf[:, :n] = rows
    for i in np.nonzero(lost)[0]:
        buf[i, :n] = rng.integers(0, 255, n).astype(rows.dtype)
    return buf


def run(c, fn, kind, pad, trace=None):
    """Runs the case's ticks through fn(x, lost, hist, rec, prm, slots, count, law) (x a view of a pitched buffer; x, hist and rec
    written in place) and through the checker, and compares buffers, histories and records after every tick, bit for bit.
    trace: a list that receives the checker's (x, hist, rec) per tick."""
    law = LAW[kind]
    prm, hist_w, rec_w = fresh(c)
    _, hist_g, rec_g = fresh(c)
    rng = np.random.default_rng(99)
    n = c["n"]
    for t, (rows, lost, slots, count) in enumerate(c["ticks"]):
        want = filled(as_kind(rows, kind), lost, pad, rng)
        got = want.copy()
        PK.conceal(want[:, :n], lost, hist_w, rec_w, prm, slots, count, law)
        fn(got[:, :n], lost, hist_g, rec_g, prm, slots, count, law)
        assert PK.same_bits(got, want), f"tick {t}: rows differ at {np.argwhere(got.view(np.uint8) != want.view(np.uint8))[:4].tolist()}"
        assert PK.same_bits(rec_g, rec_w), f"tick {t}: records differ:\n{rec_g}\n{rec_w}"
        assert PK.same_bits(hist_g, hist_w), f"tick {t}: histories differ in streams {np.unique(np.argwhere(hist_g != hist_w)[:, 0]).tolist()}"
        if trace is not None:
            trace.append((want[:, :n].copy(), hist_w.copy(), rec_w.copy()))
    assert (hist_w[:, PK.hist_len(prm):] == GUARD_H).all()


def speech_loss(packets=1200):
    """Single losses, bursts of 2 and bursts of 3."""
    lost = np.zeros(packets, np.int32)
    lost[25::20] = 1
    lost[46::60] = 1
    lost[47::120] = 1
    return lost


def speech_figures(fn, which, seconds=12, fs=16000, n=160):
    """The first `seconds` of the five `which` ("noisy" / "enh") rows of the golden examples at 16 kHz / 160 as int16 through
    fn with speech_loss(): over the lost packets whose true energy is above -40 dBov, the summed error energy of the concealed
    packets over the summed energy of the true ones (1 is what zero fill gives), the median of the per-packet ratios, and counts."""
    x = np.load(os.path.join(GOLDEN, "examples_full.npz"))[which][:, :seconds * fs]
    T = x.shape[1] // n
    lost = speech_loss(T)
    prm = PK.params(fs)
    hist, rec = np.zeros((len(x), PK.hist_len(prm)), np.int16), np.zeros((len(x), 4), np.int32)
    err, ref = [], []
    for t in range(T):
        true = x[:, t * n:(t + 1) * n]
        rows = true.copy()
        fn(rows, np.full(len(x), lost[t], np.int32), hist, rec, prm, None, None, None)
        if lost[t]:
            e = ((rows.astype(np.float64) - true) ** 2).sum(1) / 32768.0 ** 2
            r = (true.astype(np.float64) ** 2).sum(1) / 32768.0 ** 2
            keep = r / n > 1e-4
            err += e[keep].tolist()
            ref += r[keep].tolist()
    err, ref = np.array(err), np.array(ref)
    return dict(ratio=float(err.sum() / ref.sum()), median=float(np.median(err / ref)), packets=int(len(err)),
                lost_packets=int(lost.sum()) * len(x), erasures=int((rec[:, 3] & 0xFFFF).sum()))
