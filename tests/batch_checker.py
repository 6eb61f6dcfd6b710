"""The numpy statement of "training batches from a resident corpus" (include/gtcrn_micro_hip.h): Philox4x32-10 in Python
integers, and the plan, the pairs draw and the mix draw in np.int64 / np.float32 / np.float64, one rounded operation per
line where the contract says so.  Written from the contract, not from the kernels: nothing here is chunked, vectorised or
shared with csrc/batch.*."""
import numpy as np

PLAN_DTYPE = np.dtype([("sclip", "<i4"), ("sstart", "<i4"), ("nclip", "<i4"), ("nstart", "<i4"),
                       ("snr_db", "<f4"), ("snr_amp", "<f4"), ("lvl_db", "<f4"), ("lvl_amp", "<f4")])
RECORD_DTYPE = np.dtype([("Ss", "<i8"), ("Sn", "<i8"), ("Ssn", "<i8"), ("gn", "<f4"), ("Gf", "<f4"), ("peak", "<f4"),
                         ("flags", "<i4")])
M32 = 0xFFFFFFFF
f32, f64 = np.float32, np.float64


def philox4x32_10(counter, key):
    c0, c1, c2, c3 = (int(v) & M32 for v in counter)
    k0, k1 = (int(v) & M32 for v in key)
    for r in range(10):
        if r:
            k0, k1 = (k0 + 0x9E3779B9) & M32, (k1 + 0xBB67AE85) & M32
        p0, p1 = 0xD2511F53 * c0, 0xCD9E8D57 * c2
        c0, c1, c2, c3 = (p1 >> 32) ^ c1 ^ k0, p1 & M32, (p0 >> 32) ^ c3 ^ k1, p0 & M32
    return c0, c1, c2, c3


def mulhi(r, k):
    return (int(r) * int(k)) >> 32


def unit(q):
    return f32(q >> 8) * f32(2.0 ** -24)


def plan(soff, noff, B, L, seed, step, item0=0, granule=1, snr=(-5.0, 20.0), lvl=(-35.0, -15.0), clips=None):
    """soff / noff: offset tables (noff None: no noise).  Returns a PLAN_DTYPE array."""
    soff = [int(v) for v in soff]
    noff = None if noff is None else [int(v) for v in noff]
    key = (seed & M32, (seed >> 32) & M32)
    out = np.zeros(B, PLAN_DTYPE)
    for b in range(B):
        ctr = ((item0 + b) & M32, step & M32, (step >> 32) & M32)
        r, q = philox4x32_10(ctr + (0,), key), philox4x32_10(ctr + (1,), key)
        sclip = int(clips[b]) if clips is not None else mulhi(r[0], len(soff) - 1)
        len_s = soff[sclip + 1] - soff[sclip]
        ks = 1 if len_s < L else max(1, (len_s - L) // granule + 1)
        nclip = nstart = 0
        if noff is not None:
            nclip = mulhi(r[2], len(noff) - 1)
            nstart = mulhi(r[3], noff[nclip + 1] - noff[nclip])
        snr_db = f32(snr[0]) + (f32(snr[1]) - f32(snr[0])) * unit(q[0])
        lvl_db = f32(lvl[0]) + (f32(lvl[1]) - f32(lvl[0])) * unit(q[1])
        assert snr_db.dtype == np.float32 and lvl_db.dtype == np.float32
        out[b] = (sclip, granule * mulhi(r[1], ks), nclip, nstart, snr_db, f32(10.0 ** (-float(snr_db) / 20.0)), lvl_db,
                  f32(10.0 ** (float(lvl_db) / 20.0)))
    return out


def make_plan(rows):
    """rows of (sclip, sstart, nclip, nstart, snr_amp, lvl_amp) -> a PLAN_DTYPE array (the dB fields are informative)."""
    out = np.zeros(len(rows), PLAN_DTYPE)
    for b, (sc, ss, nc, ns, sa, la) in enumerate(rows):
        out[b] = (sc, ss, nc, ns, f32(-20.0 * np.log10(sa)), f32(sa), f32(20.0 * np.log10(la)), f32(la))
    return out


def window(pcm, off, clip, start, L):
    """int16 window of L samples from `start` of clip `clip`, zero past the clip's end."""
    a, e = int(off[clip]), int(off[clip + 1])
    w = np.zeros(L, np.int16)
    got = pcm[a + start:min(e, a + start + L)]
    w[:len(got)] = got
    return w


def pairs(pcm_noisy, pcm_clean, off, plan_, L):
    noisy = np.stack([window(pcm_noisy, off, int(p["sclip"]), int(p["sstart"]), L).astype(f32) / f32(32768.0) for p in plan_])
    clean = np.stack([window(pcm_clean, off, int(p["sclip"]), int(p["sstart"]), L).astype(f32) / f32(32768.0) for p in plan_])
    return noisy, clean


def mix_item(s, n, snr_amp, lvl_amp):
    """s, n: the int16 speech window and the wrapped noise window.  -> (noisy, clean, record tuple)."""
    L = len(s)
    s64, n64 = s.astype(np.int64), n.astype(np.int64)
    Ss, Sn, Ssn = int((s64 * s64).sum()), int((n64 * n64).sum()), int((s64 * n64).sum())
    flags = 0
    if Sn == 0:
        gn, flags = f32(0.0), flags | 1
    elif Ss == 0:
        gn, flags = f32(1.0), flags | 2
    else:
        gn = f32(np.sqrt(f64(Ss) / f64(Sn)) * f64(f32(snr_amp)))
    sf = s.astype(f32) / f32(32768.0)
    nf = n.astype(f32) / f32(32768.0)
    gz = (gn * nf).astype(f32)                  # a rounded multiply
    m = (sf + gz).astype(f32)                   # then a rounded add
    g = f64(gn)
    Sm = f64(Ss) + g * (f64(2.0) * f64(Ssn) + g * f64(Sn))
    Sm = max(Sm, f64(0.0))
    peak = f32(np.abs(m).max())
    if Sm == 0.0:
        G, flags = f64(1.0), flags | 4
    else:
        rms = np.sqrt(Sm / f64(L)) / f64(32768.0)
        G = f64(f32(lvl_amp)) / rms
        if f64(peak) * G > 0.99:
            G, flags = f64(0.99) / f64(peak), flags | 8
    Gf = f32(G)
    return (Gf * m).astype(f32), (Gf * sf).astype(f32), (Ss, Sn, Ssn, gn, Gf, peak, flags)


def mix(spcm, soff, npcm, noff, plan_, L):
    """-> (noisy (B, L) float32, clean (B, L) float32, records RECORD_DTYPE[B])."""
    B = len(plan_)
    noisy, clean, rec = np.zeros((B, L), f32), np.zeros((B, L), f32), np.zeros(B, RECORD_DTYPE)
    for b, p in enumerate(plan_):
        s = window(spcm, soff, int(p["sclip"]), int(p["sstart"]), L)
        a, e = int(noff[p["nclip"]]), int(noff[p["nclip"] + 1])
        n = npcm[a + (int(p["nstart"]) + np.arange(L, dtype=np.int64)) % (e - a)]
        noisy[b], clean[b], r = mix_item(s, n, p["snr_amp"], p["lvl_amp"])
        rec[b] = r
    return noisy, clean, rec


def ulp_distance(a, b):
    """|a - b| in float32 units in the last place (finite, same-sign values)."""
    ia = np.asarray(a, f32).view(np.int32).astype(np.int64)
    ib = np.asarray(b, f32).view(np.int32).astype(np.int64)
    return np.abs(ia - ib)


def assert_same_plan(got, want):
    """The plan criteria: integer fields and both dB fields bit for bit; the two amplitudes within 1 float ulp, because pow
    is not correctly rounded (libm documents 1 ulp)."""
    assert got.dtype == PLAN_DTYPE and want.dtype == PLAN_DTYPE and got.shape == want.shape
    for f in ("sclip", "sstart", "nclip", "nstart"):
        assert np.array_equal(got[f], want[f]), f
    for f in ("snr_db", "lvl_db"):
        assert np.array_equal(got[f].view(np.int32), want[f].view(np.int32)), f
    for f in ("snr_amp", "lvl_amp"):
        assert ulp_distance(got[f], want[f]).max() <= 1, f
