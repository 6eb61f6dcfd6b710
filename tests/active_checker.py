"""The numpy statement of "active levels" (include/gtcrn_micro_hip.h): the mix of batch_checker with the noise gain taken from
the levels over each side's active windows.  np.int64 energies, an integer comparison per window, then np.float64 / np.float32
with one rounded operation per line where the contract says so.  Written from the contract, not from the kernels: nothing here
is chunked, reduced across lanes or shared with csrc/batch.*."""
import numpy as np

from batch_checker import PLAN_DTYPE, make_plan, window  # noqa: F401  (re-exported for the tests)

ACTIVE_RECORD_DTYPE = np.dtype([("Ss", "<i8"), ("Sn", "<i8"), ("Ssn", "<i8"), ("As", "<i8"), ("An", "<i8"), ("Ns", "<i4"),
                                ("Nn", "<i4"), ("gn", "<f4"), ("Gf", "<f4"), ("peak", "<f4"), ("flags", "<i4")])
SPEECH_INACTIVE, NOISE_INACTIVE = 16, 32
f32, f64 = np.float32, np.float64


def active_windows(x, W, thr):
    """x: int16 row.  -> (bool per window: E_w > thr * n_w, int64 E_w per window, int64 n_w per window)."""
    L = len(x)
    x64 = x.astype(np.int64)
    edges = np.arange(0, L, W)
    E = np.add.reduceat(x64 * x64, edges)
    n = np.minimum(edges + W, L) - edges
    return E > np.int64(thr) * n, E, n


def mix_item_active(s, n, snr_amp, lvl_amp, W, thr):
    """s, n: the int16 speech window and the wrapped noise window, as mixed.  -> (noisy, clean, record tuple)."""
    L = len(s)
    s64, n64 = s.astype(np.int64), n.astype(np.int64)
    Ss, Sn, Ssn = int((s64 * s64).sum()), int((n64 * n64).sum()), int((s64 * n64).sum())
    sa, sE, sn_ = active_windows(s, W, thr)
    na, nE, nn_ = active_windows(n, W, thr)
    As, Ns = int(sE[sa].sum()), int(sn_[sa].sum())
    An, Nn = int(nE[na].sum()), int(nn_[na].sum())
    flags = 0
    if Ns == 0:
        As, Ns, flags = Ss, L, flags | SPEECH_INACTIVE
    if Nn == 0:
        An, Nn, flags = Sn, L, flags | NOISE_INACTIVE
    if An == 0:
        gn, flags = f32(0.0), flags | 1
    elif As == 0:
        gn, flags = f32(1.0), flags | 2
    else:
        r = f64(As) / f64(An)
        if Ns != Nn:
            r = r * (f64(Nn) / f64(Ns))
        gn = f32(np.sqrt(r) * f64(f32(snr_amp)))
    # from here on: batch_checker.mix_item, line for line
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
    return (Gf * m).astype(f32), (Gf * sf).astype(f32), (Ss, Sn, Ssn, As, An, Ns, Nn, gn, Gf, peak, flags)


def mix_active(spcm, soff, npcm, noff, plan_, L, W, thr, tpcm=None):
    """-> (noisy (B, L) float32, clean (B, L) float32, records ACTIVE_RECORD_DTYPE[B]).  tpcm: a target corpus under soff; clean
    is then its gained window."""
    B = len(plan_)
    noisy, clean, rec = np.zeros((B, L), f32), np.zeros((B, L), f32), np.zeros(B, ACTIVE_RECORD_DTYPE)
    for b, p in enumerate(plan_):
        s = window(spcm, soff, int(p["sclip"]), int(p["sstart"]), L)
        a, e = int(noff[p["nclip"]]), int(noff[p["nclip"] + 1])
        n = npcm[a + (int(p["nstart"]) + np.arange(L, dtype=np.int64)) % (e - a)]
        noisy[b], clean[b], r = mix_item_active(s, n, p["snr_amp"], p["lvl_amp"], W, thr)
        if tpcm is not None:
            t = window(tpcm, soff, int(p["sclip"]), int(p["sstart"]), L)
            clean[b] = (r[8] * (t.astype(f32) / f32(32768.0))).astype(f32)
        rec[b] = r
    return noisy, clean, rec
