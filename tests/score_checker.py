"""Float64 statement of the "scores" section of include/gtcrn_micro_hip.h, written from the header and independent of
the kernels: SDR and SI-SNR as eval/eval_intrusive_metrics.py:74-91 writes them, STOI as Taal et al. 2011 (the
structure pystoi's stoi(..., extended=False) follows) behind this library's own 16 kHz -> 10 kHz filter.

Not a test module: tests/test_score_checker.py pins it (to the reference's recorded numbers and to STOI's properties),
tests/test_gpu_score.py holds the kernels to it.
"""
import numpy as np
from scipy.signal import resample_poly

EPS = 2.0 ** -52
UP, DOWN, HALF = 5, 8, 256
FRAME, HOP, NFFT, NBANDS, SEG = 256, 128, 512, 15, 30
BETA_CLIP = 1.0 + 10.0 ** (15.0 / 20.0)
BAND_LO = (7, 9, 11, 14, 17, 22, 27, 34, 43, 55, 69, 87, 109, 138, 174)
BAND_HI = (9, 11, 14, 17, 22, 27, 34, 43, 55, 69, 87, 109, 138, 174, 219)


# ---- the inputs the golden numbers were recorded on (tests/golden/make_golden_score.py) and the tests reuse ----------
EXCERPT_LEN = 64000                                    # 4 s
EXCERPTS = tuple((c, o) for c in range(5) for o in (0, 8, 16))   # (clip, offset in seconds) of examples_full.npz
SNR_LADDER = (-5.0, 0.0, 5.0, 15.0, 30.0)
LADDER_EXCERPT = (2, 8)                                # the speech excerpt the white-noise ladder is built on


def excerpt_pair(ex, clip, off_s, n=EXCERPT_LEN):
    """(ref, inf) = (noisy, enhanced) float32 excerpts of examples_full.npz, as sf.read(dtype='float32') scales them."""
    a = int(off_s) * 16000
    return (ex["noisy"][clip, a:a + n].astype(np.float32) / np.float32(32768.0),
            ex["enh"][clip, a:a + n].astype(np.float32) / np.float32(32768.0))


def ladder_pair(ex, snr_db):
    """(speech, speech + white noise at snr_db) in float32; the speech is the enhanced excerpt LADDER_EXCERPT."""
    s = excerpt_pair(ex, *LADDER_EXCERPT)[1].astype(np.float64)
    noise = np.random.default_rng(20241).standard_normal(s.size)
    noise *= np.sqrt(np.sum(s ** 2) / np.sum(noise ** 2) / 10.0 ** (snr_db / 10.0))
    return s.astype(np.float32), (s + noise).astype(np.float32)


def gated_pair(ex, clip, off_s, n=EXCERPT_LEN):
    """(ref, inf) = (enhanced excerpt with every third quarter second zeroed, noisy excerpt): a reference with real
    silences, so that the keep mask drops frames and the compaction moves the rest."""
    noisy, enh = excerpt_pair(ex, clip, off_s, n)
    gate = ((np.arange(n) // 4000) % 3 != 1).astype(np.float32)
    return enh * gate, noisy


# The GPU test's batches: name -> (L, [(kind, clip, offset in s, length)]).  L = 16000 and 64000, B = 1, 3, 5, and one
# variable-length batch whose 6000- and 257-sample rows are too short for a segment (257: no analysis frame at all).
GPU_CASES = {
    "L64000_B5": (64000, [("ex", 0, 0, 64000), ("ex", 0, 8, 64000), ("ex", 0, 16, 64000), ("ex", 1, 0, 64000), ("ex", 1, 8, 64000)]),
    "L64000_B3": (64000, [("gate", 2, 8, 64000), ("gate", 3, 0, 64000), ("ex", 4, 16, 64000)]),
    "L64000_B1": (64000, [("ex", 2, 16, 64000)]),
    "L16000_B5": (16000, [("ex", 0, 16, 16000), ("ex", 1, 8, 16000), ("ex", 2, 0, 16000), ("gate", 3, 8, 16000), ("gate", 4, 0, 16000)]),
    "L16000_B3": (16000, [("ex", 0, 0, 16000), ("ex", 2, 16, 16000), ("gate", 1, 16, 16000)]),
    "L16000_B1": (16000, [("gate", 2, 8, 16000)]),
    "var": (64000, [("ex", 1, 16, 64000), ("gate", 0, 8, 16000), ("ex", 2, 0, 6000), ("ex", 4, 8, 40001), ("ex", 3, 0, 257)]),
}
MASK_MARGIN_DB = 0.01      # no frame energy of a clip used in the exact mask comparison lies this close to its threshold

_examples = None
_refs = {}


def examples():
    global _examples
    if _examples is None:
        import os
        _examples = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "examples_full.npz"))
    return _examples


def case_pair(spec):
    kind, clip, off, n = spec
    return (gated_pair if kind == "gate" else excerpt_pair)(examples(), clip, off, n)


def case_reference(spec):
    """score() of one clip of GPU_CASES, computed once and shared (callers must not change it)."""
    if spec not in _refs:
        _refs[spec] = score(*case_pair(spec))
    return _refs[spec]


def design_taps():
    """The 513 taps of the 5/8 stage in double: sinc(2 fc n) * kaiser(n; 8.95926), fc = 0.9375 * 0.5 / 8, sum == 5."""
    n = np.arange(-HALF, HALF + 1, dtype=np.float64)
    fc = 0.9375 * 0.5 / 8
    h = np.sinc(2.0 * fc * n) * np.i0(8.95926 * np.sqrt(1.0 - (n / HALF) ** 2)) / np.i0(8.95926)
    return h * (UP / h.sum())


def taps():
    """What the contract filters with: the design rounded once to float."""
    return design_taps().astype(np.float32).astype(np.float64)


def window():
    return 0.5 * (1.0 - np.cos(2.0 * np.pi * np.arange(1, FRAME + 1) / (FRAME + 1)))


def bands():
    """Nearest bins of 150 * 2^((2 j -/+ 1) / 6) Hz on the grid k * 10000 / 512."""
    f = np.arange(NFFT // 2 + 1) * (10000.0 / NFFT)
    j = np.arange(NBANDS)
    lo = [int(np.argmin((f - 150.0 * 2.0 ** ((2 * k - 1) / 6.0)) ** 2)) for k in j]
    hi = [int(np.argmin((f - 150.0 * 2.0 ** ((2 * k + 1) / 6.0)) ** 2)) for k in j]
    return lo, hi


def frames(L):
    n10 = -(-int(L) * UP // DOWN)
    return len(range(0, n10 - FRAME, HOP))


def resample10(x):
    x = np.asarray(x, np.float64)
    if x.size == 0:
        return x
    return resample_poly(x, UP, DOWN, window=taps() / UP)


def resample10_direct(x):
    """y[j] = sum_i x[i] h[8 j - 5 i + 256], the header's formula term by term (slow; pins resample10)."""
    x = np.asarray(x, np.float64)
    h = taps()
    y = np.zeros(-(-x.size * UP // DOWN))
    for j in range(y.size):
        for i in range(x.size):
            k = j * DOWN - i * UP + HALF
            if 0 <= k <= 2 * HALF:
                y[j] += x[i] * h[k]
    return y


def sdr(ref, inf):
    r = np.asarray(ref, np.float64)
    y = np.asarray(inf, np.float64)
    r = r - r.mean()
    y = y - y.mean()
    return 10.0 * np.log10((np.sum(r ** 2) + 1e-8) / (np.sum((y - r) ** 2) + 1e-8))


def sisnr(ref, inf):
    r = np.asarray(ref, np.float64)
    y = np.asarray(inf, np.float64)
    r = r - r.mean()
    y = y - y.mean()
    a = np.sum(y * r) / np.sum(r ** 2 + 1e-8)
    t = a * r
    return 10.0 * np.log10((np.sum(t ** 2) + 1e-8) / (np.sum((y - t) ** 2) + 1e-8))


def _frame(x, w):
    starts = range(0, x.size - FRAME, HOP)
    return np.array([w * x[s:s + FRAME] for s in starts]).reshape(len(starts), FRAME)


def stoi_stages(ref, inf):
    """Every stage of the STOI definition for one pair, as a dict (x10, energies, mask, envelopes, stoi, ...)."""
    w = window()
    x10, y10 = resample10(ref), resample10(inf)
    fx, fy = _frame(x10, w), _frame(y10, w)
    n = fx.shape[0]
    e = 20.0 * np.log10(np.linalg.norm(fx, axis=1) + EPS) if n else np.zeros(0)
    thr = e.max() - 40.0 if n else -np.inf
    mask = e > thr
    K = int(mask.sum())
    margin = float(np.abs(e - thr).min()) if n else np.inf
    out = dict(x10=x10, y10=y10, energies=e, mask=mask, kept_frames=K, n=n, margin_db=margin)
    M = max(K - 1, 0)
    envs = []
    for f in (fx, fy):
        ola = np.zeros((K - 1) * HOP + FRAME if K else 0)
        for k, fr in enumerate(f[mask]):
            ola[k * HOP:k * HOP + FRAME] += fr
        g = _frame(ola, w)
        assert g.shape[0] == M
        spec = np.fft.rfft(g, NFFT, axis=1) if M else np.zeros((0, NFFT // 2 + 1), complex)
        p = np.abs(spec) ** 2
        envs.append(np.array([np.sqrt(p[:, lo:hi].sum(axis=1)) for lo, hi in zip(BAND_LO, BAND_HI)]).reshape(NBANDS, M))
    X, Y = envs
    out.update(env_ref=X, env_inf=Y, M=M)
    if M < SEG:
        out.update(stoi=1e-5, segments=0)
        return out
    S = M - SEG + 1
    d = np.empty((NBANDS, S))
    for s in range(S):
        x, y = X[:, s:s + SEG], Y[:, s:s + SEG]
        alpha = np.linalg.norm(x, axis=1, keepdims=True) / (np.linalg.norm(y, axis=1, keepdims=True) + EPS)
        yp = np.minimum(alpha * y, x * BETA_CLIP)
        xc = x - x.mean(axis=1, keepdims=True)
        yc = yp - yp.mean(axis=1, keepdims=True)
        xc = xc / (np.linalg.norm(xc, axis=1, keepdims=True) + EPS)
        yc = yc / (np.linalg.norm(yc, axis=1, keepdims=True) + EPS)
        d[:, s] = np.sum(xc * yc, axis=1)
    out.update(stoi=float(d.mean()), segments=S)
    return out


def stoi(ref, inf):
    return stoi_stages(ref, inf)["stoi"]


def score(ref, inf):
    """The record gtcrn_score writes for one pair (float32 samples in, as the device reads them)."""
    ref = np.asarray(ref, np.float32)
    inf = np.asarray(inf, np.float32)
    st = stoi_stages(ref, inf)
    return dict(sdr=float(sdr(ref, inf)), sisnr=float(sisnr(ref, inf)), stoi=st["stoi"], kept_frames=st["kept_frames"],
                segments=st["segments"], stages=st)
