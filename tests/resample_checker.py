"""Float64 checker of the sample-rate conversion (include/gtcrn_micro_hip.h, gtcrn_resample): the filter's definition in
numpy and the conversion itself through scipy.signal.resample_poly -- code that shares nothing with the kernels."""
from math import gcd

import numpy as np
from scipy.signal import resample_poly

OTHER_RATES = (8000, 11025, 22050, 24000, 32000, 44100, 48000)
PAIRS = [(r, 16000) for r in OTHER_RATES] + [(16000, r) for r in OTHER_RATES]
LIVE_RATES = (8000, 24000, 32000, 48000)
BETA = 8.95926            # 0.1102 (A - 8.7), A = 90 dB


def ratio(fs_in, fs_out):
    g = gcd(fs_in, fs_out)
    return fs_out // g, fs_in // g


def design(fs_in, fs_out):
    """(up, down, half, h): the taps in float64, sum(h) == up."""
    up, down = ratio(fs_in, fs_out)
    q = max(up, down)
    half = 32 * q
    n = np.arange(-half, half + 1, dtype=np.float64)
    fc = 0.9375 * 0.5 / q
    h = np.sinc(2 * fc * n) * np.kaiser(2 * half + 1, BETA)
    return up, down, half, h * (up / h.sum())


def out_len(L, up, down):
    return -(-L * up // down)


def resample64(x, up, down, h):
    """y[j] = sum_i x[i] h[j down - i up + half], zero padding, centred; float64 along the last axis.  scipy multiplies
    the window it is given by `up` itself."""
    x = np.asarray(x, np.float64)
    return resample_poly(x, up, down, axis=-1, window=np.asarray(h, np.float64) / up)


def dot_bound(x, up, down, h):
    """Per output sample: (n + 1) 2^-24 sum |x_i| |h_k| over the n products of that sample -- the classic bound on an
    fp32 dot product of n terms (any summation order), in float64."""
    ax = np.abs(np.asarray(x, np.float64))
    ah = np.abs(np.asarray(h, np.float64))
    s = resample_poly(ax, up, down, axis=-1, window=ah / up)
    n = (len(h) - 1) // up + 1
    return (n + 1) * 2.0 ** -24 * s


def response_db(h, up, freqs, fs_grid):
    """|H(f)| / up in dB at `freqs` (Hz), the taps living on the fs_grid = fs_in * up sample grid."""
    h = np.asarray(h, np.float64)
    n = np.arange(len(h)) - (len(h) - 1) / 2
    H = np.array([np.sum(h * np.cos(2 * np.pi * f / fs_grid * n)) for f in freqs])      # symmetric taps: real response
    return 20 * np.log10(np.maximum(np.abs(H) / up, 1e-300))
