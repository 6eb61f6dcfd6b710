"""Checker of the high band on the packet forms (include/gtcrn_micro_hip.h, "high band on the packet forms"): the two fp32
mixes in numpy float32, one rounding per operation as the header states them, and the outbound stage in float64 through
tests/resample_checker.py (scipy.signal.resample_poly) -- code that shares nothing with the kernels.

For one stream, everything counted from the stream's own reset: A = the 16 kHz output of the inbound stage, P = the 16 kHz
sequence the outbound FIFO pops, x = the input at fs:
    s[t]   = fl(P[t] - fl(g A[t - L16]))                A[t < 0] = 0
    v      = causal outbound stage of s                 = the centred resampling of (d_out zeros ++ s), cut
    out[n] = fl(v[n] + fl(g x[n - LAT]))                x[n < 0] = 0, LAT = (L16 + d_in + d_out) fs / 16000
"""
import numpy as np

import highband_checker as HC
import resample_checker as RC


def live(A, P, x, gamma, L16, d_out, up, down, h, d_in=None):
    """A, P: (T,) float32 at 16 kHz; x: (T up / down,) float32 at fs; gamma: a float; L16 = 512 - gcd(n16, 256); d_out (and
    d_in, None: the same -- it is at 24, 32 and 48 kHz) the stages' delays in 16 kHz samples; up, down, h: gtcrn_resample_taps
    of 16000 -> fs.  Returns a dict: s (float32, exactly what the kernel stages), v (float64), dry (float32,
    fl(g x[n - LAT])), out (float64, v + dry: the last fp32 rounding is left to the caller's tolerance), bound (float64, per
    sample: the bound of tests/highband_checker.py -- the fp32 dot-product bound on the outbound stage plus two fp32 roundings
    of the mix), lat."""
    A, P, x = (np.asarray(t, np.float32) for t in (A, P, x))
    g = np.float32(gamma)
    assert A.ndim == P.ndim == x.ndim == 1 and A.size == P.size
    T = A.size
    assert (T * up) % down == 0 and x.size == T * up // down
    assert HC.geometry(up, down, h)[0] == d_out
    d_in = d_out if d_in is None else d_in
    lat16 = L16 + d_in + d_out
    assert (lat16 * up) % down == 0
    lat = lat16 * up // down
    ad = np.concatenate([np.zeros(L16, np.float32), A])[:T]
    ga = (g * ad).astype(np.float32)
    s = (P - ga).astype(np.float32)
    assert ga.dtype == np.float32 and s.dtype == np.float32
    fed = np.concatenate([np.zeros(d_out, np.float32), s])
    v = RC.resample64(fed, up, down, h)[:x.size]
    dot = RC.dot_bound(fed, up, down, h)[:x.size] * (1 + 2.0 ** -26)
    xd = np.concatenate([np.zeros(lat, np.float32), x])[:x.size]
    dry = (g * xd).astype(np.float32)
    out = v + dry.astype(np.float64)
    bound = dot + 2 * 2.0 ** -24 * (np.abs(v) + np.abs(dry.astype(np.float64)))
    return {"s": s, "v": v, "dry": dry, "out": out, "bound": bound, "lat": lat}
