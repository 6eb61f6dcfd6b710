"""Checker of the high band's live contract (include/gtcrn_micro_hip.h, "high band"): the two fp32 mixes in numpy float32,
one rounding per operation as the header states them, and the outbound stage in float64 through tests/resample_checker.py
(scipy.signal.resample_poly) -- code that shares nothing with the kernels.

For one stream after a reset, a = the 16 kHz hand-off of the inbound stage, w = what the wave step emitted for it, x = the
input at fs, all since the reset:
    s[k]   = fl(w[k] - fl(g a[k - 256]))                a[k < 0] = 0
    v      = causal outbound stage of s                 = the centred resampling of (half / up zeros ++ s), cut
    out[n] = fl(v[n] + fl(g x[n - LAT]))                x[n < 0] = 0, LAT = H + 2 D
"""
import numpy as np

import resample_checker as RC


def geometry(up, down, h):
    """(d16, D): the outbound stage's delay in 16 kHz samples and in samples at fs (up / down = fs / 16000)."""
    half = (len(h) - 1) // 2
    d16 = half // up
    assert d16 * up == half and (d16 * up) % down == 0
    return d16, d16 * up // down


def live(a, w, x, gamma, up, down, h):
    """a, w: (256 K,) float32; x: (H K,) float32, H = 256 up / down; gamma: a float; up, down, h: gtcrn_resample_taps of
    16000 -> fs.  Returns a dict: s (float32, exactly what the kernel stages), v (float64), dry (float32, fl(g x[n - LAT])),
    out (float64, v + dry: the last fp32 rounding is left to the caller's tolerance), bound (float64, per sample: the fp32
    dot-product bound of tests/test_gpu_resample.py on the outbound stage plus two fp32 roundings of the mix), lat."""
    a, w, x = (np.asarray(t, np.float32) for t in (a, w, x))
    g = np.float32(gamma)
    assert a.ndim == w.ndim == x.ndim == 1 and a.size == w.size and a.size % 256 == 0
    K = a.size // 256
    H = 256 * up // down
    assert H * down == 256 * up and x.size == H * K
    d16, D = geometry(up, down, h)
    lat = H + 2 * D
    ad = np.concatenate([np.zeros(256, np.float32), a])[:a.size]
    ga = (g * ad).astype(np.float32)
    s = (w - ga).astype(np.float32)
    assert ga.dtype == np.float32 and s.dtype == np.float32
    fed = np.concatenate([np.zeros(d16, np.float32), s])
    v = RC.resample64(fed, up, down, h)[:H * K]
    dot = RC.dot_bound(fed, up, down, h)[:H * K] * (1 + 2.0 ** -26)
    xd = np.concatenate([np.zeros(lat, np.float32), x])[:H * K]
    dry = (g * xd).astype(np.float32)
    out = v + dry.astype(np.float64)
    bound = dot + 2 * 2.0 ** -24 * (np.abs(v) + np.abs(dry.astype(np.float64)))
    return {"s": s, "v": v, "dry": dry, "out": out, "bound": bound, "lat": lat}
