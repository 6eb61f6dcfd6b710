"""An independent numpy restatement of the G.711 contract of include/gtcrn_micro_hip.h ("G.711 payloads"), by another route
than the library's: the decode tables straight from the formulas, the encoders by a search over the sorted decision
thresholds of the magnitude (np.searchsorted) -- no leading-bit count anywhere.  law 0: mu-law, law 1: A-law; everything on
the 16-bit linear scale of the PCM16 forms.  Used by tests/test_g711_host.py and tests/test_gpu_g711.py."""
import numpy as np

LAWS = (0, 1)
NAMES = {0: "ulaw", 1: "alaw"}
ZERO_CODE = {0: 0xFF, 1: 0xD5}          # what a structural zero leaves as


def decode_table(law):
    """D_law as int16[256]."""
    c = np.arange(256, dtype=np.int64)
    if law == 0:
        u = ~c & 0xFF
        e, m = (u >> 4) & 7, u & 15
        mag = (((m << 3) + 132) << e) - 132
        return np.where(u & 0x80, -mag, mag).astype(np.int16)
    a = c ^ 0x55
    m, s = a & 15, (a >> 4) & 7
    t = np.where(s == 0, (m << 4) + 8, ((m << 4) + 264) << np.maximum(s - 1, 0))
    return np.where(a & 0x80, t, -t).astype(np.int16)


def thresholds(law):
    """T[k], k = segment * 16 + mantissa in 0..127: the smallest magnitude that encodes to index k (ascending).
    mu-law, on a = min(|p|, 32635) + 132: index k holds a in [(16 + m) << (e + 3), (17 + m) << (e + 3)), so on |p| the lower
    edge is ((16 + m) << (e + 3)) - 132.  A-law, on g = p or ~p: q = g >> 3 is in [2 m, 2 m + 2) for s = 0 (g from 16 m),
    q >> 1 == 16 + m for s = 1 (g from 16 (16 + m)), q >> s == 16 + m above (g from (16 + m) << (s + 3))."""
    k = np.arange(128, dtype=np.int64)
    seg, m = k >> 4, k & 15
    if law == 0:
        return ((16 + m) << (seg + 3)) - 132
    return np.where(seg == 0, 16 * m, (16 + m) << (np.maximum(seg, 1) + 3))


def encode(law, p):
    """E_law of int values p in -32768 .. 32767 (any shape) -> uint8."""
    p = np.asarray(p, dtype=np.int64)
    assert p.size == 0 or (p.min() >= -32768 and p.max() <= 32767)
    T = thresholds(law)
    assert (np.diff(T) > 0).all()
    if law == 0:
        mag = np.minimum(np.abs(p), 32635)
        k = np.searchsorted(T, mag, side="right") - 1
        return (~(np.where(p < 0, 0x80, 0) | k) & 0xFF).astype(np.uint8)
    g = np.where(p >= 0, p, -p - 1)                    # ~p without a bit operation
    k = np.searchsorted(T, g, side="right") - 1
    return ((np.where(p >= 0, 0x80, 0) | k) ^ 0x55).astype(np.uint8)


def pcm16(y):
    """The PCM16 rounding of float32 values: clip(rint(y * 32768), -32768, 32767), half to even (np.rint)."""
    y = np.asarray(y, dtype=np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        return np.clip(np.rint(y * np.float32(32768.0)), -32768.0, 32767.0).astype(np.int64)
