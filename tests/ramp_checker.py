"""Checker of the gain ramps (include/gtcrn_micro_hip.h, "gain ramps"): the contract in numpy float32.

`ramp(p, g)` is the 256 dry gains of a block that ramps from p, where the stream's last emitted block ended, to g:
    beta_i = g                                   if p == g or i == 255
           = fl( p + fl( fl(g - p) * r_i ) )     otherwise,   r_i = (i + 1) / 256 (exact in float32)
every fl() one float32 rounding (numpy rounds each operation of float32 operands once: no fused multiply-add).

`ramped_stream` is what a stream emits, from the outputs of the PLAIN calls (which the other test files pin) and the delayed
inputs, exactly as tests/test_gpu_dry_gain.py builds `mix_np`: only the first block of a call ramps, a stream's block 0 is a
structural zero that does not ramp, and every call that names the stream leaves p = g."""
import numpy as np

F32 = np.float32
R = ((np.arange(256, dtype=np.float32) + F32(1)) * F32(1.0 / 256)).astype(np.float32)
assert (R.astype(np.float64) * 256 == np.arange(1, 257)).all()


def ramp(p, g):
    """beta_0..255, float32."""
    p, g = F32(p), F32(g)
    if p == g:
        return np.full(256, g, np.float32)
    with np.errstate(all="ignore"):
        d = F32(g - p)
        s = (d * R).astype(np.float32)
        b = (p + s).astype(np.float32)
    b[255] = g
    return b


def mix(beta, x, w):
    """The attenuation limit's formula: fl(fl(beta x) + fl(fl(1 - beta) w)), beta a scalar or one gain per sample."""
    beta, x, w = np.asarray(beta, np.float32), np.asarray(x, np.float32), np.asarray(w, np.float32)
    with np.errstate(all="ignore"):
        return ((beta * x).astype(np.float32) + ((F32(1) - beta).astype(np.float32) * w).astype(np.float32)).astype(np.float32)


def ramped_stream(w, x, gains_per_call, hops_per_call, first_block_index=0, p0=None):
    """One stream.  w (256 K,): the blocks the plain calls emitted; x (256 K,): the dry samples aligned with them (input hop
    k - 1 under block k; what lies under a structural zero block is not read).  Call c steps hops_per_call[c] hops (0: the
    stream is not named and nothing changes) with the dry gain gains_per_call[c]; the stream's first block here is its
    block first_block_index (0: a structural zero).  p0: the ramp word in front of the first call (None: that call's gain).
    Returns (y (256 K,) float32, the ramp word after every call)."""
    w, x = np.asarray(w, np.float32).reshape(-1), np.asarray(x, np.float32).reshape(-1)
    assert len(gains_per_call) == len(hops_per_call) and w.size == x.size == 256 * sum(hops_per_call)
    y = np.empty_like(w)
    p = F32(gains_per_call[0] if p0 is None else p0)
    k, words = 0, []
    for g, nh in zip(gains_per_call, hops_per_call):
        g = F32(g)
        for h in range(nh):
            sl = slice(256 * k, 256 * (k + 1))
            if first_block_index + k == 0:
                y[sl] = 0
            else:
                y[sl] = mix(ramp(p, g) if h == 0 else g, x[sl], w[sl])
            k += 1
        if nh:
            p = g
        words.append(p)
    return y, np.asarray(words, np.float32)


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return a.shape == b.shape and bool((a.view(np.uint32) == b.view(np.uint32)).all())
