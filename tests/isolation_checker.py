"""Helpers of the isolation tests (tests/test_isolation_host.py, tests/test_gpu_isolation.py): one non-finite element in one
stream must change no bit of another stream, and the victim itself must heal once the poison has left the model's
receptive field.  Nothing here touches a GPU; the comparisons take numpy arrays or torch tensors (CPU or device) alike."""
import numpy as np

# The model is a FIR in time.  kernels.hip's time spans recompute HALO_BLOCKS = 12 frames of the encoder / decoder blocks'
# history and HALO_GTCN = 30 frames of the two GTCN stacks' (2 stacks x dilations 1 + 2 + 4 + 8, two taps back each) --
# so a frame reaches the 1 + 2 * 12 + 2 * 30 frames that start with it and no other.  tests/test_isolation_host.py pins the
# number against the float64 port before any GPU test relies on it.
HALO_BLOCKS = 12
HALO_GTCN = 30
CONE = 1 + 2 * HALO_BLOCKS + 2 * HALO_GTCN
assert CONE == 85
RING = 16          # rows of the deepest state ring (the dilation-8 TCN block keeps 2 * 8 frames)
NBINS = 257
HOP = 256

QNAN = float(np.float32(np.nan))
PINF = float("inf")
HUGE = 1e30        # finite, but its square overflows fp32
POISONS = {"nan": QNAN, "inf": PINF, "1e30": HUGE}


def _np(a):
    if isinstance(a, np.ndarray):
        return a
    return a.detach().cpu().numpy()


def _bits(a):
    a = np.ascontiguousarray(_np(a))
    assert a.dtype.kind in "fiu" and a.dtype.itemsize in (4, 8), a.dtype
    return a.view(np.int32 if a.dtype.itemsize == 4 else np.int64)


def same_bits(a, b):
    """True when a and b have one shape and every element the same bit pattern (the int32 views are equal; int64 for the
    float64 reference).  A NaN equals only the NaN with its payload; +0 differs from -0."""
    a, b = _np(a), _np(b)
    return a.shape == b.shape and a.dtype == b.dtype and bool(np.array_equal(_bits(a), _bits(b)))


def same_bits_or_both_nonfinite(a, b):
    """same_bits, except where BOTH elements are non-finite: two forms of one arithmetic may produce a NaN where the other
    has an Inf, or NaNs of different payloads, and only there."""
    a, b = _np(a), _np(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    ok = (_bits(a) == _bits(b)) | (~np.isfinite(a) & ~np.isfinite(b))
    return bool(ok.all())


def nonfinite_frames(x, axis=-1, block=None):
    """The frames of `x` that hold a non-finite value: {frame index: True when EVERY element of it is non-finite}.
    x (..., T, ...) with the frames along `axis`; or, with block=256, a waveform (L,) cut into blocks of that many
    samples (a shorter last block counts as one)."""
    x = _np(x)
    if block is not None:
        assert x.ndim == 1
        n = -(-x.shape[0] // block)
        rows = [x[block * i:block * (i + 1)] for i in range(n)]
    else:
        x = np.moveaxis(x, axis, 0)
        rows = [x[i].ravel() for i in range(x.shape[0])]
    out = {}
    for i, r in enumerate(rows):
        bad = ~np.isfinite(r)
        if bad.any():
            out[i] = bool(bad.all())
    return out


def cone_frames(t0, T):
    """Spectrum level: the output frames a non-finite input frame t0 of a T-frame clip makes non-finite."""
    return set(range(t0, min(t0 + CONE, T)))


def cone_blocks(h, nblocks):
    """Wave level: the 256-sample output blocks a non-finite sample inside hop h (not on its first sample) makes non-finite.
    The sample lies in STFT frames h and h + 1; their cones are frames h .. h + CONE; frame t is overlap-added into blocks
    t - 1 and t: blocks h - 1 .. h + CONE, 87 of them, clipped to the clip."""
    return set(range(max(h - 1, 0), min(h + CONE + 1, nblocks)))


def resample_range(i0, up, down, half, n_out):
    """Output samples j of y[j] = sum_i x[i] h[j down - i up + half] that read input sample i0 when no tap is zero:
    |j down - i0 up| <= half, clipped to the n_out samples that exist."""
    lo = -((half - i0 * up) // down)                 # ceil((i0 up - half) / down)
    hi = (i0 * up + half) // down
    return max(lo, 0), min(hi, n_out - 1)
