"""CPU-side checks of the gain ramps (include/gtcrn_micro_hip.h, "gain ramps"): the ABI, the sizes that must not move, the
host twin gtcrn_gain_ramp_host (the function the kernel compiles) against the contract in numpy float32
(tests/ramp_checker.py), the formula's properties, and that the comparison rejects two wrong definitions."""
import ctypes
import os
import re

import numpy as np
import pytest

from conftest import ROOT
import ramp_checker as RK

import __graft_entry__ as graft

F32 = np.float32
ERR_ARG = -1
G6, G12 = F32(10.0 ** (-6 / 20)), F32(10.0 ** (-12 / 20))
TINY = F32(np.finfo(np.float32).tiny)
DEN = F32(1e-45)                                      # the smallest denormal
up = lambda v: np.nextafter(F32(v), F32(2))
down = lambda v: np.nextafter(F32(v), F32(-1))
FIXED = [(0, 1), (1, 0), (G6, G12), (G12, G6), (0, 0), (1, 1), (G6, G6), (0.3718, 0.3718),
         (0, DEN), (DEN, 0), (DEN, 1), (1, DEN), (TINY, 0), (0, TINY), (DEN, TINY), (F32(3) * DEN, F32(7) * DEN),
         (down(1), 1), (1, down(1)), (0.5, up(0.5)), (up(0.5), 0.5), (G6, up(G6)), (down(G12), G12), (DEN, F32(2) * DEN)]


@pytest.fixture(scope="module", autouse=True)
def _built():
    graft.build()


def pairs(seed=20, n=4000):
    rng = np.random.default_rng(seed)
    u = rng.random((n, 2)).astype(np.float32)
    u[: n // 4] = (10.0 ** (-rng.uniform(0, 40, (n // 4, 2)) / 20)).astype(np.float32)      # gains of 0..40 dB limits
    return [(F32(a), F32(b)) for a, b in FIXED] + [(a, b) for a, b in u]


def host(p, g):
    from gtcrn_micro_amd._lib import lib
    out = np.full(256, np.nan, np.float32)
    assert lib().gtcrn_gain_ramp_host(float(p), float(g), out.ctypes.data_as(ctypes.POINTER(ctypes.c_float))) == 0
    return out


def test_symbols_exported_and_declared_and_abi_version():
    L = ctypes.CDLL(os.path.join(ROOT, "gtcrn_micro_amd", "libgtcrn_micro_hip.so"))
    with open(os.path.join(ROOT, "include", "gtcrn_micro_hip.h")) as f:
        header = f.read()
    for n in ("gtcrn_wave_stream_set_gain_ramp", "gtcrn_gain_ramp_host"):
        assert hasattr(L, n), n
        assert re.search(r"\bint\s+%s\s*\(" % n, header), n
    assert "gain ramps:" in header
    assert re.search(r"#define\s+GTCRN_ABI_VERSION\s+1\b", header)
    assert L.gtcrn_abi_version() == 1


def test_state_sizes_unchanged():
    """The ramp word is not part of any state: the values of tests/test_dry_gain_host.py."""
    from gtcrn_micro_amd import _lib
    import resample_checker as RC
    L = _lib.lib()
    assert L.gtcrn_stream_state_bytes() == 4 * 38116
    assert L.gtcrn_wave_stream_state_bytes() == 4 * (512 + 256 + 4)
    ntp = lambda half, up_: (2 * half // up_ + 1 + 3) // 4 * 4
    for fs in (8000, 24000, 32000, 48000):
        u, _, half, _ = RC.design(fs, 16000)
        uo, _, halfo, _ = RC.design(16000, fs)
        assert _lib.rate_stream_state_bytes(fs) == 4 * (ntp(half, u) + ntp(halfo, uo)), fs
        assert _lib.packet_stream_state_bytes(fs, fs // 100) == 4 * (512 + ntp(half, u) + ntp(halfo, uo)), fs
    assert _lib.packet_stream_state_bytes(16000, 160) == 4 * 512


def test_host_twin_equals_the_checker_bit_for_bit():
    from gtcrn_micro_amd import gain_ramp
    for p, g in pairs():
        want = RK.ramp(p, g)
        assert RK.same_bits(host(p, g), want), (p, g)
    assert RK.same_bits(gain_ramp(0.0, 1.0), RK.ramp(0, 1))
    assert RK.same_bits(RK.ramp(0, 1), RK.R)                      # 0 -> 1 is r_i itself: 1/256 .. 1


def test_properties_of_the_formula():
    for p, g in pairs(seed=21):
        b = host(p, g)
        lo, hi = min(p, g), max(p, g)
        assert b[255] == g, (p, g)
        assert (b >= lo).all() and (b <= hi).all(), (p, g)
        d = np.diff(np.concatenate([[p], b]).astype(np.float64))
        assert (d >= 0).all() if g >= p else (d <= 0).all(), (p, g)
        if p == g:
            assert RK.same_bits(b, np.full(256, g, np.float32)), (p, g)
        else:
            with np.errstate(under="ignore"):
                step = F32(F32(g - p) * F32(1.0 / 256))
            assert b[0] == F32(p + step), (p, g)                  # the first step from p is (g - p) / 256


def wrong_r(p, g):
    """Seeded bug 1: r_i = i / 256 (the ramp starts AT p and never reaches g before the forced last sample)."""
    p, g = F32(p), F32(g)
    if p == g:
        return np.full(256, g, np.float32)
    r = (np.arange(256, dtype=np.float32) * F32(1.0 / 256)).astype(np.float32)
    b = (p + (F32(g - p) * r).astype(np.float32)).astype(np.float32)
    b[255] = g
    return b


def wrong_last(p, g):
    """Seeded bug 2: the last sample left to the lerp, fl(p + fl(g - p)), which is not g for every pair."""
    p, g = F32(p), F32(g)
    if p == g:
        return np.full(256, g, np.float32)
    return (p + (F32(g - p) * RK.R).astype(np.float32)).astype(np.float32)


@pytest.mark.parametrize("wrong", [wrong_r, wrong_last])
def test_the_comparison_rejects_a_wrong_definition(wrong):
    ps = pairs(seed=22)
    bad = [(p, g) for p, g in ps if not RK.same_bits(host(p, g), wrong(p, g))]
    assert bad, wrong.__name__
    if wrong is wrong_r:
        assert len(bad) == sum(1 for p, g in ps if p != g)        # every pair that ramps shows it
    else:
        assert all(F32(p + F32(g - p)) != g for p, g in bad)      # exactly the pairs whose lerp misses g


def test_checker_stream_ramps_only_the_first_block_of_a_call():
    rng = np.random.default_rng(5)
    w, x = rng.standard_normal(256 * 6).astype(np.float32), rng.standard_normal(256 * 6).astype(np.float32)
    y, words = RK.ramped_stream(w, x, [G6, G6, 1.0, 1.0], [2, 1, 2, 1])
    assert not y[:256].any() and words.tolist() == [G6, G6, 1.0, 1.0]
    assert RK.same_bits(y[256:768], RK.mix(G6, x[256:768], w[256:768]))
    assert RK.same_bits(y[768:1024], RK.mix(RK.ramp(G6, 1.0), x[768:1024], w[768:1024]))
    assert RK.same_bits(y[1024:], x[1024:])                       # at g = 1 behind the ramp: the dry samples
    # a call that does not name the stream keeps the word; the cut of hops into calls does not matter
    y2, words2 = RK.ramped_stream(w, x, [G6, G6, 0.5, G6, 1.0, 1.0, 1.0], [1, 1, 0, 1, 1, 1, 1])
    assert RK.same_bits(y, y2) and words2.tolist() == [G6, G6, G6, G6, 1.0, 1.0, 1.0]
    # a stream that is past its first block ramps from p0
    y3, _ = RK.ramped_stream(w[:256], x[:256], [0.0], [1], first_block_index=3, p0=1.0)
    assert RK.same_bits(y3, RK.mix(RK.ramp(1, 0), x[:256], w[:256]))


def test_null_handle_is_an_argument_error():
    from gtcrn_micro_amd._lib import lib
    L = lib()
    assert L.gtcrn_wave_stream_set_gain_ramp(None, ctypes.c_void_p(16)) == ERR_ARG
    assert b"null" in L.gtcrn_last_error()
    assert L.gtcrn_wave_stream_set_gain_ramp(None, None) == ERR_ARG
    assert L.gtcrn_gain_ramp_host(0.0, 1.0, None) == ERR_ARG


def test_python_layer_asks_for_the_symbol_only_with_ramp(monkeypatch):
    """An older library without the symbol: states without ramps work as before, ramp=True raises GtcrnError."""
    from gtcrn_micro_amd import _lib
    real = _lib.lib()

    class Old:
        def __getattr__(self, name):
            if name in ("gtcrn_wave_stream_set_gain_ramp", "gtcrn_gain_ramp_host"):
                raise AttributeError(name)
            return getattr(real, name)

    monkeypatch.setattr(_lib, "lib", lambda: Old())
    eng = _lib.Engine.__new__(_lib.Engine)
    st = _lib.WaveStreamState.__new__(_lib.WaveStreamState)
    st.gain_ramp = None
    eng._set_gain_ramp(st)                                       # nothing to clear, no error
    with pytest.raises(_lib.GtcrnError):
        st._new_gain_ramp()
    with pytest.raises(_lib.GtcrnError):
        _lib.gain_ramp(0.0, 1.0)
