"""CPU-side checks of the level control (include/gtcrn_micro_hip.h, "level control"): the ABI, the sizes that must not move,
the parameter words, and the host twin gtcrn_alc_block_host (the functions the kernel compiles) against the contract in numpy
float32 (tests/alc_checker.py), bit for bit, on blocks built to take every branch; the comparison rejects five wrong
definitions; the invariants hold over 10 000 random blocks."""
import ctypes
import math
import os
import re

import numpy as np
import pytest

from conftest import ROOT
import alc_checker as AK
import ramp_checker as RK

import __graft_entry__ as graft

F32 = np.float32
ERR_ARG = -1
BRANCHES = {"nonfinite", "speech", "hangover", "hangover_ends", "silence", "first_estimate", "smoothed", "clamp_a_min",
            "clamp_a_max", "inside_range", "fall_limited", "rise_limited", "reached", "pk_zero", "limiter_at_a_min", "limited",
            "limited_both", "limited_start_only", "unlimited", "tie_theta", "tie_ratio", "mode0"}


@pytest.fixture(scope="module", autouse=True)
def _built():
    graft.build()


def host(params, rec, w, x, m):
    from gtcrn_micro_amd import alc_block
    return alc_block(params, rec, w, x, m)


def words(**kw):
    from gtcrn_micro_amd import alc_params
    return alc_params(**kw)


def random_params(rng):
    """Parameter words that move fast enough for every branch to be met inside a few blocks."""
    return words(target_dbov=rng.uniform(-50, -5), min_gain_db=-rng.uniform(0, 20), max_gain_db=rng.uniform(0, 30),
                 rise_db_s=rng.choice([0, 6, 100, 900]), fall_db_s=rng.choice([0, 30, 300, 2000]),
                 ceiling_dbov=rng.uniform(-30, 0), floor_dbov=rng.uniform(-70, -20), ratio_db=rng.uniform(-20, 3),
                 hang_ms=rng.choice([0, 16, 32, 50]), alpha=rng.choice([0, 1 / 16, 0.5, 1]), mode=int(rng.random() > 0.1))


def blocks(rng, K):
    """K blocks of one stream: w and x of independent seeded noise at amplitudes from exact zeros to loud, m the mix at a
    random dry gain or w itself."""
    aw = rng.choice([0.0, 1e-3, 0.03, 0.3, 1.0], K)
    ax = rng.choice([0.0, 1e-3, 0.03, 0.3, 3.0], K)
    w = (rng.standard_normal((K, 256)) * aw[:, None]).astype(np.float32)
    x = (rng.standard_normal((K, 256)) * ax[:, None]).astype(np.float32)
    g = rng.choice([0.0, 0.0, 0.25, 1.0], K).astype(np.float32)
    m = np.stack([w[k] if g[k] == 0 else RK.mix(g[k], x[k], w[k]) for k in range(K)])
    return w, x, m


def poison(rng, w, x, m):
    """NaN, +-Inf and a value whose square overflows, in w, in x and in both (m follows: it is made from them)."""
    bad = [np.nan, np.inf, -np.inf, 1e30]
    for i, k in enumerate(range(3, len(w), 5)):
        v, where = F32(bad[i % 4]), (i // 4) % 3
        if where in (0, 2):
            w[k, rng.integers(256)] = v
            m[k] = w[k]
        if where in (1, 2):
            x[k, rng.integers(256)] = v
    return w, x, m


def run_both(params, w, x, m, wrong=None, record=None):
    """The host twin, block by block, against the checker; returns the traces and the blocks that differ."""
    rec_h = AK.INIT.copy() if record is None else np.array(record, np.float32)
    rec_c, traces, differ, prev = rec_h.copy(), [], [], None
    for k in range(len(w)):
        yh, rec_h = host(params, rec_h, w[k], x[k], m[k])
        yc, rec_c, tr, prev = AK.block(params, rec_c, w[k], x[k], m[k], wrong, prev)
        traces.append(tr)
        if not (AK.same_bits(yh, yc) and AK.same_bits(rec_h, rec_c)):
            differ.append(k)
            rec_c = rec_h.copy()                          # (go on from the twin's record: later blocks are compared on their own)
    return traces, differ


def tie_cases():
    """E_w == theta and E_w == fl(rho E_x), built from the checker's own sums."""
    rng = np.random.default_rng(77)
    w = (rng.standard_normal((1, 256)) * 0.1).astype(np.float32)
    p = words(hang_ms=32)
    p[0] = AK.hop_sum(w[0])
    yield p, w, np.zeros_like(w), w
    p = words(hang_ms=32, ratio_db=0)
    assert p[1] == 1.0
    yield p, w, w.copy(), w


def test_symbols_exported_and_declared_and_abi_version():
    L = ctypes.CDLL(os.path.join(ROOT, "gtcrn_micro_amd", "libgtcrn_micro_hip.so"))
    with open(os.path.join(ROOT, "include", "gtcrn_micro_hip.h")) as f:
        header = f.read()
    for n in ("gtcrn_wave_stream_set_alc", "gtcrn_alc_params_host", "gtcrn_alc_block_host"):
        assert hasattr(L, n), n
        assert re.search(r"\bint\s+%s\s*\(" % n, header), n
    assert "level control:" in header and "gtcrn_alc_config" in header
    assert re.search(r"#define\s+GTCRN_ABI_VERSION\s+1\b", header)
    assert L.gtcrn_abi_version() == 1


def test_state_sizes_unchanged():
    """The record and the parameter words are no part of any state: the values of tests/test_gain_ramp_host.py."""
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


def test_the_timing_list_is_what_it_was():
    """A launch with level control is timed in the row of the form it stands in for, as a ramped launch is."""
    from gtcrn_micro_amd import Engine
    names = Engine.kernel_names()
    assert names[-1] == "k_wave_synthesis_meter" and not any("alc" in n for n in names)


def test_parameter_words_on_exact_cases():
    d = words()
    f = lambda v: F32(v)
    assert d.dtype == np.float32 and d.shape == (16,) and not d[11:].any()
    assert d[0] == f(256 * 10 ** -4.5) and d[1] == f(10 ** -1.0) and d[2] == 13.0 and d[3] == 0.0625
    assert d[4] == f(256 * 10 ** -2.6) and d[5] == f(10 ** (-6 / 20)) and d[6] == f(10 ** (24 / 20))
    assert d[7] == f(10 ** (6 * 0.016 / 20)) and d[8] == f(10 ** (-30 * 0.016 / 20)) and d[9] == f(10 ** (-1 / 20))
    assert d[10] == 1.0 and words(mode=0)[10] == 0.0
    p = words(target_dbov=0, min_gain_db=0, max_gain_db=0, rise_db_s=0, fall_db_s=0, ceiling_dbov=0, floor_dbov=0, ratio_db=0,
              hang_ms=0, alpha=1)
    assert p[:11].tolist() == [256, 1, 0, 1, 256, 1, 1, 1, 1, 1, 1]
    assert [words(hang_ms=h)[2] for h in (0, 1, 16, 16.5, 32, 200)] == [0, 1, 1, 2, 2, 13]
    # the clamps: theta >= 1e-30, 0 < a_min <= 1 <= a_max
    assert words(floor_dbov=-400)[0] == F32(1e-30)
    assert words(min_gain_db=3, max_gain_db=5)[5] == 1.0 and words(min_gain_db=-9, max_gain_db=-3)[6] == 1.0
    assert 0 < words(min_gain_db=-2000)[5] <= np.finfo(np.float32).tiny


@pytest.mark.parametrize("bad", [dict(alpha=-0.1), dict(alpha=1.5), dict(min_gain_db=3, max_gain_db=2), dict(rise_db_s=-1),
                                 dict(fall_db_s=-1), dict(hang_ms=-1), dict(mode=2), dict(target_dbov=math.nan),
                                 dict(ceiling_dbov=math.inf), dict(floor_dbov=-math.inf), dict(hang_ms=1e12)])
def test_parameter_argument_errors(bad):
    from gtcrn_micro_amd import GtcrnError
    with pytest.raises(GtcrnError):
        words(**bad)


def test_null_pointers_are_argument_errors():
    from gtcrn_micro_amd import _lib, GtcrnError
    L = _lib.lib()
    fp = ctypes.POINTER(ctypes.c_float)
    buf = (ctypes.c_float * 256)()
    assert L.gtcrn_alc_params_host(None, ctypes.cast(buf, fp)) == ERR_ARG
    assert L.gtcrn_alc_params_host(ctypes.byref(_lib.AlcConfig()), None) == ERR_ARG
    assert L.gtcrn_alc_block_host(None, None, None, None, None, None) == ERR_ARG
    assert L.gtcrn_wave_stream_set_alc(None, None, None) == ERR_ARG and b"null" in L.gtcrn_last_error()
    with pytest.raises(GtcrnError):
        words(treshold=3)


def test_host_twin_equals_the_checker_and_every_branch_is_taken():
    rng = np.random.default_rng(31)
    taken = set()
    for s in range(60):
        p = random_params(rng)
        w, x, m = blocks(rng, 24)
        if s % 3 == 0:
            w, x, m = poison(rng, w, x, m)
        traces, differ = run_both(p, w, x, m)
        assert not differ, (s, differ, traces[differ[0]])
        taken |= AK.seen(traces)
    for p, w, x, m in tie_cases():
        traces, differ = run_both(p, w, x, m)
        assert not differ
        taken |= AK.seen(traces)
    assert BRANCHES <= taken, sorted(BRANCHES - taken)


def nonfinite_cases():
    """The twelve combinations of step 3: a NaN, +Inf, -Inf and a finite value whose square overflows (1e30), in w alone, in x
    alone and in both.  m is w (no gains), so a poisoned x alone leaves w, m and pk finite: E_x is then the only evidence.
    Yields (label, w, x, m, the trace tags the block must carry)."""
    rng = np.random.default_rng(78)
    kinds = {"nan": (np.nan, "_nan"), "+inf": (np.inf, "_inf"), "-inf": (-np.inf, "_inf"), "overflow": (1e30, "_inf")}
    for kind, (v, tag) in kinds.items():
        for where in ("w", "x", "both"):
            w = (rng.standard_normal(256) * 0.1).astype(np.float32)
            x = (rng.standard_normal(256) * 0.1).astype(np.float32)
            tags = set()
            if where in ("w", "both"):
                w[rng.integers(256)] = v
                tags.add("Ew" + tag)
                if kind in ("+inf", "-inf"):
                    tags.add("pk_inf")                    # (max |m| drops a NaN and keeps 1e30, whose square is what overflows)
            if where in ("x", "both"):
                x[rng.integers(256)] = v
                tags.add("Ex" + tag)
            yield kind + " in " + where, w, x, w.copy(), tags


def test_every_non_finite_case_holds_the_record_bit_for_bit():
    """Step 3 on each of the twelve combinations, host twin against checker: y = fl(a m), voice = 0, blocks + 1, and a, S,
    hang and voiced exactly as they were; the block after it moves the record again.  The trace says which of E_w, E_x, pk
    was non-finite and of what kind, so the twelve are told apart."""
    p = words(hang_ms=48, floor_dbov=-40, rise_db_s=300, target_dbov=-10)
    rng = np.random.default_rng(79)
    good = (rng.standard_normal((3, 256)) * 0.1).astype(np.float32)
    taken = {}
    for mode in (1, 0):
        p[10] = mode
        for label, w, x, m, tags in nonfinite_cases():
            rec = AK.INIT.copy()
            for k in range(2):                                    # two speech blocks: S, hang and a gain off 1 to hold
                _, rec = host(p, rec, good[k], good[k], good[k])
            assert rec[1] > 0 and rec[2] == 3 and rec[3] == 1 and (rec[0] != 1 or mode == 0), label
            yh, rh = host(p, rec, w, x, m)
            yc, rc, tr, _ = AK.block(p, rec, w, x, m)
            assert AK.same_bits(yh, yc) and AK.same_bits(rh, rc), label
            assert "nonfinite" in tr and {t for t in tr if t[:2] in ("Ew", "Ex", "pk")} == tags, (label, sorted(tr))
            assert AK.same_bits(rh[:3], rec[:3]) and rh[3] == 0 and rh[4] == rec[4] and rh[5] == rec[5] + 1, (label, rh)
            with np.errstate(all="ignore"):
                assert AK.same_bits(yh, (rec[0] * m).astype(np.float32)), label
            if "x" in label.split()[-1] and "w" not in label:
                assert np.isfinite(w).all() and np.isfinite(m).all() and np.isfinite(yh).all(), label
            _, after = host(p, rh, good[2], good[2], good[2])
            assert after[3] == 1 and after[4] == rh[4] + 1 and not AK.same_bits(after[1:2], rh[1:2]), label
            taken[(mode, label)] = tr
    assert len(taken) == 24 and len({label for _, label in taken}) == 12
    assert {frozenset(t - {"nonfinite", "mode0"}) for t in taken.values()} >= {
        frozenset(s) for s in ({"Ew_nan"}, {"Ex_nan"}, {"Ew_nan", "Ex_nan"}, {"Ew_inf", "pk_inf"}, {"Ex_inf"},
                               {"Ew_inf", "pk_inf", "Ex_inf"}, {"Ew_inf"}, {"Ew_inf", "Ex_inf"})}


def test_hangover_counts_down_and_the_gain_waits():
    """H = 2: speech, two hangover blocks that keep voice and leave S alone, then silence with the gain held."""
    rng = np.random.default_rng(5)
    p = words(hang_ms=32, floor_dbov=-40, rise_db_s=100)
    loud = (rng.standard_normal((1, 256)) * 0.02).astype(np.float32)        # -34 dBov: above the floor, below the target
    w = np.concatenate([loud, np.zeros((4, 256), np.float32)])
    y, recs, traces = AK.stream(p, w, np.zeros_like(w), w, first_block_index=1)
    assert [sorted(t & {"speech", "hangover", "silence"}) for t in traces] == [["speech"], ["hangover"], ["hangover"],
                                                                                ["silence"], ["silence"]]
    assert recs[:, 3].tolist() == [1, 1, 1, 0, 0] and recs[:, 2].tolist() == [2, 1, 0, 0, 0] and recs[-1, 4] == 3
    assert len(set(recs[:, 1].tolist())) == 1 and recs[0, 1] == AK.hop_sum(loud[0])
    assert recs[0, 0] < recs[1, 0] < recs[2, 0] == recs[3, 0] == recs[4, 0]      # moves while voiced, not in the pause
    rec = AK.INIT.copy()
    for k in range(5):
        yh, rec = host(p, rec, w[k], w[k] * 0, w[k])
        assert AK.same_bits(rec, recs[k]) and AK.same_bits(yh, y[k]), k


@pytest.mark.parametrize("wrong", AK.WRONG)
def test_the_comparison_rejects_a_wrong_definition(wrong):
    rng = np.random.default_rng(32)
    rejected = 0
    for s in range(40):
        p = random_params(rng)
        w, x, m = blocks(rng, 24)
        _, differ = run_both(p, w, x, m, wrong=wrong)
        rejected += len(differ)
    assert rejected >= 5, (wrong, rejected)


def test_invariants_over_random_blocks():
    """a in [a_min, a_max], S finite and >= 0, the counts as stated; mode 0 gives y == m bit for bit."""
    rng = np.random.default_rng(33)
    n = 0
    for s in range(100):
        p = random_params(rng)
        p0 = p.copy()
        p0[10] = 0
        w, x, m = poison(rng, *blocks(rng, 100))
        rec, rec0 = AK.INIT.copy(), AK.INIT.copy()
        for k in range(100):
            before = rec.copy()
            y, rec = host(p, rec, w[k], x[k], m[k])
            y0, rec0 = host(p0, rec0, w[k], x[k], m[k])
            assert AK.same_bits(y0, m[k]) and rec0[0] == 1.0, (s, k)
            assert p[5] <= rec[0] <= p[6] and np.isfinite(rec[1]) and rec[1] >= 0, (s, k, rec)
            assert rec[3] in (0.0, 1.0) and rec[5] == before[5] + 1 and rec[4] == before[4] + rec[3] and not rec[6:].any()
            assert 0 <= rec[2] <= p[2] or rec[2] == before[2], (s, k)
            n += 1
    assert n == 10000


def test_python_layer_asks_for_the_symbols_only_with_alc(monkeypatch):
    """An older library without the symbols: states without level control work as before, alc= raises GtcrnError."""
    from gtcrn_micro_amd import _lib
    real = _lib.lib()

    class Old:
        def __getattr__(self, name):
            if name in ("gtcrn_wave_stream_set_alc", "gtcrn_alc_params_host", "gtcrn_alc_block_host"):
                raise AttributeError(name)
            return getattr(real, name)

    monkeypatch.setattr(_lib, "lib", lambda: Old())
    eng = _lib.Engine.__new__(_lib.Engine)
    st = _lib.WaveStreamState.__new__(_lib.WaveStreamState)
    st.alc = None
    eng._set_alc(st)                                             # nothing to clear, no error
    for call in (lambda: st._new_alc(True), lambda: _lib.alc_params(), lambda: st.voice()):
        with pytest.raises(_lib.GtcrnError):
            call()


def test_alc_forms_of_the_constructor_argument():
    from gtcrn_micro_amd import _lib
    assert _lib._alc_fields("vad")["mode"] == 0 and _lib._alc_fields(True) == _lib.ALC_DEFAULTS
    assert _lib._alc_fields({"hang_ms": 32})["hang_ms"] == 32
    for bad in ("on", 1.5):
        with pytest.raises(_lib.GtcrnError):
            _lib._alc_fields(bad)
    with pytest.raises(_lib.GtcrnError):
        _lib._alc_without_highband(True, 0.5)
    # None and False are off, as meters=False and ramp=False are
    assert not _lib._alc_on(None) and not _lib._alc_on(False) and _lib._alc_on(True) and _lib._alc_on("vad") and _lib._alc_on({})
    _lib._alc_without_highband(False, 0.5)
    _lib._alc_without_highband(None, 0.5)
