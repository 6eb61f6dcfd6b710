"""CPU-side checks of the tone guard (include/gtcrn_micro_hip.h, "tone guard"): the ABI, the sizes that must not move, the
table, the parameter words, and the host twin gtcrn_tone_block_host (the functions the kernel compiles) against the contract
in numpy float32 (tests/tone_checker.py), bit for bit, on blocks built to take every branch; the comparison rejects six wrong
definitions.  Then the behaviour gate, on the checker with the defaults: what the detector must find and must leave alone."""
import ctypes
import math
import os

import numpy as np
import pytest

from conftest import ROOT
import tone_checker as TK

import __graft_entry__ as graft

F32 = np.float32
ERR_ARG = -1
BRANCHES = {"pair", "single", "singles_off", "none", "nonfinite", "argmax_tie", "run_continues", "run_broken_by_other",
            "guard_candidate", "guard_hold", "tone_kept_in_hold", "unguarded", "candidate_waits", "event", "event_continues",
            "reported", "pair_fails_floor_alone", "pair_fails_twist_alone", "pair_fails_dominance_alone",
            "pair_fails_purity_alone"}
TAB = TK.table()


@pytest.fixture(scope="module", autouse=True)
def _built():
    graft.build()


def host(params, rec, x):
    from gtcrn_micro_amd import tone_block
    return tone_block(params, TAB, rec, x)


def words(**kw):
    from gtcrn_micro_amd import tone_params
    return tone_params(**kw)


def tone(f, n=256, amp=0.1, start=0):
    return amp * np.sin(2 * np.pi * f * (start + np.arange(n)) / 16000.0)


def scenario(rng, K=40):
    """K blocks of one stream in segments of 1 .. 6 blocks: silence, noise, digits (clean, twisted, off frequency, noisy,
    with a second row tone, faint), 1100 / 2100 Hz, and blocks with a non-finite sample.  Digits may follow each other
    without a gap."""
    x = np.zeros(256 * K)
    k = 0
    while k < K:
        n = min(int(rng.integers(1, 7)), K - k)
        kind = rng.choice(["silence", "noise", "digit", "digit", "twisted", "off", "noisy", "two_rows", "faint", "single", "bad"])
        lo, ln = 256 * k + (int(rng.integers(0, 256)) if rng.random() < 0.3 and k + n < K else 0), 256 * n
        code = int(rng.integers(1, 17))
        if kind == "noise":
            x[lo:lo + ln] += 0.05 * rng.standard_normal(ln)
        elif kind in ("digit", "bad"):
            x[lo:lo + ln] += TK.dtmf(code, ln, 0)
        elif kind == "twisted":
            x[lo:lo + ln] += TK.dtmf(code, ln, 0, twist_db=float(rng.choice([-12, -6, 6, 12])))
        elif kind == "off":
            x[lo:lo + ln] += TK.dtmf(code, ln, 0, df=float(rng.choice([-0.035, -0.015, 0.015, 0.035])))
        elif kind == "noisy":
            x[lo:lo + ln] += TK.dtmf(code, ln, 0) + float(rng.choice([0.02, 0.08, 0.15])) * rng.standard_normal(ln)
        elif kind == "two_rows":
            x[lo:lo + ln] += TK.dtmf(code, ln, 0) + tone(TK.FREQS[(code // 4 + 1) % 4], ln, 0.06)
        elif kind == "faint":
            x[lo:lo + ln] += TK.dtmf(code, ln, 0, amp=float(rng.choice([0.003, 0.006])))
        elif kind == "single":
            n = min(n + 4, K - k)
            x[lo:256 * (k + n)] += tone(float(rng.choice([1100, 2100])), 256 * (k + n) - lo, 0.2)
        if kind == "bad":
            x[256 * k + int(rng.integers(256))] = rng.choice([np.nan, np.inf, -np.inf, 1e30])
        k += n
    with np.errstate(all="ignore"):
        return x.astype(np.float32).reshape(K, 256)


def random_params(rng):
    return words(guard_blocks=int(rng.choice([1, 2])), digit_blocks=int(rng.choice([1, 2, 3])), single_blocks=int(rng.choice([2, 4])),
                 hold_blocks=int(rng.choice([0, 1, 2])), mode=int(rng.random() > 0.2), singles=int(rng.random() > 0.25),
                 min_dbov=float(rng.choice([-45, -38])), pair_purity=float(rng.choice([0.6, 0.9])))


def run_both(params, xb, wrong=None, edge=False):
    """The host twin, block by block, against the checker; returns the traces and the blocks that differ.  edge: word 0 is
    set, per block, to the smaller of the correct e_r, e_c, so that the floor holds with equality."""
    rec_h = np.zeros(8, np.float32)
    rec_c, traces, differ = rec_h.copy(), [], []
    for k in range(len(xb)):
        p = np.array(params, np.float32)
        if edge:
            _, P = TK.powers(xb[k], TAB)
            if np.isfinite(P).all():
                p[0] = min(P[:4].max(), P[4:8].max()) * F32(0.0078125)
        rec_h, gh = host(p, rec_h, xb[k])
        rec_c, gc, tr = TK.block(p, TAB, rec_c, xb[k], wrong)
        traces.append(tr)
        if not TK.same_bits(rec_h, rec_c) or gh != gc:
            differ.append(k)
            rec_c = rec_h.copy()                                 # (go on from the same record: one bug, many blocks)
    return traces, differ


# ------------------------------------------------------------------------------------------------------ ABI, sizes, table, words
def test_symbols_sizes_and_header():
    from gtcrn_micro_amd import _lib
    L = _lib.lib()
    for name in ("gtcrn_wave_stream_set_tone", "gtcrn_tone_params_host", "gtcrn_tone_table_host", "gtcrn_tone_block_host"):
        assert hasattr(L, name), name
    assert _lib.Engine.wave_state_bytes() == 3088 and int(L.gtcrn_stream_state_bytes()) == 152464     # no state moved
    hdr = open(os.path.join(ROOT, "include", "gtcrn_micro_hip.h")).read()
    assert "#define GTCRN_ABI_VERSION 1" in hdr or "GTCRN_ABI_VERSION (1)" in hdr
    for decl in ("int gtcrn_wave_stream_set_tone(gtcrn_model *m, float *d_tone, const float *d_tone_params, const float *d_tone_table);",
                 "int gtcrn_tone_params_host(const gtcrn_tone_config *config, float *out16);",
                 "int gtcrn_tone_block_host(const float *params16, const float *table, float *record8, const float *x256, int *guard_out);",
                 "#define GTCRN_TONE_DEFAULTS {-45.0, 8.0, 8.0, 0.6, 0.8, 1, 2, 4, 1, 1, 1}"):
        assert decl in hdr, decl
    assert ctypes.sizeof(_lib.ToneConfig) == 5 * 8 + 6 * 4         # five doubles, six ints
    assert L.gtcrn_wave_stream_set_tone(None, None, None, None) == ERR_ARG      # a null model: no device is touched


def test_table_is_double_cos_sin_rounded_once():
    from gtcrn_micro_amd import tone_table
    t = tone_table()
    assert t.shape == (10, 256, 2) and t.dtype == np.float32
    assert TK.same_bits(t, TAB)
    assert t[:, 0, 0].tolist() == [1.0] * 10 and t[:, 0, 1].tolist() == [0.0] * 10
    f, i = 9, 200
    assert t[f, i, 0] == F32(math.cos(2 * math.pi * 2100 * i / 16000)) and t[f, i, 1] == F32(math.sin(2 * math.pi * 2100 * i / 16000))


def test_parameter_words_and_their_argument_errors():
    from gtcrn_micro_amd import _lib
    p = words()
    assert TK.same_bits(p, TK.params()) and not p[11:].any()
    assert p[3:11].tolist() == [F32(0.6), F32(0.8), 1, 2, 4, 1, 1, 1]
    q = words(min_dbov=0.0, twist_db=0.0, dominance_db=10.0, pair_purity=1.0, single_purity=0.5, guard_blocks=3, digit_blocks=0,
              single_blocks=7, hold_blocks=5, mode=0, singles=0)
    assert q[:11].tolist() == [256.0, 1.0, F32(0.1), 1.0, 0.5, 3, 0, 7, 5, 0, 0]
    assert words(min_dbov=-10.0)[0] == F32(25.6) and words(twist_db=10.0)[1] == 10.0
    for bad in (dict(min_dbov=math.nan), dict(twist_db=math.inf), dict(dominance_db=-math.inf), dict(pair_purity=0.0),
                dict(pair_purity=1.0001), dict(single_purity=-0.5), dict(single_purity=math.nan), dict(guard_blocks=-1),
                dict(digit_blocks=-2), dict(single_blocks=-1), dict(hold_blocks=-1), dict(mode=2), dict(mode=-1), dict(singles=2)):
        with pytest.raises(_lib.GtcrnError):
            words(**bad)
    with pytest.raises(_lib.GtcrnError):
        words(no_such_field=1)
    L, fp = _lib.lib(), ctypes.POINTER(ctypes.c_float)
    out = np.zeros(16, np.float32)
    assert L.gtcrn_tone_params_host(None, out.ctypes.data_as(fp)) == ERR_ARG
    assert L.gtcrn_tone_params_host(ctypes.byref(_lib.ToneConfig()), None) == ERR_ARG
    assert L.gtcrn_tone_table_host(None) == ERR_ARG
    assert L.gtcrn_tone_block_host(out.ctypes.data_as(fp), None, None, None, None) == ERR_ARG


# ------------------------------------------------------------------------------------------------------ checker == host twin
def test_host_twin_equals_the_checker_and_every_branch_occurs():
    rng = np.random.default_rng(71)
    seen, blocks = set(), 0
    for s in range(60):
        xb = scenario(rng)
        traces, differ = run_both(random_params(rng), xb)
        assert not differ, (s, differ)
        seen |= TK.seen(traces)
        blocks += len(xb)
    seen |= TK.seen(built_cases())
    assert BRANCHES <= seen, sorted(BRANCHES - seen)


def built_cases():
    """Blocks built for the branches chance does not reach: each failing condition of step 3 alone, and a tie in both argmaxes
    that decides the digit.  Each is compared with the host twin."""
    rng = np.random.default_rng(72)
    p = words()
    loud = TK.dtmf(6, 256, 0)
    cases = [("pair_fails_floor_alone", p, TK.dtmf(6, 256, 0, amp=0.004)),
             ("pair_fails_twist_alone", p, TK.dtmf(6, 256, 0, twist_db=12.0)),
             ("pair_fails_dominance_alone", p, loud + tone(697, 256, 0.06)),
             ("pair_fails_purity_alone", p, loud + 0.12 * rng.standard_normal(256))]
    impulse = np.zeros(256)
    impulse[0] = 2.0                                             # c_f = 2, s_f = 0 for every f: all ten powers are 4
    cases.append(("argmax_tie", words(dominance_db=0.0, pair_purity=0.01, singles=0), impulse))
    traces = []
    for name, pw, x in cases:
        x = x.astype(np.float32)
        rec_c, gc, tr = TK.block(pw, TAB, np.zeros(8, np.float32), x)
        rec_h, gh = host(pw, np.zeros(8, np.float32), x)
        assert TK.same_bits(rec_c, rec_h) and gc == gh, name
        assert name in tr, (name, sorted(tr))
        if name == "argmax_tie":
            assert rec_c[1] == 1, rec_c                          # the FIRST argmax of both groups: row 0, column 0
        traces.append(tr)
    return traces


def test_run_hold_and_report_sequences():
    """A digit broken by another digit, the hold counting down with `tone` kept, no new event on a continuing digit, a single
    tone that waits N1 blocks, singles off, and a non-finite block -- record by record, host twin included."""
    p = words(hold_blocks=2)
    x = np.concatenate([TK.dtmf(1, 768, 0), TK.dtmf(16, 768, 0), np.zeros(1024)]).astype(np.float32).reshape(-1, 256)
    recs, traces = TK.detect(p, TAB, x)
    assert recs[:, 1].tolist() == [1, 1, 1, 16, 16, 16, 0, 0, 0, 0]
    assert recs[:, 2].tolist() == [1, 2, 3, 1, 2, 3, 0, 0, 0, 0] and "run_broken_by_other" in traces[3]
    assert recs[:, 0].tolist() == [0, 1, 1, 1, 16, 16, 16, 16, 0, 0]      # reported after N2 = 2; kept through the hold
    assert recs[:, 3].tolist() == [2, 2, 2, 2, 2, 2, 1, 0, 0, 0] and recs[:, 4].tolist() == [1] * 8 + [0, 0]
    assert recs[:, 5].tolist() == [0, 1, 1, 1, 2, 2, 2, 2, 2, 2] and "event_continues" in traces[2]
    assert "tone_kept_in_hold" in traces[6] and "guard_hold" in traces[7]
    assert recs[-1, 6] == 8 and recs[-1, 7] == 10
    rec = np.zeros(8, np.float32)
    for k in range(len(x)):
        rec, g = host(p, rec, x[k])
        assert TK.same_bits(rec[:6], recs[k, :6]) and g == bool(recs[k, 4]) and not rec[6:].any(), k
    # a single tone: guarded and reported from its N1-th block on, not at all with singles off
    s = tone(2100, 256 * 6, 0.2).astype(np.float32)
    recs, traces = TK.detect(words(), TAB, s)
    assert recs[:, 0].tolist() == [0, 0, 0, 18, 18, 18] and recs[:, 4].tolist() == [0, 0, 0, 1, 1, 1] and recs[-1, 5] == 1
    assert "candidate_waits" in traces[0]
    recs, traces = TK.detect(words(singles=0), TAB, s)
    assert not recs[:, :6].any() and all("singles_off" in t for t in traces)
    # a non-finite sample: no candidate; the hold of the digit before it still runs, and the record stays finite
    x = np.concatenate([TK.dtmf(6, 512, 0), TK.dtmf(6, 256, 0), np.zeros(256)]).astype(np.float32).reshape(-1, 256)
    for bad in (np.nan, np.inf, -np.inf, 1e30):
        x[2, 77] = bad
        recs, traces = TK.detect(words(), TAB, x)
        assert "nonfinite" in traces[2] and recs[2, 1] == 0 and recs[2, 4] == 1 and recs[3, 4] == 0 and np.isfinite(recs).all()
        rec = np.zeros(8, np.float32)
        for k in range(4):
            rec, _ = host(words(), rec, x[k])
            assert TK.same_bits(rec[:6], recs[k, :6])


@pytest.mark.parametrize("wrong", TK.WRONG)
def test_the_comparison_rejects_a_wrong_definition(wrong):
    rng = np.random.default_rng(73)
    rejected = 0
    for s in range(30):
        xb = scenario(rng)
        _, differ = run_both(random_params(rng), xb, wrong=wrong, edge=wrong == "pairwise")
        rejected += len(differ)
    if wrong == "last_argmax":                                   # (a tie that decides needs equal powers: the impulse block)
        impulse = np.zeros((1, 256), np.float32)
        impulse[0, 0] = 2.0
        rejected += 5 * len(run_both(words(dominance_db=0.0, pair_purity=0.01), impulse, wrong=wrong)[1])
    assert rejected >= 5, (wrong, rejected)


def test_python_layer_asks_for_the_symbols_only_with_tones(monkeypatch):
    """An older library without the symbols: states without tones work as before, tones= raises GtcrnError."""
    from gtcrn_micro_amd import _lib
    real = _lib.lib()

    class Old:
        def __getattr__(self, name):
            if "tone" in name:
                raise AttributeError(name)
            return getattr(real, name)

    monkeypatch.setattr(_lib, "lib", lambda: Old())
    eng = _lib.Engine.__new__(_lib.Engine)
    st = _lib.WaveStreamState.__new__(_lib.WaveStreamState)
    st.tones = None
    eng._set_tones(st)                                           # nothing to clear, no error
    for call in (lambda: st._new_tones(True), lambda: _lib.tone_params(), lambda: _lib.tone_table(), lambda: st.tone()):
        with pytest.raises(_lib.GtcrnError):
            call()


def test_forms_of_the_constructor_argument():
    from gtcrn_micro_amd import _lib
    assert _lib._tone_fields("detect")["mode"] == 0 and _lib._tone_fields(True) == _lib.TONE_DEFAULTS
    assert _lib._tone_fields({"hold_blocks": 3})["hold_blocks"] == 3 and _lib.TONE_DEFAULTS == TK.DEFAULTS
    for bad in ("on", 1.5):
        with pytest.raises(_lib.GtcrnError):
            _lib._tone_fields(bad)
    assert not _lib._tones_on(None) and not _lib._tones_on(False) and _lib._tones_on(True) and _lib._tones_on("detect")
    assert _lib.TONE_FREQS == TK.FREQS


# ------------------------------------------------------------------------------------------------------ the behaviour gate
def digits_found(n, rng=None, snr_db=None, **kw):
    """All 16 digits of n samples at the 16 start offsets 0, 16, .., 240 within a block, amplitude 0.1 per tone, through the
    checker with the defaults -> (digits reported, wrong digits reported)."""
    p, found, wrong = TK.params(), 0, 0
    for code in range(1, 17):
        for off in range(0, 256, 16):
            total = 256 * (3 + -(-n // 256))
            x = TK.dtmf(code, n, 256 + off, total=total, **kw)
            if snr_db is not None:                               # white noise under the whole buffer; the digit's power is 0.01
                x = x + math.sqrt(0.01 / 10 ** (snr_db / 10)) * rng.standard_normal(total)
            recs, _ = TK.detect(p, TAB, x.astype(np.float32))
            codes = TK.reported_codes(recs)
            found += code in codes
            wrong += any(c != code for c in codes)
    return found, wrong


def test_40_ms_digits_are_all_reported():
    rng = np.random.default_rng(74)
    assert digits_found(640) == (256, 0)
    for df in (-0.015, 0.015):
        assert digits_found(640, df=df) == (256, 0), df
    for tw in (-6.0, 6.0):
        assert digits_found(640, twist_db=tw) == (256, 0), tw
    assert digits_found(640, rng, snr_db=15.0) == (256, 0)


def test_digits_off_by_3_5_percent_are_not_reported():
    for df in (-0.035, 0.035):
        assert digits_found(640, df=df) == (0, 0), df


def test_fax_tones_of_a_quarter_second_are_reported():
    for f, code in ((1100, 17), (2100, 18)):
        for off in (0, 100, 200):
            x = np.zeros(256 * 19)
            x[256 + off:256 + off + 4000] = tone(f, 4000, 0.1)
            recs, _ = TK.detect(TK.params(), TAB, x.astype(np.float32))
            assert TK.reported_codes(recs) == [code], (f, off)


def test_noisy_speech_raises_no_event():
    """The five noisy rows of tests/golden/examples_full.npz, 1 937 blocks each: no event, and at most 1 % of the blocks
    guarded."""
    noisy = np.load(os.path.join(ROOT, "tests", "golden", "examples_full.npz"))["noisy"]
    assert noisy.shape[0] == 5
    for row in noisy:
        x = (row[:256 * (len(row) // 256)].astype(np.float32) / F32(32768)).astype(np.float32)
        recs, _ = TK.detect(TK.params(), TAB, x)
        assert len(recs) == 1937
        assert recs[-1, 5] == 0, recs[-1]
        assert recs[-1, 6] <= 0.01 * len(recs), recs[-1]
