"""CPU-side checks of the packet loss concealment (include/gtcrn_micro_hip.h, "packet loss concealment"): the ABI, the parameter
words and their refusals, and the host twins gtcrn_plc_rows_host / _pcm16_host / _g711_host (the functions the kernel compiles)
against the contract in numpy (tests/plc_checker.py), bit for bit, over the cases of tests/plc_cases.py; then what the cases
are named for, and the waveform error on the speech examples against zero fill."""
import ctypes
import json
import os
import re

import numpy as np
import pytest

from conftest import ROOT
import plc_checker as PK
import plc_cases as PC

import __graft_entry__ as graft

F = np.float32
ERR_ARG = -1
CASES = PC.all_cases()
NAMES = ("gtcrn_plc_params_host", "gtcrn_plc_rows", "gtcrn_plc_rows_pcm16", "gtcrn_plc_rows_g711", "gtcrn_plc_reset",
         "gtcrn_plc_rows_host", "gtcrn_plc_rows_pcm16_host", "gtcrn_plc_rows_g711_host")


@pytest.fixture(scope="module", autouse=True)
def _built():
    graft.build()


def host(x, lost, hist, rec, prm, slots, count, law):
    from gtcrn_micro_amd import plc_rows_host
    plc_rows_host(x, lost, hist, rec, prm, slots, count, law)


def test_symbols_exported_and_declared_and_abi_version():
    L = ctypes.CDLL(os.path.join(ROOT, "gtcrn_micro_amd", "libgtcrn_micro_hip.so"))
    with open(os.path.join(ROOT, "include", "gtcrn_micro_hip.h")) as f:
        header = f.read()
    from gtcrn_micro_amd import _lib
    for n in NAMES:
        assert hasattr(L, n), n
        assert re.search(r"\bint\s+%s\s*\(" % n, header), n
        assert getattr(_lib.lib(), n).argtypes, n
    assert "packet loss concealment --" in header and "gtcrn_plc_config" in header and "GTCRN_PLC_DEFAULTS" in header
    assert re.search(r"#define\s+GTCRN_PLC_MAX_HISTORY\s+1680\b", header)
    assert re.search(r"#define\s+GTCRN_ABI_VERSION\s+1\b", header)
    assert L.gtcrn_abi_version() == 1
    import gtcrn_micro_amd
    assert all(hasattr(gtcrn_micro_amd, n) and n in gtcrn_micro_amd.__all__ for n in ("Concealer", "plc_params", "plc_rows_host"))


def test_params_words_and_refusals():
    from gtcrn_micro_amd import GtcrnError, _lib, plc_params
    assert plc_params(16000).tolist() == [80, 240, 320, 2, 160, 800, 80, 16000]
    assert plc_params(44100).tolist() == [220, 661, 882, 5, 441, 2205, 220, 44100]
    for fs in PK.RATES:
        assert PK.same_bits(plc_params(fs), PK.params(fs)), fs
        for kw in (dict(hold_ms=0, fade_ms=1, recover_ms=0), dict(hold_ms=200, fade_ms=200, recover_ms=200), dict(hold_ms=7, fade_ms=33, recover_ms=3)):
            assert PK.same_bits(plc_params(fs, **kw), PK.params(fs, **kw)), (fs, kw)
        assert plc_params(fs, recover_ms=0)[6] == 1 and PK.hist_len(plc_params(fs)) <= 1680
    assert PK.hist_len(plc_params(48000)) == 1680
    for fs, kw, reason in ((11025, {}, "fs must be one of 8000, 16000, 22050, 24000, 32000, 44100, 48000"), (0, {}, "fs must be one of"),
                           (16000, dict(hold_ms=-1), "hold_ms must lie in 0 .. 200"), (16000, dict(hold_ms=201), "hold_ms must lie in 0 .. 200"),
                           (16000, dict(fade_ms=0), "fade_ms must lie in 1 .. 200"), (16000, dict(fade_ms=201), "fade_ms must lie in 1 .. 200"),
                           (16000, dict(recover_ms=-1), "recover_ms must lie in 0 .. 200"), (16000, dict(recover_ms=201), "recover_ms must lie in 0 .. 200"),
                           (16000, dict(fade_ms=2.5), "whole number"), (16000.5, {}, "whole number"), (16000, dict(comfort=1), "unknown concealment fields")):
        with pytest.raises(GtcrnError, match=re.escape(reason)):
            plc_params(fs, **kw)
    assert _lib.lib().gtcrn_plc_params_host(None, None) == ERR_ARG
    assert b"null pointer" in _lib.lib().gtcrn_last_error()


def test_argument_errors_have_reasons():
    from gtcrn_micro_amd import GtcrnError, _lib, plc_rows_host
    L = _lib.lib()
    buf = np.zeros(4096, np.uint8)
    base = buf.ctypes.data + (-buf.ctypes.data) % 16
    x, lost, slots, count, hist, rec, prm = base, base + 1024, base + 1088, base + 1152, base + 1216, base + 3472, base + 3536
    np.frombuffer(buf, np.int32, 8, prm - buf.ctypes.data)[:] = PK.params(8000)
    good = [x, 40, 4, 40, slots, lost, count, hist, 280, rec, 4, prm]
    np.frombuffer(buf, np.int32, 4, slots - buf.ctypes.data)[:] = [0, 1, 2, 3]
    np.frombuffer(buf, np.int32, 1, count - buf.ctypes.data)[:] = 4
    assert L.gtcrn_plc_rows_host(*good) == 0 and L.gtcrn_plc_rows_pcm16_host(*good) == 0 and L.gtcrn_plc_rows_g711_host(*good, 1) == 0
    for pos, val, reason in ((3, 0, "n must lie in 1 .. 1024"), (3, 1025, "n must lie in 1 .. 1024"), (2, -1, "negative count"),
                             (10, -1, "negative count"), (0, None, "null pointer"), (5, None, "null pointer"), (7, None, "null pointer"),
                             (9, None, "null pointer"), (11, None, "null pointer"), (1, 39, "stride is shorter"), (8, 0, "hist_stride"),
                             (0, x + 2, "misaligned"), (7, hist + 1, "misaligned"), (4, slots + 2, "misaligned"), (5, lost + 1, "misaligned"),
                             (6, count + 2, "misaligned"), (9, rec + 8, "misaligned"), (11, prm + 4, "misaligned")):
        bad = list(good)
        bad[pos] = val
        assert L.gtcrn_plc_rows_host(*bad) == ERR_ARG, (pos, val)
        assert reason.encode() in L.gtcrn_last_error(), (reason, L.gtcrn_last_error())
        assert L.gtcrn_plc_rows(*bad, None) == ERR_ARG, (pos, val)        # refused before any launch: no device is touched
    assert L.gtcrn_plc_rows_g711_host(*good, 2) == ERR_ARG and b"law must be 0" in L.gtcrn_last_error()
    assert L.gtcrn_plc_rows_g711(*good, -1, None) == ERR_ARG
    assert L.gtcrn_plc_reset(None, 280, rec, 4, prm, None, 4, None, None) == ERR_ARG and b"null pointer" in L.gtcrn_last_error()
    assert L.gtcrn_plc_reset(hist, 280, rec + 4, 4, prm, None, 4, None, None) == ERR_ARG and b"misaligned" in L.gtcrn_last_error()
    # words that gtcrn_plc_params_host did not make: a history longer than its pitch turns the call into a no-op
    rows, h, r = np.ones((2, 40), np.int16), np.zeros((2, 100), np.int16), np.zeros((2, 4), np.int32)
    plc_rows_host(rows, [0, 0], h, r, PK.params(8000))
    assert not h.any() and not r.any()
    for args, kw, reason in (((np.zeros((2, 40), np.uint8), [0, 0], h, r, PK.params(8000)), {}, "G.711 codes"),
                             ((np.zeros((2, 40), np.float64), [0, 0], h, r, PK.params(8000)), {}, "float32, int16 or uint8"),
                             ((rows, [0], h, r, PK.params(8000)), {}, "a word per row"), ((rows, [0, 0], h, r[:1], PK.params(8000)), {}, "a record per history"),
                             ((rows, [0, 0], h, r, PK.params(8000)), dict(slots=[0]), "an id per row")):
        with pytest.raises(GtcrnError, match=reason):
            plc_rows_host(*args, **kw)


@pytest.mark.parametrize("pad", [5, 0])
@pytest.mark.parametrize("kind", PC.KINDS)
@pytest.mark.parametrize("name,c", CASES, ids=[n for n, _ in CASES])
def test_host_twin_equals_checker(name, c, kind, pad):
    PC.run(c, host, kind, pad)


def test_host_twin_equals_checker_on_non_finite_rows():
    for _, c in PC.poison_cases():
        PC.run(c, host, "f32", 5)
        PC.run(c, host, "f32", 0)


# ---- what the cases are named for ------------------------------------------------------------------------------------------------
def stream(x, lost, fs, n, kind="pcm16", fn=None, **kw):
    """One stream through `fn` (the host twin) packet by packet: returns the rows as written (T, n) and the records per tick."""
    prm = PK.params(fs, **kw)
    hist, rec = np.zeros((1, PK.hist_len(prm)), np.int16), np.zeros((1, 4), np.int32)
    out, recs = [], []
    for t, l in enumerate(lost):
        rows = PC.as_kind(x[None, t * n:(t + 1) * n], kind)
        (fn or host)(rows, np.array([l], np.int32), hist, rec, prm, None, None, PC.LAW[kind])
        out.append(rows[0].copy())
        recs.append(rec[0].copy())
    return np.stack(out), np.stack(recs)


def test_the_lag_of_the_periodic_signals():
    for fs, n in ((8000, 80), (16000, 160), (48000, 480)):
        prm = PK.params(fs)
        pmin, D = int(prm[0]), int(prm[3])
        lost = [0] * 12 + [1]
        pmax = int(prm[1])
        for P in (pmin + 5 * D, pmin, pmax, pmax - 3 * D - (1 if D > 1 else 0)):     # on the grid; the two ends; off it, 2 P > pmax
            _, recs = stream(PC.periodic(P, 13 * n), lost, fs, n)
            # the score of an exactly periodic signal is the same at P and 2 P (c = e): the tie goes to the smaller lag
            assert int(recs[-1][1]) == P, (fs, P, recs[-1])
        # off the coarse grid with 2 P on it: the coarse search meets the exact match at 2 P, and the lag is that multiple of P
        P = pmin + 8 * D + (1 if D > 1 else 0)
        lag = int(stream(PC.periodic(P, 13 * n), lost, fs, n)[1][-1][1])
        assert lag == (2 * P if D > 1 and (2 * P - pmin) % D == 0 else P) and lag % P == 0, (fs, P, lag)
    # silence, and a loss on the first packet after a reset: no positive score, the lag is pmax and the packet is zeros
    for x, lost in ((np.zeros(1600, np.int16), [0] * 9 + [1]), (PC.periodic(100, 160), [1])):
        out, recs = stream(x, lost, 16000, 160)
        assert int(recs[-1][1]) == 240 and not out[-1].any() and int(recs[-1][3]) == 0x10001
    # full scale: m = 32768, s = 6
    sq = np.where((np.arange(1600) // 50) % 2 == 0, -32768, 32767).astype(np.int16)
    assert int(stream(sq, [0] * 9 + [1], 16000, 160)[1][-1][1]) == 100


def test_an_integer_period_is_continued_bit_for_bit_through_the_hold():
    """P = 100 at 16 kHz / 160: the lag is a multiple of P (here P itself), so the first T0 samples of a concealed packet are the
    true continuation; after the hold they are its attenuation."""
    P, n = 100, 160
    x = PC.periodic(P, 14 * n)
    lost = [0] * 10 + [1, 1, 0, 0]
    prm = PK.params(16000)
    for kind in ("pcm16", "f32"):
        out, recs = stream(x, lost, 16000, n, kind)
        assert int(recs[10][1]) % P == 0 and int(prm[4]) == n
        assert PK.same_bits(out[10], PC.as_kind(x[None, 10 * n:11 * n], kind)[0])
        assert not PK.same_bits(out[11], PC.as_kind(x[None, 11 * n:12 * n], kind)[0])
        want = (x[11 * n:12 * n].astype(np.int64) * PK.gain(n + np.arange(n), prm) + 16384) >> 15
        assert PK.same_bits(out[11], PK.stored(want, out.dtype, None))
        assert recs[:, 2].tolist() == [0] * 10 + [n, 2 * n, 0, 0]


def test_the_fade_out_reaches_zero_and_stays_there():
    n = 160
    x = PC.periodic(100, 30 * n, amp=32000)
    lost = [0] * 10 + [1] * 8 + [0] * 4
    for kind in PC.KINDS:
        out, recs = stream(x, lost, 16000, n, kind)
        zero = PC.as_kind(np.zeros((1, n), np.int16), kind)[0]
        T = 160 + 800                                            # T0 + T1: six packets
        assert recs[10:18, 2].tolist() == [160, 320, 480, 640, 800, 960, 960, 960]
        assert PK.same_bits(out[16], zero) and PK.same_bits(out[17], zero) and T == 960
        flat = np.concatenate(out[10:16])
        assert (PK.int16_of(flat, PC.LAW[kind])[-40:] != 0).any() and recs[17][3] == 0x80001
        # the history went on unattenuated: recovery cross-fades from silence (erased is saturated), into the full signal
        assert int(recs[18][2]) == 0 and PK.same_bits(out[19], PC.as_kind(x[None, 19 * n:20 * n], kind)[0])


def test_the_last_recovery_sample_is_the_input_sample_and_the_rest_is_not_written():
    n = 160
    x = PC.speech(16000, 20 * n, 2)
    lost = [0] * 8 + [1, 0, 0, 1, 1, 0] + [0] * 6
    for kind in PC.KINDS:
        for kw, f in ((dict(), 80), (dict(recover_ms=200), n), (dict(recover_ms=0), 1)):
            out, recs = stream(x, lost, 16000, n, kind, **kw)
            for t in (9, 13):
                true = PC.as_kind(x[None, t * n:(t + 1) * n], kind)[0]
                assert PK.same_bits(out[t][f:], true[f:])
                assert PK.int16_of(out[t][f - 1:f], PC.LAW[kind])[0] == PK.int16_of(true[f - 1:f], PC.LAW[kind])[0]
                assert f == 1 or not PK.same_bits(out[t][:f - 1], true[:f - 1])
                assert int(recs[t][2]) == 0 and int(recs[t - 1][2]) > 0


def test_a_received_packet_outside_recovery_is_not_written():
    """Values that a rewrite would change stay as they are: a NaN with a payload, -0.0 and 1e30 in float rows, the second zero
    code 0x7F in mu-law rows (E(D(0x7F)) is 0xFF); guards stand behind the row."""
    prm = PK.params(16000)
    for kind in PC.KINDS:
        buf = np.full((1, 165), PC.GUARD[PC.as_kind(np.zeros((1, 1), np.int16), kind).dtype])
        buf[:, :160] = PC.as_kind(PC.speech(16000, 160, 1)[None], kind)
        if kind == "f32":
            buf[0, :4] = np.array([0x7FC01234, 0x80000000, 0x7149F2CA, 0xFF800000], np.uint32).view(F)
        if kind == "ulaw":
            buf[0, :2] = [0x7F, 0xFF]
        keep = buf.copy()
        hist, rec = np.zeros((1, 560), np.int16), np.zeros((1, 4), np.int32)
        host(buf[:, :160], [0], hist, rec, prm, None, None, PC.LAW[kind])
        assert PK.same_bits(buf, keep) and rec.tolist() == [[160, 0, 0, 0]]
        assert PK.same_bits(hist[0, :160], PK.int16_of(keep[0, :160], PC.LAW[kind]).astype(np.int16)) and not hist[0, 160:].any()


def test_a_permutation_of_the_rows_and_other_streams_beside_give_every_stream_the_same_bits():
    c = PC.stream_case(16000, 160, seed=31, shift=2)
    for kind in ("f32", "ulaw"):
        law = PC.LAW[kind]
        prm, h0, r0 = PC.fresh(c, pad=0)
        _, h1, r1 = PC.fresh(dict(c, S=13), pad=0)
        rng = np.random.default_rng(7)
        for rows, lost, _, _ in c["ticks"]:
            a = PC.as_kind(rows, kind)
            host(a, lost, h0, r0, prm, None, None, law)
            perm = rng.permutation(8)
            ids = (perm + 3).astype(np.int32)                      # the same streams in slots 3 .. 10 of 13, rows shuffled
            b = np.concatenate([PC.as_kind(rows, kind)[perm], PC.as_kind(rows[:2], kind)])
            host(b, np.concatenate([lost[perm], [1, 0]]), h1, r1, prm, np.concatenate([ids, [0, 12]]).astype(np.int32), None, law)
            assert PK.same_bits(b[np.argsort(perm)], a)
        assert PK.same_bits(h1[3:11], h0) and PK.same_bits(r1[3:11], r0)


def test_a_non_finite_sample_moves_no_bit_of_another_stream():
    runs = []
    for poisoned in (False, True):
        c = PC.poison_case(poisoned)
        prm, hist, rec = PC.fresh(c, pad=0)
        outs = []
        for rows, lost, _, _ in c["ticks"]:
            x = rows.copy()
            host(x, lost, hist, rec, prm, None, None, None)
            outs.append(x)
        runs.append((np.stack(outs), PK.history(hist, rec, prm), rec))
    others = [0, 1, 3, 4, 5, 6, 7]
    assert PK.same_bits(runs[0][0][:, others], runs[1][0][:, others])
    assert PK.same_bits(runs[0][1][others], runs[1][1][others]) and PK.same_bits(runs[0][2][others], runs[1][2][others])
    assert np.isnan(runs[1][0][:, 2]).any() and (runs[1][1][2] == -32768).any()


def test_speech_examples_against_zero_fill():
    """Waveform error over the lost packets above -40 dBov, relative to the energy of the true packets (what zero fill leaves):
    below 1 for the noisy and for the enhanced examples.  Waveform error understates what a concealment does for the ear (a
    continuation that is right in pitch and spectrum but off in phase scores worse than silence) and nothing more is claimed.
    The figures of record are in profiles/plc_examples.json (tools/plc_examples.py writes them from this very function)."""
    with open(os.path.join(ROOT, "profiles", "plc_examples.json")) as f:
        record = json.load(f)
    for which in ("noisy", "enh"):
        fig = PC.speech_figures(host, which)
        print(which, fig)
        assert fig["packets"] > 200 and fig["lost_packets"] == 445 and fig["erasures"] == 295
        assert fig["ratio"] < 1.0, fig
        assert record[which]["packets"] == fig["packets"] and abs(record[which]["ratio"] - fig["ratio"]) < 1e-9
    assert np.array_equal(np.flatnonzero(PC.speech_loss(130)), [25, 45, 46, 47, 65, 85, 105, 106, 125])
