"""CPU-side checks of "active levels" (include/gtcrn_micro_hip.h): the numpy checker (tests/active_checker.py) against a
brute-force float64 statement and against batch_checker where every window is active, the exact tie, the fallback flags, the
achieved SNR, the threshold from dB, the exported symbols, the argument errors and the workspace size."""
import ctypes
import os
import re

import numpy as np
import pytest

from conftest import ROOT

import __graft_entry__ as graft
import active_checker as AC
import batch_checker as BC

ACTIVE_SYMBOLS = ["gtcrn_batch_active_workspace_bytes", "gtcrn_batch_mix_active"]
ERR_ARG = -1
GRID_L = [1, 7, 8, 9, 15, 16, 17, 255, 1027, 4099]
GRID_W = [8, 16, 1600]


@pytest.fixture(scope="module", autouse=True)
def _built():
    graft.build()


def _speech_with_pauses(rng, L, W, amp=9000):
    """Random samples with stretches of digital silence that start and end on window edges."""
    x = rng.integers(-amp, amp, L).astype(np.int16)
    x[x == 0] = 1
    nw = (L + W - 1) // W
    for w in rng.choice(nw, max(1, nw // 3), replace=False):
        x[w * W:(w + 1) * W] = 0
    return x


def _brute(s, n, snr_amp, W, thr):
    """The definition in plain float64, window by window: -> (speech-active set, noise-active set, gn or None)."""
    L = len(s)
    act, power = [], []
    for x in (s, n):
        on, e_sum, n_sum = set(), 0.0, 0.0
        for w in range((L + W - 1) // W):
            seg = [float(v) for v in x[w * W:min((w + 1) * W, L)]]
            e = sum(v * v for v in seg)
            if e / len(seg) > float(thr):
                on.add(w)
                e_sum += e
                n_sum += len(seg)
        if not on:
            e_sum, n_sum = sum(float(v) ** 2 for v in x), float(L)
        act.append(on)
        power.append(e_sum / n_sum)
    if power[0] == 0.0 or power[1] == 0.0:
        return act[0], act[1], None
    return act[0], act[1], np.sqrt(power[0]) / np.sqrt(power[1]) * float(np.float32(snr_amp))


@pytest.mark.parametrize("L,W", [(17, 8), (255, 16), (1027, 16), (4099, 1600), (4099, 8)])
def test_checker_equals_a_brute_force_float64_definition(L, W):
    rng = np.random.default_rng(L * 31 + W)
    for trial in range(6):
        s = _speech_with_pauses(rng, L, W)
        n = _speech_with_pauses(rng, L, W, 2000) if trial % 2 else rng.integers(-2000, 2000, L).astype(np.int16)
        thr = [0, 10737, 400000, 30000000][trial % 4]            # the last two switch random windows of the 2000-amplitude side off
        snr_amp = 10.0 ** (-float(rng.uniform(-5, 20)) / 20.0)
        _, _, rec = AC.mix_item_active(s, n, snr_amp, 0.05, W, thr)
        sa, _, _ = AC.active_windows(s, W, thr)
        na, _, _ = AC.active_windows(n, W, thr)
        bs, bn, gn = _brute(s, n, snr_amp, W, thr)
        assert set(np.flatnonzero(sa).tolist()) == bs and set(np.flatnonzero(na).tolist()) == bn
        assert bool(rec[10] & 16) == (not bs) and bool(rec[10] & 32) == (not bn)
        assert gn is not None and BC.ulp_distance(rec[7], np.float32(gn)) <= 1, (rec[7], gn)


def test_a_window_exactly_at_the_threshold_is_inactive():
    s = np.full(8, 100, np.int16)
    n = np.full(8, -100, np.int16)
    for x in (s, n):
        assert not AC.active_windows(x, 8, 10000)[0].any()
        assert AC.active_windows(x, 8, 9999)[0].all()
    at = AC.mix_item_active(s, n, 0.5, 0.05, 8, 10000)[2]
    below = AC.mix_item_active(s, n, 0.5, 0.05, 8, 9999)[2]
    assert at[10] & 48 == 48 and (at[3], at[4], at[5], at[6]) == (80000, 80000, 8, 8)      # the fallback: the whole row
    assert below[10] & 48 == 0 and (below[3], below[4], below[5], below[6]) == (80000, 80000, 8, 8)
    # one side at the tie, the other above it
    s2 = np.concatenate([s, np.full(8, 101, np.int16)])
    r = AC.mix_item_active(s2, np.concatenate([n, n]), 0.5, 0.05, 8, 10000)[2]
    assert (r[3], r[5], r[10] & 48) == (8 * 101 * 101, 8, 32)


@pytest.mark.parametrize("W", GRID_W)
@pytest.mark.parametrize("L", GRID_L)
def test_rows_with_every_window_active_equal_the_plain_mix_bit_for_bit(L, W):
    rng = np.random.default_rng(L * 7 + W)
    for snr_amp, lvl_amp in ((0.5, 0.05), (1e-3, 0.05), (3.0, 1.0)):
        s = rng.integers(1, 12000, L).astype(np.int16) * rng.choice([-1, 1], L).astype(np.int16)
        n = rng.integers(1, 3000, L).astype(np.int16) * rng.choice([-1, 1], L).astype(np.int16)
        an, ac, ar = AC.mix_item_active(s, n, snr_amp, lvl_amp, W, 0)
        pn, pc, pr = BC.mix_item(s, n, snr_amp, lvl_amp)
        assert (ar[5], ar[6]) == (L, L) and (ar[3], ar[4]) == (pr[0], pr[1])
        assert ar[:3] == pr[:3] and ar[10] == pr[6]
        for a, p in zip(ar[7:10], pr[3:6]):
            assert np.float32(a).tobytes() == np.float32(p).tobytes()
        assert an.tobytes() == pn.tobytes() and ac.tobytes() == pc.tobytes()


def test_fallback_flags_alone_and_with_the_zero_flags():
    W, L, thr = 8, 32, 10000
    rng = np.random.default_rng(3)
    loud = rng.integers(2000, 9000, L).astype(np.int16)
    quiet = rng.integers(1, 50, L).astype(np.int16)          # not zero, below the threshold everywhere
    zero = np.zeros(L, np.int16)
    flags = lambda s, n: int(AC.mix_item_active(s, n, 0.5, 0.05, W, thr)[2][10]) & ~8      # noqa: E731
    assert flags(loud, loud[::-1].copy()) == 0
    assert flags(quiet, loud) == 16
    assert flags(loud, quiet) == 32
    assert flags(quiet, quiet[::-1].copy()) == 48
    assert flags(zero, loud) == 16 | 2                       # zero speech: inactive, and the noise alone
    assert flags(loud, zero) == 32 | 1                       # zero noise
    assert flags(zero, zero) == 48 | 1 | 4                   # both zero: as the plain mix, flags 1 and 4
    assert flags(zero, quiet) == 48 | 2
    # the fallback levels the quiet side over the whole row
    r = AC.mix_item_active(quiet, loud, 0.5, 0.05, W, thr)[2]
    assert (r[3], r[5]) == (r[0], L) and (r[4], r[6]) == (r[1], L)


def test_achieved_snr_is_the_drawn_one_over_active_windows():
    from gtcrn_micro_amd import data
    assert data.ACTIVE_RECORD_DTYPE == AC.ACTIVE_RECORD_DTYPE and data.ACTIVE_RECORD_DTYPE.itemsize == 64
    rng = np.random.default_rng(11)
    L, W, thr = 6400, 160, 10737
    B = 12
    snr_db = rng.uniform(-5, 20, B)
    rec = np.zeros(B + 2, AC.ACTIVE_RECORD_DTYPE)
    plan = BC.make_plan([(0, 0, 0, 0, 10.0 ** (-d / 20.0), 0.05) for d in snr_db])
    for b in range(B):
        s = _speech_with_pauses(rng, L, W)
        n = _speech_with_pauses(rng, L, W, 3000) if b % 2 else rng.integers(-3000, 3000, L).astype(np.int16)
        rec[b] = AC.mix_item_active(s, n, plan["snr_amp"][b], plan["lvl_amp"][b], W, thr)[2]
    rec[B] = AC.mix_item_active(np.zeros(L, np.int16), s, 0.5, 0.05, W, thr)[2]           # flag 2
    rec[B + 1] = AC.mix_item_active(s, np.zeros(L, np.int16), 0.5, 0.05, W, thr)[2]       # flag 1
    active, plain = data.achieved_snr_db(rec)
    assert np.all(rec["Ns"][:B] < L) and np.any(rec["Nn"][:B] < L), "the rows have no pauses"
    assert np.abs(active[:B] - plan["snr_db"].astype(np.float64)).max() <= 1e-4
    assert np.abs(active[:B] - snr_db).max() <= 1e-4
    # the pauses are digital silence, so As == Ss and An == Sn: the plain SNR is off by the two activity shares alone
    off = 10.0 * np.log10((rec["Ns"][:B] / L) / (rec["Nn"][:B] / L))
    assert np.abs(plain[:B] - active[:B] - off).max() <= 1e-9
    assert np.abs(off).max() > 0.5, "the rows do not tell the two SNRs apart"
    assert np.isnan(active[B:]).all() and np.isnan(plain[B:]).all()
    with pytest.raises(data.GtcrnError):
        data.achieved_snr_db(np.zeros(2, BC.RECORD_DTYPE))


def test_active_threshold_from_db():
    from gtcrn_micro_amd import GtcrnError
    from gtcrn_micro_amd.data import active_threshold
    assert active_threshold(-50) == 10737 and active_threshold(-60) == 1073 and active_threshold(-40) == 107374
    assert active_threshold(0) == 1 << 30 and active_threshold(-400) == 0
    for bad in (0.1, float("nan")):
        with pytest.raises(GtcrnError):
            active_threshold(bad)


def test_active_symbols_exported_declared_and_abi_version_unchanged():
    L = ctypes.CDLL(os.path.join(ROOT, "gtcrn_micro_amd", "libgtcrn_micro_hip.so"))
    header = open(os.path.join(ROOT, "include", "gtcrn_micro_hip.h")).read()
    from gtcrn_micro_amd import _lib
    for n in ACTIVE_SYMBOLS:
        assert hasattr(L, n), n
        assert re.search(r"\b%s\(" % n, header), f"{n} is not declared in the header"
        assert getattr(_lib.lib(), n).argtypes is not None, f"{n} has no ctypes declaration"
    assert "gtcrn_batch_active_record" in header
    assert L.gtcrn_abi_version() == 1
    assert "#define GTCRN_ABI_VERSION 1" in header


def test_argument_errors_come_before_anything_is_enqueued():
    """Every refusal below is decided on the arguments alone: no device is touched, so this runs without a GPU."""
    from gtcrn_micro_amd._lib import lib
    Lb = lib()
    x = 0x1000                                           # a stand-in for a device address: refusals never follow it

    def mix(a=x, ao=x, na=2, b=x, bo=x, nb=2, tg=None, plan_=x, B=4, L=8, noisy=x, ns=8, clean=x, cs=8, W=8, thr=0, rec=x, ws=x,
            passes=7):
        return Lb.gtcrn_batch_mix_active(a, ao, na, b, bo, nb, tg, plan_, B, L, noisy, ns, clean, cs, W, thr, rec, ws, passes, None)

    for kw in (dict(B=0), dict(L=0), dict(L=1 << 31), dict(na=0), dict(nb=0), dict(a=None), dict(ao=None), dict(b=None), dict(bo=None),
               dict(plan_=None), dict(noisy=None), dict(clean=None), dict(ns=7), dict(cs=7), dict(noisy=x + 2), dict(rec=None),
               dict(ws=None), dict(tg=x + 1), dict(rec=x + 4), dict(ws=x + 8), dict(passes=0), dict(passes=8),
               dict(W=0), dict(W=4), dict(W=12), dict(W=-8), dict(W=1604), dict(W=(1 << 20) + 8),
               dict(thr=-1), dict(thr=(1 << 30) + 1)):
        assert mix(**kw) == ERR_ARG, kw
        assert Lb.gtcrn_last_error()
    # the order: an existing check is reported before the window, the window before the threshold
    assert mix(passes=0, W=4, thr=-1) == ERR_ARG and b"passes" in Lb.gtcrn_last_error()
    assert mix(W=4, thr=-1) == ERR_ARG and b"window" in Lb.gtcrn_last_error()
    assert mix(thr=-1) == ERR_ARG and b"threshold" in Lb.gtcrn_last_error()
    f = Lb.gtcrn_batch_active_workspace_bytes
    for bad in ((0, 8, 8), (4, 0, 8), (4, 1 << 31, 8), (4, 8, 0), (4, 8, 12), (4, 8, 4), (4, 8, (1 << 20) + 8), (1 << 30, 64000, 1600)):
        assert f(*bad) == 0, bad


def _geometry(L, W):
    """batch.h's active_* functions, restated: -> (samples per chunk, chunks)."""
    k = max(-(-4096 // W), -(-(-(-L // W)) // 256))
    return k * W, -(-L // (k * W))


@pytest.mark.parametrize("L,W,chunks", [(1, 8, 1), (4099, 16, 2), (64000, 1600, 14), (64000, 8, 16), ((1 << 31) - 1, 1600, 256)])
def test_workspace_size_matches_the_geometry(L, W, chunks):
    from gtcrn_micro_amd.data import active_workspace_bytes
    ch, n = _geometry(L, W)
    assert n == chunks and n <= 256 and ch % W == 0 and (ch >= 4096 or W > 4096)
    for B in (1, 3, 512):
        assert active_workspace_bytes(B, L, W) == (B * n * (7 * 8 + 4) + 15) // 16 * 16
    if (L, W) == (64000, 1600):
        assert ch == 4800


def test_python_layer_refuses_what_the_library_would():
    from gtcrn_micro_amd import GtcrnError
    from gtcrn_micro_amd.data import BatchSource, active_workspace_bytes
    corpus = object()                                    # the refusals come before any corpus is looked at
    with pytest.raises(GtcrnError, match="active_db"):
        BatchSource(corpus, paired_clean=corpus, active_db=-50.0)
    for w in (0, 4, 12, 1604, (1 << 20) + 8, 1600.5):
        with pytest.raises(GtcrnError, match="active_window"):
            BatchSource(corpus, noise=corpus, active_db=-50.0, active_window=w)
    with pytest.raises(GtcrnError, match="active_db"):
        BatchSource(corpus, noise=corpus, active_db=3.0)
    with pytest.raises(GtcrnError):
        active_workspace_bytes(4, 64000, 12)
    with pytest.raises(GtcrnError, match="Corpus"):      # with good arguments the next check is the corpora's
        BatchSource(corpus, noise=corpus, active_db=-50.0)
