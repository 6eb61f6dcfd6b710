"""CPU-side checks of "dereverberation targets: early or direct clean" (include/gtcrn_micro_hip.h): the exported symbols, the
split table's scheme restated in numpy tile for tile -- early segment, seam block, rest segment, the accumulators carried
over the seam, both biases -- against np.convolve, the digit sums at the largest operands, split_for's rounding, and the
argument errors."""
import ctypes
import os
import re

import numpy as np
import pytest

from conftest import ROOT

import __graft_entry__ as graft
import reverb_checker as RC
import target_checker as TC

TARGET_SYMBOLS = ["gtcrn_batch_reverb_split_table_bytes", "gtcrn_batch_reverb_split_prepare", "gtcrn_batch_reverb_split_workspace_bytes",
                  "gtcrn_batch_reverb_split", "gtcrn_batch_mix_target"]
ERR_ARG = -1
KS = [1, 17, 256, 257, 700, 16384]


def _splits(K):
    return sorted({E for E in (1, 16, 255, 256, 257, K - 1, K) if 1 <= E <= K})


@pytest.fixture(scope="module", autouse=True)
def _built():
    graft.build()


def test_target_symbols_exported_declared_and_abi_version_unchanged():
    L = ctypes.CDLL(os.path.join(ROOT, "gtcrn_micro_amd", "libgtcrn_micro_hip.so"))
    header = open(os.path.join(ROOT, "include", "gtcrn_micro_hip.h")).read()
    from gtcrn_micro_amd import _lib
    for n in TARGET_SYMBOLS:
        assert hasattr(L, n), n
        assert re.search(r"\b%s\(" % n, header), f"{n} is not declared in the header"
        assert getattr(_lib.lib(), n).argtypes is not None, f"{n} has no ctypes declaration"
    assert L.gtcrn_abi_version() == 1
    from gtcrn_micro_amd import data
    assert data.REVERB_SPLIT_RECORD_DTYPE.itemsize == 32 and data.REVERB_SPLIT_RECORD_DTYPE == TC.SPLIT_RECORD_DTYPE
    assert "gtcrn_reverb_split_record" in header and "/* 32 bytes */" in header


# ---- the split table, restated ---------------------------------------------------------------------------------------------
def _tap_digits(h):
    h = np.asarray(h, np.int64)
    lo = ((h + 128) & 255) - 128
    return (h - lo) >> 8, lo


def _speech_digits(x):
    x = np.asarray(x, np.int64)
    return x >> 8, (x & 255) - 128


def _groups(K):
    return 16 * ((K + 15 + 255) // 256)


def _tiles(h, k0, k1, m0, m1):
    """Groups m0 .. m1 - 1 of the response whose taps outside k0 .. k1 - 1 are stored as zero: T[m][j][e] = h[16 m + j - e]."""
    idx = 16 * np.arange(m0, m1)[:, None, None] + np.arange(16)[None, :, None] - np.arange(16)[None, None, :]
    return np.where((idx >= k0) & (idx < k1), h.astype(np.int64)[np.clip(idx, 0, len(h) - 1)], 0)


def _split_table(h, E):
    """-> (tiles of both segments, contiguous; groups of the early segment; first group of the rest segment)."""
    K = len(h)
    Me, first = _groups(E), 16 * (E // 256)
    early = _tiles(h, 0, E, 0, Me)
    rest = _tiles(h, E, K, first, _groups(K)) if E < K else np.zeros((0, 16, 16), np.int64)
    assert Me % 16 == 0 and len(rest) % 16 == 0, "segments are whole fours of 64-tap chunks"
    assert len(early) + len(rest) <= _groups(K) + 32 and (E % 256 > 241 or len(early) + len(rest) <= _groups(K) + 16)
    return np.concatenate([early, rest]), Me, first


def _split_matrix_form(clip, s0, L, h, E, block=2048):
    """One walk over the table's groups per 256-output tile: the early segment, the target's epilogue, the accumulators NOT
    reset, the rest segment with the data side stepped back to the block that holds E, the wet row's epilogue."""
    K = len(h)
    M = _groups(K)
    T, Me, first = _split_table(h, E)
    Th, Tl = _tap_digits(T)
    x = clip.astype(np.int64)
    sums = (int(h[:E].astype(np.int64).sum()), int(h.astype(np.int64).sum()))
    outs = [np.zeros((L + block - 1) // block * block, np.int64) for _ in range(2)]
    for o0 in range(0, L, block):
        NG = block // 16 + M - 1
        j = s0 + o0 - 16 * (M - 1) + np.arange(NG * 16)
        span = np.where((j >= 0) & (j < len(x)), x[np.clip(j, 0, len(x) - 1)], 0)
        Xh, Xl = (d.reshape(NG, 16) for d in _speech_digits(span))
        for t in range(min(block, L - o0 + 255) // 256):
            hh, mid, ll = (np.zeros((16, 16), np.int64) for _ in range(3))
            for seg, (g0, g1) in enumerate(((0, Me), (Me, len(T)))):
                g = np.arange(g0, g1)
                m = g if seg == 0 else first + (g - Me)                  # the data side's group of table group g
                q = 16 * t + np.arange(16)[None, :] + M - 1 - m[:, None]     # [group][column i]
                assert q.size == 0 or (q.min() >= 0 and q.max() < NG)
                hh += np.einsum("mje,mie->ji", Th[g], Xh[q])
                mid += np.einsum("mje,mie->ji", Th[g], Xl[q]) + np.einsum("mje,mie->ji", Tl[g], Xh[q])
                ll += np.einsum("mje,mie->ji", Tl[g], Xl[q])
                for a in (hh, mid, ll):
                    assert np.abs(a).max() < 1 << 31
                acc = 65536 * hh + 256 * mid + ll + 128 * sums[seg]
                outs[seg][o0 + 256 * t:o0 + 256 * (t + 1)] = acc.T.reshape(256)
    res = []
    for o in outs:
        v = (o[:L] + 16384) >> 15
        res.append((np.clip(v, -32768, 32767).astype(np.int16), int(((v < -32768) | (v > 32767)).sum())))
    return res          # [(target, clamped), (wet, clamped)]


@pytest.mark.parametrize("K", KS)
def test_split_table_scheme_in_numpy_equals_np_convolve(K):
    rng = np.random.default_rng(K)
    L, s0 = 300, K // 2 + 3
    clip = rng.integers(-32768, 32768, s0 + L - 20).astype(np.int16)          # shorter than the window: the tail rings out
    clip[:4] = [32767, -32768, 32767, -32768]
    h = (rng.integers(-RC.TAP_MAX, RC.TAP_MAX + 1, K) // (1 if K < 300 else 16)).astype(np.int16)
    h[0] = RC.TAP_MAX
    want_wet = RC.wet_row(clip, s0, L, h)
    for E in _splits(K):
        (tgt, tsat), (wet, sat) = _split_matrix_form(clip, s0, L, h, E)
        want_tgt = RC.wet_row(clip, s0, L, h[:E])
        assert np.array_equal(tgt, want_tgt[0]) and tsat == want_tgt[1], E
        assert np.array_equal(wet, want_wet[0]) and sat == want_wet[1], E
        if E == K:
            assert np.array_equal(tgt, wet)
    (tgt, _), (wet, _) = _split_matrix_form(clip, s0, L, h, min(K, 16), block=8192)
    assert np.array_equal(wet, want_wet[0]) and np.array_equal(tgt, RC.wet_row(clip, s0, L, h[:min(K, 16)])[0])


def test_split_table_bytes_is_the_header_and_both_segments():
    from gtcrn_micro_amd._lib import lib
    tb = lib().gtcrn_batch_reverb_split_table_bytes
    lens = [1, 17, 256, 257, 700, 16384, 16384, 700]
    off = np.zeros(len(lens) + 1, np.int64)
    np.cumsum(lens, out=off[1:])
    split = np.array([1, 16, 256, 256, 255, 8191, 16384, 250], np.int32)
    want = 256                                           # eight responses of 32 header bytes
    for K, E in zip(lens, split):
        want += 512 * (_groups(E) + (0 if E == K else _groups(K) - 16 * (E // 256)))
    assert tb(off.ctypes.data, split.ctypes.data, len(lens)) == want
    # a split outside 1 .. K counts as clamped into it
    wild = np.array([0, 99, -5, 256, 255, 8191, 1 << 30, 250], np.int32)
    assert tb(off.ctypes.data, wild.ctypes.data, len(lens)) == tb(off.ctypes.data, np.array([1, 17, 1, 256, 255, 8191, 16384, 250],
                                                                                          np.int32).ctypes.data, len(lens))
    assert tb(None, split.ctypes.data, 8) == 0 and tb(off.ctypes.data, None, 8) == 0 and tb(off.ctypes.data, split.ctypes.data, 0) == 0
    assert tb(np.array([0, 16385], np.int64).ctypes.data, split.ctypes.data, 1) == 0


@pytest.mark.parametrize("E", [8191, 8192])
@pytest.mark.parametrize("xv", [32767, -32768])
@pytest.mark.parametrize("hv", [RC.TAP_MAX, -RC.TAP_MAX])
def test_digit_sums_of_16384_extreme_taps_split_stay_inside_int32_and_recombine_exactly(xv, hv, E):
    K = RC.MAX_TAPS
    x = np.full(K, xv, np.int64)
    th, tl = _tap_digits(np.full(K, hv, np.int64))
    xh, xl = _speech_digits(x)
    early = np.arange(K) < E
    hh = mid = ll = 0
    for seg, sel in enumerate((early, ~early)):          # the accumulators run on over the seam
        hh += int((th * xh)[sel].sum())
        mid += int((th * xl)[sel].sum() + (tl * xh)[sel].sum())
        ll += int((tl * xl)[sel].sum())
        for s in (hh, mid, ll):
            assert abs(s) < 1 << 31
        taps = E if seg == 0 else K
        assert 65536 * hh + 256 * mid + ll + 128 * int(hv) * taps == int(hv) * int(xv) * taps
    # the padding of both segments is zero taps: every term above is there once, so the sums of absolutes bound both epilogues
    for s in (np.abs(th * xh).sum(), np.abs(th * xl).sum() + np.abs(tl * xh).sum(), np.abs(tl * xl).sum()):
        assert int(s) < 1 << 31


def test_split_for_rounds_half_to_even_takes_the_first_peak_and_clamps():
    from gtcrn_micro_amd import GtcrnError
    from gtcrn_micro_amd.data import split_for
    trimmed = np.r_[30000, np.arange(999, 0, -1)].astype(np.int16)            # direct path at tap 0, 1000 taps
    late = np.r_[5, -7, 0, -20000, 20000, np.arange(100, 0, -1)].astype(np.int16)   # first peak at tap 3, 105 taps
    one = np.array([-9], np.int16)
    bank = [trimmed, late, one]
    assert split_for(bank, 0).tolist() == [1, 4, 1] and split_for(bank, 0).dtype == np.int32
    # 16 samples a millisecond; rint is half to even: 0.5 -> 0, 1.5 -> 2, 2.5 -> 2, 3.5 -> 4
    for ms, more in ((1 / 32, 0), (3 / 32, 2), (5 / 32, 2), (7 / 32, 4), (2.5, 40), (0.5, 8), (50, 800)):
        assert split_for(bank, ms).tolist() == [min(1000, 1 + more), min(105, 4 + more), 1], ms
        assert np.array_equal(split_for(bank, ms), TC.split_for(bank, ms))
    assert split_for(bank, 62.4375).tolist() == [1000, 105, 1] and split_for(bank, 62.375).tolist() == [999, 105, 1]
    assert split_for(bank, 1e6).tolist() == [1000, 105, 1]
    for bad in (-0.001, float("nan"), float("inf"), -float("inf")):
        with pytest.raises(GtcrnError):
            split_for(bank, bad)


def test_argument_errors_come_before_anything_is_enqueued():
    """Every refusal below is decided on the arguments alone: no device is touched, so this runs without a GPU."""
    from gtcrn_micro_amd._lib import lib
    Lb = lib()
    x = 0x1000                                           # a stand-in for a device address: refusals never follow it

    def split(pcm=x, soff=x, ns=2, taps=x, roff=x, sp=x, nr=2, table=x, tb=1 << 20, plan=x, rplan=x, B=4, L=8, staged=x, tgt=x,
              stride=8, so=x, spl=x, rec=x, ws=x, form=0):
        return Lb.gtcrn_batch_reverb_split(pcm, soff, ns, taps, roff, sp, nr, table, tb, plan, rplan, B, L, staged, tgt, stride, so,
                                           spl, rec, ws, form, None)

    for kw in (dict(B=0), dict(L=0), dict(L=1 << 31), dict(ns=0), dict(nr=0), dict(pcm=None), dict(soff=None), dict(taps=None),
               dict(roff=None), dict(plan=None), dict(rplan=None), dict(staged=None), dict(so=None), dict(spl=None), dict(rec=None),
               dict(ws=None), dict(stride=7), dict(form=-1), dict(form=5), dict(table=None), dict(table=None, form=2),
               dict(table=None, form=3), dict(table=None, form=4), dict(table=x + 8), dict(tb=8), dict(so=x + 4),
               dict(staged=x + 1), dict(plan=x + 2), dict(rec=x + 2),
               dict(sp=None), dict(tgt=None), dict(sp=None, form=1), dict(tgt=None, form=1), dict(sp=x + 2), dict(tgt=x + 1)):
        assert split(**kw) == ERR_ARG, kw
    assert Lb.gtcrn_last_error()

    def prepare(taps=x, roff=x, sp=x, n=2, table=x, tb=1 << 20):
        return Lb.gtcrn_batch_reverb_split_prepare(taps, roff, sp, n, table, tb, None)

    for kw in (dict(taps=None), dict(roff=None), dict(sp=None), dict(table=None), dict(n=0), dict(table=x + 8), dict(tb=0),
               dict(tb=256), dict(sp=x + 2)):
        assert prepare(**kw) == ERR_ARG, kw
    f = Lb.gtcrn_batch_reverb_split_workspace_bytes
    assert f(0, 8) == 0 and f(4, 0) == 0 and f(4, 1 << 31) == 0
    assert f(1, 1) == 16 and f(8, 64000) == 2 * 8 * 32 * 4 and f(8, 64000) == 2 * Lb.gtcrn_batch_reverb_workspace_bytes(8, 64000)

    def mix(spcm=x, soff=x, ns=2, npcm=x, noff=x, nn=2, tpcm=x, plan=x, B=4, L=8, noisy=x, nst=8, clean=x, cst=8, rec=x, ws=x, passes=7):
        return Lb.gtcrn_batch_mix_target(spcm, soff, ns, npcm, noff, nn, tpcm, plan, B, L, noisy, nst, clean, cst, rec, ws, passes, None)

    for kw in (dict(B=0), dict(L=0), dict(L=1 << 31), dict(ns=0), dict(nn=0), dict(spcm=None), dict(soff=None), dict(npcm=None),
               dict(noff=None), dict(tpcm=None), dict(plan=None), dict(noisy=None), dict(clean=None), dict(rec=None), dict(ws=None),
               dict(nst=7), dict(cst=7), dict(passes=0), dict(passes=8), dict(tpcm=x + 1), dict(noisy=x + 2), dict(rec=x + 4),
               dict(ws=x + 8)):
        assert mix(**kw) == ERR_ARG, kw
    assert Lb.gtcrn_last_error()


def test_python_layer_refuses_what_the_library_would():
    from gtcrn_micro_amd import GtcrnError
    from gtcrn_micro_amd.data import BatchSource, reverb_split_workspace_bytes
    with pytest.raises(GtcrnError):
        reverb_split_workspace_bytes(0, 8)
    with pytest.raises(GtcrnError):
        reverb_split_workspace_bytes(4, 1 << 31)
    with pytest.raises(GtcrnError):
        BatchSource(np.zeros(4, np.int16), noise=np.zeros(4, np.int16), target_ms=5.0)      # host arrays: there is no CPU path
