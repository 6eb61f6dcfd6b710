"""CPU-side checks of "reverberant speech: exact RIR convolution" (include/gtcrn_micro_hip.h): gtcrn_batch_reverb_plan_host
(the device plan's own function body, run on the host) against the checker, the digit scheme of the matrix form restated in
numpy on the boundary values, the matrix formulation itself restated in numpy against np.convolve, RirBank's host-side
scaling and trimming, the exported symbols and the argument errors."""
import ctypes
import os
import re

import numpy as np
import pytest

from conftest import ROOT

import __graft_entry__ as graft
import batch_checker as BC
import reverb_checker as RC

REVERB_SYMBOLS = ["gtcrn_batch_reverb_plan", "gtcrn_batch_reverb_plan_host", "gtcrn_batch_reverb_table_bytes",
                  "gtcrn_batch_reverb_prepare", "gtcrn_batch_reverb_workspace_bytes", "gtcrn_batch_reverb",
                  "gtcrn_selftest_mfma_i8"]
ERR_ARG = -1
BOUNDARY = [-32768, -32767, -129, -128, -1, 0, 1, 127, 128, 32639, 32640, 32767]


@pytest.fixture(scope="module", autouse=True)
def _built():
    graft.build()


def test_reverb_symbols_exported_declared_and_abi_version_unchanged():
    L = ctypes.CDLL(os.path.join(ROOT, "gtcrn_micro_amd", "libgtcrn_micro_hip.so"))
    header = open(os.path.join(ROOT, "include", "gtcrn_micro_hip.h")).read()
    from gtcrn_micro_amd import _lib
    for n in REVERB_SYMBOLS:
        assert hasattr(L, n), n
        assert re.search(r"\b%s\(" % n, header), f"{n} is not declared in the header"
        assert getattr(_lib.lib(), n).argtypes is not None, f"{n} has no ctypes declaration"
    assert L.gtcrn_abi_version() == 1
    import gtcrn_micro_amd
    from gtcrn_micro_amd import data
    assert gtcrn_micro_amd.RirBank is data.RirBank
    assert data.REVERB_PLAN_DTYPE.itemsize == 8 and data.REVERB_RECORD_DTYPE.itemsize == 16
    assert data.REVERB_PLAN_DTYPE == RC.REVERB_PLAN_DTYPE and data.REVERB_RECORD_DTYPE == RC.REVERB_RECORD_DTYPE
    assert data.REVERB_MAX_TAPS == RC.MAX_TAPS == 16384 and data.REVERB_TAP_MAX == RC.TAP_MAX == 32639
    assert "#define GTCRN_REVERB_MAX_TAPS 16384" in header and "#define GTCRN_REVERB_TAP_MAX 32639" in header


@pytest.mark.parametrize("p", [0.0, 0.3, 1.0])
def test_reverb_plan_host_equals_the_checker(p):
    from gtcrn_micro_amd.data import reverb_plan_host
    B = 96
    for seed, step, item0, n_rir in ((0, 0, 0, 1), (0x123456789abcdef0, 7, 1000, 37), ((1 << 64) - 1, (1 << 40) + 3, 5, 1000),
                                     (11, 5, (1 << 32) - B, (1 << 31) - 1)):
        got = reverb_plan_host(n_rir, p, B, seed, step, item0=item0)
        want = RC.reverb_plan(n_rir, p, B, seed, step, item0=item0)
        assert got.dtype == RC.REVERB_PLAN_DTYPE and got.tobytes() == want.tobytes(), (seed, step, item0, n_rir)
        assert not got["reserved"].any()
        if p == 0.0:
            assert np.all(got["rir"] == -1)
        elif p == 1.0:
            assert np.all((got["rir"] >= 0) & (got["rir"] < n_rir))
        else:
            wet = int((got["rir"] >= 0).sum())
            assert 0 < wet < B and np.all(got["rir"] < n_rir)


def test_ranks_cut_one_global_reverb_plan_and_the_batch_plan_is_untouched():
    from gtcrn_micro_amd.data import plan_host, reverb_plan_host
    B, world, seed, step = 8, 4, 77, 9
    whole = reverb_plan_host(50, 0.5, B * world, seed, step)
    for rank in range(world):
        part = reverb_plan_host(50, 0.5, B, seed, step, item0=rank * B)
        assert part.tobytes() == whole[rank * B:(rank + 1) * B].tobytes()
    assert reverb_plan_host(50, 0.5, B, seed, step + 1).tobytes() != whole[:B].tobytes()
    # block k = 2 is its own: the batch plan (k = 0, 1) of the same seed and step is what the checker always said
    off = np.array([0, 30000, 80000], np.int64)
    BC.assert_same_plan(plan_host(off, off, B, 4000, seed, step), BC.plan(off, off, B, 4000, seed, step))


# ---- the digit scheme, restated: tap = 256 th + tl (balanced), sample = 256 (x >> 8) + ((x & 255) - 128) + 128 ---------------
def _tap_digits(h):
    h = np.asarray(h, np.int64)
    lo = ((h + 128) & 255) - 128
    return (h - lo) >> 8, lo


def _speech_digits(x):
    x = np.asarray(x, np.int64)
    return x >> 8, (x & 255) - 128


def test_digit_scheme_is_exact_on_the_boundary_values():
    x = np.array(BOUNDARY, np.int64)
    h = np.unique(np.clip(np.array(BOUNDARY, np.int64), -RC.TAP_MAX, RC.TAP_MAX))
    th, tl = _tap_digits(h)
    xh, xl = _speech_digits(x)
    for d in (th, tl, xh, xl):
        assert d.min() >= -128 and d.max() <= 127, "a digit does not fit int8"
    assert np.array_equal(256 * th + tl, h) and np.array_equal(256 * xh + xl + 128, x)
    assert _speech_digits(0) == (0, -128)                # the digits zero padding is stored as
    H, X = np.meshgrid(h, x, indexing="ij")
    TH, XH = np.meshgrid(th, xh, indexing="ij")
    TL, XL = np.meshgrid(tl, xl, indexing="ij")
    assert np.array_equal(65536 * TH * XH + 256 * (TH * XL + TL * XH) + TL * XL + 128 * H, H * X)
    # every int16 sample and every legal tap, digit ranges only
    for d in _speech_digits(np.arange(-32768, 32768)) + _tap_digits(np.arange(-RC.TAP_MAX, RC.TAP_MAX + 1)):
        assert d.min() >= -128 and d.max() <= 127


@pytest.mark.parametrize("xv", [32767, -32768])
@pytest.mark.parametrize("hv", [RC.TAP_MAX, -RC.TAP_MAX])
def test_digit_sums_of_16384_extreme_taps_stay_inside_int32_and_recombine_exactly(xv, hv):
    K = RC.MAX_TAPS
    h = np.full(K, hv, np.int64)
    x = np.full(K + 63, xv, np.int64)                    # a whole number of 64-chunks: at most K + 63 terms, the rest zero taps
    hp = np.concatenate([h, np.zeros(63, np.int64)])
    th, tl = _tap_digits(hp)
    xh, xl = _speech_digits(x)
    hh, mid, ll = int((th * xh).sum()), int((th * xl).sum() + (tl * xh).sum()), int((tl * xl).sum())
    for s in (hh, mid, ll, int(np.abs(th * xh).sum()), int(np.abs(th * xl).sum() + np.abs(tl * xh).sum()), int(np.abs(tl * xl).sum())):
        assert abs(s) < 1 << 31
    assert 65536 * hh + 256 * mid + ll + 128 * int(h.sum()) == int(hv) * int(xv) * K


# ---- the matrix formulation, restated: out[16 i + j] = sum_u Hk[j][u] D[u][i], the k order of both reversed -------------------
def _matrix_form(clip, s0, L, h, block=2048):
    K = len(h)
    M = 16 * ((K + 15 + 255) // 256)                     # 16-tap groups: whole 64-tap chunks, and of those whole fours
    idx = 16 * np.arange(M)[:, None, None] + np.arange(16)[None, :, None] - np.arange(16)[None, None, :]      # T[m][j][e] = h[16 m + j - e]
    T = np.where((idx >= 0) & (idx < K), h.astype(np.int64)[np.clip(idx, 0, K - 1)], 0)
    Th, Tl = _tap_digits(T)
    out = np.zeros((L + block - 1) // block * block, np.int64)
    x = clip.astype(np.int64)
    for o0 in range(0, L, block):
        NG = block // 16 + M - 1
        j = s0 + o0 - 16 * (M - 1) + np.arange(NG * 16)                  # the span: block + 16 (M - 1) samples
        span = np.where((j >= 0) & (j < len(x)), x[np.clip(j, 0, len(x) - 1)], 0)
        Xh, Xl = (d.reshape(NG, 16) for d in _speech_digits(span))       # one aligned 16-group per row
        for t in range(block // 256):
            hh, mid, ll = (np.zeros((16, 16), np.int64) for _ in range(3))   # [j][i]
            for m in range(M):
                q = 16 * t + np.arange(16) + M - 1 - m                   # the group column i reads
                hh += Th[m] @ Xh[q].T
                mid += Th[m] @ Xl[q].T + Tl[m] @ Xh[q].T
                ll += Tl[m] @ Xl[q].T
            for a in (hh, mid, ll):
                assert np.abs(a).max() < 1 << 31
            acc = 65536 * hh + 256 * mid + ll + 128 * int(h.astype(np.int64).sum())
            out[o0 + 256 * t:o0 + 256 * (t + 1)] = acc.T.reshape(256)     # out[16 i + j]
    v = (out[:L] + 16384) >> 15
    return np.clip(v, -32768, 32767).astype(np.int16), int(((v < -32768) | (v > 32767)).sum())


@pytest.mark.parametrize("K,L,s0,n", [(1, 17, 0, 40), (15, 255, 14, 300), (16, 16, 16, 20), (17, 300, 1, 200), (63, 100, 62, 500),
                                      (64, 2049, 64, 3000), (65, 2047, 66, 1500), (1000, 257, 999, 1100)])
def test_matrix_formulation_in_numpy_equals_np_convolve(K, L, s0, n):
    rng = np.random.default_rng(K * 7 + L)
    clip = rng.integers(-32768, 32768, n).astype(np.int16)
    clip[:4] = [32767, -32768, 32767, -32768]
    h = rng.integers(-RC.TAP_MAX, RC.TAP_MAX + 1, K).astype(np.int16)
    want, wsat = RC.wet_row(clip, s0, L, h)
    got, gsat = _matrix_form(clip, s0, L, h)
    assert np.array_equal(got, want) and gsat == wsat and (wsat > 0 or K == 1)      # (one tap below 1.0 cannot clamp)
    quiet = (h // 64).astype(np.int16)
    want, wsat = RC.wet_row(clip, s0, L, quiet)
    got, gsat = _matrix_form(clip, s0, L, quiet, block=8192)
    assert np.array_equal(got, want) and gsat == wsat


def test_checker_convolution_is_the_contracts_sum_written_out():
    rng = np.random.default_rng(1)
    clip = rng.integers(-32768, 32768, 50).astype(np.int16)
    h = rng.integers(-3000, 3000, 7).astype(np.int16)
    for s0, L in ((0, 10), (3, 60), (49, 5), (60, 4)):
        got, _ = RC.wet_row(clip, s0, L, h)
        for i in range(L):
            acc = sum(int(h[k]) * int(clip[s0 + i - k]) for k in range(7) if 0 <= s0 + i - k < 50)
            assert int(got[i]) == max(-32768, min(32767, (acc + 16384) >> 15))
        dry, sat = RC.wet_row(clip, s0, L, None)
        assert sat == 0 and np.array_equal(dry, BC.window(clip, np.array([0, 50]), 0, s0, L))


# ---- RirBank's host side -------------------------------------------------------------------------------------------------
def test_quantize_rirs_scales_and_trims():
    from gtcrn_micro_amd import GtcrnError
    from gtcrn_micro_amd.data import quantize_rirs
    h = np.array([0.0, 0.001, -0.5, 0.25, 0.125, 0.0])
    (q,) = quantize_rirs([h], "peak", True)
    assert q.dtype == np.int16 and q.tolist() == [-32639, int(np.rint(0.5 * 32639)), int(np.rint(0.25 * 32639)), 0]
    (q,) = quantize_rirs([h], "peak", False)
    assert q.size == 6 and q[2] == -32639 and q[0] == 0 and q[1] == int(np.rint(0.002 * 32639))
    # energy: sum of squares 1 where the peak allows it
    e = np.array([0.3, 0.2, -0.1, 0.05] * 8)
    (q,) = quantize_rirs([e], "energy", False)
    assert abs(float((q.astype(np.float64) ** 2).sum()) / 32768.0 ** 2 - 1.0) < 1e-3
    (q,) = quantize_rirs([np.array([2.0, 0.1])], "energy", False)         # a lone peak: bounded by the tap range instead
    assert q.tolist() == [32639, int(np.rint(0.05 * 32639))]
    # the first of two equal peaks is the direct path
    (q,) = quantize_rirs([np.array([0.1, 1.0, -1.0, 0.5])], "peak", True)
    assert q.tolist() == [32639, -32639, int(np.rint(0.5 * 32639))]
    # int16 taps are Q15 as they stand
    (q,) = quantize_rirs([np.array([5, -32639, 7], np.int16)], "peak", False)
    assert q.tolist() == [5, -32639, 7]
    (q,) = quantize_rirs([np.array([5, -32639, 7], np.int16)], "peak", True)
    assert q.tolist() == [-32639, 7]
    for bad in ([np.array([1, 32640], np.int16)], [np.zeros(4)], [np.zeros((2, 2))], [np.array([np.nan, 1.0])], [],
                [np.ones(16385)], [np.arange(3)]):
        with pytest.raises(GtcrnError):
            quantize_rirs(bad, "peak", False)
    with pytest.raises(GtcrnError):
        quantize_rirs([h], "rms", True)
    assert quantize_rirs([np.r_[np.zeros(100), np.ones(16384)]], "peak", True)[0].size == 16384


def test_argument_errors_come_before_anything_is_enqueued():
    """Every refusal below is decided on the arguments alone: no device is touched, so this runs without a GPU."""
    from gtcrn_micro_amd._lib import lib
    Lb = lib()
    ss = np.zeros(2, np.uint64)
    rp = np.zeros(4, RC.REVERB_PLAN_DTYPE)
    s, p = ss.ctypes.data, rp.ctypes.data

    def host(n=3, pr=0.5, B=4, item0=0, seed=s, out=p):
        return Lb.gtcrn_batch_reverb_plan_host(n, pr, B, item0, seed, out)

    def dev(n=3, pr=0.5, B=4, item0=0, seed=s, out=p):
        return Lb.gtcrn_batch_reverb_plan(n, pr, B, item0, seed, out, None)

    assert host() == 0
    for f in (host, dev):
        for kw in (dict(n=0), dict(n=-1), dict(pr=-0.1), dict(pr=1.5), dict(pr=float("nan")), dict(B=0), dict(item0=-1),
                   dict(item0=(1 << 32) - 3), dict(seed=None), dict(out=None), dict(seed=s + 4), dict(out=p + 1)):
            assert f(**kw) == ERR_ARG, (f.__name__, kw)
        assert Lb.gtcrn_last_error()

    x = 0x1000                                           # a stand-in for a device address: refusals never follow it

    def reverb(pcm=x, soff=x, ns=2, taps=x, roff=x, nr=2, table=x, tb=1 << 20, plan=x, rplan=x, B=4, L=8, staged=x, stride=8,
               so=x, sp=x, rec=x, ws=x, form=0):
        return Lb.gtcrn_batch_reverb(pcm, soff, ns, taps, roff, nr, table, tb, plan, rplan, B, L, staged, stride, so, sp, rec, ws,
                                     form, None)

    for kw in (dict(B=0), dict(L=0), dict(L=1 << 31), dict(ns=0), dict(nr=0), dict(pcm=None), dict(soff=None), dict(taps=None),
               dict(roff=None), dict(plan=None), dict(rplan=None), dict(staged=None), dict(so=None), dict(sp=None), dict(rec=None),
               dict(ws=None), dict(stride=7), dict(form=-1), dict(form=5), dict(table=None), dict(table=None, form=2),
               dict(table=None, form=3), dict(table=None, form=4),
               dict(table=x + 8), dict(tb=8), dict(so=x + 4), dict(staged=x + 1), dict(plan=x + 2), dict(rec=x + 2)):
        assert reverb(**kw) == ERR_ARG, kw
    assert Lb.gtcrn_last_error()

    def prepare(taps=x, roff=x, n=2, table=x, tb=1 << 20):
        return Lb.gtcrn_batch_reverb_prepare(taps, roff, n, table, tb, None)

    for kw in (dict(taps=None), dict(roff=None), dict(table=None), dict(n=0), dict(table=x + 8), dict(tb=0), dict(tb=256)):
        assert prepare(**kw) == ERR_ARG, kw
    off = np.array([0, 1, 50, 50 + 16384], np.int64)
    tb = Lb.gtcrn_batch_reverb_table_bytes
    # a 16-tap group is 512 bytes; a response of K taps holds ceil((K + 15) / 256) times sixteen groups, behind a 256-byte header
    assert tb(off.ctypes.data, 3) == 256 + 512 * 16 * (1 + 1 + 65)
    assert tb(None, 3) == 0 and tb(off.ctypes.data, 0) == 0
    assert tb(np.array([0, 0], np.int64).ctypes.data, 1) == 0 and tb(np.array([0, 16385], np.int64).ctypes.data, 1) == 0
    f = Lb.gtcrn_batch_reverb_workspace_bytes
    assert f(0, 8) == 0 and f(4, 0) == 0 and f(4, 1 << 31) == 0
    assert f(1, 1) == 16 and f(8, 64000) == 8 * 32 * 4 and f(3, 64001) >= f(3, 64000)


def test_python_layer_refuses_what_the_library_would():
    from gtcrn_micro_amd import GtcrnError
    from gtcrn_micro_amd.data import RirBank, reverb_plan_host
    with pytest.raises(GtcrnError):
        reverb_plan_host(0, 0.5, 4, 0, 0)
    with pytest.raises(GtcrnError):
        reverb_plan_host(3, 1.5, 4, 0, 0)
    with pytest.raises(GtcrnError):
        RirBank(np.zeros(4, np.int16), np.zeros(2, np.int64))         # host arrays: there is no CPU path
    with pytest.raises(GtcrnError):
        RirBank.from_arrays([])
