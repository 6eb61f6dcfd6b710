"""CPU-side checks of "telephone-channel rows: exact 8 kHz band + G.711" (include/gtcrn_micro_hip.h): the filter table against
the checker's design and the header's figures, gtcrn_batch_phone_plan_host (the device plan's own function body, run on the
host) against the checker, gtcrn_batch_phone_host -- the very functions the kernel compiles, run row by row on the host --
against tests/phone_checker.py BIT FOR BIT for every codec and both targets, the exported symbols and the argument errors.
Nothing below has a tolerance: the contract is integers."""
import ctypes
import os
import re

import numpy as np
import pytest

from conftest import ROOT

import __graft_entry__ as graft
import batch_checker as BC
import phone_checker as PC
import reverb_checker as RC

PHONE_SYMBOLS = ["gtcrn_batch_phone_taps", "gtcrn_batch_phone_chunk", "gtcrn_batch_phone_plan", "gtcrn_batch_phone_plan_host",
                 "gtcrn_batch_phone", "gtcrn_batch_phone_host"]
ERR_ARG = -1
TARGETS = [("narrow", 0), ("wide", 1)]


@pytest.fixture(scope="module", autouse=True)
def _built():
    graft.build()


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.int32)


def test_phone_symbols_exported_declared_and_abi_version_unchanged():
    L = ctypes.CDLL(os.path.join(ROOT, "gtcrn_micro_amd", "libgtcrn_micro_hip.so"))
    header = open(os.path.join(ROOT, "include", "gtcrn_micro_hip.h")).read()
    from gtcrn_micro_amd import _lib, data
    for n in PHONE_SYMBOLS:
        assert hasattr(L, n), n
        assert re.search(r"\b%s\(" % n, header), f"{n} is not declared in the header"
        assert getattr(_lib.lib(), n).argtypes is not None, f"{n} has no ctypes declaration"
    assert L.gtcrn_abi_version() == 1
    assert data.PHONE_PLAN_DTYPE.itemsize == 8 and data.PHONE_RECORD_DTYPE.itemsize == 16
    assert data.PHONE_PLAN_DTYPE == PC.PHONE_PLAN_DTYPE and data.PHONE_RECORD_DTYPE == PC.PHONE_RECORD_DTYPE
    assert data.PHONE_CODECS == PC.CODECS
    assert "#define GTCRN_PHONE_TAPS 129" in header
    C = data.phone_chunk()
    assert C == L.gtcrn_batch_phone_chunk() and C >= 512 and C % 4 == 0


def test_taps_equal_the_checkers_table_and_the_headers_figures():
    from gtcrn_micro_amd.data import phone_taps
    got = phone_taps()
    T, h = PC.taps()
    assert got.dtype == np.int32 and got.shape == (129,) and np.array_equal(got, T)
    assert int(T.sum()) == 32766 and int(T.max()) == 15360 == int(T[64]) and int(np.abs(T).sum()) == 69558
    assert int((T == 0).sum()) == 10 and np.array_equal(T, T[::-1])
    assert int(T[0::2].sum()) == 16378 and int(T[1::2].sum()) == 16388
    x = 32768.0 * h
    assert np.abs(np.abs(x - np.floor(x)) - 0.5).min() > 0.003      # no entry near a rounding tie: two designs cannot disagree
    # the response of the integer table itself
    f = np.arange(0.0, 8000.5, 5.0)
    H = np.abs(np.exp(-2j * np.pi * np.outer(f, np.arange(129) - 64) / 16000.0) @ (T / 32768.0))
    dB = 20.0 * np.log10(np.maximum(H, 1e-12))
    assert dB[f <= 3500].max() < 0.0025 and dB[f <= 3500].min() > -0.1125
    assert dB[f >= 4500].max() < -70.0 and abs(dB[-1] + 70.3) < 0.05
    # the bounds the kernel's 32-bit partial sums rest on (csrc/phone.h)
    for part in (T[65:], T[:65], T[0::2], T[1::2]):
        assert 32768 * int(np.abs(part).sum()) < 1 << 31
    assert 32768 * int(np.abs(T).sum()) >= 1 << 31


@pytest.mark.parametrize("p", [0.0, 0.3, 1.0])
def test_phone_plan_host_equals_the_checker(p):
    from gtcrn_micro_amd.data import phone_plan_host
    B = 96
    for seed, step, item0, mask in ((0, 0, 0, 7), (0x123456789abcdef0, 7, 1000, 5), ((1 << 64) - 1, (1 << 40) + 3, 5, 6),
                                    (11, 5, (1 << 32) - B, 2)):
        got = phone_plan_host(p, mask, B, seed, step, item0=item0)
        want = PC.phone_plan(p, mask, B, seed, step, item0=item0)
        assert got.dtype == PC.PHONE_PLAN_DTYPE and got.tobytes() == want.tobytes(), (seed, step, item0, mask)
        assert not got["reserved"].any()
        if p == 0.0:
            assert np.all(got["codec"] == -1)
        elif p == 1.0:
            assert np.all(got["codec"] >= 0)
        else:
            n = int((got["codec"] >= 0).sum())
            assert 0 < n < B


@pytest.mark.parametrize("mask", [1, 2, 3, 4, 5, 6, 7])
def test_every_mask_yields_only_and_all_of_its_own_codecs(mask):
    from gtcrn_micro_amd.data import PHONE_CODECS, phone_plan_host
    own = {c for c in range(3) if (mask >> c) & 1}
    got = phone_plan_host(1.0, mask, 200, 5, 3)
    assert set(got["codec"].tolist()) == own
    assert got.tobytes() == PC.phone_plan(1.0, mask, 200, 5, 3).tobytes()
    names = [n for n, c in PHONE_CODECS.items() if c in own]
    assert phone_plan_host(1.0, names, 200, 5, 3).tobytes() == got.tobytes()


def test_ranks_cut_one_global_phone_plan_and_the_other_plans_are_untouched():
    from gtcrn_micro_amd.data import phone_plan_host, plan_host, reverb_plan_host
    B, world, seed, step = 8, 4, 77, 9
    whole = phone_plan_host(0.5, 7, B * world, seed, step)
    for rank in range(world):
        part = phone_plan_host(0.5, 7, B, seed, step, item0=rank * B)
        assert part.tobytes() == whole[rank * B:(rank + 1) * B].tobytes()
    assert phone_plan_host(0.5, 7, 64, seed, step + 1).tobytes() != phone_plan_host(0.5, 7, 64, seed, step).tobytes()
    # block k = 3 is its own: the batch plan (k = 0, 1) and the reverb plan (k = 2) of the same seed and step are what their
    # checkers always said
    off = np.array([0, 30000, 80000], np.int64)
    BC.assert_same_plan(plan_host(off, off, B, 4000, seed, step), BC.plan(off, off, B, 4000, seed, step))
    assert reverb_plan_host(50, 0.5, B, seed, step).tobytes() == RC.reverb_plan(50, 0.5, B, seed, step).tobytes()


# ---- the channel: the host twin against the checker ---------------------------------------------------------------------------
def _lengths():
    from gtcrn_micro_amd.data import phone_chunk
    C = phone_chunk()
    return [1, 2, 63, 64, 65, 127, 128, 129, 257, C - 1, C, C + 1, 2 * C + 3]


@pytest.mark.parametrize("codec", [0, 1, 2])
def test_host_twin_equals_the_checker_bit_for_bit(codec):
    from gtcrn_micro_amd.data import phone_channel_host
    clipped_down = clipped_up = 0
    for L in _lengths():
        n, c = PC.rows_for(L)
        plan = PC.make_plan([codec] * len(n))
        for name, tg in TARGETS:
            wn, wc, wr = PC.phone(n, c, plan, tg)
            gn, gc, gr = phone_channel_host(n, c, plan, name)
            assert gr.tobytes() == wr.tobytes(), (L, name, gr, wr)
            assert np.array_equal(_bits(gn), _bits(wn)), (L, name, np.argwhere(_bits(gn) != _bits(wn))[:4])
            assert np.array_equal(_bits(gc), _bits(wc)), (L, name, np.argwhere(_bits(gc) != _bits(wc))[:4])
            if tg == 1:
                assert np.array_equal(_bits(gc), _bits(c))
        gn, gc, gr = phone_channel_host(n, None, plan, "narrow")        # noisy only
        assert gc is None and gr.tobytes() == wr.tobytes() and np.array_equal(_bits(gn), _bits(wn))
        # the all-zero row stays all zero -- but through A-law, which has no zero: D_A[E_A(0)] = 8
        assert int(wr["saturated_down"][2]) == 0 and int(wr["saturated_up"][2]) == 0 and (codec == 2) == bool(_bits(wn[2]).any())
        clipped_down += int(wr["saturated_down"].sum())
        clipped_up += int(wr["saturated_up"].sum())
    assert clipped_down > 0 and clipped_up > 0, "no case clipped a sample"


def test_mixed_plans_wide_band_rows_and_entries_out_of_range():
    from gtcrn_micro_amd.data import phone_channel_host
    L = 301
    n, c = PC.rows_for(L, seed=3)
    plan = PC.make_plan([0, 1, 2, -1, 7, -5])
    for name, tg in TARGETS:
        wn, wc, wr = PC.phone(n, c, plan, tg)
        gn, gc, gr = phone_channel_host(n, c, plan, name)
        assert gr.tobytes() == wr.tobytes() and np.array_equal(_bits(gn), _bits(wn)) and np.array_equal(_bits(gc), _bits(wc))
        assert gr["codec"].tolist() == [0, 1, 2, -1, -1, -1]
        assert np.array_equal(_bits(gn[3:]), _bits(n[3:])) and np.array_equal(_bits(gc[3:]), _bits(c[3:]))
    # the codecs differ from one another and from the source
    assert not np.array_equal(wn[0], wn[1]) and not np.array_equal(wn[0], n[0])


def test_full_scale_pattern_clips_the_decimator():
    from gtcrn_micro_amd.data import phone_channel_host
    x = PC.full_scale(3000)[None]
    _, down, up, _, _ = PC.channel_row(x[0], 0)
    assert down == 642 and up > 0
    for codec in (0, 1, 2):
        plan = PC.make_plan([codec])
        wn, _, wr = PC.phone(x, None, plan, 0)
        gn, _, gr = phone_channel_host(x, None, plan, "narrow")
        assert int(wr["saturated_down"][0]) == 642 and gr.tobytes() == wr.tobytes() and np.array_equal(_bits(gn), _bits(wn))


def test_checker_sanity_a_tone_in_the_band_comes_back_within_one_lsb():
    """Checker only (the device and the host twin must equal it): a 1 kHz tone of amplitude 8000 through codec 0."""
    t = np.arange(4000)
    x = (8000.0 * np.sin(2.0 * np.pi * 1000.0 * t / 16000.0) / 32768.0).astype(np.float32)
    out, down, up, _, _ = PC.channel_row(x, 0)
    err = (np.rint(out.astype(np.float64) * 32768.0) - PC.pcm16(x))[300:-300]
    assert down == 0 and up == 0 and np.abs(err).max() <= 1
    # and a 6 kHz tone does not come back at all: 70 dB down is below one LSB at this amplitude
    y = (8000.0 * np.sin(2.0 * np.pi * 6000.0 * t / 16000.0) / 32768.0).astype(np.float32)
    out, _, _, _, _ = PC.channel_row(y, 0)
    assert np.abs(np.rint(out.astype(np.float64) * 32768.0))[300:-300].max() <= 4


def test_checker_g711_maps_are_the_librarys():
    """The checker restates both laws from the header's formulas; the library's host calls run the kernels' own functions."""
    from gtcrn_micro_amd._lib import lib
    Lb = lib()
    p = np.arange(-32768, 32768)
    for law, enc, dec in ((0, PC.ulaw_encode, PC.ulaw_decode), (1, PC.alaw_encode, PC.alaw_decode)):
        table = np.zeros(256, np.int16)
        assert Lb.gtcrn_g711_decode_table(law, table.ctypes.data_as(ctypes.POINTER(ctypes.c_short))) == 0
        assert np.array_equal(dec(np.arange(256)), table.astype(np.int64))
        step = 7 if law else 5
        assert all(int(enc(np.array([v]))[0]) == Lb.gtcrn_g711_encode_pcm16(law, int(v)) for v in p[::step])
        assert np.abs(dec(enc(p)) - p).max() <= 1024 and np.all(np.diff(dec(enc(p))) >= 0)


def test_a_nan_or_inf_row_changes_no_bit_of_another_row():
    from gtcrn_micro_amd.data import phone_channel_host
    n, c = PC.rows_for(500, seed=5)
    plan = PC.make_plan([0, 1, 2, 1, -1, 2])
    gn, gc, gr = phone_channel_host(n, c, plan, "narrow")
    bad_n, bad_c = n.copy(), c.copy()
    bad_n[1, 100], bad_n[1, 101], bad_c[1, 7] = np.nan, np.inf, -np.inf
    hn, hc, hr = phone_channel_host(bad_n, bad_c, plan, "narrow")
    keep = [0, 2, 3, 4, 5]
    assert np.array_equal(_bits(hn[keep]), _bits(gn[keep])) and np.array_equal(_bits(hc[keep]), _bits(gc[keep]))
    assert hr[keep].tobytes() == gr[keep].tobytes()


def test_argument_errors_come_before_anything_is_enqueued():
    """Every refusal below is decided on the arguments alone: no device is touched, so this runs without a GPU."""
    from gtcrn_micro_amd._lib import lib
    Lb = lib()

    def why():
        return Lb.gtcrn_last_error().decode()

    ss = np.zeros(2, np.uint64)
    pl = np.zeros(4, PC.PHONE_PLAN_DTYPE)
    s, p = ss.ctypes.data, pl.ctypes.data

    def host(pr=0.5, mask=7, B=4, item0=0, seed=s, out=p):
        return Lb.gtcrn_batch_phone_plan_host(pr, mask, B, item0, seed, out)

    def dev(pr=0.5, mask=7, B=4, item0=0, seed=s, out=p):
        return Lb.gtcrn_batch_phone_plan(pr, mask, B, item0, seed, out, None)

    assert host() == 0
    for f in (host, dev):
        for kw, word in ((dict(pr=-0.1), "p_phone"), (dict(pr=1.5), "p_phone"), (dict(pr=float("nan")), "p_phone"),
                         (dict(mask=0), "codec_mask"), (dict(mask=8), "codec_mask"), (dict(mask=-1), "codec_mask"),
                         (dict(B=0), "B must"), (dict(item0=-1), "item0"), (dict(item0=(1 << 32) - 3), "item0"),
                         (dict(seed=None), "null"), (dict(out=None), "null"), (dict(seed=s + 4), "misaligned"),
                         (dict(out=p + 1), "misaligned")):
            assert f(**kw) == ERR_ARG, (f.__name__, kw)
            assert word in why(), (f.__name__, kw, why())

    B, L = 3, 40
    src_n, src_c = np.zeros((B, L), np.float32), np.zeros((B, L), np.float32)
    out_n, out_c = np.zeros((B, L), np.float32), np.zeros((B, L), np.float32)
    plan, rec = PC.make_plan([0, 1, -1]), np.zeros(B, PC.PHONE_RECORD_DTYPE)
    x = 0x10000                                          # stand-ins for device addresses, apart: refusals never follow them
    cases = ((dict(B=0), "positive"), (dict(L=0), "positive"), (dict(L=1 << 31), "positive"), (dict(sn=None), "null"),
             (dict(on=None), "null"), (dict(plan=None), "null"), (dict(rec=None), "null"), (dict(sc=None), "both"),
             (dict(oc=None), "both"), (dict(sns=L - 1), "stride"), (dict(ons=L - 1), "stride"), (dict(scs=L - 1), "stride"),
             (dict(ocs=L - 1), "stride"), (dict(target=2), "target"), (dict(target=-1), "target"), (dict(sn_off=2), "misaligned"),
             (dict(rec_off=2), "misaligned"), (dict(on="sn"), "overlaps"), (dict(oc="sc"), "overlaps"), (dict(on="sc"), "overlaps"),
             (dict(oc="sn"), "overlaps"), (dict(on="sn", on_off=4 * (B * L - 1)), "overlaps"),
             (dict(on="sn", on_off=-4 * (B * L - 1)), "overlaps"))

    def host_call(ptr):
        def f(B=B, L=L, sn="sn", sc="sc", on="on", oc="oc", plan="plan", rec="rec", sns=L, scs=L, ons=L, ocs=L, target=0, sn_off=0,
              rec_off=0, on_off=0):
            a = {k: (None if v is None else ptr[v]) for k, v in dict(sn=sn, sc=sc, on=on, oc=oc, plan=plan, rec=rec).items()}
            a["sn"] = a["sn"] + sn_off if a["sn"] is not None else None
            a["rec"] = a["rec"] + rec_off if a["rec"] is not None else None
            a["on"] = a["on"] + on_off if a["on"] is not None else None
            return a, (a["sn"], sns, a["sc"], scs, a["plan"], B, L, a["on"], ons, a["oc"], ocs, target, a["rec"])
        return f

    host_ptr = dict(sn=src_n.ctypes.data, sc=src_c.ctypes.data, on=out_n.ctypes.data, oc=out_c.ctypes.data, plan=plan.ctypes.data,
                    rec=rec.ctypes.data)
    fake_ptr = dict(sn=x, sc=2 * x, on=3 * x, oc=4 * x, plan=5 * x, rec=6 * x)
    assert Lb.gtcrn_batch_phone_host(*host_call(host_ptr)()[1]) == 0
    for kw, word in cases:
        assert Lb.gtcrn_batch_phone_host(*host_call(host_ptr)(**kw)[1]) == ERR_ARG, kw
        assert word in why(), (kw, why())
        assert Lb.gtcrn_batch_phone(*host_call(fake_ptr)(**kw)[1], None) == ERR_ARG, kw
        assert word in why(), (kw, why())
    # rows that interleave without sharing a byte are ranges that overlap all the same: refused
    wide = np.zeros((B, 2 * L), np.float32)
    a = (wide.ctypes.data, 2 * L, None, 0, plan.ctypes.data, B, L, wide.ctypes.data + 4 * L, 2 * L, None, 0, 0, rec.ctypes.data)
    assert Lb.gtcrn_batch_phone_host(*a) == ERR_ARG and "overlaps" in why()


def test_python_layer_refuses_what_the_library_would():
    from gtcrn_micro_amd import GtcrnError
    from gtcrn_micro_amd.data import phone_channel, phone_channel_host, phone_plan_host
    for bad in (dict(p_phone=1.5, codecs=7), dict(p_phone=0.5, codecs=0), dict(p_phone=0.5, codecs=8),
                dict(p_phone=0.5, codecs=("gsm",)), dict(p_phone=0.5, codecs=())):
        with pytest.raises(GtcrnError):
            phone_plan_host(bad["p_phone"], bad["codecs"], 4, 0, 0)
    n = np.zeros((2, 10), np.float32)
    with pytest.raises(GtcrnError):
        phone_channel_host(n, None, PC.make_plan([0, 1]), "medium")
    with pytest.raises(GtcrnError):
        phone_channel_host(n, None, PC.make_plan([0]), "narrow")
    with pytest.raises(GtcrnError):
        phone_channel(n)                                 # host arrays: the device call takes device tensors
