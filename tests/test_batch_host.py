"""CPU-side checks of "training batches from a resident corpus" (include/gtcrn_micro_hip.h): the checker's Philox against
the Random123 known answers, gtcrn_batch_plan_host (the device plan's own function body, run on the host) against the
checker, the exported symbols and the argument errors."""
import ctypes
import os
import re

import numpy as np
import pytest

from conftest import ROOT

import __graft_entry__ as graft
import batch_checker as BC

BATCH_SYMBOLS = ["gtcrn_batch_plan", "gtcrn_batch_plan_host", "gtcrn_batch_workspace_bytes", "gtcrn_batch_pairs",
                 "gtcrn_batch_mix"]
ERR_ARG = -1
G = 16000


@pytest.fixture(scope="module", autouse=True)
def _built():
    graft.build()


def test_checker_philox_reproduces_the_random123_known_answers():
    kat = [((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
           ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
           ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0),
            (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1))]
    for ctr, key, want in kat:
        assert BC.philox4x32_10(ctr, key) == want


def test_batch_symbols_exported_declared_and_abi_version_unchanged():
    L = ctypes.CDLL(os.path.join(ROOT, "gtcrn_micro_amd", "libgtcrn_micro_hip.so"))
    header = open(os.path.join(ROOT, "include", "gtcrn_micro_hip.h")).read()
    from gtcrn_micro_amd import _lib
    for n in BATCH_SYMBOLS:
        assert hasattr(L, n), n
        assert re.search(r"\b%s\(" % n, header), f"{n} is not declared in the header"
        assert getattr(_lib.lib(), n).argtypes is not None, f"{n} has no ctypes declaration"
    assert L.gtcrn_abi_version() == 1
    assert "#define GTCRN_ABI_VERSION 1" in header
    import gtcrn_micro_amd
    from gtcrn_micro_amd import data
    assert gtcrn_micro_amd.BatchSource is data.BatchSource and gtcrn_micro_amd.Corpus is data.Corpus
    assert data.PLAN_DTYPE.itemsize == 32 and data.RECORD_DTYPE.itemsize == 40
    assert data.PLAN_DTYPE == BC.PLAN_DTYPE and data.RECORD_DTYPE == BC.RECORD_DTYPE


def _offsets(lengths):
    return np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)


L0 = 4000
EDGE_LENGTHS = [1, L0 - 1, L0, L0 + 1, L0 + 1, L0 + G, L0 + G, L0 + 3 * G + 5, 7, 160000, 52001]


@pytest.mark.parametrize("granule", [1, G])
@pytest.mark.parametrize("item0", [0, 1000])
@pytest.mark.parametrize("given", [False, True])
def test_plan_host_equals_the_checker(granule, item0, given):
    from gtcrn_micro_amd.data import plan_host
    rng = np.random.default_rng(5)
    soff = _offsets(EDGE_LENGTHS + list(rng.integers(1, 200000, 300)))
    noff = _offsets([1, 3, 100, L0 + 5] + list(rng.integers(1, 50000, 40)))
    B = 64
    n = soff.size - 1
    # every edge length is drawn at least once when the clips are given
    clips = (np.arange(B) % len(EDGE_LENGTHS)).astype(np.int32) if given else None
    for seed, step in ((0, 0), (0x123456789abcdef0, 7), ((1 << 64) - 1, (1 << 40) + 3)):
        got = plan_host(soff, noff, B, L0, seed, step, item0=item0, granule=granule, clips=clips)
        want = BC.plan(soff, noff, B, L0, seed, step, item0=item0, granule=granule, clips=clips)
        BC.assert_same_plan(got, want)
        lens = (soff[1:] - soff[:-1])[got["sclip"]]
        assert np.all((got["sclip"] >= 0) & (got["sclip"] < n))
        assert np.all(got["sstart"] % granule == 0)
        assert np.all(np.where(lens >= L0, got["sstart"] + L0 <= lens, got["sstart"] == 0))
        nlens = (noff[1:] - noff[:-1])[got["nclip"]]
        assert np.all((got["nstart"] >= 0) & (got["nstart"] < nlens))
        assert np.all((got["snr_db"] >= -5) & (got["snr_db"] <= 20) & (got["lvl_db"] >= -35) & (got["lvl_db"] <= -15))
    # pairs: no noise table
    got = plan_host(soff, None, B, L0, 3, 4, item0=item0, granule=granule, clips=clips)
    BC.assert_same_plan(got, BC.plan(soff, None, B, L0, 3, 4, item0=item0, granule=granule, clips=clips))
    assert not got["nclip"].any() and not got["nstart"].any()


def test_step_and_item0_enter_only_through_the_counter():
    from gtcrn_micro_amd.data import plan_host
    soff, noff = _offsets([30000, 50000, 4000, 99]), _offsets([777, 5])
    a = plan_host(soff, noff, 8, 4000, 11, 5, item0=20)
    b = plan_host(soff, noff, 1, 4000, 11, 5, item0=23)
    assert a[3:4].tobytes() == b.tobytes()
    assert plan_host(soff, noff, 8, 4000, 11, 6, item0=20).tobytes() != a.tobytes()
    assert plan_host(soff, noff, 8, 4000, 12, 5, item0=20).tobytes() != a.tobytes()
    assert plan_host(soff, noff, 8, 4000, 11, 5, item0=20).tobytes() == a.tobytes()


@pytest.mark.parametrize("granule", [1, G])
def test_every_legal_start_occurs_and_no_illegal_one(granule):
    from gtcrn_micro_amd.data import plan_host
    L = 4000
    soff = _offsets([L + 3 * granule + (granule - 1)])          # Ks = 4, and the clip's tail does not make a fifth
    p = plan_host(soff, None, 256, L, 2, 0, granule=granule)
    assert sorted(set(p["sstart"].tolist())) == [0, granule, 2 * granule, 3 * granule]


def test_argument_errors_come_before_anything_is_enqueued():
    """Every refusal below is decided on the arguments alone: no device is touched, so this runs without a GPU."""
    from gtcrn_micro_amd._lib import lib
    Lb = lib()
    off = _offsets([10, 20])
    o = off.ctypes.data
    ss = np.zeros(2, np.uint64)
    plan = np.zeros(4, BC.PLAN_DTYPE)
    s, p = ss.ctypes.data, plan.ctypes.data

    def host(soff=o, n=2, noff=o, nn=2, B=4, L=8, item0=0, granule=1, snr=(-5.0, 20.0), lvl=(-35.0, -15.0), seed=s, out=p):
        return Lb.gtcrn_batch_plan_host(soff, n, noff, nn, B, L, item0, granule, snr[0], snr[1], lvl[0], lvl[1], None, seed, out)

    def dev(soff=o, n=2, noff=o, nn=2, B=4, L=8, item0=0, granule=1, snr=(-5.0, 20.0), lvl=(-35.0, -15.0), seed=s, out=p):
        return Lb.gtcrn_batch_plan(soff, n, noff, nn, B, L, item0, granule, snr[0], snr[1], lvl[0], lvl[1], None, seed, 1, out, None)

    assert host() == 0
    for f in (host, dev):
        bad = [dict(B=0), dict(B=-1), dict(L=0), dict(L=-5), dict(n=0), dict(nn=0), dict(soff=None), dict(seed=None), dict(out=None),
               dict(granule=0), dict(snr=(1.0, 0.5)), dict(lvl=(-15.0, -35.0)), dict(item0=-1), dict(L=1 << 31)]
        for kw in bad:
            assert f(**kw) == ERR_ARG, (f.__name__, kw)
        assert Lb.gtcrn_last_error()
    assert host(noff=None, nn=0) == 0                    # no noise table is the pairs form, not an error
    assert host(snr=(3.0, 3.0), lvl=(-20.0, -20.0)) == 0 and np.all(plan["snr_db"] == 3.0) and np.all(plan["lvl_db"] == -20.0)

    x = 0x1000                                           # a stand-in for a device address: refusals never follow it

    def pairs(a=x, b=x, off_=x, n=2, plan_=x, B=4, L=8, noisy=x, ns=8, clean=x, cs=8):
        return Lb.gtcrn_batch_pairs(a, b, off_, n, plan_, B, L, noisy, ns, clean, cs, None)

    def mix(a=x, ao=x, na=2, b=x, bo=x, nb=2, plan_=x, B=4, L=8, noisy=x, ns=8, clean=x, cs=8, rec=x, ws=x, passes=7):
        return Lb.gtcrn_batch_mix(a, ao, na, b, bo, nb, plan_, B, L, noisy, ns, clean, cs, rec, ws, passes, None)

    for kw in (dict(B=0), dict(L=0), dict(n=0), dict(a=None), dict(b=None), dict(off_=None), dict(plan_=None), dict(noisy=None),
               dict(clean=None), dict(ns=7), dict(cs=7)):
        assert pairs(**kw) == ERR_ARG, kw
    for kw in (dict(B=0), dict(L=0), dict(na=0), dict(nb=0), dict(a=None), dict(ao=None), dict(b=None), dict(bo=None),
               dict(plan_=None), dict(noisy=None), dict(clean=None), dict(ns=7), dict(cs=7), dict(rec=None), dict(ws=None),
               dict(passes=0), dict(passes=8)):
        assert mix(**kw) == ERR_ARG, kw
    f = Lb.gtcrn_batch_workspace_bytes
    assert f(0, 8) == 0 and f(4, 0) == 0 and f(4, 1 << 31) == 0
    assert f(1, 1) > 0 and f(1, 1) % 16 == 0 and f(6, 64000) == 6 * f(1, 64000) and f(3, 64001) >= f(3, 64000)


def test_python_layer_refuses_what_the_library_would():
    from gtcrn_micro_amd import GtcrnError
    from gtcrn_micro_amd.data import Corpus, plan_host
    with pytest.raises(GtcrnError):
        plan_host(_offsets([5]), None, 2, 4, 0, 0, granule=0)
    with pytest.raises(GtcrnError):
        plan_host(_offsets([5]), None, 2, 4, 0, 0, snr_db=(5.0, 4.0))
    with pytest.raises(GtcrnError):
        Corpus.from_arrays([])
    with pytest.raises(GtcrnError):
        Corpus.from_arrays([np.zeros(4, np.float32)])
    with pytest.raises(GtcrnError):
        Corpus(np.zeros(4, np.int16), np.zeros(2, np.int64))      # host arrays: there is no CPU path


def test_from_wavs_refuses_other_rates_and_layouts(tmp_path):
    from gtcrn_micro_amd import GtcrnError
    from gtcrn_micro_amd.data import Corpus
    from gtcrn_micro_amd.infer import write_wav_pcm16
    from scipy.io import wavfile
    p8, pst, pf = str(tmp_path / "a8k.wav"), str(tmp_path / "stereo.wav"), str(tmp_path / "f32.wav")
    write_wav_pcm16(p8, np.zeros(100, np.float32), fs=8000)
    wavfile.write(pst, 16000, np.zeros((100, 2), np.int16))
    wavfile.write(pf, 16000, np.zeros(100, np.float32))
    for p in (p8, pst, pf):
        with pytest.raises(GtcrnError, match="16 kHz mono 16-bit"):
            Corpus.from_wavs([p])
