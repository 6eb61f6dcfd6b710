"""CPU-side checks of the level meters (include/gtcrn_micro_hip.h, "level meters"): the checker of tests/meter_checker.py
accepts the stated accumulation order and rejects five seeded bugs; gtcrn_level_dbov on exact cases; the ABI version and
the state sizes are what they were; the setter without a model is an argument error before the device is touched."""
import ctypes
import os

import numpy as np
import pytest

from conftest import ROOT

import __graft_entry__ as graft
import meter_checker as MC

torch = pytest.importorskip("torch")

K = 12


@pytest.fixture(scope="module", autouse=True)
def _built():
    graft.build()


@pytest.fixture(scope="module")
def stream():
    """One stream of K hops: `out` the emitted blocks (block 0 the structural zero block), `dry` the blocks aligned with
    them (the input one hop late, zeros for block 0), `x` the input hops.  The largest output sample is negative."""
    rng = np.random.default_rng(11)
    x = (rng.standard_normal((K, 256)) * 0.1).astype(np.float32)
    out = (rng.standard_normal((K, 256)) * 0.05).astype(np.float32)
    out[0] = 0
    out[5, 77] = -0.9
    dry = np.concatenate([np.zeros((1, 256), np.float32), x[:-1]])
    return x, out, dry


def test_header_states_the_depth():
    assert MC.header_depth() == 10


def test_checker_accepts_the_stated_order(stream):
    _, out, dry = stream
    rec = MC.emulate(out, dry)
    assert MC.problems(rec, out, dry) == []
    assert rec[3] == K and rec[2] == np.float32(0.9)
    # a window that starts from an earlier record; a subset of the hops
    first = MC.emulate(out, dry, range(5))
    assert MC.same_bits(MC.emulate(out, dry, range(5, K), start=first), rec)
    assert MC.problems(MC.emulate(out, dry, range(5, K), start=first), out, dry, range(5, K), start=first) == []
    assert MC.problems(MC.emulate(out, dry, [3, 4]), out, dry, [3, 4]) == []
    # zeros: exact
    z = np.zeros((3, 256), np.float32)
    assert MC.same_bits(MC.emulate(z, z), np.array([0, 0, 0, 3], np.float32))
    MC.check(MC.emulate(z, z), z, z)
    # the float32 record is NOT the float64 sum: the bound is doing work, and it is tight enough to see one sample
    e64 = MC.reference(out, dry)
    assert float(rec[1]) != e64[1] and abs(float(rec[1]) - e64[1]) <= MC.bound(K) * e64[1] < e64[1] / (256 * K) / 100


def test_checker_rejects_a_sample_left_out(stream):
    _, out, dry = stream
    for which, blocks in ((1, out), (0, dry)):
        cut = blocks.copy()
        cut[7, 255] = 0                    # the device "forgot" sample 255 of hop 7
        rec = MC.emulate(cut if which else out, dry if which else cut)
        bad = MC.problems(rec, out, dry)
        assert len(bad) == 1 and bad[0].startswith("E_out" if which else "E_dry"), bad


def test_checker_rejects_the_dry_block_one_hop_late(stream):
    _, out, dry = stream
    late = np.concatenate([np.zeros((1, 256), np.float32), dry[:-1]])
    bad = MC.problems(MC.emulate(out, late), out, dry)
    assert len(bad) == 1 and bad[0].startswith("E_dry"), bad


def test_checker_rejects_a_peak_without_the_absolute_value(stream):
    _, out, dry = stream
    rec = MC.emulate(out, dry)
    rec[2] = out.max()                     # max y instead of max |y|: the largest sample is negative
    assert rec[2] < np.float32(0.9)
    bad = MC.problems(rec, out, dry)
    assert len(bad) == 1 and bad[0].startswith("peak"), bad


def test_checker_rejects_an_uncounted_zero_block(stream):
    _, out, dry = stream
    rec = MC.emulate(out, dry, range(1, K))          # the first hop's zero block skipped: the energies are right
    bad = MC.problems(rec, out, dry)
    assert len(bad) == 1 and bad[0].startswith("blocks"), bad


def _per_call(out, dry, calls):
    """The seeded bug: the hops of a call are summed first and the call's sum is added to the record."""
    rec = np.zeros(4, np.float32)
    k = 0
    for n in calls:
        part = MC.emulate(out, dry, range(k, k + n))
        rec[0] = np.float32(rec[0] + part[0])
        rec[1] = np.float32(rec[1] + part[1])
        rec[2] = max(rec[2], part[2])
        rec[3] = np.float32(rec[3] + part[3])
        k += n
    return rec


def test_accumulation_per_hop_is_partition_invariant_and_per_call_is_not(stream):
    _, out, dry = stream
    parts = ([1] * 12, [3] * 4, [6, 6])

    def stated(calls):
        rec, k = None, 0
        for n in calls:
            rec = MC.emulate(out, dry, range(k, k + n), start=rec)
            k += n
        return rec
    recs = [stated(c) for c in parts]
    assert all(MC.same_bits(r, recs[0]) for r in recs)
    wrong = [_per_call(out, dry, c) for c in parts]
    assert MC.same_bits(wrong[0], recs[0])                                       # one hop per call: the same thing
    assert not MC.same_bits(wrong[1], wrong[0]) or not MC.same_bits(wrong[2], wrong[0])
    assert not MC.same_bits(wrong[2], recs[0])
    for w in wrong:                        # (within the bound all the same: only the bit pattern shows this bug)
        assert MC.problems(w, out, dry) == []


def test_level_dbov_exact_cases():
    from gtcrn_micro_amd import level_dbov
    from gtcrn_micro_amd._lib import lib
    L = lib()
    assert L.gtcrn_level_dbov(256.0, 256.0) == 0                    # mean square 1.0
    assert L.gtcrn_level_dbov(128.0, 256.0) == 3                    # 0.5: a full-scale sine
    assert L.gtcrn_level_dbov(1e-6, 1.0) == 60
    assert L.gtcrn_level_dbov(10.0 ** -12.74, 1.0) == 127           # 127.4 dB down: clamped
    assert L.gtcrn_level_dbov(0.0, 256.0) == 127
    assert L.gtcrn_level_dbov(-1.0, 256.0) == 127
    assert L.gtcrn_level_dbov(-0.0, 256.0) == 127
    assert L.gtcrn_level_dbov(512.0, 256.0) == 0                    # above full scale: clamped
    assert L.gtcrn_level_dbov(1.0, 0.0) == 127
    assert L.gtcrn_level_dbov(1.0, -4.0) == 127
    # a quarter of a dB either side of the rounding boundaries at 19.5, 59.5 and 126.5 dB
    for edge in (19.5, 59.5, 126.5):
        assert L.gtcrn_level_dbov(10.0 ** (-(edge - 0.25) / 10), 1.0) == int(edge - 0.5), edge
        assert L.gtcrn_level_dbov(10.0 ** (-(edge + 0.25) / 10), 1.0) == int(edge + 0.5), edge
    assert L.gtcrn_level_dbov(10.0 ** (-0.25 / 10), 1.0) == 0 and L.gtcrn_level_dbov(10.0 ** (-0.75 / 10), 1.0) == 1
    # the Python helper: scalars and arrays
    assert level_dbov(128.0, 256) == 3 and isinstance(level_dbov(128.0, 256), int)
    got = level_dbov(np.array([256.0, 128.0, 0.0, 2.56e-4]), 256.0)
    assert got.dtype == np.int32 and got.tolist() == [0, 3, 127, 60]
    assert level_dbov(np.array([[1.0], [0.5]]), np.array([1.0, 0.0])).tolist() == [[0, 127], [3, 127]]


def test_symbols_exported_and_declared():
    L = ctypes.CDLL(os.path.join(ROOT, "gtcrn_micro_amd", "libgtcrn_micro_hip.so"))
    with open(os.path.join(ROOT, "include", "gtcrn_micro_hip.h")) as f:
        header = f.read()
    assert hasattr(L, "gtcrn_wave_stream_set_meters") and hasattr(L, "gtcrn_level_dbov")
    assert "int gtcrn_wave_stream_set_meters(gtcrn_model *m, float *d_meters);" in header
    assert "int gtcrn_level_dbov(double energy, double nsamples);" in header


def test_abi_version_and_state_sizes_unchanged():
    from gtcrn_micro_amd import Engine
    from gtcrn_micro_amd._lib import lib, packet_stream_state_bytes, rate_stream_state_bytes
    assert hasattr(lib(), "gtcrn_wave_stream_set_meters")
    assert lib().gtcrn_abi_version() == 1
    assert Engine.state_bytes() == 4 * 38116 == 152464
    assert Engine.wave_state_bytes() == 4 * (512 + 256 + 4) == 3088
    assert rate_stream_state_bytes(48000) == 1056 and packet_stream_state_bytes(16000, 160) == 2048      # as before the meters


def test_setter_without_a_model_is_an_argument_error():
    from gtcrn_micro_amd._lib import lib
    L = lib()
    p = ctypes.c_void_p(16)           # never dereferenced: the call is rejected before the device is touched
    assert L.gtcrn_wave_stream_set_meters(None, p) == -1
    assert b"null model" in L.gtcrn_last_error()
    assert L.gtcrn_wave_stream_set_meters(None, None) == -1
