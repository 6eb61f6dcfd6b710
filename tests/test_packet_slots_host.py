"""CPU-side checks of packet stream slots (gtcrn_packet_stream_*_slots, include/gtcrn_micro_hip.h): the symbols, the ABI and
state sizes the feature must leave alone, the plan emulator against the library's own hop schedule, and the argument checks
that answer before the device is touched."""
import ctypes
import os
from math import gcd

import pytest

from conftest import ROOT

import __graft_entry__ as graft
import packet_plan_emulator as PE

SLOT_SYMBOLS = ["gtcrn_packet_stream_reset_slots", "gtcrn_packet_stream_step_slots", "gtcrn_packet_stream_step_slots_pcm16"]
ERR_ARG = -1


@pytest.fixture(scope="module", autouse=True)
def _built():
    graft.build()


@pytest.fixture(scope="module")
def L():
    lib = ctypes.CDLL(os.path.join(ROOT, "gtcrn_micro_amd", "libgtcrn_micro_hip.so"))
    lib.gtcrn_packet_stream_state_bytes.restype = ctypes.c_size_t
    lib.gtcrn_stream_state_bytes.restype = ctypes.c_size_t
    lib.gtcrn_wave_stream_state_bytes.restype = ctypes.c_size_t
    lib.gtcrn_rate_stream_state_bytes.restype = ctypes.c_size_t
    return lib


def test_symbols_exported_and_abi_version_unchanged(L):
    for n in SLOT_SYMBOLS:
        assert hasattr(L, n), n
    assert L.gtcrn_abi_version() == 1


def test_state_sizes_unchanged(L):
    """The phase is a NEW array: none of the existing per-stream states grew."""
    assert L.gtcrn_stream_state_bytes() == 152464
    assert L.gtcrn_wave_stream_state_bytes() == 3088
    assert L.gtcrn_packet_stream_state_bytes(16000, 160) == 2048
    assert L.gtcrn_packet_stream_state_bytes(16000, 320) == 2048
    # [two FIFOs of 256 | the two stage histories]: the packet form's own formula (tests/test_packet_host.py)
    import resample_checker as RC
    for fs, n in ((48000, 480), (8000, 80), (44100, 441)):
        up, _, half, _ = RC.design(fs, 16000)
        upo, _, halfo, _ = RC.design(16000, fs)
        ntp = lambda h, u: (2 * h // u + 1 + 3) // 4 * 4
        assert L.gtcrn_packet_stream_state_bytes(fs, n) == 4 * (512 + ntp(half, up) + ntp(halfo, upo)), (fs, n)
    assert L.gtcrn_rate_stream_state_bytes(48000) == L.gtcrn_packet_stream_state_bytes(48000, 480) - 2048


@pytest.mark.parametrize("n16", [160, 320, 256, 147])
def test_plan_emulator_against_the_library_schedule(L, n16):
    """Every start phase that is a multiple of g, one whole period and one call more: the emulator's hops and next phase
    are gtcrn_packet_stream_schedule's, and its tables list the stepping rows in row order."""
    g = gcd(n16, 256)
    period = 256 // g
    assert PE.hmax_of(n16) == (256 - g + n16) // 256
    nxt = ctypes.c_int()
    starts = list(range(0, 256, g))
    phase = list(starts)                       # slot s starts at phase starts[s]
    slots = list(range(len(starts)))[::-1]     # (named in descending order: the tables must follow the ROWS)
    lib_phase = list(starts)
    for _ in range(period + 1):
        before = list(phase)
        h, tabs, pos, old = PE.plan(phase, slots, len(slots), n16)
        for i, s in enumerate(slots):
            want_h = L.gtcrn_packet_stream_schedule(16000, n16, lib_phase[s], ctypes.byref(nxt))
            assert (h[i], phase[s], old[i]) == (want_h, nxt.value, before[s]), (n16, s)
            lib_phase[s] = nxt.value
        for r, tab in enumerate(tabs):
            assert tab == [s for i, s in enumerate(slots) if h[i] > r]
            assert [pos[r][i] for i in range(len(slots)) if h[i] > r] == list(range(len(tab)))
            assert all(pos[r][i] == -1 for i in range(len(slots)) if h[i] <= r)
        assert max(h) <= PE.hmax_of(n16) and len(tabs) == PE.hmax_of(n16)
    assert phase != starts or period == 1      # one call past the period: not where it began
    for _ in range(period - 1):
        PE.plan(phase, slots, len(slots), n16)
    assert phase == starts                     # 2 period calls: back


def test_plan_emulator_clamps_the_count_and_leaves_other_slots():
    phase = [0, 96, 192, 32]
    h, tabs, _, old = PE.plan(phase, [2, 0, 3, 1], 7, 160, max_active=3)
    assert h == [1, 0, 0] and old == [192, 0, 32] and tabs == [[2]]
    assert phase == [160, 96, 96, 192]                       # slot 1 (row 3, beyond max_active) keeps its phase
    assert PE.plan(phase, [2, 0], -4, 160)[0] == [] and phase == [160, 96, 96, 192]


def test_argument_errors_answer_before_the_device(L):
    """Null handle: GTCRN_ERR_ARG from all three entry points (no device is needed to say so)."""
    vp = ctypes.c_void_p
    buf = ctypes.create_string_buffer(64)
    p = ctypes.cast(buf, vp)
    L.gtcrn_packet_stream_reset_slots.argtypes = [vp] * 7 + [ctypes.c_int, vp]
    assert L.gtcrn_packet_stream_reset_slots(None, p, p, p, p, p, None, 4, None) == ERR_ARG
    for fn in ("gtcrn_packet_stream_step_slots", "gtcrn_packet_stream_step_slots_pcm16"):
        f = getattr(L, fn)
        f.argtypes = [vp] * 7 + [ctypes.c_int, vp, ctypes.c_long, vp, ctypes.c_long, vp, vp]
        assert f(None, p, p, p, p, p, None, 4, p, 160, p, 160, p, None) == ERR_ARG, fn
