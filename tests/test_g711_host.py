"""CPU-side checks of the G.711 payloads (include/gtcrn_micro_hip.h, "G.711 payloads"): the symbols and their Python
declarations, the ABI and the state sizes the feature must leave alone, and the two host-only calls -- which run the very
functions the kernels compile -- against tests/g711_checker.py on every code and every int16 value.  No tolerance anywhere."""
import ctypes
import os

import numpy as np
import pytest

from conftest import ROOT

import __graft_entry__ as graft
import g711_checker as GC

SYMBOLS = ["gtcrn_packet_stream_step_g711", "gtcrn_packet_stream_step_slots_g711", "gtcrn_g711_to_f32", "gtcrn_f32_to_g711",
           "gtcrn_g711_decode_table", "gtcrn_g711_encode_pcm16"]
ERR_ARG = -1
ALL_P = np.arange(-32768, 32768, dtype=np.int64)


@pytest.fixture(scope="module", autouse=True)
def _built():
    graft.build()


@pytest.fixture(scope="module")
def L():
    lib = ctypes.CDLL(os.path.join(ROOT, "gtcrn_micro_amd", "libgtcrn_micro_hip.so"))
    for n in ("gtcrn_packet_stream_state_bytes", "gtcrn_stream_state_bytes", "gtcrn_wave_stream_state_bytes",
              "gtcrn_rate_stream_state_bytes"):
        getattr(lib, n).restype = ctypes.c_size_t
    return lib


@pytest.fixture(scope="module")
def host(L):
    """{law: (D int16[256] from the library, E uint8[65536] from the library over every p)}"""
    out = {}
    for law in GC.LAWS:
        tab = (ctypes.c_short * 256)()
        assert L.gtcrn_g711_decode_table(law, tab) == 0
        enc = np.array([L.gtcrn_g711_encode_pcm16(law, int(p)) for p in ALL_P])
        out[law] = (np.array(tab, dtype=np.int16), enc)
    return out


def test_symbols_exported_and_declared(L):
    for n in SYMBOLS:
        assert hasattr(L, n), n
    from gtcrn_micro_amd import _lib
    P = _lib.lib()
    for n in SYMBOLS:
        assert getattr(P, n).argtypes is not None, n
    assert len(P.gtcrn_packet_stream_step_g711.argtypes) == len(P.gtcrn_packet_stream_step_pcm16.argtypes) + 1
    assert len(P.gtcrn_packet_stream_step_slots_g711.argtypes) == len(P.gtcrn_packet_stream_step_slots_pcm16.argtypes) + 1
    import gtcrn_micro_amd as G
    for n in ("g711_to_f32", "f32_to_g711", "g711_decode_table", "g711_encode_pcm16"):
        assert callable(getattr(G, n)) and n in G.__all__, n
    header = open(os.path.join(ROOT, "include", "gtcrn_micro_hip.h")).read()
    for n in SYMBOLS:
        assert f"int {n}(" in header, n


def test_abi_version_and_state_sizes_unchanged(L):
    assert L.gtcrn_abi_version() == 1
    assert L.gtcrn_stream_state_bytes() == 152464
    assert L.gtcrn_wave_stream_state_bytes() == 3088
    assert L.gtcrn_packet_stream_state_bytes(16000, 160) == 2048
    import resample_checker as RC
    for fs, n in ((8000, 80), (8000, 160)):
        up, _, half, _ = RC.design(fs, 16000)
        upo, _, halfo, _ = RC.design(16000, fs)
        ntp = lambda h, u: (2 * h // u + 1 + 3) // 4 * 4      # noqa: E731
        assert L.gtcrn_packet_stream_state_bytes(fs, n) == 4 * (512 + ntp(half, up) + ntp(halfo, upo)), (fs, n)
    assert L.gtcrn_rate_stream_state_bytes(48000) == L.gtcrn_packet_stream_state_bytes(48000, 480) - 2048


@pytest.mark.parametrize("law", GC.LAWS)
def test_decode_table_equals_the_checker(host, law):
    D = host[law][0]
    assert np.array_equal(D, GC.decode_table(law))
    if law == 0:
        assert (D.min(), D.max()) == (-32124, 32124) and len(set(D.tolist())) == 255 and D[0xFF] == 0 and D[0x7F] == 0
    else:
        assert (D.min(), D.max()) == (-32256, 32256) and len(set(D.tolist())) == 256 and 0 not in D


@pytest.mark.parametrize("law", GC.LAWS)
def test_encoder_equals_the_checker_on_every_int16(host, law):
    assert np.array_equal(host[law][1], GC.encode(law, ALL_P))


@pytest.mark.parametrize("law", GC.LAWS)
def test_round_trip_monotonicity_symmetry_and_zero(host, law):
    D, E = host[law]
    back = E[D.astype(np.int64) + 32768]
    bad = np.nonzero(back != np.arange(256))[0].tolist()
    assert bad == ([0x7F] if law == 0 else []), bad            # mu-law negative zero re-encodes as 0xFF
    if law == 0:
        assert back[0x7F] == 0xFF
    # monotone in p: the decoded value of the code never decreases as p grows
    assert (np.diff(D[E].astype(np.int64)) >= 0).all()
    assert E[32768] == GC.ZERO_CODE[law]                        # p = 0
    if law == 0:
        pos = np.arange(1, 32768)
        assert np.array_equal(E[32768 - pos], E[32768 + pos] ^ 0x80)          # E(-p) == E(p) ^ 0x80, p != 0
        assert E[0] == E[1]                                                   # (-32768 clips like -32767)
    from gtcrn_micro_amd import g711_decode_table, g711_encode_pcm16
    assert np.array_equal(g711_decode_table(GC.NAMES[law]), D) and g711_decode_table(law).dtype == np.int16
    for p in (-32768, -1, 0, 1, 777, 32767):
        assert g711_encode_pcm16(GC.NAMES[law], p) == E[p + 32768]


def test_bad_law_and_bad_p_are_argument_errors(L):
    tab = (ctypes.c_short * 256)()
    for law in (-1, 2, 255):
        assert L.gtcrn_g711_decode_table(law, tab) == ERR_ARG
        assert L.gtcrn_g711_encode_pcm16(law, 0) == ERR_ARG
    assert L.gtcrn_g711_decode_table(0, None) == ERR_ARG
    for p in (-32769, 32768, 1 << 20, -(1 << 20)):
        for law in GC.LAWS:
            assert L.gtcrn_g711_encode_pcm16(law, p) == ERR_ARG
    L.gtcrn_last_error.restype = ctypes.c_char_p
    assert L.gtcrn_last_error()
    from gtcrn_micro_amd import GtcrnError, g711_decode_table, g711_encode_pcm16
    for bad in ("mulaw", 2, None, True):
        with pytest.raises(GtcrnError):
            g711_decode_table(bad)
    with pytest.raises(GtcrnError):
        g711_encode_pcm16("alaw", 40000)
    # null handles / bad laws of the device calls answer before the device is touched
    vp, ci, cl = ctypes.c_void_p, ctypes.c_int, ctypes.c_long
    buf = ctypes.create_string_buffer(64)
    p = ctypes.cast(buf, vp)
    f = L.gtcrn_packet_stream_step_g711
    f.argtypes = [vp, vp, vp, vp, vp, cl, vp, cl, ci, ci, vp, vp]
    assert f(None, p, p, p, p, 160, p, 160, 1, 0, p, None) == ERR_ARG
    assert f(None, p, p, p, p, 160, p, 160, 1, 2, p, None) == ERR_ARG
    g = L.gtcrn_packet_stream_step_slots_g711
    g.argtypes = [vp] * 7 + [ci, vp, cl, vp, cl, ci, vp, vp]
    assert g(None, p, p, p, p, p, None, 4, p, 160, p, 160, 1, p, None) == ERR_ARG
    assert g(None, p, p, p, p, p, None, 4, p, 160, p, 160, -1, p, None) == ERR_ARG
    for name in ("gtcrn_g711_to_f32", "gtcrn_f32_to_g711"):
        h = getattr(L, name)
        h.argtypes = [ci, ci, vp, vp, cl, vp]
        assert h(0, 2, p, p, 16, None) == ERR_ARG, name
        assert h(0, 0, None, p, 16, None) == ERR_ARG, name
        assert h(0, 0, p, p, 24, None) == ERR_ARG, name


def test_against_audioop_where_it_exists(host):
    """Python <= 3.12 only: the module is gone from 3.13, and nothing else here needs it."""
    try:
        import audioop
    except ImportError:
        return
    pcm = ALL_P.astype(np.int16).tobytes()
    codes = bytes(range(256))
    for law, dec, enc in ((0, audioop.ulaw2lin, audioop.lin2ulaw), (1, audioop.alaw2lin, audioop.lin2alaw)):
        D, E = host[law]
        assert np.array_equal(np.frombuffer(dec(codes, 2), dtype=np.int16), D)
        ref = np.frombuffer(enc(pcm, 2), dtype=np.uint8)
        differ = np.nonzero(ref != E)[0]
        if law == 1:
            assert differ.size == 0
        else:
            # audioop floors p >> 2 before it takes the magnitude; the library's encoder is symmetric (by design)
            assert differ.size == 381 and (ALL_P[differ] < 0).all()


class _NoLibrary:
    def __call__(self):
        raise AssertionError("the library was called")


def test_python_wrappers_reject_uint8_on_a_lawless_state_before_any_library_call(monkeypatch):
    import torch
    from gtcrn_micro_amd import _lib
    from gtcrn_micro_amd.streaming.gtcrn_micro_stream import StreamGTCRNMicro
    eng = object.__new__(_lib.Engine)
    group = object.__new__(_lib.PacketStreamState)
    slot = object.__new__(_lib.PacketSlotState)
    for st in (group, slot):
        st.g711 = None
        st.packet = 160
    codes = torch.zeros((2, 160), dtype=torch.uint8)
    monkeypatch.setattr(_lib, "lib", _NoLibrary())
    with pytest.raises(_lib.GtcrnError, match="g711"):
        eng.packet_stream_step(group, codes)
    with pytest.raises(_lib.GtcrnError, match="g711"):
        eng.packet_stream_step_slots(slot, torch.zeros(2, dtype=torch.int32), codes)
    # the hop and rate forms take no uint8 at all, law or not
    wave = object.__new__(_lib.WaveStreamState)
    with pytest.raises(_lib.GtcrnError):
        eng._wave_rows(wave, codes, "x")
    for bad in ("mulaw", 2, True):
        with pytest.raises(_lib.GtcrnError):
            _lib.g711_law(bad)
    assert (_lib.g711_law("ulaw"), _lib.g711_law("alaw"), _lib.g711_law(None), _lib.g711_law(1)) == (0, 1, None, 1)
    with pytest.raises(_lib.GtcrnError):
        StreamGTCRNMicro.init_wave_state(object.__new__(StreamGTCRNMicro), 2, None, g711="ulaw")      # g711= without packet=
