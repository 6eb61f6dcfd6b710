"""CPU-side checks of the conference mix (include/gtcrn_micro_hip.h, "conference rooms"): the ABI, the parameter words and their
refusals, and the host twins gtcrn_mix_rooms_host / _pcm16_host (the functions the kernel compiles) against the contract in
numpy float32 (tests/mixer_checker.py), bit for bit, over the cases of tests/mixer_cases.py; then the stated consequences:
rooms do not see each other, a lone participant hears zeros, a steady mix is the plain sum, a talker leaves over one block,
a NaN or Inf leg is an absent leg."""
import ctypes
import os
import re

import numpy as np
import pytest

from conftest import ROOT
import mixer_checker as MK
import mixer_cases as MC

import __graft_entry__ as graft

F = np.float32
ERR_ARG = -1
CASES = MC.all_cases()
POISON = MC.poison_cases()


@pytest.fixture(scope="module", autouse=True)
def _built():
    graft.build()


def host(x, out, room_start, seats, rec, params, nrooms, voice):
    from gtcrn_micro_amd import mix_rooms_host
    mix_rooms_host(x, out, room_start, seats, rec, params, nrooms, voice)


def test_symbols_exported_and_declared_and_abi_version():
    L = ctypes.CDLL(os.path.join(ROOT, "gtcrn_micro_amd", "libgtcrn_micro_hip.so"))
    with open(os.path.join(ROOT, "include", "gtcrn_micro_hip.h")) as f:
        header = f.read()
    from gtcrn_micro_amd import _lib
    for n in ("gtcrn_mix_rooms", "gtcrn_mix_rooms_pcm16", "gtcrn_mix_rooms_host", "gtcrn_mix_rooms_pcm16_host", "gtcrn_mix_params_host"):
        assert hasattr(L, n), n
        assert re.search(r"\bint\s+%s\s*\(" % n, header), n
        assert getattr(_lib.lib(), n).argtypes, n
    assert "conference rooms:" in header and "gtcrn_mix_config" in header
    assert re.search(r"#define\s+GTCRN_MIX_MAX_ROOM\s+1024\b", header) and "GTCRN_MIX_DEFAULTS" in header
    assert re.search(r"#define\s+GTCRN_ABI_VERSION\s+1\b", header)
    assert L.gtcrn_abi_version() == 1


def test_params_words_and_refusals():
    from gtcrn_micro_amd import GtcrnError, mix_params
    assert MK.same_bits(mix_params(), MK.params())
    assert mix_params().tolist()[:4] == [3.0, float(F(1e-5)), 0.125, float(F(10 ** 0.3))]
    for kw in (dict(k=1), dict(k=8, floor_dbov=-37.5), dict(release=0.0), dict(release=1.0, incumbent_db=0.0),
               dict(k=5, floor_dbov=-61.3, release=0.3, incumbent_db=7.7)):
        ck = dict(kw)
        if "release" in ck:
            ck["alpha"] = ck.pop("release")
        assert MK.same_bits(mix_params(**kw), MK.params(**ck)), kw
    for kw, reason in ((dict(k=0), "k must lie in 1 .. 8"), (dict(k=9), "k must lie in 1 .. 8"),
                       (dict(release=-0.01), "alpha outside [0, 1]"), (dict(release=1.5), "alpha outside [0, 1]"),
                       (dict(incumbent_db=-1.0), "incumbent_db is negative"), (dict(floor_dbov=float("nan")), "not finite"),
                       (dict(release=float("inf")), "not finite"), (dict(incumbent_db=float("inf")), "not finite"),
                       (dict(loudness=1), "unknown mixer fields")):
        with pytest.raises(GtcrnError, match=re.escape(reason)):
            mix_params(**kw)
    from gtcrn_micro_amd import _lib
    assert _lib.lib().gtcrn_mix_params_host(None, None) == ERR_ARG
    assert b"null pointer" in _lib.lib().gtcrn_last_error()


def test_argument_errors_have_reasons():
    from gtcrn_micro_amd import _lib
    L = _lib.lib()
    c = MC.sizes_case(160)
    x, out = c["ticks"][0][0], np.zeros((20, 160), F)
    buf = np.zeros(512, np.uint8)
    base = buf.ctypes.data + (-buf.ctypes.data) % 16
    seats, rec, prm = base, base + 64 * 4, base + 64 * 4 + 64
    start = c["room_start"]
    good = [x.ctypes.data, 160, 20, out.ctypes.data, 160, 20, 160, start.ctypes.data, seats, 0, 0, None, rec, 1, prm, None, 0]
    assert L.gtcrn_mix_rooms_host(*good) == 0
    for pos, val, reason in ((6, 0, "n must lie"), (6, 1025, "n must lie"), (2, -1, "negative count"), (10, -1, "negative count"),
                             (13, -2, "negative count"), (7, None, "null pointer"), (8, None, "null pointer"),
                             (12, None, "null pointer"), (14, None, "null pointer"), (0, None, "null pointer"),
                             (1, 159, "stride"), (4, 100, "stride"), (8, seats + 4, "misaligned"), (12, rec + 8, "misaligned"),
                             (14, prm + 4, "misaligned"), (0, x.ctypes.data + 2, "misaligned"),
                             (3, x.ctypes.data + 4 * 160, "overlap"), (15, rec, "voice_stride")):
        bad = list(good)
        bad[pos] = val
        assert L.gtcrn_mix_rooms_host(*bad) == ERR_ARG, (pos, val)
        assert reason.encode() in L.gtcrn_last_error(), (reason, L.gtcrn_last_error())
        assert L.gtcrn_mix_rooms(*bad, None) == ERR_ARG, (pos, val)      # refused before any launch: no device is touched


@pytest.mark.parametrize("pad", [5, 0])
@pytest.mark.parametrize("pcm", [False, True], ids=["f32", "pcm16"])
@pytest.mark.parametrize("name,c", CASES, ids=[n for n, _ in CASES])
def test_host_twin_equals_checker(name, c, pcm, pad):
    MC.run(c, host, pcm, pad)


@pytest.mark.parametrize("name,c", POISON, ids=[n for n, _ in POISON])
def test_host_twin_equals_checker_on_non_finite_blocks(name, c):
    MC.run(c, host, False, 5)
    MC.run(c, host, False, 0)


def test_the_cases_take_the_branches_they_are_named_for():
    """What the checker did with the cases: who was picked, who faded, how many contributed."""
    g = lambda trace, t: trace[t][1][:, 0].tolist()
    tr = MC.run(MC.tie_case(), host, False, 5)
    assert g(tr, 0) == [1, 1, 0, 0, 0], "equal keys: the two lowest seat positions of the four (rec 0 and 1; rec 4 is quiet)"
    tr = MC.run(MC.incumbent_case(2.0), host, False, 5)
    assert g(tr, 0) == [1, 0, 0] and g(tr, 1) == [1, 0, 0], "2 dB above an incumbent with 3 dB of incumbency: it stays"
    tr = MC.run(MC.incumbent_case(4.0), host, False, 5)
    assert g(tr, 0) == [1, 0, 0] and g(tr, 1) == [0, 1, 0], "4 dB above: the challenger takes the place"
    for k in (3, 8):
        c = MC.change_case(k)
        tr = MC.run(c, host, False, 5)
        assert g(tr, 0)[:2 * k] == [1] * k + [0] * k and g(tr, 1)[:2 * k] == [0] * k + [1] * k
        # block 1: the listeners in the tail hear k fading out and k fading in; block 2: the k new talkers at full gain
        x1, x2 = c["ticks"][1][0], c["ticks"][2][0]
        ramp = np.arange(1, 161).astype(F) / F(160)
        want = np.zeros(160, F)
        for p in range(2 * k):
            want = want + (F(1) - ramp if p < k else ramp) * x1[p]
        assert MK.same_bits(tr[1][0][2 * k], want) and want[-1] != 0
        steady = np.zeros(160, F)
        for p in range(k, 2 * k):
            steady = steady + x2[p]
        assert MK.same_bits(tr[2][0][2 * k], steady), "no change of talkers: the plain ordered sum"
        last = (F(1) - ramp)[-1]
        assert last == 0, "a fade-out ends at exactly zero: the talker is gone after one block"
    tr = MC.run(MC.saturating_case(), host, True, 5)
    assert tr[1][0][3].tolist() == [32767, -32768] * 80 and tr[1][0][0].tolist() == [32767, -32768] * 80
    tr = MC.run(MC.silent_case(), host, False, 0)
    assert not tr[1][0][:5].any() and not tr[1][1][:, :3].any() and tr[1][1][:, 3].tolist() == [2.0] * 5
    tr = MC.run(MC.sizes_case(160), host, False, 5)
    assert not tr[1][0][0].any(), "a lone participant hears zeros"


def _per_room(c, trace_out, trace_rec):
    """{room's tuple of recs: (its output rows, its records)} of a case whose seats have out_row = rec."""
    rooms = {}
    for r in range(len(c["room_start"]) - 1):
        ids = [int(s[2]) for s in c["seats"][c["room_start"][r]:c["room_start"][r + 1]]]
        rooms[tuple(ids)] = (trace_out[ids].tobytes(), trace_rec[ids].tobytes())
    return rooms


@pytest.mark.parametrize("pcm", [False, True], ids=["f32", "pcm16"])
def test_rooms_do_not_see_each_other(pcm):
    """A permutation of the rooms, and the same rooms among others, give every room the same bits."""
    c = MC.sequence_case()
    base = MC.run(c, host, pcm, 5)
    rooms = [[tuple(int(v) for v in s[:3]) for s in c["seats"][c["room_start"][r]:c["room_start"][r + 1]]] for r in range(4)]
    extra = [(20 + i, 20 + i, 20 + i) for i in range(5)]
    rng = np.random.default_rng(3)
    more = [np.concatenate([x, np.zeros((1, 160), F), MC.noise(rng, 5, 160, [0.3])]) for x, _, _ in c["ticks"]]
    for order, ticks in (([2, 0, 3, 1], c["ticks"]), ([3, 2, 1, 0], c["ticks"]), ([1, "extra", 0, 3, 2], [(x, None, None) for x in more])):
        c2 = MC.case(160, [extra if r == "extra" else rooms[r] for r in order], ticks, n_rec=25 if "extra" in order else None, alpha=0.25)
        other = MC.run(c2, host, pcm, 5)
        for t in range(len(base)):
            a, b = _per_room(c, *base[t]), _per_room(c2, *other[t])
            for ids in a:
                assert a[ids] == b[ids], (order, t, ids)


def test_rooms_at_or_above_nrooms_are_untouched():
    c = MC.nrooms_case(2)
    tr = MC.run(c, host, False, 5)
    out, rec = tr[1]
    assert (out[7:] == MC.GUARD_F).all() and not rec[7:].any(), "rooms 2 and 3 (participants 7 ..): no output, no record"
    assert (rec[:7, 3] == 2).all() and (out[:7] != MC.GUARD_F).all()


@pytest.mark.parametrize("bad", [np.nan, np.inf, -np.inf, 1e30], ids=["nan", "inf", "-inf", "square_overflows"])
def test_a_non_finite_leg_is_an_absent_leg_and_moves_no_other_room(bad):
    poisoned = MC.run(MC.poisoned_case(F(bad)), host, False, 5)
    clean = MC.run(MC.poisoned_case(F(bad), clean=True), host, False, 5)
    for t in range(3):
        for rows in (slice(0, 3), slice(7, 10)):
            assert MK.same_bits(poisoned[t][0][rows], clean[t][0][rows]) and MK.same_bits(poisoned[t][1][rows], clean[t][1][rows])
        assert np.isfinite(poisoned[t][0][:10]).all() and np.isfinite(poisoned[t][1]).all()
    # in its own room the block is a lost packet: the same bits as a table whose seat has in_row = -1 in that block
    c = MC.poisoned_case(F(bad), clean=True)
    lost = MC.poisoned_case(F(bad), absent=True)
    rec = np.zeros((10, 4), F)
    for t, (x, _, _) in enumerate(c["ticks"]):
        out = np.full((12, 160), MC.GUARD_F, F)
        tab = lost if t == 1 else c
        MK.mix(x, out, tab["room_start"], tab["seats"], rec, c["params"])
        assert MK.same_bits(out, poisoned[t][0]) and MK.same_bits(rec, poisoned[t][1]), t
