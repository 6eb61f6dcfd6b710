"""The cases of the conference mix that tests/test_mixer_host.py runs through the host twin and tests/test_gpu_mixer.py through
the kernel, each against tests/mixer_checker.py, bit for bit.  A case is a dict: n, room_start, seats (S, 4), n_rec, params,
ticks: a list of (x, voice or None, nrooms or None), x (n_in, n) float32; the records are carried from tick to tick."""
import numpy as np

import mixer_checker as MK

F = np.float32
GUARD_F, GUARD_I = F(12345.0), np.int16(12345)
AMPS = [0.0, 1e-3, 0.03, 0.1, 0.3]
SIZES_N = (1, 63, 64, 65, 160, 256, 441, 960, 1024)


def tables(rooms):
    """rooms: lists of seats (in_row, out_row, rec) -> room_start, seats."""
    start = np.cumsum([0] + [len(r) for r in rooms]).astype(np.int32)
    seats = np.array([s + (0,) for r in rooms for s in r] or np.zeros((0, 4)), np.int32).reshape(-1, 4)
    return start, seats


def plain_rooms(sizes, first=0):
    """Rooms of the given sizes over consecutive participants: row = rec = id."""
    rooms, p = [], first
    for s in sizes:
        rooms.append([(p + i, p + i, p + i) for i in range(s)])
        p += s
    return rooms, p


def noise(rng, rows, n, amps=AMPS):
    return (rng.standard_normal((rows, n)) * rng.choice(amps, rows)[:, None]).astype(F)


def case(n, rooms, ticks, n_rec=None, params=None, rec0=None, **kw):
    start, seats = tables(rooms) if isinstance(rooms, list) else rooms
    n_rec = n_rec if n_rec is not None else int(max([s[2] for s in seats] + [0])) + 1
    return dict(n=n, room_start=start, seats=seats, n_rec=n_rec, params=MK.params(**kw) if params is None else params,
                ticks=ticks, rec0=rec0)


def sizes_case(n, seed=0, big=False):
    """Rooms of 0, 1, 2, 3, K, K + 1 and 2K + 1 seats (with big: of 65 and 1024 too), two blocks of noise at mixed levels."""
    rng = np.random.default_rng(1000 * n + seed)
    rooms, total = plain_rooms([0, 1, 2, 3, 3, 4, 7] + ([65, 1024] if big else []))
    return case(n, rooms, [(noise(rng, total, n), None, None) for _ in range(2)])


def absent_case():
    rng = np.random.default_rng(5)
    rooms = [[(0, 0, 0), (-1, 1, 1), (2, -1, 2), (-1, -1, 3), (4, 4, 4)], [(5, 5, 5), (-1, 6, 6)]]
    return case(160, rooms, [(noise(rng, 7, 160, [0.1, 0.3]), None, None) for _ in range(3)], k=2)


def tie_case():
    """Equal blocks, so equal levels and keys: the lower seat positions win."""
    rng = np.random.default_rng(6)
    w = noise(rng, 1, 160, [0.1])
    x = np.concatenate([np.repeat(w, 4, 0), noise(rng, 1, 160, [0.01])])
    rooms = [[(4, 4, 4), (0, 0, 0), (1, 1, 1), (2, 2, 2), (3, 3, 3)]]
    return case(160, rooms, [(x, None, None), (x, None, None)], k=2)


def incumbent_case(db):
    """K = 1.  Block 0 puts seat 0 in the mix; in block 1 seat 1 is `db` dB above it."""
    rng = np.random.default_rng(7)
    w = noise(rng, 1, 160, [0.05])[0]
    x0 = np.stack([w, np.zeros(160, F), np.zeros(160, F)])
    x1 = np.stack([w, (w.astype(np.float64) * 10 ** (db / 20)).astype(F), np.zeros(160, F)])
    rooms, _ = plain_rooms([3])
    return case(160, rooms, [(x0, None, None), (x1, None, None)], k=1)


def change_case(k):
    """All k talkers change in one block (alpha = 1: the levels follow at once): k fade out, k fade in, 2k contributors."""
    rng = np.random.default_rng(8 + k)
    size = 2 * k + 2
    loud, soft = lambda: noise(rng, k, 160, [0.3]), lambda: noise(rng, k, 160, [0.02])
    tail = lambda: noise(rng, 2, 160, [1e-3])
    rooms, _ = plain_rooms([size])
    return case(160, rooms, [(np.concatenate([loud(), soft(), tail()]), None, None),
                             (np.concatenate([soft(), loud(), tail()]), None, None),
                             (np.concatenate([soft(), loud(), tail()]), None, None)], k=k, alpha=1.0)


def sequence_case(n=160):
    rng = np.random.default_rng(9)
    rooms, total = plain_rooms([2, 5, 9, 3])
    return case(n, rooms, [(noise(rng, total, n), None, None) for _ in range(6)], alpha=0.25)


def voice_case():
    """The voice words decide (at a stride of 8, as in a level-control record); the floor is out of reach."""
    rng = np.random.default_rng(10)
    rooms, total = plain_rooms([4, 6])
    ticks = []
    for _ in range(4):
        v = np.zeros(8 * total, F)
        v[3::8] = rng.choice([0.0, 1.0, 1.0], total)
        ticks.append((noise(rng, total, 256, [0.03, 0.3]), v[3::8], None))
    return case(256, rooms, ticks, floor_dbov=60.0)


def silent_case():
    rooms, total = plain_rooms([4, 1])
    return case(320, rooms, [(np.zeros((total, 320), F), None, None)] * 2)


def saturating_case():
    """Three full-scale in-phase talkers: a listener's sum is 3, the int16 form clips."""
    x = np.ones((4, 160), F)
    x[:, 1::2] = -1.0
    x[3] = 0
    rooms, _ = plain_rooms([4])
    return case(160, rooms, [(x, None, None), (x, None, None)])


def poisoned_case(bad, clean=False, absent=False):
    """Three rooms; in block 1 seat 1 of room 1 holds `bad` in one sample (clean: it does not; absent: its in_row is -1 in every
    block, which a non-finite block must equal in that room)."""
    rng = np.random.default_rng(11)
    rooms, total = plain_rooms([3, 4, 3])
    if absent:
        rooms[1][1] = (-1, 4, 4)
    xs = [noise(rng, total, 160, [0.1, 0.3]) for _ in range(3)]
    if not clean:
        xs[1][4, 77] = bad
    return case(160, rooms, [(x, None, None) for x in xs])


def wild_table_case():
    """Rows and rec out of range: the rows count as -1, the seats of a bad rec are ignored."""
    rng = np.random.default_rng(12)
    rooms = [[(0, 0, 0), (99999, 1, 1), (-7, 2, 2), (3, 6, 3), (4, -2, 4), (5, 5, -3), (1, 3, 6), (2, 4, 5)]]
    return case(160, rooms, [(noise(rng, 6, 160, [0.1, 0.3]), None, None) for _ in range(2)], n_rec=6)


def broken_rooms_case():
    """room_start decreases (room 1), spans 1025 seats (room 3) and leaves the table (room 5); rooms 0, 2 and 4 are live."""
    rng = np.random.default_rng(13)
    start = np.array([3, 6, 1, 3, 1028, 1031, 99999], np.int32)
    seats = np.zeros((1031, 4), np.int32)
    seats[:, :3] = 8                                      # (never run)
    for k, s in enumerate([1, 2, 3, 4, 5, 1028, 1029, 1030]):
        seats[s, :3] = k
    return case(160, (start, seats), [(noise(rng, 9, 160, [0.1, 0.3]), None, None) for _ in range(2)], n_rec=9)


def nrooms_case(live):
    rng = np.random.default_rng(14)
    rooms, total = plain_rooms([3, 4, 2, 5])
    return case(160, rooms, [(noise(rng, total, 160, [0.1, 0.3]), None, live) for _ in range(2)])


def all_cases():
    """(name, case) of every case both forms, float32 and int16, run."""
    out = [("sizes_n%d" % n, sizes_case(n)) for n in SIZES_N]
    out += [("big_rooms_n160", sizes_case(160, 1, big=True)), ("big_rooms_n64", sizes_case(64, 2, big=True)),
            ("absent", absent_case()), ("tie", tie_case()), ("incumbent_2db", incumbent_case(2.0)),
            ("incumbent_4db", incumbent_case(4.0)), ("change_k3", change_case(3)), ("change_k8", change_case(8)),
            ("sequence", sequence_case()), ("sequence_n441", sequence_case(441)), ("voice", voice_case()), ("silent", silent_case()),
            ("saturating", saturating_case()), ("wild_table", wild_table_case()), ("broken_rooms", broken_rooms_case()),
            ("nrooms_2", nrooms_case(2)), ("nrooms_0", nrooms_case(0))]
    return out


def poison_cases():
    """The cases only float32 can hold: a NaN, an Inf and a finite sample whose square overflows."""
    return [("poison_%s" % name, poisoned_case(F(v))) for name, v in (("nan", np.nan), ("inf", np.inf), ("square_overflows", 1e30))]


def to_pcm(x):
    return np.clip(np.rint(x.astype(np.float64) * 32768), -32768, 32767).astype(np.int16)


def rows_of(c):
    """(n_in, n_out) of a case: the input rows it has and as many output rows, two of which no seat names."""
    n_in = c["ticks"][0][0].shape[0]
    return n_in, n_in + 2


def run(c, impl, pcm, pad):
    """Runs the case through impl(x, out, room_start, seats, rec, params, nrooms, voice) -- x and out views of rows n + pad
    apart, out and rec written in place -- and through the checker; asserts equal bits of every output buffer (guards behind
    the rows and in unnamed rows included) and of the records after every block.  Returns the per-block (out, rec) of the
    checker."""
    n = c["n"]
    n_in, n_out = rows_of(c)
    guard = GUARD_I if pcm else GUARD_F
    rec_i = np.zeros((c["n_rec"], 4), F) if c["rec0"] is None else np.array(c["rec0"], F)
    rec_c, trace = rec_i.copy(), []
    for t, (x, voice, nrooms) in enumerate(c["ticks"]):
        x = to_pcm(x) if pcm else x
        xbuf = np.full((n_in, n + pad), guard, x.dtype)
        xbuf[:, :n] = x
        obuf = np.full((n_out, n + pad), guard, x.dtype)
        impl(xbuf[:, :n], obuf[:, :n], c["room_start"], c["seats"], rec_i, c["params"], nrooms, voice)
        want = np.full((n_out, n), guard, x.dtype)
        MK.mix(x, want, c["room_start"], c["seats"], rec_c, c["params"], nrooms, voice, 1)
        assert MK.same_bits(obuf[:, :n], want), "block %d: outputs differ in rows %s" % (
            t, sorted(set(np.nonzero(obuf[:, :n].view(np.uint8).reshape(n_out, -1) != want.view(np.uint8).reshape(n_out, -1))[0])))
        assert (obuf[:, n:] == guard).all(), "block %d: a store went behind a row" % t
        assert MK.same_bits(rec_i, rec_c), "block %d: records differ at %s" % (
            t, sorted(set(np.nonzero(rec_i.view(np.uint32) != rec_c.view(np.uint32))[0])))
        trace.append((want, rec_c.copy()))
    return trace
