"""Conference rooms (include/gtcrn_micro_hip.h, "conference rooms"): every participant of a room receives
the sum of the other talkers, limited to the few who speak and faded when they change, on the device where a live step has
just written the enhanced blocks.  `Mixer` owns the device tables of a bridge; `mix_params` and `mix_rooms_host` are the host
side of the same contract (the parameter words, and the functions the kernel compiles run on numpy arrays)."""
import ctypes

import numpy as np

from ._lib import GtcrnError, _check, _stream_ptr, lib

MIX_DEFAULTS = {"k": 3, "floor_dbov": -50.0, "release": 0.125, "incumbent_db": 3.0}
MIX_MAX_ROOM = 1024


class MixConfig(ctypes.Structure):
    _fields_ = [("k", ctypes.c_int), ("floor_dbov", ctypes.c_double), ("alpha", ctypes.c_double), ("incumbent_db", ctypes.c_double)]


def mix_params(**fields):
    """The 8 parameter words of the mix for the defaults (k=3, floor_dbov=-50, release=0.125, incumbent_db=3) with `fields`
    replaced: a float32 array from gtcrn_mix_params_host, the one place the words are made.  `release` is the contract's alpha."""
    unknown = set(fields) - set(MIX_DEFAULTS)
    if unknown:
        raise GtcrnError(f"unknown mixer fields {sorted(unknown)}: the config has {sorted(MIX_DEFAULTS)}")
    f = dict(MIX_DEFAULTS, **fields)
    if isinstance(f["k"], float) and not f["k"].is_integer():
        raise GtcrnError(f"k must be an integer, got {f['k']}")
    try:
        k = int(f["k"])
    except (OverflowError, ValueError):
        raise GtcrnError(f"k must be an integer, got {f['k']}") from None
    cfg = MixConfig(max(min(k, 1 << 30), -(1 << 30)), float(f["floor_dbov"]), float(f["release"]), float(f["incumbent_db"]))
    out = np.empty(8, np.float32)
    _check(lib().gtcrn_mix_params_host(ctypes.byref(cfg), out.ctypes.data))
    return out


def _aligned(n, dtype):
    """A zeroed array of n elements whose first byte is 16-byte aligned."""
    item = np.dtype(dtype).itemsize
    raw = np.zeros(n * item + 16, np.uint8)
    off = (-raw.ctypes.data) % 16
    return raw[off:off + n * item].view(dtype)


def mix_rooms_host(x, out, room_start, seats, rec, params, nrooms=None, voice=None):
    """gtcrn_mix_rooms_host / _pcm16_host on numpy arrays: x (n_in, n) float32 or int16 (rows may be a strided view), out
    (n_out, n) of the same type and rec (n_rec, 4) float32 are written in place; room_start (R + 1,) and seats (S, 4) int32;
    params the 8 words; nrooms None or a count; voice None or a 1-D float32 array or view indexed by rec."""
    pcm = x.dtype == np.int16
    if x.dtype not in (np.float32, np.int16) or out.dtype != x.dtype or x.ndim != 2 or out.ndim != 2 or x.shape[1] != out.shape[1]:
        raise GtcrnError("x and out must be (rows, n) arrays of one type, float32 or int16")
    item = x.dtype.itemsize
    for v in (x, out):
        if v.shape[1] > 1 and v.strides[1] != item or v.strides[0] % item:
            raise GtcrnError("the samples of a row must be contiguous")
    if rec.dtype != np.float32 or rec.ndim != 2 or rec.shape[1] != 4 or not rec.flags.c_contiguous or not out.flags.writeable:
        raise GtcrnError("rec must be a contiguous (n_rec, 4) float32 array")
    n = x.shape[1]
    starts = np.ascontiguousarray(room_start, np.int32)
    table = _aligned(4 * len(seats), np.int32)
    table[:] = np.asarray(seats, np.int32).reshape(-1)
    words = _aligned(8, np.float32)
    words[:] = np.asarray(params, np.float32)
    records = _aligned(rec.size, np.float32)
    records[:] = rec.reshape(-1)
    count = None if nrooms is None else np.array([nrooms], np.int32)
    vptr, vstride = None, 0
    if voice is not None:
        if voice.dtype != np.float32 or voice.ndim != 1 or voice.strides[0] % 4 or voice.strides[0] <= 0:
            raise GtcrnError("voice must be a 1-D float32 array or view")
        vptr, vstride = voice.ctypes.data, voice.strides[0] // 4
    fn = lib().gtcrn_mix_rooms_pcm16_host if pcm else lib().gtcrn_mix_rooms_host
    stride = lambda v: max(v.strides[0] // item, n) if v.shape[0] > 1 else n
    _check(fn(x.ctypes.data, stride(x), x.shape[0], out.ctypes.data, stride(out), out.shape[0], n, starts.ctypes.data,
              table.ctypes.data, len(seats), len(starts) - 1, None if count is None else count.ctypes.data, records.ctypes.data,
              rec.shape[0], words.ctypes.data, vptr, vstride))
    rec[:] = records.reshape(rec.shape)


class Mixer:
    """The rooms of a bridge on one device: `participants` records, tables for at most `max_rooms` rooms and `max_seats` seats in
    all, and the parameter words, all of fixed capacity and fixed address, so that a captured graph that holds a `mix` call
    stays valid while rooms, parameters and the room count change between replays."""

    def __init__(self, participants, max_rooms, max_seats, device, k=3, floor_dbov=-50.0, release=0.125, incumbent_db=3.0):
        import torch
        self.device = torch.device("cuda", device) if isinstance(device, int) else torch.device(device)
        if self.device.type != "cuda":
            raise GtcrnError("a Mixer lives on a CUDA (ROCm) device: there is no CPU path")
        self.participants, self.max_rooms, self.max_seats = int(participants), int(max_rooms), int(max_seats)
        if self.participants < 1 or self.max_rooms < 1 or self.max_seats < 1:
            raise GtcrnError("participants, max_rooms and max_seats must be positive")
        z = lambda shape, dt: torch.zeros(shape, device=self.device, dtype=dt)
        self.rec = z((self.participants, 4), torch.float32)
        self.room_start = z((self.max_rooms + 1,), torch.int32)
        self.seats = z((self.max_seats, 4), torch.int32)
        self.nrooms = z((1,), torch.int32)
        self.params = z((8,), torch.float32)
        self.fields = dict(MIX_DEFAULTS)
        self._rows = (-1, -1)           # the largest input and output row the tables name
        self.set_params(k=k, floor_dbov=floor_dbov, release=release, incumbent_db=incumbent_db)

    def _upload(self, dst, arr):
        import torch
        if arr.size == 0:
            return
        src = torch.from_numpy(np.ascontiguousarray(arr)).pin_memory()
        dst.view(-1)[:src.numel()].copy_(src.view(-1), non_blocking=True)

    def set_params(self, **fields):
        """Replaces the named fields (k, floor_dbov, release, incumbent_db) and writes the parameter words in place."""
        words = mix_params(**dict(self.fields, **fields))
        self.fields.update(fields)
        self._upload(self.params, words)

    def set_rooms(self, rooms, in_rows=None, out_rows=None):
        """rooms: a list of lists of participant ids, a seat per id in that order.  in_rows / out_rows map a participant to
        the row of x / out it sends in / listens on (a mapping, or a sequence indexed by id); None: the id itself; -1 or missing:
        absent.  A participant or an output row named twice, an id outside the records, more rooms or seats than the tables
        hold or a room above 1024 seats is refused here; the tables and the room count are then written in place."""
        def row_of(table, p):
            if table is None:
                return p
            if hasattr(table, "get"):
                return int(table.get(p, -1))
            return int(table[p]) if p < len(table) else -1
        rooms = [list(r) for r in rooms]
        total = sum(len(r) for r in rooms)
        if len(rooms) > self.max_rooms or total > self.max_seats:
            raise GtcrnError(f"{len(rooms)} rooms and {total} seats: the tables hold {self.max_rooms} and {self.max_seats}")
        starts = np.full(self.max_rooms + 1, total, np.int32)
        table = np.zeros((max(total, 1), 4), np.int32)
        seen, heard, k = set(), set(), 0
        for r, room in enumerate(rooms):
            if len(room) > MIX_MAX_ROOM:
                raise GtcrnError(f"room {r} has {len(room)} seats: at most {MIX_MAX_ROOM}")
            starts[r] = k
            for p in room:
                p = int(p)
                if not 0 <= p < self.participants:
                    raise GtcrnError(f"participant {p} of room {r} is outside 0 .. {self.participants - 1}")
                if p in seen:
                    raise GtcrnError(f"participant {p} is named twice")
                seen.add(p)
                i, o = row_of(in_rows, p), row_of(out_rows, p)
                if i < -1 or o < -1:
                    raise GtcrnError(f"participant {p}: a row is -1 (absent) or a row index")
                if o >= 0:
                    if o in heard:
                        raise GtcrnError(f"output row {o} is named twice")
                    heard.add(o)
                table[k] = (i, o, p, 0)
                k += 1
        self._upload(self.room_start, starts)
        self._upload(self.seats, table[:total])
        self._upload(self.nrooms, np.array([len(rooms)], np.int32))
        self._rows = (max((int(t[0]) for t in table[:total]), default=-1), max((int(t[1]) for t in table[:total]), default=-1))

    def mix(self, x, out=None, voice=None):
        """One tick: x (rows, n) float32 or int16 on the device, the enhanced blocks; returns `out` (None: zeros of x's shape),
        its rows written as set_rooms named them.  voice: a 1-D float32 tensor or strided view indexed by participant, such as
        state.alc[:, 3]; None: the energy floor decides who speaks.  One launch, asynchronous, capturable when `out` is given."""
        import torch
        if not isinstance(x, torch.Tensor) or x.device != self.device or x.dtype not in (torch.float32, torch.int16) or x.dim() != 2:
            raise GtcrnError(f"x must be a (rows, n) float32 or int16 tensor on {self.device}")
        if x.stride(1) != 1 and x.shape[1] > 1:
            x = x.contiguous()
        n = x.shape[1]
        if out is None:
            out = torch.zeros_like(x, memory_format=torch.contiguous_format)
        if not isinstance(out, torch.Tensor) or out.device != self.device or out.dtype != x.dtype or out.dim() != 2 or \
                out.shape[1] != n or (out.stride(1) != 1 and n > 1):
            raise GtcrnError("out must be a (rows, n) tensor of x's type and device with contiguous rows")
        rows = self._rows
        if rows[0] >= x.shape[0] or rows[1] >= out.shape[0]:
            raise GtcrnError(f"the rooms name input row {rows[0]} and output row {rows[1]}: x has {x.shape[0]} rows, out {out.shape[0]}")
        vptr, vstride = None, 0
        if voice is not None:
            if not isinstance(voice, torch.Tensor) or voice.device != self.device or voice.dtype != torch.float32 or \
                    voice.dim() != 1 or voice.shape[0] < self.participants or voice.stride(0) < 1:
                raise GtcrnError(f"voice must be a 1-D float32 tensor or view of at least {self.participants} words on {self.device}")
            vptr, vstride = voice.data_ptr(), voice.stride(0)
        fn = lib().gtcrn_mix_rooms_pcm16 if x.dtype == torch.int16 else lib().gtcrn_mix_rooms
        with torch.cuda.device(self.device):
            _check(fn(x.data_ptr(), max(x.stride(0), n), x.shape[0], out.data_ptr(), max(out.stride(0), n), out.shape[0], n,
                      self.room_start.data_ptr(), self.seats.data_ptr(), self.max_seats, self.max_rooms, self.nrooms.data_ptr(),
                      self.rec.data_ptr(), self.participants, self.params.data_ptr(), vptr, vstride, _stream_ptr()))
        return out

    def records(self):
        """A copy of the records: (participants, 4) float32 {g, level, picked, blocks}."""
        return self.rec.clone()

    def selected(self):
        """(participants,) bool: who ended the last block in the mix."""
        return self.rec[:, 0] == 1

    def reset(self, ids=None):
        """Zeroes the records of `ids` (None: all): fresh participants."""
        import torch
        if ids is None:
            self.rec.zero_()
        else:
            idx = torch.as_tensor(ids, device=self.device, dtype=torch.long).view(-1)
            if idx.numel() and (int(idx.min()) < 0 or int(idx.max()) >= self.participants):
                raise GtcrnError(f"ids must lie in 0 .. {self.participants - 1}")
            self.rec[idx] = 0
